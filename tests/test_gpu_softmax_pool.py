"""kgx_softmax_pool / kgx_softmax_pool_backward against a float64 restatement.

The reference arithmetic (attention_pooling.py:175-180, :409-412) is
ops.softmax(scores, axis=0) then ops.sum(weights * inputs, axis=0), per graph;
`ref_pool` below is that in float64, and torch autograd through it is the
reference's gradient.  Bar: |a - b| <= 1e-5 * max(1, |b|).  x carries a
constant 2.0 so the pooled values are O(1) and the bar is relative.  Schedules
are built with chunk length 64, so 65..197-node segments and the 5000-node
graph (79 chunks) take the split path and its fix-up.
"""

import functools

import numpy as np
import pytest
import torch

from keras_geometric_amd import _native as nat
from keras_geometric_amd import graph as G
from keras_geometric_amd import ops as kops

pytestmark = pytest.mark.gpu

CHUNK = 64
SIZES = [0, 1, 2, 63, 64, 65, 127, 128, 129, 3 * 64 + 5]
WIDTHS = [1, 3, 4, 16, 100, 128, 256]
INF = float("inf")


def assert_bar(a, b, what=""):
    a = a.detach().cpu().double().numpy() if isinstance(a, torch.Tensor) else np.asarray(a, dtype=np.float64)
    b = b.detach().cpu().double().numpy() if isinstance(b, torch.Tensor) else np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape, f"{what}: shape {a.shape} vs {b.shape}"
    err = np.abs(a - b) / np.maximum(1.0, np.abs(b))
    worst = float(err.max()) if err.size else 0.0
    print(f"{what} max scaled err {worst:.3e}")
    assert worst <= 1e-5, f"{what}: max scaled err {worst:.3g}"


def ref_pool(x, s, seg, n_seg):
    """float64: out[g] = sum_{i: seg[i] == g} softmax(s[seg == g])_i x[i]; ids outside [0, n_seg) pool nowhere."""
    rows = []
    for g in range(n_seg):
        sel = (seg == g).nonzero().reshape(-1)
        if sel.numel() == 0:
            rows.append(torch.zeros(x.shape[1], dtype=x.dtype))
            continue
        w = torch.softmax(s[sel], dim=0)
        rows.append((w.unsqueeze(1) * x[sel]).sum(0))
    return torch.stack(rows)


def batch_vector(shuffled: bool) -> np.ndarray:
    b = np.repeat(np.arange(len(SIZES)), SIZES).astype(np.int32)
    if shuffled:
        b = b[np.random.default_rng(11).permutation(b.size)]
    return b


@functools.lru_cache(maxsize=None)
def batch_case(F: int, shuffled: bool):
    """(x, s, batch, float64 reference) of the ten-segment batch, made once per width and order."""
    rng = np.random.default_rng(100 + F)
    b = batch_vector(shuffled)
    x = (rng.standard_normal((b.size, F)) + 2.0).astype(np.float32)
    s = (3.0 * rng.standard_normal(b.size)).astype(np.float32)
    ref = ref_pool(torch.from_numpy(x).double(), torch.from_numpy(s).double(), torch.from_numpy(b).long(), len(SIZES))
    return x, s, b, ref


def seg_graph(batch: np.ndarray, n_seg: int, dev, split_len: int = CHUNK) -> G.CSRGraph:
    n = batch.size
    src = torch.arange(n, dtype=torch.int32, device=dev)
    return G.build_csr(src, torch.from_numpy(batch).to(dev), n, n_seg, segment_only=True, split_len=split_len)


T = torch.from_numpy


# -- forward, segments --------------------------------------------------------
@pytest.mark.parametrize("shuffled", [False, True], ids=["sorted", "shuffled"])
@pytest.mark.parametrize("F", WIDTHS)
def test_forward_segments(dev, F, shuffled):
    x, s, b, ref = batch_case(F, shuffled)
    g = seg_graph(b, len(SIZES), dev)
    assert g.n_split == sum(1 for n in SIZES if n >= CHUNK)
    out = kops.softmax_pool(g, T(x).to(dev), T(s).to(dev))
    assert out.shape == (len(SIZES), F)
    assert_bar(out, ref, f"segments F={F}")
    assert (out[0] == 0).all()  # the empty segment: the sum over no rows


# -- forward, one graph of 5000 nodes (79 chunks) -----------------------------
N1 = 5000


@functools.lru_cache(maxsize=None)
def one_graph_x():
    return (np.random.default_rng(5).standard_normal((N1, 128)) + 2.0).astype(np.float32)


def one_graph_scores(kind: str) -> np.ndarray:
    rng = np.random.default_rng(6)
    if kind == "ramp":  # early chunks underflow entirely against the last ones
        return np.linspace(-200.0, 50.0, N1).astype(np.float32)
    if kind == "equal":
        return np.full(N1, 0.75, dtype=np.float32)
    if kind == "huge":  # exp(1e4) overflows unless the max is subtracted
        return (1e4 + rng.standard_normal(N1)).astype(np.float32)
    s = rng.standard_normal(N1).astype(np.float32)  # "neg_inf": one node with weight 0
    s[1234] = -INF
    return s


@pytest.mark.parametrize("kind", ["ramp", "equal", "huge", "neg_inf"])
def test_forward_one_graph(dev, kind):
    x, s = one_graph_x(), one_graph_scores(kind)
    g = G.single_segment_graph(N1, dev, chunk_len=CHUNK)
    assert g.n_items == 79 and g.n_split == 1 and g.col is None
    out = kops.softmax_pool(g, T(x).to(dev), T(s).to(dev))
    xd, sd = T(x).double(), T(s).double()
    ref = ref_pool(xd, sd, torch.zeros(N1, dtype=torch.long), 1)
    assert_bar(out, ref, f"one graph {kind}")
    assert torch.isfinite(out).all()
    if kind == "equal":
        assert_bar(out, xd.mean(0, keepdim=True), "equal scores = mean")
    if kind == "neg_inf":
        keep = np.arange(N1) != 1234
        assert_bar(out, ref_pool(xd[keep], sd[keep], torch.zeros(N1 - 1, dtype=torch.long), 1), "-inf has weight 0")


# -- forward, edge cases ------------------------------------------------------
def test_all_neg_inf_segment_is_nan_in_its_row_alone(dev):
    sizes = [5, 130, 3, 0, 70, 200]  # segments 0 (whole) and 1 (split in 3 chunks) are all -inf
    b = np.repeat(np.arange(len(sizes)), sizes).astype(np.int32)
    rng = np.random.default_rng(8)
    x = (rng.standard_normal((b.size, 16)) + 2.0).astype(np.float32)
    s = rng.standard_normal(b.size).astype(np.float32)
    s[b <= 1] = -INF
    s[b == 5] = np.where(np.arange(200) < 150, -INF, s[b == 5])  # whole chunks of -inf before finite ones
    g = seg_graph(b, len(sizes), dev)
    out = kops.softmax_pool(g, T(x).to(dev), T(s).to(dev)).cpu()
    assert torch.isnan(out[0]).all() and torch.isnan(out[1]).all()
    assert (out[3] == 0).all()  # empty
    ref = ref_pool(T(x).double(), T(s).double(), T(b).long(), len(sizes))
    assert torch.isnan(ref[0]).all() and torch.isnan(ref[1]).all()  # what torch.softmax gives
    assert_bar(out[[2, 4, 5]], ref[[2, 4, 5]], "rows beside the NaN rows")
    # +inf / NaN scores poison their own row only
    s2 = rng.standard_normal(b.size).astype(np.float32)
    s2[np.flatnonzero(b == 1)[70]] = INF
    s2[np.flatnonzero(b == 4)[3]] = np.nan
    out2 = kops.softmax_pool(g, T(x).to(dev), T(s2).to(dev)).cpu()
    assert torch.isnan(out2[1]).all() and torch.isnan(out2[4]).all()
    ref2 = ref_pool(T(x).double(), T(s2).double(), T(b).long(), len(sizes))
    assert_bar(out2[[0, 2, 3, 5]], ref2[[0, 2, 3, 5]], "rows beside the poisoned rows")


# -- forward, input layouts ---------------------------------------------------
def test_input_layouts(dev):
    _, s, b, _ = batch_case(128, False)
    rng = np.random.default_rng(9)
    wide = (rng.standard_normal((b.size, 300)) + 2.0).astype(np.float32)
    wd = T(wide).to(dev)
    g = seg_graph(b, len(SIZES), dev)
    sd, bl = T(s).to(dev), T(b).long()

    def ref(cols):
        return ref_pool(T(wide[:, cols]).double(), T(s).double(), bl, len(SIZES))

    # a column slice of a wider tensor: ld_x = 300 > F, rows still 16-byte aligned (float4 lanes)
    v = wd[:, 16:144]
    assert v.stride(0) == 300 and v.data_ptr() % 16 == 0 and kops.softmax_pool_supported(v)
    assert_bar(kops.softmax_pool(g, v, sd), ref(slice(16, 144)), "ld_x > F")
    # a 4-byte aligned view: the scalar lanes, two and four features per lane
    for lo, hi in ((1, 129), (1, 257)):
        v = wd[:, lo:hi]
        assert v.data_ptr() % 16 == 4 and kops.softmax_pool_supported(v)
        assert_bar(kops.softmax_pool(g, v, sd), ref(slice(lo, hi)), f"4-byte aligned view F={hi - lo}")
    # F above the kernel's maximum: the composed torch form, same answer
    v = wd[:, :260].contiguous()
    assert not kops.softmax_pool_supported(v)
    assert_bar(kops.softmax_pool(g, v, sd), ref(slice(0, 260)), "F = 260 (composed)")
    # a strided last dimension: composed too
    v = wd[:, 0:256:2]
    assert not kops.softmax_pool_supported(v)
    assert_bar(kops.softmax_pool(g, v, sd), ref(slice(0, 256, 2)), "strided columns (composed)")
    # and the composed form on the single graph
    g1 = G.single_segment_graph(b.size, dev, chunk_len=CHUNK)
    v = wd[:, :260].contiguous()
    assert_bar(kops.softmax_pool(g1, v, sd),
               ref_pool(T(wide[:, :260]).double(), T(s).double(), torch.zeros(b.size, dtype=torch.long), 1),
               "F = 260 single graph (composed)")


# -- fused score --------------------------------------------------------------
@pytest.mark.parametrize("tanh", [True, False], ids=["tanh", "linear"])
@pytest.mark.parametrize("F", [3, 100, 128])
def test_fused_score(dev, F, tanh):
    x, _, b, _ = batch_case(F, True)
    rng = np.random.default_rng(12)
    u = (rng.standard_normal(F) / np.sqrt(F)).astype(np.float32)
    c = rng.standard_normal(len(SIZES)).astype(np.float32)
    z = T(x).double() @ T(u).double() + T(c).double()[T(b).long()]
    s64 = torch.tanh(z) if tanh else z
    ref = ref_pool(T(x).double(), s64, T(b).long(), len(SIZES))
    g = seg_graph(b, len(SIZES), dev)
    items, _, split, _, n_slots = g.work(False)
    out, stats, s_out = torch.ops.kgx.softmax_pool_save(
        T(x).to(dev), g.rowptr, g.rows, items, split, g.col, None, T(u).to(dev), T(c).to(dev), tanh, n_slots)
    assert_bar(s_out, s64, f"s_out F={F}")
    assert_bar(out, ref, f"fused score F={F}")
    assert_bar(kops.softmax_pool(g, T(x).to(dev), score_u=T(u).to(dev), score_c=T(c).to(dev), tanh=tanh), ref,
               "public form")
    # stats = (max, denominator) of every non-empty segment
    for r in range(1, len(SIZES)):
        sr = s64[T(b).long() == r]
        assert_bar(stats[r].cpu(), torch.stack([sr.max(), torch.exp(sr - sr.max()).sum()]), f"stats[{r}]")


def test_fused_score_one_graph(dev):
    x = one_graph_x()
    rng = np.random.default_rng(13)
    u = (rng.standard_normal(128) / 8).astype(np.float32)
    c = np.array([0.3], dtype=np.float32)
    s64 = torch.tanh(T(x).double() @ T(u).double() + 0.3)
    g = G.single_segment_graph(N1, dev, chunk_len=CHUNK)
    out = kops.softmax_pool(g, T(x).to(dev), score_u=T(u).to(dev), score_c=T(c).to(dev), tanh=True)
    assert_bar(out, ref_pool(T(x).double(), s64, torch.zeros(N1, dtype=torch.long), 1), "fused one graph")


# -- chunking -----------------------------------------------------------------
@pytest.mark.parametrize("F", [4, 100, 256])
def test_split_unsplit_and_rows_agree(dev, F):
    x, s, b, ref = batch_case(F, True)
    xd, sd = T(x).to(dev), T(s).to(dev)
    g = seg_graph(b, len(SIZES), dev)
    g0 = seg_graph(b, len(SIZES), dev, split_len=0)
    assert g.n_split > 0 and g0.n_split == 0 and g0.n_items == len(SIZES)
    split = kops.softmax_pool(g, xd, sd)
    unsplit = kops.softmax_pool(g0, xd, sd)
    rows = torch.ops.kgx.softmax_pool(xd, g.rowptr, g.rows, None, None, g.col, sd, None, None, False, 0)
    for name, out in (("split", split), ("unsplit", unsplit), ("items = NULL", rows)):
        assert_bar(out, ref, f"{name} F={F}")
    assert_bar(split, unsplit.double(), "split vs unsplit")
    assert_bar(rows, unsplit.double(), "rows vs unsplit")


# -- determinism --------------------------------------------------------------
def test_bit_identical_runs(dev):
    x, s, b, _ = batch_case(128, True)
    rng = np.random.default_rng(14)
    u = T((rng.standard_normal(128) / 11).astype(np.float32)).to(dev)
    c = T(rng.standard_normal(len(SIZES)).astype(np.float32)).to(dev)
    gout = T(rng.standard_normal((len(SIZES), 128)).astype(np.float32)).to(dev)
    g = seg_graph(b, len(SIZES), dev)

    def run(fused):
        xd = T(x).to(dev).requires_grad_(True)
        if fused:
            ud, cd = u.clone().requires_grad_(True), c.clone().requires_grad_(True)
            out = kops.softmax_pool(g, xd, score_u=ud, score_c=cd, tanh=True)
            out.backward(gout)
            return out.detach(), xd.grad, ud.grad, cd.grad
        sd = T(s).to(dev).requires_grad_(True)
        out = kops.softmax_pool(g, xd, sd)
        out.backward(gout)
        return out.detach(), xd.grad, sd.grad

    for fused in (False, True):
        for a, bb in zip(run(fused), run(fused)):
            assert torch.equal(a, bb)
    g1 = G.single_segment_graph(N1, dev, chunk_len=CHUNK)
    x1, s1 = T(one_graph_x()).to(dev), T(one_graph_scores("ramp")).to(dev)
    assert torch.equal(kops.softmax_pool(g1, x1, s1), kops.softmax_pool(g1, x1, s1))


# -- backward -----------------------------------------------------------------
def _loss_weights(n_seg, F, seed=15):
    return np.random.default_rng(seed).standard_normal((n_seg, F)).astype(np.float32)


@pytest.mark.parametrize("F", [3, 100, 128])
def test_backward_given_scores(dev, F):
    x, s, b, _ = batch_case(F, True)
    gw = _loss_weights(len(SIZES), F)
    g = seg_graph(b, len(SIZES), dev)
    xd, sd = T(x).to(dev).requires_grad_(True), T(s).to(dev).requires_grad_(True)
    kops.softmax_pool(g, xd, sd).backward(T(gw).to(dev))
    xr, sr = T(x).double().requires_grad_(True), T(s).double().requires_grad_(True)
    ref_pool(xr, sr, T(b).long(), len(SIZES)).backward(T(gw).double())
    assert_bar(xd.grad, xr.grad, f"grad_x F={F}")
    assert_bar(sd.grad, sr.grad, f"grad_s F={F}")


@pytest.mark.parametrize("F", [3, 100, 128])
def test_backward_fused_scores(dev, F):
    x, _, b, _ = batch_case(F, True)
    rng = np.random.default_rng(16)
    u = (rng.standard_normal(F) / np.sqrt(F)).astype(np.float32)
    c = rng.standard_normal(len(SIZES)).astype(np.float32)
    gw = _loss_weights(len(SIZES), F)
    g = seg_graph(b, len(SIZES), dev)
    xd, ud, cd = (T(a).to(dev).requires_grad_(True) for a in (x, u, c))
    kops.softmax_pool(g, xd, score_u=ud, score_c=cd, tanh=True).backward(T(gw).to(dev))
    xr, ur, cr = (T(a).double().requires_grad_(True) for a in (x, u, c))
    s64 = torch.tanh(xr @ ur + cr[T(b).long()])
    ref_pool(xr, s64, T(b).long(), len(SIZES)).backward(T(gw).double())
    assert_bar(xd.grad, xr.grad, f"fused grad_x F={F}")
    assert_bar(ud.grad, ur.grad, f"grad_u F={F}")
    assert_bar(cd.grad, cr.grad, f"grad_c F={F}")


def test_backward_one_graph_ramp(dev):
    x, s = one_graph_x(), one_graph_scores("ramp")
    gw = _loss_weights(1, 128)
    g = G.single_segment_graph(N1, dev, chunk_len=CHUNK)
    seg0 = torch.zeros(N1, dtype=torch.long)
    xd, sd = T(x).to(dev).requires_grad_(True), T(s).to(dev).requires_grad_(True)
    kops.softmax_pool(g, xd, sd).backward(T(gw).to(dev))
    xr, sr = T(x).double().requires_grad_(True), T(s).double().requires_grad_(True)
    ref_pool(xr, sr, seg0, 1).backward(T(gw).double())
    assert_bar(xd.grad, xr.grad, "ramp grad_x")
    assert_bar(sd.grad, sr.grad, "ramp grad_s")
    # fused: the ramp comes from x itself (column 0 scaled), through tanh
    rng = np.random.default_rng(17)
    u = (rng.standard_normal(128) / 8).astype(np.float32)
    c = np.array([-0.2], dtype=np.float32)
    xd, ud, cd = (T(a).to(dev).requires_grad_(True) for a in (x, u, c))
    kops.softmax_pool(g, xd, score_u=ud, score_c=cd, tanh=True).backward(T(gw).to(dev))
    xr, ur, cr = (T(a).double().requires_grad_(True) for a in (x, u, c))
    ref_pool(xr, torch.tanh(xr @ ur + cr[0]), seg0, 1).backward(T(gw).double())
    assert_bar(xd.grad, xr.grad, "one graph fused grad_x")
    assert_bar(ud.grad, ur.grad, "one graph grad_u")
    assert_bar(cd.grad, cr.grad, "one graph grad_c")


def test_backward_out_of_range_segments_get_zeros(dev):
    x, s, b, _ = batch_case(16, True)
    b = b.copy()
    b[::7] = -1
    b[3::11] = len(SIZES) + 3
    outside = (b < 0) | (b >= len(SIZES))
    gw = _loss_weights(len(SIZES), 16)
    g = seg_graph(b, len(SIZES), dev)
    xd, sd = T(x).to(dev).requires_grad_(True), T(s).to(dev).requires_grad_(True)
    out = kops.softmax_pool(g, xd, sd)
    out.backward(T(gw).to(dev))
    xr, sr = T(x).double().requires_grad_(True), T(s).double().requires_grad_(True)
    ref = ref_pool(xr, sr, T(b).long(), len(SIZES))
    ref.backward(T(gw).double())
    assert_bar(out, ref, "forward with dropped ids")
    assert (xd.grad[T(outside).to(dev)] == 0).all() and (sd.grad[T(outside).to(dev)] == 0).all()
    assert_bar(xd.grad, xr.grad, "grad_x with dropped ids")
    assert_bar(sd.grad, sr.grad, "grad_s with dropped ids")
    # the kernel itself, with the raw batch vector as `seg`
    items, _, split, _, n_slots = g.work(False)
    o, stats, _ = torch.ops.kgx.softmax_pool_save(xd.detach(), g.rowptr, g.rows, items, split, g.col, sd.detach(),
                                                  None, None, False, n_slots)
    gx, gs = torch.ops.kgx.softmax_pool_backward(xd.detach(), T(b).to(dev), sd.detach(), stats, o, T(gw).to(dev))
    assert torch.equal(gx, xd.grad) and torch.equal(gs, sd.grad)


def test_unsupported_width_is_an_error_at_the_abi(dev):
    x = torch.zeros((4, nat.POOL_MAX_F + 4), device=dev)
    g = G.single_segment_graph(4, dev)
    with pytest.raises(ValueError, match="unsupported"):
        torch.ops.kgx.softmax_pool(x, g.rowptr, g.rows, None, None, None, torch.zeros(4, device=dev), None, None,
                                   False, 0)
