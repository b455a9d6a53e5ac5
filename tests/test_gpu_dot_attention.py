"""kgx_dot_attention / kgx_dot_attention_backward at op level (kops.dot_attention
on given q, k, v) against the float64 restatement of tests/dot_attention_ref.py:
split hub rows in both directions, every channels-per-lane layout, empty rows,
a bipartite graph, non-contiguous k / v, attention dropout on the split path,
the online-softmax rescale and fix-up merge, -inf scores, bit identity from
run to run, and the argument errors of the C entry points.

Graphs (gatv2_ref.make_graph): bipartite, multi-edges, destination 0 without
in-edges, the last source without out-edges, built with split_len=16; the
transposed graph is scheduled by graph.transpose with default_split_len = 256.
  small  60 -> 50, 600 random edges + 300 into destination 3 (19 chunks)
         + 600 out of source 7 (3 chunks of 256)
  deep   500 -> 400, 6000 random + 1000 into destination 3 (63 chunks: more
         than the forward fix-up's batch of 16, not a multiple of the backward
         fix-up's 8) + 2500 out of source 7 (10 chunks, the last one partial)

Lane layouts: K = channels per lane, LH = lanes per head; one rule for the
forward and both backward passes (mirrored and asserted on the CPU in
tests/test_dot_attention_ref_host.py):
  (8,16) 8/2   (8,64) 8/8   (8,128) 16/8   (4,256) 16/16   (1,64) 8/8
  (3,12) 4/4, padding sub-lane and padding head
  (2,7)  1/8, scalar loads, padding sub-lane
  (3,6)  2/4, row stride 18 (not a multiple of 4), float2 loads

Bounds, float64 reference throughout (the project's own, test_gpu_gatv2_op.py):
  out              |got - ref| <= 1e-5 * max(1, |ref|)
  d q, d k, d v    |got - ref| <= 1e-5 * max(1, A)
A is the sum of the magnitudes of the per-edge contributions to that element
(dot_attention_ref.dot_attention_grads64).

Largest err / bound (GPU: MI355X, all cases of this module; fp32 restatement:
tests/test_dot_attention_ref_host.py on the lane-layout inputs):

  quantity   GPU     fp32 restatement
  out        0.05    0.10
  d q        0.26    0.15
  d k        0.12    0.11
  d v        0.12    0.09
No ratio is above 0.5.  The largest, d q 0.26, is the dominant-edge case at
8 x 16 (a hub row of 1000 edges whose scores span e^30), in both modes alike.
"""

from __future__ import annotations

import ctypes

import pytest
import torch

import dot_attention_ref as DR
from keras_geometric_amd import graph as G
from keras_geometric_amd import ops as kops

pytestmark = pytest.mark.gpu

_GRAPHS: dict = {}
_WORST: dict = {}


def _build(dev, src, dst, n_src, n_dst):
    return G.build_csr(src.to(torch.int32).to(dev), dst.to(torch.int32).to(dev), n_src, n_dst,
                       split_len=DR.SPLIT_LEN)


def _graph(dev, name):
    g = _GRAPHS.get(name)
    if g is None:
        g = _GRAPHS[name] = _build(dev, *DR.make_graph(name))
    return g


def _assert_split(g):
    """The split path is the point: both directions have chunked rows."""
    t = G.transpose(g)
    assert g.split_len == DR.SPLIT_LEN and g.n_split > 0 and t.n_split > 0
    assert t.split_len == 256
    return t


def _run(dev, g, x, heads, channels, exact, dropout=0.0, seed=0, halves=False):
    """Forward + backward of the op on the device: {out, d_q, d_k, d_v}.
    halves: k and v are the two column halves of one [n_src, 2 H C] tensor."""
    hc = heads * channels
    q = x["q"].to(dev).requires_grad_(True)
    if halves:
        kv = torch.cat([x["k"], x["v"]], dim=1).to(dev).requires_grad_(True)
        k, v = kv[:, :hc], kv[:, hc:]
        assert not k.is_contiguous() and not v.is_contiguous() and k.stride(0) == 2 * hc
    else:
        k, v = (x[n].to(dev).requires_grad_(True) for n in ("k", "v"))
    out = kops.dot_attention(g, q, k, v, heads, channels, exact=exact, dropout=dropout, seed=seed)
    out.backward(x["gout"].to(dev))
    if halves:
        return {"out": out.detach(), "d_q": q.grad, "d_k": kv.grad[:, :hc], "d_v": kv.grad[:, hc:]}
    return {"out": out.detach(), "d_q": q.grad, "d_k": k.grad, "d_v": v.grad}


def _check(label, got, ref):
    for k, v in got.items():
        assert bool(torch.isfinite(v).all()), f"{label}: {k} not finite"
    r = DR.ratios(got, ref)
    for k, v in r.items():
        _WORST[k] = max(_WORST.get(k, 0.0), v)
    msg = f"{label}: err / bound " + ", ".join(f"{k} {v:.3f}" for k, v in r.items())
    print(msg + " | worst so far " + ", ".join(f"{k} {v:.3f}" for k, v in _WORST.items()))
    assert all(v <= 1.0 for v in r.values()), msg
    return r


def _check_empty_rows(label, got, g):
    """Destination 0 has no in-edge, the last source no out-edge: exact zeros."""
    assert not bool(got["out"][0].any()), f"{label}: out of the empty destination is not 0"
    assert not bool(got["d_q"][0].any()), f"{label}: d q of the empty destination is not 0"
    assert not bool(got["d_k"][g.n_src - 1].any()), f"{label}: d k of the source without edges is not 0"
    assert not bool(got["d_v"][g.n_src - 1].any()), f"{label}: d v of the source without edges is not 0"


_LANE_SHAPES = DR.SHAPES + [(3, 6)]


# a. every lane layout (padding lanes, float2 and scalar loads included), split and unsplit, forward and backward
@pytest.mark.parametrize("exact", [False, True], ids=["split", "exact"])
@pytest.mark.parametrize("heads,channels", _LANE_SHAPES, ids=[f"{h}x{c}" for h, c in _LANE_SHAPES])
def test_lane_layouts(dev, heads, channels, exact):
    g = _graph(dev, "small")
    _assert_split(g)
    assert g.n_src != g.n_dst and int(g.deg[0]) == 0 and int(G.transpose(g).deg[g.n_src - 1]) == 0
    x = DR.make_inputs("small", heads, channels)
    got = _run(dev, g, x, heads, channels, exact)
    label = f"small {heads}x{channels} {'exact' if exact else 'split'}"
    _check(label, got, DR.reference("small", heads, channels))
    _check_empty_rows(label, got, g)


# b. split depth: more chunks than either fix-up loads per step
@pytest.mark.parametrize("heads,channels", DR.DEEP_SHAPES, ids=[f"{h}x{c}" for h, c in DR.DEEP_SHAPES])
def test_split_depth(dev, heads, channels):
    g = _graph(dev, "deep")
    t = _assert_split(g)
    sp, tsp = g.split.cpu(), t.split.cpu()
    assert sp[sp[:, 0] == DR.HUB_DST, 2].tolist() == [63]  # {row, first slot, chunks, _}
    assert tsp[tsp[:, 0] == DR.HUB_SRC, 2].tolist() == [10]
    x = DR.make_inputs("deep", heads, channels)
    ref = DR.reference("deep", heads, channels)
    got = {}
    for exact in (False, True):
        label = f"deep {heads}x{channels} {'exact' if exact else 'split'}"
        got[exact] = _run(dev, g, x, heads, channels, exact)
        _check(label, got[exact], ref)
        _check_empty_rows(label, got[exact], g)
    # rows below the chunk length take the same kernel path in both modes and
    # depend on their own row only: bit-identical
    short = g.deg.long() < DR.SPLIT_LEN
    assert 1 < int(short.sum()) < g.n_dst
    for k in ("out", "d_q"):
        assert torch.equal(got[False][k][short], got[True][k][short]), f"{k} of unsplit rows differs between modes"


# c. k and v as the two column halves of one tensor (what one kgx_dense with [W_k | W_v] writes)
@pytest.mark.parametrize("exact", [False, True], ids=["split", "exact"])
@pytest.mark.parametrize("heads,channels", [(8, 16), (3, 6)], ids=["8x16", "3x6"])
def test_noncontiguous_key_value(dev, heads, channels, exact):
    g = _graph(dev, "small")
    x = DR.make_inputs("small", heads, channels)
    got = _run(dev, g, x, heads, channels, exact, halves=True)
    _check(f"small {heads}x{channels} halves {'exact' if exact else 'split'}", got,
           DR.reference("small", heads, channels))
    plain = _run(dev, g, x, heads, channels, exact)
    for k in got:  # same lane layout, same operation order: the leading dimension changes addresses only
        assert torch.equal(got[k], plain[k]), k


# d. attention dropout on the split path
def test_attention_dropout_split(dev):
    (heads, channels), p, seed = DR.DROPOUT_SHAPE, DR.DROPOUT_P, DR.DROPOUT_SEED
    g = _graph(dev, "deep")
    _assert_split(g)
    src, dst, _, n_dst = DR.make_graph("deep")
    E = src.numel()
    mask = kops.dropout_mask(seed, p, torch.arange(E, dtype=torch.int32, device=dev), heads).cpu()
    dropped = float((mask == 0).float().mean())
    assert abs(dropped - p) < 0.02 and set(mask.unique().tolist()) == {0.0, float(mask.max())}
    x = DR.make_inputs("deep", heads, channels)
    ref = DR.dot_attention_grads64(x["q"], x["k"], x["v"], src, dst, n_dst, heads, channels, x["gout"],
                                   mask=mask.double())
    got = _run(dev, g, x, heads, channels, False, dropout=p, seed=seed)
    _check(f"deep {heads}x{channels} dropout split", got, ref)
    _check_empty_rows("deep dropout", got, g)
    plain = DR.reference("deep", heads, channels)
    assert DR.ratio(got["out"], plain["out"], plain["out"]) > 100  # the mask was applied
    # p = 0 is the no-dropout call bit for bit, through the layer-facing op and with keys handed to the kernel
    q, k, v = (x[n].to(dev) for n in ("q", "k", "v"))
    base = kops.dot_attention(g, q, k, v, heads, channels)
    assert torch.equal(kops.dot_attention(g, q, k, v, heads, channels, dropout=0.0, seed=seed), base)
    items, _, split, _, n_slots = g.work(False)
    keyed = torch.ops.kgx.dot_attention(q, k, v, g.rowptr, g.rows, items, split, g.col, heads, channels,
                                        channels ** -0.5, n_slots, g.eid, 0.0, seed)
    assert torch.equal(keyed, base)


# e. online-softmax rescale and fix-up merge: one edge outweighs the row by about e^30
@pytest.mark.parametrize("exact", [False, True], ids=["split", "exact"])
@pytest.mark.parametrize("heads,channels", DR.DOMINANT_SHAPES, ids=[f"{h}x{c}" for h, c in DR.DOMINANT_SHAPES])
@pytest.mark.parametrize("pos", list(DR.DOMINANT_POS))
def test_dominant_edge(dev, pos, heads, channels, exact):
    """The dominant edge sits at the first slot, at slot 17, in chunk 40 or at
    the last slot of the hub row: whatever was summed before it is rescaled by
    e^-30 (main loop in exact mode, fix-up merge in split mode), and the row
    comes out as (nearly) the dominant source's value row."""
    key = ("dominant", pos)
    g = _GRAPHS.get(key)
    src, dst, n_src, n_dst = DR.dominant_graph(DR.DOMINANT_POS[pos])
    if g is None:
        g = _GRAPHS[key] = _build(dev, src, dst, n_src, n_dst)
    assert g.n_split > 0
    row = g.col[int(g.rowptr[DR.HUB_DST]): int(g.rowptr[DR.HUB_DST + 1])]
    assert row.numel() == 1000
    assert torch.nonzero(row == DR.DOMINANT_SRC).flatten().tolist() == [DR.DOMINANT_POS[pos]]  # stable CSR order
    x = DR.dominant_inputs(heads, channels)
    ref = DR.dot_attention_grads64(x["q"], x["k"], x["v"], src, dst, n_dst, heads, channels, x["gout"])
    got = _run(dev, g, x, heads, channels, exact)
    _check(f"dominant {pos} {heads}x{channels} {'exact' if exact else 'split'}", got, ref)
    want = x["v"][DR.DOMINANT_SRC].to(dev)
    assert float((got["out"][DR.HUB_DST] - want).abs().max()) <= 1e-5 * max(1.0, float(want.abs().max()))


# f. no atomics anywhere: the same bits every run
@pytest.mark.parametrize("exact", [False, True], ids=["split", "exact"])
def test_bit_identical_run_to_run(dev, exact):
    g = _graph(dev, "deep")
    x = DR.make_inputs("deep", 8, 16)
    a = _run(dev, g, x, 8, 16, exact, dropout=0.25, seed=7)
    b = _run(dev, g, x, 8, 16, exact, dropout=0.25, seed=7)
    for k in ("out", "d_q", "d_k", "d_v"):
        assert torch.equal(a[k], b[k]), f"{k} differs between two runs"


# g. -inf scores
def _inf_case(heads, channels, hstar):
    """6 sources -> 5 destinations; source 1's key has -inf in channel 0 of head
    hstar and q's channel 0 of that head is positive, so every edge out of
    source 1 scores -inf in head hstar (and finite elsewhere).  Destination 0
    is empty, destination 2 has edges from source 1 only (twice)."""
    src = torch.tensor([0, 1, 2, 1, 1, 1, 3, 4, 5])
    dst = torch.tensor([1, 1, 1, 2, 2, 3, 3, 4, 4])
    g = torch.Generator().manual_seed(606)
    hc = heads * channels
    q, k, v = torch.randn(5, hc, generator=g), torch.randn(6, hc, generator=g), torch.randn(6, hc, generator=g)
    q[:, hstar * channels] = q[:, hstar * channels].abs() + 0.5
    k[1, hstar * channels] = float("-inf")
    return src, dst, q, k, v


@pytest.mark.parametrize("exact", [False, True], ids=["sched", "exact"])
@pytest.mark.parametrize("heads,channels", [(4, 8), (3, 12)], ids=["4x8", "3x12"])
def test_minus_inf_scores(dev, heads, channels, exact):
    hstar = 1
    src, dst, q, k, v = _inf_case(heads, channels, hstar)
    g = _build(dev, src, dst, 6, 5)
    with torch.no_grad():
        out = kops.dot_attention(g, q.to(dev), k.to(dev), v.to(dev), heads, channels, exact=exact).cpu()
    ref = DR.dot_attention_ref(q.double(), k.double(), v.double(), src, dst, 5, heads, channels)
    blk = torch.zeros(5, heads * channels, dtype=torch.bool)
    blk[2, hstar * channels:(hstar + 1) * channels] = True  # all scores -inf: NaN in its own block only
    assert bool(torch.isnan(ref[blk]).all()) and bool(torch.isfinite(ref[~blk]).all())  # the restatement agrees
    assert bool(torch.isnan(out[blk]).all()), "an all -inf (row, head) must be NaN"
    assert bool(torch.isfinite(out[~blk]).all()), "NaN outside the all -inf block"
    assert DR.ratio(out[~blk], ref[~blk], ref[~blk]) <= 1.0  # -inf edges weigh 0 in rows 1 and 3
    assert not bool(out[0].any())


@pytest.mark.parametrize("exact", [False, True], ids=["split", "exact"])
def test_minus_inf_chunks_of_a_split_row(dev, exact):
    """Chunks 0 and 2 of the hub row (slots 0-15 and 32-47) hold -inf scores
    only in head 1: the main loop starts on blocks that weigh nothing, and the
    fix-up merges chunks whose max is -inf, first and in between."""
    heads, channels, hstar, S = 8, 16, 1, DR.DOMINANT_SRC
    src, dst, n_src, n_dst = DR.make_graph("deep")
    src = src.clone()
    row = torch.nonzero(dst == DR.HUB_DST).flatten()
    src[row[src[row] == S]] = S + 1
    src[row[0:16]] = S
    src[row[32:48]] = S
    g = _build(dev, src, dst, n_src, n_dst)
    assert g.n_split > 0 and g.col[int(g.rowptr[DR.HUB_DST]):][:16].tolist() == [S] * 16
    x = DR.make_inputs("deep", heads, channels)
    q, k, v = x["q"].clone(), x["k"].clone(), x["v"]
    q[:, hstar * channels] = q[:, hstar * channels].abs() + 0.5
    k[S, hstar * channels] = float("-inf")
    with torch.no_grad():
        out = kops.dot_attention(g, q.to(dev), k.to(dev), v.to(dev), heads, channels, exact=exact).cpu()
    ref = DR.dot_attention_ref(q.double(), k.double(), v.double(), src, dst, n_dst, heads, channels)
    ok = torch.isfinite(ref)  # destinations fed by source S alone are NaN in head 1 in both
    assert bool(ok[DR.HUB_DST].all())
    assert torch.equal(torch.isnan(out), torch.isnan(ref))
    assert DR.ratio(out[ok], ref[ok], ref[ok]) <= 1.0


# h. argument errors of the C entry points: no launch, no device memory touched
def test_argument_errors():
    from keras_geometric_amd import _native as nat

    lib = nat.lib()
    P = ctypes.c_void_p

    def fwd(heads=8, channels=16, ld=128, q=16, ptr=16, drop_p=0.0, items=None, n_split=0):
        return lib.kgx_dot_attention(P(ptr), P(ptr), 1, items, 1 if items else 0, None, n_split, P(ptr),
                                     P(q) if q else None, ld, P(ptr), ld, P(ptr), ld, heads, channels, 0.25,
                                     P(ptr), max(ld, heads * channels), None, None, None, drop_p, 0, None)

    assert fwd(q=0) == nat.KGX_ERR_ARG and b"null pointer" in lib.kgx_last_error()
    assert fwd(ld=127) == nat.KGX_ERR_ARG and b"leading dimension" in lib.kgx_last_error()
    assert fwd(ld=2**31) == nat.KGX_ERR_ARG and b"2^31" in lib.kgx_last_error()
    assert fwd(drop_p=1.0) == nat.KGX_ERR_ARG and b"dropout" in lib.kgx_last_error()
    assert fwd(items=P(16), n_split=1) == nat.KGX_ERR_ARG and b"split" in lib.kgx_last_error()
    assert fwd(heads=0) == nat.KGX_ERR_ARG
    # more than 64 lanes per row at the widest usable K
    assert fwd(heads=16, channels=128, ld=2048) == nat.KGX_ERR_UNSUPPORTED and b"64 lanes" in lib.kgx_last_error()
    assert fwd(heads=64, channels=33, ld=64 * 33) == nat.KGX_ERR_UNSUPPORTED
    # 16 x 64 fits at 16 channels per lane only; pointers that allow no float4 loads leave it without a layout
    assert fwd(heads=16, channels=64, ld=1024, ptr=4, q=4) == nat.KGX_ERR_UNSUPPORTED

    def bwd(heads=8, channels=16, ld=128, stats=16, ptr=16):
        return lib.kgx_dot_attention_backward(
            P(ptr), P(ptr), 1, None, 0, None, 0, P(ptr), P(ptr), ld, P(ptr), ld, P(ptr), ld, heads, channels, 0.25,
            P(ptr), ld, P(stats) if stats else None, P(ptr), ld, P(ptr), P(ptr), 1, None, 0, None, 0, P(ptr),
            P(ptr), P(ptr), ld, P(ptr), ld, P(ptr), ld, P(ptr), None, None, 0.0, 0, None)

    assert bwd(stats=0) == nat.KGX_ERR_ARG and b"null pointer" in lib.kgx_last_error()
    assert bwd(ld=100) == nat.KGX_ERR_ARG and b"leading dimension" in lib.kgx_last_error()
    assert bwd(heads=16, channels=128, ld=2048) == nat.KGX_ERR_UNSUPPORTED
    assert bwd(heads=16, channels=64, ld=1024, ptr=4) == nat.KGX_ERR_UNSUPPORTED
