"""kgx_dot_attention_edge / kgx_dot_attention_edge_backward at op level
(kops.dot_attention(edge=...) on given q, k, v and projected edge rows e)
against the float64 restatement of tests/dot_attention_edge_ref.py: every lane
layout on split and unsplit rows, split depth, the two edge orders, e and
grad_e as column slices of wider tensors, attention dropout on the split path,
bit identity from run to run, a self-loop graph whose added slots carry no
feature, a NaN in one edge row, a cross-check through the op WITHOUT edge
features on the expanded graph, and the argument errors of the C entry points.

Graphs and lane layouts are those of tests/test_gpu_dot_attention.py
(gatv2_ref.make_graph "small" and "deep", split_len=16 forward and 256
transposed); inputs are dot_attention_ref.make_inputs plus a seeded e ~ N(0, 1)
of [E, H*C] in input-edge order (dot_attention_edge_ref.make_edge).

Bounds, float64 reference throughout (the project's own):
  out                   |got - ref| <= 1e-5 * max(1, |ref|)
  d q, d k, d v, d e    |got - ref| <= 1e-5 * max(1, A)
A is the sum of the magnitudes of the per-edge contributions to that element;
for d e the two uses of e (score and message) are the two contributions.

Largest err / bound (GPU: MI355X, all cases of this module; fp32 restatement:
tests/test_dot_attention_edge_ref_host.py):

  quantity   GPU     fp32 restatement
  out        0.11    0.13
  d q        0.15    0.19
  d k        0.09    0.08
  d v        0.04    0.05
  d e        0.10    0.11
No ratio is above 0.5.  The largest, d q 0.15, is 8 x 16 on `deep` in exact mode
(the hub row of 1000 edges summed in one chain).  The cross-check through the
op without edge features on the expanded graph (case 9) measured out 0.04,
d q 0.05, d k 0.04, d v 0.03, d e 0.04 and is not in the table.
"""

from __future__ import annotations

import ctypes

import pytest
import torch

import dot_attention_edge_ref as ER
import dot_attention_ref as DR
from keras_geometric_amd import _native as nat
from keras_geometric_amd import graph as G
from keras_geometric_amd import ops as kops

pytestmark = pytest.mark.gpu

_GRAPHS: dict = {}
_WORST: dict = {}
KEYS = ("out", "d_q", "d_k", "d_v", "d_e")


def _build(dev, src, dst, n_src, n_dst, **kw):
    return G.build_csr(src.to(torch.int32).to(dev), dst.to(torch.int32).to(dev), n_src, n_dst,
                       split_len=DR.SPLIT_LEN, **kw)


def _graph(dev, name):
    g = _GRAPHS.get(name)
    if g is None:
        g = _GRAPHS[name] = _build(dev, *DR.make_graph(name))
        t = G.transpose(g)
        assert g.split_len == DR.SPLIT_LEN and g.n_split > 0 and t.n_split > 0 and t.split_len == 256
        assert g.kept == g.n_input_edges
    return g


def _run(dev, g, x, e, heads, channels, exact, order="input", dropout=0.0, seed=0, pad=0):
    """Forward + backward of the op on the device: {out, d_q, d_k, d_v, d_e}, d e
    in input-edge order.  order="csr": the table is handed over permuted into
    CSR slot order and its gradient un-permuted.  pad > 0: e is the middle
    column block of a [E, pad + H C + pad] tensor."""
    hc = heads * channels
    q, k, v = (x[n].to(dev).requires_grad_(True) for n in ("q", "k", "v"))
    table = e.to(dev)
    if order == "csr":
        table = table[g.eid.long()].contiguous()
    if pad:
        wide = torch.cat([torch.full((table.shape[0], pad), 7.0, device=dev), table,
                          torch.full((table.shape[0], pad), -7.0, device=dev)], dim=1).requires_grad_(True)
        ev = wide[:, pad:pad + hc]
        assert not ev.is_contiguous() and ev.stride(0) == hc + 2 * pad
    else:
        wide = ev = table.requires_grad_(True)
    out = kops.dot_attention(g, q, k, v, heads, channels, exact=exact, dropout=dropout, seed=seed, edge=ev,
                             edge_order=order)
    out.backward(x["gout"].to(dev))
    d_e = wide.grad
    if pad:
        assert not bool(d_e[:, :pad].any()) and not bool(d_e[:, pad + hc:].any())
        d_e = d_e[:, pad:pad + hc]
    if order == "csr":
        back = torch.empty_like(d_e)
        back[g.eid.long()] = d_e
        d_e = back
    return {"out": out.detach(), "d_q": q.grad, "d_k": k.grad, "d_v": v.grad, "d_e": d_e}


def _check(label, got, ref):
    for k, v in got.items():
        assert bool(torch.isfinite(v).all()), f"{label}: {k} not finite"
    r = ER.ratios(got, ref)
    assert set(r) == set(got)
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


# 1. every lane layout, split and unsplit, all five quantities
@pytest.mark.parametrize("exact", [False, True], ids=["split", "exact"])
@pytest.mark.parametrize("heads,channels", _LANE_SHAPES, ids=[f"{h}x{c}" for h, c in _LANE_SHAPES])
def test_lane_layouts(dev, heads, channels, exact):
    g = _graph(dev, "small")
    assert g.n_src != g.n_dst and int(g.deg[0]) == 0 and int(G.transpose(g).deg[g.n_src - 1]) == 0
    x, e = DR.make_inputs("small", heads, channels), ER.make_edge("small", heads, channels)
    got = _run(dev, g, x, e, heads, channels, exact)
    label = f"small {heads}x{channels} {'exact' if exact else 'split'}"
    _check(label, got, ER.reference("small", heads, channels))
    _check_empty_rows(label, got, g)


# 2. split depth: more chunks than either fix-up loads per step
@pytest.mark.parametrize("heads,channels", DR.DEEP_SHAPES, ids=[f"{h}x{c}" for h, c in DR.DEEP_SHAPES])
def test_split_depth(dev, heads, channels):
    g = _graph(dev, "deep")
    sp = g.split.cpu()
    assert sp[sp[:, 0] == DR.HUB_DST, 2].tolist() == [63]
    x, e = DR.make_inputs("deep", heads, channels), ER.make_edge("deep", heads, channels)
    ref = ER.reference("deep", heads, channels)
    for exact in (False, True):
        label = f"deep {heads}x{channels} {'exact' if exact else 'split'}"
        got = _run(dev, g, x, e, heads, channels, exact)
        _check(label, got, ref)
        _check_empty_rows(label, got, g)


# 3. the two edge orders: the same arithmetic, other addresses
@pytest.mark.parametrize("exact", [False, True], ids=["split", "exact"])
@pytest.mark.parametrize("heads,channels", [(8, 16), (3, 12)], ids=["8x16", "3x12"])
def test_csr_order_is_input_order_bit_for_bit(dev, heads, channels, exact):
    g = _graph(dev, "small")
    assert not torch.equal(g.eid.cpu(), torch.arange(g.kept, dtype=torch.int32))  # a real permutation
    x, e = DR.make_inputs("small", heads, channels), ER.make_edge("small", heads, channels)
    a = _run(dev, g, x, e, heads, channels, exact, order="input")
    b = _run(dev, g, x, e, heads, channels, exact, order="csr")
    for k in KEYS:
        assert torch.equal(a[k], b[k]), f"{k} differs between the edge orders"
    _check(f"small {heads}x{channels} csr {'exact' if exact else 'split'}", b, ER.reference("small", heads, channels))


# 4. e a column slice of a wider tensor; grad_e written into a strided view
@pytest.mark.parametrize("heads,channels", [(8, 16), (3, 6)], ids=["8x16", "3x6"])
def test_strided_edge_table_and_gradient(dev, heads, channels):
    g = _graph(dev, "small")
    hc, pad = heads * channels, 4
    assert DR.layout(heads, channels, ld=hc + 2 * pad) == DR.layout(heads, channels)  # same lanes: same bits
    x, e = DR.make_inputs("small", heads, channels), ER.make_edge("small", heads, channels)
    plain = _run(dev, g, x, e, heads, channels, False)
    got = _run(dev, g, x, e, heads, channels, False, pad=pad)
    _check(f"small {heads}x{channels} strided e", got, ER.reference("small", heads, channels))
    for k in KEYS:
        assert torch.equal(got[k], plain[k]), k
    # the raw backward with grad_e a column block of a wider buffer (ld_ge != H C)
    t = G.transpose(g)
    items, _, split, _, n_slots = g.work(False)
    t_items, _, t_split, _, t_slots = t.work(False)
    q, k, v = (x[n].to(dev) for n in ("q", "k", "v"))
    wide = torch.cat([torch.zeros(e.shape[0], pad), e, torch.zeros(e.shape[0], pad)], dim=1).to(dev)
    ev = wide[:, pad:pad + hc]
    scale = channels ** -0.5
    out, stats = torch.ops.kgx.dot_attention_save(q, k, v, g.rowptr, g.rows, items, split, g.col, heads, channels,
                                                  scale, n_slots, None, 0.0, 0, ev, g.eid)
    assert torch.equal(out, plain["out"])
    buf = torch.full((e.shape[0], hc + 2 * pad), 5.0, device=dev)
    g_q, g_k, g_v = kops.dot_attention_edge_backward_into(
        buf[:, pad:pad + hc], x["gout"].to(dev), q, k, v, ev, out, stats, g.rowptr, g.rows, items, split, g.col,
        n_slots, t.rowptr, t.rows, t_items, t_split, t.col, t.eid, t_slots, heads, channels, scale, g.eid, t.eid)
    assert torch.equal(buf[:, pad:pad + hc], plain["d_e"])
    assert bool((buf[:, :pad] == 5.0).all()) and bool((buf[:, pad + hc:] == 5.0).all())
    assert torch.equal(g_q, plain["d_q"]) and torch.equal(g_k, plain["d_k"]) and torch.equal(g_v, plain["d_v"])


# 5. attention dropout on the split path
def test_attention_dropout_split(dev):
    (heads, channels), p, seed = DR.DROPOUT_SHAPE, DR.DROPOUT_P, DR.DROPOUT_SEED
    g = _graph(dev, "deep")
    src, dst, _, n_dst = DR.make_graph("deep")
    E = src.numel()
    mask = kops.dropout_mask(seed, p, torch.arange(E, dtype=torch.int32, device=dev), heads).cpu()
    assert abs(float((mask == 0).float().mean()) - p) < 0.02
    x, e = DR.make_inputs("deep", heads, channels), ER.make_edge("deep", heads, channels)
    ref = ER.dot_attention_edge_grads64(x["q"], x["k"], x["v"], e, src, dst, n_dst, heads, channels, x["gout"],
                                        mask=mask.double())
    got = _run(dev, g, x, e, heads, channels, False, dropout=p, seed=seed)
    _check(f"deep {heads}x{channels} dropout split", got, ref)
    _check_empty_rows("deep dropout", got, g)
    plain = ER.reference("deep", heads, channels)
    assert DR.ratio(got["out"], plain["out"], plain["out"]) > 100  # the mask was applied


# 6. no atomics anywhere: the same bits every run
@pytest.mark.parametrize("exact", [False, True], ids=["split", "exact"])
def test_bit_identical_run_to_run(dev, exact):
    g = _graph(dev, "deep")
    x, e = DR.make_inputs("deep", 8, 16), ER.make_edge("deep", 8, 16)
    a = _run(dev, g, x, e, 8, 16, exact, dropout=0.25, seed=7)
    b = _run(dev, g, x, e, 8, 16, exact, dropout=0.25, seed=7)
    for k in KEYS:
        assert torch.equal(a[k], b[k]), f"{k} differs between two runs"


# 7. a KGX_CSR_SELF_LOOPS graph: the added slots (edge id E + i) have no edge row
@pytest.mark.parametrize("exact", [False, True], ids=["split", "exact"])
def test_self_loop_slots_carry_no_feature(dev, exact):
    heads, channels, n = 4, 8, 40
    hc = heads * channels
    gen = torch.Generator().manual_seed(4242)
    src = torch.cat([torch.randint(0, n, (300,), generator=gen), torch.randint(0, n, (100,), generator=gen)])
    dst = torch.cat([torch.randint(0, n, (300,), generator=gen), torch.full((100,), 3)])
    E = src.numel()
    g = _build(dev, src, dst, n, n, self_loops=True)
    assert g.flags & nat.CSR_SELF_LOOPS and g.kept == E + n and g.n_input_edges == E and g.n_split > 0
    assert int((g.eid >= E).sum()) == n
    x = {name: torch.randn(n, hc, generator=gen) for name in ("q", "k", "v", "gout")}
    e = torch.randn(E, hc, generator=gen)
    loops = torch.arange(n)
    ref = ER.dot_attention_edge_grads64(x["q"], x["k"], x["v"], torch.cat([e, torch.zeros(n, hc)]),
                                        torch.cat([src, loops]), torch.cat([dst, loops]), n, heads, channels,
                                        x["gout"])
    ref = {k: (v[:E] if k in ("d_e", "A_e") else v) for k, v in ref.items()}
    got = _run(dev, g, x, e, heads, channels, exact)
    assert got["d_e"].shape == (E, hc)
    _check(f"self loops {'exact' if exact else 'split'}", got, ref)
    # exactly the E rows of the table are written: the n rows after them keep what they held
    t = G.transpose(g)
    items, _, split, _, n_slots = g.work(exact)
    t_items, _, t_split, _, t_slots = t.work(exact)
    q, k, v, ed = (a.to(dev) for a in (x["q"], x["k"], x["v"], e))
    scale = channels ** -0.5
    out, stats = torch.ops.kgx.dot_attention_save(q, k, v, g.rowptr, g.rows, items, split, g.col, heads, channels,
                                                  scale, n_slots, None, 0.0, 0, ed, g.eid)
    buf = torch.full((E + n, hc), 5.0, device=dev)
    kops.dot_attention_edge_backward_into(
        buf[:E], x["gout"].to(dev), q, k, v, ed, out, stats, g.rowptr, g.rows, items, split, g.col, n_slots,
        t.rowptr, t.rows, t_items, t_split, t.col, t.eid, t_slots, heads, channels, scale, g.eid, t.eid)
    assert torch.equal(buf[:E], got["d_e"]) and bool((buf[E:] == 5.0).all())


# 8. one NaN in an edge row poisons its (row, head) block only
@pytest.mark.parametrize("exact", [False, True], ids=["split", "exact"])
def test_nan_in_one_edge_row(dev, exact):
    heads, channels, h0 = 3, 12, 1  # padding sub-lane and padding head
    g = _graph(dev, "small")
    src, dst, _, n_dst = DR.make_graph("small")
    x = DR.make_inputs("small", heads, channels)
    e = ER.make_edge("small", heads, channels).clone()
    t0 = int(torch.nonzero(dst == DR.HUB_DST).flatten()[17])  # an edge of the split hub row
    e[t0, h0 * channels + 5] = float("nan")
    with torch.no_grad():
        out = kops.dot_attention(g, x["q"].to(dev), x["k"].to(dev), x["v"].to(dev), heads, channels, exact=exact,
                                 edge=e.to(dev)).cpu()
    blk = torch.zeros(n_dst, heads * channels, dtype=torch.bool)
    blk[DR.HUB_DST, h0 * channels:(h0 + 1) * channels] = True
    assert bool(torch.isnan(out[blk]).all()), "the block of the NaN edge row must be NaN"
    assert bool(torch.isfinite(out[~blk]).all()), "NaN outside the (row, head) block of the NaN edge row"
    ref = ER.reference("small", heads, channels)["out"]
    assert DR.ratio(out[~blk], ref[~blk], ref[~blk]) <= 1.0


# 9. cross-check that does not go through the new kernel path: the op WITHOUT
#    edge features on the expanded graph, k' and v' materialised
@pytest.mark.parametrize("heads,channels", [(8, 16), (3, 12)], ids=["8x16", "3x12"])
def test_no_edge_op_on_the_expanded_graph(dev, heads, channels):
    src, dst, n_src, n_dst = DR.make_graph("small")
    x, e = DR.make_inputs("small", heads, channels), ER.make_edge("small", heads, channels)
    E = src.numel()
    g2 = _build(dev, torch.arange(E), dst, E, n_dst)
    q = x["q"].to(dev).requires_grad_(True)
    k, v, ed = (a.to(dev).requires_grad_(True) for a in (x["k"], x["v"], e))
    sl = src.to(dev)
    out = kops.dot_attention(g2, q, k[sl] + ed, v[sl] + ed, heads, channels)
    out.backward(x["gout"].to(dev))
    got = {"out": out.detach(), "d_q": q.grad, "d_k": k.grad, "d_v": v.grad, "d_e": ed.grad}
    _WORST_BEFORE = dict(_WORST)
    _check(f"small {heads}x{channels} expanded, no-edge op", got, ER.reference("small", heads, channels))
    _WORST.clear()
    _WORST.update(_WORST_BEFORE)  # the docstring's table is of the edge kernels


# python-level argument errors
def test_python_argument_errors(dev):
    g = _graph(dev, "small")
    x = DR.make_inputs("small", 8, 16)
    q, k, v = (x[n].to(dev) for n in ("q", "k", "v"))
    e = ER.make_edge("small", 8, 16).to(dev)
    with pytest.raises(ValueError, match="edge"):
        kops.dot_attention(g, q, k, v, 8, 16, edge=e[:-1])
    with pytest.raises(ValueError, match="edge"):
        kops.dot_attention(g, q, k, v, 8, 16, edge=e[:, :64])
    with pytest.raises(ValueError, match="edge_order"):
        kops.dot_attention(g, q, k, v, 8, 16, edge=e, edge_order="coo")


# 10. argument errors of the C entry points: no launch, no device memory touched
def test_argument_errors():
    lib = nat.lib()
    P = ctypes.c_void_p

    def fwd(heads=8, channels=16, ld=128, ld_e=128, n_e=1, e=16, ptr=16):
        return lib.kgx_dot_attention_edge(P(ptr), P(ptr), 1, None, 0, None, 0, P(ptr), P(ptr), ld, P(ptr), ld,
                                          P(ptr), ld, P(e) if e else None, ld_e, n_e, None, heads, channels, 0.25,
                                          P(ptr), max(ld, heads * channels), None, None, None, 0.0, 0, None)

    assert fwd(ld_e=127) == nat.KGX_ERR_ARG and b"leading dimension" in lib.kgx_last_error()
    assert fwd(ld_e=2**31) == nat.KGX_ERR_ARG and b"2^31" in lib.kgx_last_error()
    assert fwd(n_e=-1) == nat.KGX_ERR_ARG and b"edge table" in lib.kgx_last_error()
    assert fwd(ld=127) == nat.KGX_ERR_ARG and b"leading dimension" in lib.kgx_last_error()
    assert fwd(heads=0) == nat.KGX_ERR_ARG
    # unsupported exactly where the op without edge features is
    assert fwd(heads=16, channels=128, ld=2048, ld_e=2048) == nat.KGX_ERR_UNSUPPORTED
    assert b"64 lanes" in lib.kgx_last_error()
    assert fwd(heads=16, channels=64, ld=1024, ld_e=1024, ptr=4, e=4) == nat.KGX_ERR_UNSUPPORTED
    # the edge table joins the alignment inputs: 16 x 64 needs float4 lanes, which a 4-byte aligned e rules out
    assert fwd(heads=16, channels=64, ld=1024, ld_e=1024, e=4) == nat.KGX_ERR_UNSUPPORTED

    def bwd(heads=8, channels=16, ld=128, ld_e=128, ld_ge=128, n_e=1, e=16, grad_e=16, t_e_idx=16, ptr=16):
        return lib.kgx_dot_attention_edge_backward(
            P(ptr), P(ptr), 1, None, 0, None, 0, P(ptr), P(ptr), ld, P(ptr), ld, P(ptr), ld,
            P(e) if e else None, ld_e, n_e, None, heads, channels, 0.25,
            P(ptr), ld, P(ptr), P(ptr), ld, P(ptr), P(ptr), 1, None, 0, None, 0, P(ptr), P(ptr),
            P(t_e_idx) if t_e_idx else None, P(ptr), ld, P(ptr), ld, P(ptr), ld,
            P(grad_e) if grad_e else None, ld_ge, P(ptr), None, None, 0.0, 0, None)

    assert bwd(grad_e=0) == nat.KGX_ERR_ARG and b"grad_e" in lib.kgx_last_error()
    assert bwd(t_e_idx=0) == nat.KGX_ERR_ARG and b"t_e_idx" in lib.kgx_last_error()
    assert bwd(ld_e=100) == nat.KGX_ERR_ARG and b"leading dimension" in lib.kgx_last_error()
    assert bwd(ld_ge=100) == nat.KGX_ERR_ARG and b"leading dimension" in lib.kgx_last_error()
    assert bwd(ld_ge=2**31) == nat.KGX_ERR_ARG and b"2^31" in lib.kgx_last_error()
    assert bwd(n_e=-1) == nat.KGX_ERR_ARG
    assert bwd(ld=100) == nat.KGX_ERR_ARG and b"leading dimension" in lib.kgx_last_error()
    assert bwd(heads=16, channels=128, ld=2048, ld_e=2048, ld_ge=2048) == nat.KGX_ERR_UNSUPPORTED
    assert bwd(heads=16, channels=64, ld=1024, ld_e=1024, ld_ge=1024, grad_e=4) == nat.KGX_ERR_UNSUPPORTED
