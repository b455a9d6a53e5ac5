"""kgx_gatv2_edge / kgx_gatv2_edge_backward at op level
(kops.gatv2_aggregate(edge=...) on given h_src, h_dst and projected edge rows e)
against the float64 restatement of tests/gatv2_edge_ref.py: every lane layout on
split and unsplit rows, split depth, the two edge orders, e and grad_e as column
slices of wider tensors, attention dropout on the split path, bit identity from
run to run, an all-zero table against the op without one, a self-loop graph
with and without loop rows, a graph that dropped input edges, and the argument
errors of the C entry points.

Graphs and lane layouts are those of tests/test_gpu_gatv2_op.py
(gatv2_ref.make_graph "small" and "deep", split_len=16 forward and 256
transposed; gatv2_ref.LAYOUTS); inputs are gatv2_ref.make_inputs, without the
bias (the empty destination's row is then an exact 0), plus a seeded e ~ N(0, 1)
of [E, H*C] in input-edge order (gatv2_edge_ref.make_edge).

The leaky-ReLU input is (h_dst[i] + h_src[j]) + e, two rounded fp32 adds of the
test's own inputs, which the fp32 restatement forms bit for bit as the kernels
do; tests/test_gatv2_edge_ref_host.py holds that on every fixture of this module
the float64 sum has the same sign, so no branch mask is needed.

Bounds, float64 reference throughout (the project's own):
  out                            |got - ref| <= 1e-5 * max(1, |ref|)
  d h_src, d h_dst, d att, d e   |got - ref| <= 1e-5 * max(1, A)
A is the sum of the magnitudes of the per-edge contributions to that element
(an edge row has one use: A_e = |d e|).

Largest err / bound (GPU: MI355X, all cases of this module; fp32 restatement:
tests/test_gatv2_edge_ref_host.py on the same inputs):

  quantity   GPU     fp32 restatement
  out        0.18    0.30
  d h_src    0.35    0.23
  d h_dst    0.40    0.26
  d att      0.04    0.03
  d e        0.38    0.48
No ratio is above 0.5.  The largest on the GPU, d h_dst 0.40, is 4 x 256 on
`small` in exact mode (8 x 128 measures 0.38; tests/test_gpu_gatv2_op.py has 0.41
there without edge features); the largest of the fp32 restatement, d e 0.48
at 8 x 128, is close to the 0.5 the host module holds it to: an element of d e
is one product of a score gradient that sums 128 or 256 channels, and its bound
is its own magnitude.  d att moves between runs with the order of its atomic
adds.
"""

from __future__ import annotations

import ctypes

import pytest
import torch

import gatv2_edge_ref as ER
import gatv2_ref as GR
from keras_geometric_amd import _native as nat
from keras_geometric_amd import graph as G
from keras_geometric_amd import ops as kops

pytestmark = pytest.mark.gpu

_GRAPHS: dict = {}
_WORST: dict = {}
KEYS = ER.KEYS
BIT_KEYS = ("out", "d_src", "d_dst", "d_e")  # d att is summed with atomics


def _build(dev, src, dst, n_src, n_dst, **kw):
    return G.build_csr(src.to(torch.int32).to(dev), dst.to(torch.int32).to(dev), n_src, n_dst,
                       split_len=GR.SPLIT_LEN, **kw)


def _graph(dev, name):
    g = _GRAPHS.get(name)
    if g is None:
        g = _GRAPHS[name] = _build(dev, *GR.make_graph(name))
        t = G.transpose(g)
        assert g.split_len == GR.SPLIT_LEN and g.n_split > 0 and t.n_split > 0 and t.split_len == 256
        assert g.kept == g.n_input_edges
    return g


def _run(dev, g, x, e, heads, channels, exact, order="input", dropout=0.0, seed=0, pad=0):
    """Forward + backward of the op on the device: {out, d_src, d_dst, d_att, d_e},
    d e in the order of `e`'s rows.  order="csr": the table is handed over permuted
    into CSR slot order and its gradient un-permuted.  pad > 0: e is the middle
    column block of a [n_e, pad + H C + pad] tensor."""
    hc = heads * channels
    hs, hd, att = (x[k].to(dev).requires_grad_(True) for k in ("h_src", "h_dst", "att"))
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
    out = kops.gatv2_aggregate(g, hs, hd, att, heads, channels, GR.SLOPE, bias=None, exact=exact, dropout=dropout,
                               seed=seed, edge=ev, edge_order=order)
    out.backward(x["gout"].to(dev))
    d_e = wide.grad
    if pad:
        assert not bool(d_e[:, :pad].any()) and not bool(d_e[:, pad + hc:].any()), "pad columns' gradient is not 0"
        d_e = d_e[:, pad:pad + hc]
    if order == "csr":
        back = torch.empty_like(d_e)
        back[g.eid.long()] = d_e
        d_e = back
    return {"out": out.detach(), "d_src": hs.grad, "d_dst": hd.grad, "d_att": att.grad.reshape(-1), "d_e": d_e}


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
    """Destination 0 has no in-edge, the last source no out-edge: exact zeros (no bias)."""
    assert not bool(got["out"][0].any()), f"{label}: out of the empty destination is not 0"
    assert not bool(got["d_dst"][0].any()), f"{label}: d h_dst of the empty destination is not 0"
    assert not bool(got["d_src"][g.n_src - 1].any()), f"{label}: d h_src of the source without edges is not 0"


# 1. every lane layout, split and unsplit, all five quantities
@pytest.mark.parametrize("exact", [False, True], ids=["split", "exact"])
@pytest.mark.parametrize("heads,channels", GR.SHAPES, ids=[f"{h}x{c}" for h, c in GR.SHAPES])
def test_lane_layouts(dev, heads, channels, exact):
    g = _graph(dev, "small")
    assert g.n_src != g.n_dst and int(g.deg[0]) == 0 and int(G.transpose(g).deg[g.n_src - 1]) == 0
    x, e = GR.make_inputs("small", heads, channels), ER.make_edge("small", heads, channels)
    got = _run(dev, g, x, e, heads, channels, exact)
    label = f"small {heads}x{channels} {'exact' if exact else 'split'}"
    _check(label, got, ER.reference("small", heads, channels))
    _check_empty_rows(label, got, g)


# 2. split depth: more chunks than either fix-up loads per step
@pytest.mark.parametrize("heads,channels", GR.DEEP_SHAPES, ids=[f"{h}x{c}" for h, c in GR.DEEP_SHAPES])
def test_split_depth(dev, heads, channels):
    g = _graph(dev, "deep")
    sp, tsp = g.split.cpu(), G.transpose(g).split.cpu()
    assert sp[sp[:, 0] == GR.HUB_DST, 2].tolist() == [63]  # {row, first slot, chunks, _}
    assert tsp[tsp[:, 0] == GR.HUB_SRC, 2].tolist() == [10]
    x, e = GR.make_inputs("deep", heads, channels), ER.make_edge("deep", heads, channels)
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
    x, e = GR.make_inputs("small", heads, channels), ER.make_edge("small", heads, channels)
    a = _run(dev, g, x, e, heads, channels, exact, order="input")
    b = _run(dev, g, x, e, heads, channels, exact, order="csr")
    for k in BIT_KEYS:
        assert torch.equal(a[k], b[k]), f"{k} differs between the edge orders"
    _check(f"small {heads}x{channels} csr {'exact' if exact else 'split'}", b, ER.reference("small", heads, channels))


# 4. e a column slice of a wider tensor; grad_e written into a strided view
@pytest.mark.parametrize("heads,channels", [(8, 16), (3, 6)], ids=["8x16", "3x6"])
def test_strided_edge_table_and_gradient(dev, heads, channels):
    g = _graph(dev, "small")
    hc, pad = heads * channels, 4
    assert GR.fwd_layout(heads, channels, ld=hc + 2 * pad) == GR.fwd_layout(heads, channels)  # same lanes: same bits
    assert GR.bwd_layout(heads, channels, ld=hc + 2 * pad) == GR.bwd_layout(heads, channels)
    x, e = GR.make_inputs("small", heads, channels), ER.make_edge("small", heads, channels)
    plain = _run(dev, g, x, e, heads, channels, False)
    got = _run(dev, g, x, e, heads, channels, False, pad=pad)
    _check(f"small {heads}x{channels} strided e", got, ER.reference("small", heads, channels))
    for k in BIT_KEYS:
        assert torch.equal(got[k], plain[k]), k
    # the raw backward with grad_e a column block of a wider buffer (ld_ge != H C)
    t = G.transpose(g)
    items, _, split, _, n_slots = g.work(False)
    t_items, _, t_split, _, t_slots = t.work(False)
    hs, hd, att = (x[n].to(dev) for n in ("h_src", "h_dst", "att"))
    wide = torch.cat([torch.zeros(e.shape[0], pad), e, torch.zeros(e.shape[0], pad)], dim=1).to(dev)
    ev = wide[:, pad:pad + hc]
    out, stats = torch.ops.kgx.gatv2_save(hs, hd, g.rowptr, g.rows, items, split, g.col, att.reshape(-1), heads,
                                          channels, GR.SLOPE, None, n_slots, None, 0.0, 0, ev, g.eid)
    assert torch.equal(out, plain["out"])
    buf = torch.full((e.shape[0], hc + 2 * pad), 5.0, device=dev)
    g_src, g_dst, g_att = kops.gatv2_edge_backward_into(
        buf[:, pad:pad + hc], x["gout"].to(dev), hs, hd, att, None, ev, out, stats, g.rowptr, g.rows, items, split,
        g.col, n_slots, t.rowptr, t.rows, t_items, t_split, t.col, t.extras["fwd_slot"].to(torch.int32), t_slots,
        heads, channels, GR.SLOPE, g.eid, t.eid)
    assert torch.equal(buf[:, pad:pad + hc], plain["d_e"])
    assert bool((buf[:, :pad] == 5.0).all()) and bool((buf[:, pad + hc:] == 5.0).all())
    assert torch.equal(g_src, plain["d_src"]) and torch.equal(g_dst, plain["d_dst"])
    assert GR.ratio(g_att, plain["d_att"], ER.reference("small", heads, channels)["A_att"]) <= 1.0


# 5. attention dropout on the split path
def test_attention_dropout_split(dev):
    (heads, channels), p, seed = GR.DROPOUT_SHAPE, GR.DROPOUT_P, GR.DROPOUT_SEED
    g = _graph(dev, "deep")
    src, dst, _, n_dst = GR.make_graph("deep")
    E = src.numel()
    mask = kops.dropout_mask(seed, p, torch.arange(E, dtype=torch.int32, device=dev), heads).cpu()
    assert abs(float((mask == 0).float().mean()) - p) < 0.02
    x, e = GR.make_inputs("deep", heads, channels), ER.make_edge("deep", heads, channels)
    ref = ER.gatv2_edge_grads64(x["h_src"], x["h_dst"], x["att"], None, e, src, dst, n_dst, heads, channels,
                                GR.SLOPE, x["gout"], mask=mask.double())
    got = _run(dev, g, x, e, heads, channels, False, dropout=p, seed=seed)
    _check(f"deep {heads}x{channels} dropout split", got, ref)
    _check_empty_rows("deep dropout", got, g)
    plain = ER.reference("deep", heads, channels)
    assert GR.ratio(got["out"], plain["out"], plain["out"]) > 100  # the mask was applied


# 6. one writer per element of out, d h_src, d h_dst and d e: the same bits every run
@pytest.mark.parametrize("exact", [False, True], ids=["split", "exact"])
def test_bit_identical_run_to_run(dev, exact):
    g = _graph(dev, "deep")
    x, e = GR.make_inputs("deep", 8, 16), ER.make_edge("deep", 8, 16)
    a = _run(dev, g, x, e, 8, 16, exact, dropout=0.25, seed=7)
    b = _run(dev, g, x, e, 8, 16, exact, dropout=0.25, seed=7)
    for k in BIT_KEYS:
        assert torch.equal(a[k], b[k]), f"{k} differs between two runs"
    ref = ER.reference("deep", 8, 16)
    assert GR.ratio(a["d_att"], b["d_att"], ref["A_att"]) <= 1.0  # atomically summed: tolerance only


# 7. an all-zero table: x + 0.0f is exact and the order of adds is fixed
@pytest.mark.parametrize("exact", [False, True], ids=["split", "exact"])
@pytest.mark.parametrize("heads,channels", GR.SHAPES, ids=[f"{h}x{c}" for h, c in GR.SHAPES])
def test_zero_table_is_the_op_without_edge(dev, heads, channels, exact):
    g = _graph(dev, "small")
    x = GR.make_inputs("small", heads, channels)
    hs, hd, att = (x[k].to(dev) for k in ("h_src", "h_dst", "att"))
    with torch.no_grad():
        want = kops.gatv2_aggregate(g, hs, hd, att, heads, channels, GR.SLOPE, exact=exact)
        for order, rows in (("input", g.n_input_edges), ("csr", g.kept)):
            zero = torch.zeros(rows, heads * channels, device=dev)
            got = kops.gatv2_aggregate(g, hs, hd, att, heads, channels, GR.SLOPE, exact=exact, edge=zero,
                                       edge_order=order)
            assert torch.equal(got, want), f"{order}: max |diff| {float((got - want).abs().max()):.3g}"


# 8. a KGX_CSR_SELF_LOOPS graph: with E rows the added slots (edge id E + i) have no edge row,
#    with E + n rows the loop rows are used and receive gradient
def _loop_case(dev):
    heads, channels, n = 4, 8, 40
    hc = heads * channels
    gen = torch.Generator().manual_seed(4242)
    src = torch.cat([torch.randint(0, n, (300,), generator=gen), torch.randint(0, n, (100,), generator=gen)])
    dst = torch.cat([torch.randint(0, n, (300,), generator=gen), torch.full((100,), 3)])
    E = src.numel()
    g = _build(dev, src, dst, n, n, self_loops=True)
    assert g.flags & nat.CSR_SELF_LOOPS and g.kept == E + n and g.n_input_edges == E and g.n_split > 0
    assert int((g.eid >= E).sum()) == n
    h = torch.randn(n, hc, generator=gen)
    x = {"h_src": h, "h_dst": torch.randn(n, hc, generator=gen), "att": 0.3 * torch.randn(heads, channels, generator=gen),
         "gout": torch.randn(n, hc, generator=gen)}
    e = torch.randn(E + n, hc, generator=gen)
    loops = torch.arange(n)
    return heads, channels, n, E, g, x, e, torch.cat([src, loops]), torch.cat([dst, loops])


@pytest.mark.parametrize("exact", [False, True], ids=["split", "exact"])
def test_self_loop_slots_without_rows_carry_no_feature(dev, exact):
    heads, channels, n, E, g, x, e, src, dst = _loop_case(dev)
    hc = heads * channels
    ref = ER.gatv2_edge_grads64(x["h_src"], x["h_dst"], x["att"], None, torch.cat([e[:E], torch.zeros(n, hc)]),
                                src, dst, n, heads, channels, GR.SLOPE, x["gout"])
    ref = {k: (v[:E] if k in ("d_e", "A_e") else v) for k, v in ref.items()}
    got = _run(dev, g, x, e[:E], heads, channels, exact)
    assert got["d_e"].shape == (E, hc)  # the loop slots' rows do not exist
    _check(f"self loops, E rows {'exact' if exact else 'split'}", got, ref)
    # exactly the E rows of the table are written: the n rows after them keep what they held
    t = G.transpose(g)
    items, _, split, _, n_slots = g.work(exact)
    t_items, _, t_split, _, t_slots = t.work(exact)
    hs, hd, att, ed = (a.to(dev) for a in (x["h_src"], x["h_dst"], x["att"], e[:E]))
    out, stats = torch.ops.kgx.gatv2_save(hs, hd, g.rowptr, g.rows, items, split, g.col, att.reshape(-1), heads,
                                          channels, GR.SLOPE, None, n_slots, None, 0.0, 0, ed, g.eid)
    buf = torch.full((E + n, hc), 5.0, device=dev)
    kops.gatv2_edge_backward_into(
        buf[:E], x["gout"].to(dev), hs, hd, att, None, ed, out, stats, g.rowptr, g.rows, items, split, g.col,
        n_slots, t.rowptr, t.rows, t_items, t_split, t.col, t.extras["fwd_slot"].to(torch.int32), t_slots, heads,
        channels, GR.SLOPE, g.eid, t.eid)
    assert torch.equal(buf[:E], got["d_e"]) and bool((buf[E:] == 5.0).all())


@pytest.mark.parametrize("exact", [False, True], ids=["split", "exact"])
def test_self_loop_rows_are_used_and_receive_gradient(dev, exact):
    heads, channels, n, E, g, x, e, src, dst = _loop_case(dev)
    ref = ER.gatv2_edge_grads64(x["h_src"], x["h_dst"], x["att"], None, e, src, dst, n, heads, channels, GR.SLOPE,
                                x["gout"])
    got = _run(dev, g, x, e, heads, channels, exact)
    assert got["d_e"].shape == (E + n, heads * channels)
    _check(f"self loops, E + n rows {'exact' if exact else 'split'}", got, ref)
    assert bool(got["d_e"][E:].any(dim=1).all()), "a loop row received no gradient"
    without = _run(dev, g, x, e[:E], heads, channels, exact)
    assert GR.ratio(got["out"], without["out"], ref["out"]) > 100  # the loop rows were used


# 9. a graph that dropped out-of-range input edges: their grad_e rows are exactly 0
@pytest.mark.parametrize("exact", [False, True], ids=["split", "exact"])
def test_dropped_input_edges_have_zero_gradient(dev, exact):
    heads, channels = 3, 12
    src, dst, n_src, n_dst = GR.make_graph("small")
    src, dst = src.clone(), dst.clone()
    bad = torch.tensor([5, 77, 400, 901, src.numel() - 1])
    dst[bad] = -1  # a negative destination: the build drops these input edges (segment_sum's out-of-range bucket)
    g = _build(dev, src, dst, n_src, n_dst)
    assert g.n_input_edges == src.numel() and g.kept == src.numel() - bad.numel()
    keep = torch.ones(src.numel(), dtype=torch.bool)
    keep[bad] = False
    x, e = GR.make_inputs("small", heads, channels), ER.make_edge("small", heads, channels)
    ref = ER.gatv2_edge_grads64(x["h_src"], x["h_dst"], x["att"], None, e[keep], src[keep], dst[keep], n_dst, heads,
                                channels, GR.SLOPE, x["gout"])
    got = _run(dev, g, x, e, heads, channels, exact)
    assert got["d_e"].shape == e.shape
    assert not bool(got["d_e"][bad].any()), "a dropped edge's grad_e row is not 0"
    _check(f"dropped edges {'exact' if exact else 'split'}", dict(got, d_e=got["d_e"][keep]), ref)


# python-level argument errors
def test_python_argument_errors(dev):
    g = _graph(dev, "small")
    x = GR.make_inputs("small", 8, 16)
    hs, hd, att = (x[n].to(dev) for n in ("h_src", "h_dst", "att"))
    e = ER.make_edge("small", 8, 16).to(dev)
    with pytest.raises(ValueError, match="edge"):
        kops.gatv2_aggregate(g, hs, hd, att, 8, 16, GR.SLOPE, edge=e[:-1])
    with pytest.raises(ValueError, match="edge"):
        kops.gatv2_aggregate(g, hs, hd, att, 8, 16, GR.SLOPE, edge=e[:, :64])
    with pytest.raises(ValueError, match="edge"):  # E + n rows need a graph with self-loop slots
        kops.gatv2_aggregate(g, hs, hd, att, 8, 16, GR.SLOPE, edge=torch.cat([e, e[:g.n_dst]]))
    with pytest.raises(ValueError, match="edge_order"):
        kops.gatv2_aggregate(g, hs, hd, att, 8, 16, GR.SLOPE, edge=e, edge_order="coo")


# 10. argument errors of the C entry points: no launch, no device memory touched
def test_argument_errors():
    lib = nat.lib()
    P = ctypes.c_void_p

    def fwd(heads=8, channels=16, ld=128, ld_e=128, n_e=1, e=16, ptr=16):
        return lib.kgx_gatv2_edge(P(ptr), P(ptr), 1, None, 0, None, 0, P(ptr), P(ptr), P(ptr), ld,
                                  P(e) if e else None, ld_e, n_e, None, P(ptr), heads, channels, 0.2,
                                  P(ptr), max(ld, heads * channels), None, None, None, None, 0.0, 0, None)

    assert fwd(ld_e=127) == nat.KGX_ERR_ARG and b"leading dimension" in lib.kgx_last_error()
    assert fwd(ld_e=2**31) == nat.KGX_ERR_ARG and b"2^31" in lib.kgx_last_error()
    assert fwd(n_e=-1) == nat.KGX_ERR_ARG and b"edge table" in lib.kgx_last_error()
    assert fwd(n_e=2**31) == nat.KGX_ERR_ARG and b"edge table" in lib.kgx_last_error()
    assert fwd(ld=127) == nat.KGX_ERR_ARG and b"leading dimension" in lib.kgx_last_error()
    assert fwd(heads=0) == nat.KGX_ERR_ARG
    # unsupported exactly where the op without edge features is
    assert fwd(heads=16, channels=128, ld=2048, ld_e=2048) == nat.KGX_ERR_UNSUPPORTED
    assert b"64 lanes" in lib.kgx_last_error()
    # the edge table joins the alignment inputs: 16 x 64 needs float4 lanes, which a 4-byte aligned e rules out
    assert fwd(heads=16, channels=64, ld=1024, ld_e=1024, e=4) == nat.KGX_ERR_UNSUPPORTED

    def bwd(heads=8, channels=16, ld=128, ld_e=128, ld_ge=128, n_e=1, e=16, grad_e=16, t_e_idx=16, ptr=16):
        return lib.kgx_gatv2_edge_backward(
            P(ptr), P(ptr), 1, None, 0, None, 0, P(ptr), P(ptr), P(ptr), ld,
            P(e) if e else None, ld_e, n_e, None, P(ptr), heads, channels, 0.2,
            P(ptr), ld, None, P(ptr), P(ptr), ld,
            P(ptr), P(ptr), 1, None, 0, None, 0, P(ptr), P(ptr), P(t_e_idx) if t_e_idx else None,
            P(ptr), P(ptr), ld, P(ptr), P(grad_e) if grad_e else None, ld_ge, P(ptr), P(ptr), None,
            None, 0.0, 0, None)

    assert bwd(grad_e=0) == nat.KGX_ERR_ARG and b"grad_e" in lib.kgx_last_error()
    assert bwd(t_e_idx=0) == nat.KGX_ERR_ARG and b"t_e_idx" in lib.kgx_last_error()
    assert bwd(ld_e=100) == nat.KGX_ERR_ARG and b"leading dimension" in lib.kgx_last_error()
    assert bwd(ld_ge=100) == nat.KGX_ERR_ARG and b"leading dimension" in lib.kgx_last_error()
    assert bwd(ld_e=2**31) == nat.KGX_ERR_ARG and b"2^31" in lib.kgx_last_error()
    assert bwd(ld_ge=2**31) == nat.KGX_ERR_ARG and b"2^31" in lib.kgx_last_error()
    assert bwd(n_e=-1) == nat.KGX_ERR_ARG and b"edge table" in lib.kgx_last_error()
    assert bwd(n_e=2**31) == nat.KGX_ERR_ARG and b"edge table" in lib.kgx_last_error()
    assert bwd(ld=100) == nat.KGX_ERR_ARG and b"leading dimension" in lib.kgx_last_error()
    assert bwd(heads=16, channels=128, ld=2048, ld_e=2048, ld_ge=2048) == nat.KGX_ERR_UNSUPPORTED
    # 4 x 256 fits 64 lanes only with float4 lanes (K = 16), which a 4-byte aligned grad_e rules out
    assert bwd(heads=4, channels=256, ld=1024, ld_e=1024, ld_ge=1024, grad_e=4) == nat.KGX_ERR_UNSUPPORTED
