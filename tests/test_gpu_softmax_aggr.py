"""kgx_softmax_aggr / kgx_softmax_aggr_backward at op level (kops.softmax_aggregate) and GENConv against the
float64 restatements of tests/softmax_aggr_ref.py, on the graphs of tests/gatv2_ref.py (`small` 60 -> 50 and
`deep` 500 -> 400, bipartite, split_len 16, an empty destination, a source without out-edges; the transposed
graph splits at 256).

Bounds: |got - ref| <= 1e-5 max(1, A) for out and every gradient, A the sum of the magnitudes of the
element's per-edge contributions (gine_ref.ratio); for d temp over all edges.  The layer is held to
1e-5 max(1, |ref|) with the cotangent N(0, 1/16), as the GATConv test.

Largest err / bound printed on an MI355X (all cases of this module):
  out 0.034   d x 0.095   d edge 0.133   d temp 0.085   layer 0.102
(d edge at F = 512 on `small`, GEN message with an edge table, split mode; the layer's largest is d mlp.1.kernel).
"""

from __future__ import annotations

import pytest
import torch

import gatv2_edge_ref as ER
import gatv2_ref as GR
import softmax_aggr_ref as SR
from keras_geometric_amd import graph as G
from keras_geometric_amd import ops as kops

pytestmark = pytest.mark.gpu

WIDTHS = [4, 12, 64, 100, 256, 260, 512]  # 260: the first width of two pieces per lane, the second nearly all padding
MODES = pytest.mark.parametrize("exact", [False, True], ids=["split", "exact"])
_GRAPHS: dict = {}
_WORST: dict = {}


def _graph(dev, name, coo=None):
    if name not in _GRAPHS:
        src, dst, n_src, n_dst = coo or GR.make_graph(name)
        _GRAPHS[name] = G.build_csr(src.to(torch.int32).to(dev), dst.to(torch.int32).to(dev), n_src, n_dst,
                                    split_len=GR.SPLIT_LEN)
        assert _GRAPHS[name].n_split > 0 and G.transpose(_GRAPHS[name]).n_split > 0  # both directions chunked
    return _GRAPHS[name]


def _check(label, got, ref, ratios=SR.ratios):
    r = ratios(got, ref)
    for k, v in r.items():
        key = k if ratios is SR.ratios else "layer"
        _WORST[key] = max(_WORST.get(key, 0.0), v)
    msg = f"{label}: err / bound " + ", ".join(f"{k} {v:.3f}" for k, v in r.items())
    print(msg + " | worst so far " + ", ".join(f"{k} {v:.3f}" for k, v in _WORST.items()))
    assert all(v <= 1.0 for v in r.values()), msg


def _finite(got):
    return all(bool(torch.isfinite(t).all()) for t in got.values() if t is not None)


# 1. every lane layout, both modes, the three forms; a per-channel temp that needs its gradient
@pytest.mark.parametrize("form", SR.FORMS)
@MODES
@pytest.mark.parametrize("F", WIDTHS)
def test_lane_layouts(dev, F, exact, form):
    g = _graph(dev, "small")
    got = SR.run_op(kops, g, SR.inputs("small", F), form, dev, exact=exact)
    _check(f"small F={F} exact={exact} {form}", got, SR.reference("small", F, form))
    assert not bool(got["out"][0].any())  # destination 0 has no in-edge: exact zeros
    assert got["d_x"] is None or not bool(got["d_x"][g.n_src - 1].any())  # the source without out-edges


# 2. split depth (63 forward chunks, 10 transposed ones), run to run, short rows equal between modes
@pytest.mark.parametrize("F", [16, 128])
def test_split_depth_and_run_to_run(dev, F):
    g = _graph(dev, "deep")
    sp, tsp = g.split.cpu(), G.transpose(g).split.cpu()
    assert sp[sp[:, 0] == GR.HUB_DST, 2].tolist() == [63] and tsp[tsp[:, 0] == GR.HUB_SRC, 2].tolist() == [10]
    v, got = SR.inputs("deep", F), {}
    for exact in (False, True):
        got[exact] = SR.run_op(kops, g, v, "node_edge_gen", dev, exact=exact)
        _check(f"deep F={F} exact={exact}", got[exact], SR.reference("deep", F, "node_edge_gen"))
        again = SR.run_op(kops, g, v, "node_edge_gen", dev, exact=exact)
        assert all(torch.equal(got[exact][k], again[k]) for k in again), "not the same bits from run to run"
    short = g.deg.long() < GR.SPLIT_LEN
    assert 1 < int(short.sum()) < g.n_dst
    assert torch.equal(got[False]["out"][short], got[True]["out"][short])
    in_short = short.cpu()[GR.make_graph("deep")[1]]
    assert torch.equal(got[False]["d_e"][in_short], got[True]["d_e"][in_short])


# 3a. temp * m = 160, past expf's overflow: one source owns the hub row, every other slot weighs exactly 0
@MODES
def test_saturated_weight(dev, exact):
    F, g = 16, _graph(dev, "deep")
    src, dst, n_src, n_dst = GR.make_graph("deep")
    hub = dst == GR.HUB_DST
    J = int(src[hub][20])  # a source of the hub row's second chunk
    x = SR.inputs("deep", F)["x"].clone()
    x[J] = 80.0
    kw = dict(x=x, temp=torch.full((F,), 2.0), exact=exact)
    got = SR.run_op(kops, g, SR.inputs("deep", F), "node", dev, **kw)
    assert _finite(got)
    want = torch.full((F,), 80.0)
    assert SR.ratio(got["out"][GR.HUB_DST], want, want) <= 1.0
    # the other slots add exact zeros to d x: the bits of the graph without them
    keep = ~hub | (src == J)
    rest = SR.run_op(kops, _graph(dev, "deep_one_source", (src[keep], dst[keep], n_src, n_dst)),
                     SR.inputs("deep", F), "node", dev, **kw)
    assert torch.equal(got["d_x"], rest["d_x"]) and torch.equal(got["out"], rest["out"])


# 3b. the GEN message with every x + edge of the hub row negative: out = eps, no gradient through its slots
@MODES
def test_closed_gen_row(dev, exact):
    F, g = 16, _graph(dev, "deep")
    src, dst, n_src, n_dst = GR.make_graph("deep")
    hub = dst == GR.HUB_DST
    v = SR.inputs("deep", F)
    e = v["e"].clone()
    e[hub] = -(v["x"][src[hub]].abs() + 1.0)
    got = SR.run_op(kops, g, v, "node_edge_gen", dev, e=e, exact=exact)
    assert _finite(got)
    eps = torch.tensor(SR.EPS, dtype=torch.float32)
    assert bool(((got["out"][GR.HUB_DST].cpu() - eps).abs() <= eps * 2.0 ** -23).all())  # one ulp
    assert not bool(got["d_e"][hub.to(dev)].any())
    rest = SR.run_op(kops, _graph(dev, "deep_no_hub", (src[~hub], dst[~hub], n_src, n_dst)), v, "node_edge_gen", dev,
                     e=e[~hub], exact=exact)
    assert torch.equal(got["d_x"], rest["d_x"])


# 4. temp = 0 is the mean of the messages; temp = -1 leans to the smallest one
def test_zero_and_negative_temp(dev):
    F, g, v = 12, _graph(dev, "small"), SR.inputs("small", 12)
    src, dst, _, n_dst = GR.make_graph("small")
    out = {}
    for t in (0.0, -1.0):
        temp = torch.full((F,), t)
        got = SR.run_op(kops, g, v, "node", dev, temp=temp)
        _check(f"small temp={t}", got, SR.softmax64(v["x"], None, temp, src, dst, n_dst, v["gout"]))
        out[t] = got["out"].cpu().double()
    m = v["x"].double()[src]
    cnt = torch.bincount(dst, minlength=n_dst).clamp_min(1)[:, None]
    mean = torch.zeros(n_dst, F, dtype=torch.float64).index_add_(0, dst, m) / cnt
    assert SR.ratio(out[0.0], mean, torch.zeros(n_dst, F, dtype=torch.float64).index_add_(0, dst, m.abs()) / cnt) <= 1.0
    assert bool((out[-1.0] <= mean + 1e-5).all()) and bool((out[-1.0] < mean - 0.1).any())


# 5. input edges the graph dropped: zero rows of d edge
def test_dropped_edges(dev):
    F = 20
    src, dst, n_src, n_dst = GR.make_graph("small")
    bad = torch.tensor([3, 64, 700, src.numel() - 1])
    dst = dst.clone()
    dst[bad] = -1  # the build drops these input edges
    g = _graph(dev, "small_dropped", (src, dst, n_src, n_dst))
    keep = torch.ones(src.numel(), dtype=torch.bool)
    keep[bad] = False
    assert g.kept == int(keep.sum()) and g.n_input_edges == src.numel()
    v = SR.inputs("small", F)
    got = SR.run_op(kops, g, v, "node_edge_gen", dev)
    assert not bool(got["d_e"][bad].any()), "a dropped edge's grad_e row is not 0"
    got["d_e"] = got["d_e"][keep]
    _check("small dropped edges", got,
           SR.softmax64(v["x"], v["e"][keep], v["temp"], src[keep], dst[keep], n_dst, v["gout"], True))


# 6. the layer: widths equal and different, without and with edge_attr (projected and not)
@pytest.mark.parametrize("f_in,edge_dim", [(24, None), (24, SR.LAYER_D), (20, SR.LAYER_D), (20, 24)])
def test_layer_against_float64(dev, f_in, edge_dim):
    _check(f"layer f_in={f_in} edge_dim={edge_dim}", SR.run_layer(dev, f_in, 24, edge_dim),
           SR.layer_ref(f_in, 24, edge_dim), ratios=ER.layer_ratios)
