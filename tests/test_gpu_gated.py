"""kgx_gated / kgx_gated_backward at op level (kops.gated_aggregate) and ResGatedGraphConv against the
float64 restatements of tests/gated_ref.py, on the graphs of tests/gatv2_ref.py (`small` 60 -> 50 and `deep`
500 -> 400, bipartite, split_len 16, an empty destination, a source without out-edges; the transposed graph
splits at 256).

Bounds: |got - ref| <= 1e-5 max(1, A) for out and every gradient, A the sum of the magnitudes of the
element's per-edge contributions (gine_ref.ratio).  The layer is held to 1e-5 max(1, |ref|) with the
cotangent N(0, 1/16), as the GATConv test.

Largest err / bound printed on an MI355X (all cases of this module):
  out 0.056   d k 0.148   d q 0.091   d v 0.100   d edge 0.069   layer 0.096
(d k at F = 512 on `small`, split and exact alike; the layer's largest is d lin_value.kernel).
"""

from __future__ import annotations

import pytest
import torch

import gated_ref as DR
import gatv2_edge_ref as ER
import gatv2_ref as GR
from keras_geometric_amd import graph as G
from keras_geometric_amd import ops as kops

pytestmark = pytest.mark.gpu

WIDTHS = [4, 12, 64, 100, 256, 260, 512]  # 260: the first width of two pieces per lane, the second nearly all padding
_GRAPHS: dict = {}
_WORST: dict = {}


def _graph(dev, name, coo=None):
    if name not in _GRAPHS:
        src, dst, n_src, n_dst = coo or GR.make_graph(name)
        _GRAPHS[name] = G.build_csr(src.to(torch.int32).to(dev), dst.to(torch.int32).to(dev), n_src, n_dst,
                                    split_len=GR.SPLIT_LEN)
        assert _GRAPHS[name].n_split > 0 and G.transpose(_GRAPHS[name]).n_split > 0  # both directions chunked
    return _GRAPHS[name]


def _run(dev, g, x, exact, with_edge, **kw):
    """Forward + backward of the op on the device: {out, d_k, d_q, d_v, d_e}."""
    t = {n: x[n].to(dev).requires_grad_(True) for n in ("k", "q", "v", "root", "bias")}
    e = x["e"].to(dev).requires_grad_(True) if with_edge else None
    out = kops.gated_aggregate(g, t["k"], t["q"], t["v"], edge=e, root=t["root"], bias=t["bias"], exact=exact, **kw)
    gout = x["gout"].to(dev)
    out.backward(gout)
    assert torch.equal(t["bias"].grad, gout.sum(0)) and torch.equal(t["root"].grad, gout)
    return {"out": out.detach(), "d_k": t["k"].grad, "d_q": t["q"].grad, "d_v": t["v"].grad,
            "d_e": e.grad if with_edge else None}


def _check(label, got, ref, ratios=DR.ratios):
    r = ratios(got, ref)
    for k, v in r.items():
        key = k if ratios is DR.ratios else "layer"
        _WORST[key] = max(_WORST.get(key, 0.0), v)
    msg = f"{label}: err / bound " + ", ".join(f"{k} {v:.3f}" for k, v in r.items())
    print(msg + " | worst so far " + ", ".join(f"{k} {v:.3f}" for k, v in _WORST.items()))
    assert all(v <= 1.0 for v in r.values()), msg


# 1. every lane layout, both modes, without and with an edge table in input order
@pytest.mark.parametrize("with_edge", [False, True], ids=["plain", "edge"])
@pytest.mark.parametrize("exact", [False, True], ids=["split", "exact"])
@pytest.mark.parametrize("F", WIDTHS)
def test_lane_layouts(dev, F, exact, with_edge):
    g, x = _graph(dev, "small"), DR.inputs("small", F)
    got = _run(dev, g, x, exact, with_edge)
    _check(f"small F={F} exact={exact} edge={with_edge}", got, DR.reference("small", F, with_edge))
    assert torch.equal(got["out"][0].cpu(), x["root"][0] + x["bias"])  # destination 0 has no in-edge
    assert not bool(got["d_k"][0].any())
    assert not bool(got["d_q"][g.n_src - 1].any()) and not bool(got["d_v"][g.n_src - 1].any())


# 2. split depth (63 forward chunks, 10 transposed ones), run to run, short rows equal between modes
@pytest.mark.parametrize("F", [16, 128])
def test_split_depth_and_run_to_run(dev, F):
    g = _graph(dev, "deep")
    sp, tsp = g.split.cpu(), G.transpose(g).split.cpu()
    assert sp[sp[:, 0] == GR.HUB_DST, 2].tolist() == [63] and tsp[tsp[:, 0] == GR.HUB_SRC, 2].tolist() == [10]
    x, got = DR.inputs("deep", F), {}
    for exact in (False, True):
        got[exact] = _run(dev, g, x, exact, True)
        _check(f"deep F={F} exact={exact}", got[exact], DR.reference("deep", F, True))
        again = _run(dev, g, x, exact, True)
        assert all(torch.equal(got[exact][k], again[k]) for k in again), "not the same bits from run to run"
    short = g.deg.long() < GR.SPLIT_LEN
    assert 1 < int(short.sum()) < g.n_dst
    for k in ("out", "d_k"):
        assert torch.equal(got[False][k][short], got[True][k][short]), k


# 3. the gate at z = +-200: exactly 1 and exactly 0, nothing but finite values
@pytest.mark.parametrize("exact", [False, True], ids=["split", "exact"])
def test_saturated_gate(dev, exact):
    F, g = 16, _graph(dev, "deep")
    src, dst, n_src, n_dst = GR.make_graph("deep")
    hub = dst == GR.HUB_DST
    x = dict(DR.inputs("deep", F))
    x["k"] = x["k"].clone()
    x["k"][GR.HUB_DST] = 200.0
    got = _run(dev, g, x, exact, True)
    assert all(bool(torch.isfinite(t).all()) for t in got.values())
    v = x["v"].double()[src[hub]]
    want, A = v.sum(0) + x["root"][GR.HUB_DST].double() + x["bias"].double(), v.abs().sum(0)
    assert DR.ratio(got["out"][GR.HUB_DST], want, A) <= 1.0
    x["k"][GR.HUB_DST] = -200.0
    got = _run(dev, g, x, exact, True)
    assert all(bool(torch.isfinite(t).all()) for t in got.values())
    assert torch.equal(got["out"][GR.HUB_DST].cpu(), x["root"][GR.HUB_DST] + x["bias"])
    assert not bool(got["d_k"][GR.HUB_DST].any())
    # the closed row adds exact zeros to d q and d v: the bits of the graph without its in-edges
    y = dict(x, e=x["e"][~hub])
    rest = _run(dev, _graph(dev, "deep_closed", (src[~hub], dst[~hub], n_src, n_dst)), y, exact, True)
    assert torch.equal(got["d_q"], rest["d_q"]) and torch.equal(got["d_v"], rest["d_v"])


# 4. the layer's layout: k, q, v, root as column views of one table
@pytest.mark.parametrize("F", [12, 64])
def test_strided_inputs(dev, F):
    src, dst, n_src, n_dst = GR.make_graph("small")
    g = _graph(dev, "small_square", (src, dst % n_src, n_src, n_src))  # square, so that one table serves both sides
    table = torch.randn(n_src, 4 * F, generator=torch.Generator().manual_seed(F)).to(dev)
    outs = []
    for cols in (lambda t: t, lambda t: t.contiguous()):
        t = table.clone().requires_grad_(True)
        out = kops.gated_aggregate(g, cols(t[:, :F]), cols(t[:, F:2 * F]), cols(t[:, 2 * F:3 * F]),
                                   root=cols(t[:, 3 * F:]))
        out.backward(torch.ones_like(out))
        outs.append((out.detach(), t.grad))
    for (a, b), what in zip(zip(*outs), ("out", "d table")):
        assert GR.ratio(a, b, b) <= 1.0, what


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
    x = DR.inputs("small", F)
    got = _run(dev, g, x, False, True)
    assert not bool(got["d_e"][bad].any()), "a dropped edge's grad_e row is not 0"
    got["d_e"] = got["d_e"][keep]
    _check("small dropped edges", got, DR.gated64(x["k"], x["q"], x["v"], x["e"][keep], x["root"], x["bias"],
                                                   src[keep], dst[keep], n_dst, x["gout"]))


# 6. the layer
@pytest.mark.parametrize("root_weight", [True, False], ids=["root", "noroot"])
@pytest.mark.parametrize("edge_dim", [None, DR.LAYER_D], ids=["plain", "edge_dim"])
def test_layer_against_float64(dev, edge_dim, root_weight):
    _check(f"layer edge_dim={edge_dim} root_weight={root_weight}", DR.run_layer(dev, edge_dim, root_weight),
           DR.layer_ref(edge_dim, root_weight), ratios=ER.layer_ratios)
