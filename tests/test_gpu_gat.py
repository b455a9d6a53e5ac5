"""kgx_gat / kgx_gat_backward at op level (kops.gat_aggregate) and GATConv against
the float64 restatement of tests/gat_ref.py, on the graphs of tests/gatv2_ref.py
(`small` 60 -> 50 and `deep` 500 -> 400, bipartite, split_len 16, an empty
destination, a source without out-edges; the transposed graph splits at 256).

Bounds: |out - ref| <= 1e-5 max(1, |ref|); each gradient <= 1e-5 max(1, A), A
the sum of the magnitudes of the per-edge contributions.  The reference takes
the leaky-ReLU branch from the fp32 z of the kernel's two adds.  The layer is
held to 1e-5 max(1, |ref|) with the cotangent N(0, 1/16), as the GATv2Conv
edge test.

Largest err / bound printed on an MI355X (all cases of this module):
  out 0.038   d h_src 0.086   d a_src 0.046   d a_dst 0.226   d a_edge 0.122   layer 0.063
(d a_dst at 8 x 128 on `small`, split and exact alike; the layer's largest is d linear_transform.kernel).
"""

from __future__ import annotations

import pytest
import torch

import gat_ref as AR
import gatv2_edge_ref as ER
import gatv2_ref as GR
import keras_geometric_amd as kgx
from keras_geometric_amd import graph as G
from keras_geometric_amd import ops as kops

pytestmark = pytest.mark.gpu

SHAPES = [(8, 16), (8, 128), (3, 12), (16, 4), (2, 7), (1, 64), (5, 24)]
CUT = 137  # the edge table stops this many input edges early: those slots have no row
_GRAPHS: dict = {}
_REFS: dict = {}
_WORST: dict = {}


def _graph(dev, name, coo=None):
    if name not in _GRAPHS:
        src, dst, n_src, n_dst = coo or GR.make_graph(name)
        _GRAPHS[name] = G.build_csr(src.to(torch.int32).to(dev), dst.to(torch.int32).to(dev), n_src, n_dst,
                                    split_len=GR.SPLIT_LEN)
        assert _GRAPHS[name].n_split > 0 and G.transpose(_GRAPHS[name]).n_split > 0  # both directions chunked
    return _GRAPHS[name]


def _edge(x, with_edge):
    return x["a_edge"][: x["a_edge"].shape[0] - CUT] if with_edge else None


def _ref(name, heads, channels, with_edge, mask=None):
    key = (name, heads, channels, with_edge)
    if mask is not None or key not in _REFS:
        src, dst, _, n_dst = GR.make_graph(name)
        x = AR.inputs(name, heads, channels)
        r = AR.gat_grads64(x["h_src"], x["a_src"], x["a_dst"], _edge(x, with_edge), x["bias"], src, dst, n_dst,
                           heads, channels, GR.SLOPE, x["gout"], mask=mask)
        if mask is not None:
            return r
        _REFS[key] = r
    return _REFS[key]


def _run(dev, g, x, heads, channels, exact, with_edge, bias=True, **kw):
    """Forward + backward of the op on the device: {out, d_src, d_asrc, d_adst, d_edge}."""
    hs, a_s, a_d = (x[k].to(dev).requires_grad_(True) for k in ("h_src", "a_src", "a_dst"))
    b = x["bias"].to(dev).requires_grad_(True) if bias else None
    e = _edge(x, with_edge).to(dev).requires_grad_(True) if with_edge else None
    out = kops.gat_aggregate(g, hs, a_s, a_d, heads, channels, GR.SLOPE, bias=b, exact=exact, edge=e, **kw)
    out.backward(x["gout"].to(dev))
    if bias:
        assert torch.equal(b.grad, x["gout"].to(dev).sum(0)), "d bias is grad_out.sum(0)"
    return {"out": out.detach(), "d_src": hs.grad, "d_asrc": a_s.grad, "d_adst": a_d.grad,
            "d_edge": e.grad if with_edge else None}


def _check(label, got, ref, ratios=AR.ratios):
    r = ratios(got, ref)
    for k, v in r.items():
        _WORST[k] = max(_WORST.get(k, 0.0), v)
    msg = f"{label}: err / bound " + ", ".join(f"{k} {v:.3f}" for k, v in r.items())
    print(msg + " | worst so far " + ", ".join(f"{k} {v:.3f}" for k, v in _WORST.items()))
    assert all(v <= 1.0 for v in r.values()), msg


# 1 + 3. every lane layout, both modes, without and with a short edge table in input order
@pytest.mark.parametrize("with_edge", [False, True], ids=["plain", "edge"])
@pytest.mark.parametrize("exact", [False, True], ids=["split", "exact"])
@pytest.mark.parametrize("heads,channels", SHAPES, ids=[f"{h}x{c}" for h, c in SHAPES])
def test_lane_layouts(dev, heads, channels, exact, with_edge):
    g = _graph(dev, "small")
    x = AR.inputs("small", heads, channels)
    for bias in (True, False):
        got = _run(dev, g, x, heads, channels, exact, with_edge, bias=bias)
        if bias:
            _check(f"small {heads}x{channels} exact={exact} edge={with_edge}", got,
                   _ref("small", heads, channels, with_edge))
        want = x["bias"].to(dev) if bias else torch.zeros(heads * channels, device=dev)
        assert torch.equal(got["out"][0], want)  # destination 0 has no in-edge
        assert not bool(got["d_adst"][0].any())
        assert not bool(got["d_src"][g.n_src - 1].any()) and not bool(got["d_asrc"][g.n_src - 1].any())
    if with_edge:  # a slot without a row scores with 0: the same bits as the table with zero rows appended
        full = torch.cat([_edge(x, True), torch.zeros(CUT, heads)]).to(dev)
        with torch.no_grad():
            a = kops.gat_aggregate(g, x["h_src"].to(dev), x["a_src"].to(dev), x["a_dst"].to(dev), heads, channels,
                                   GR.SLOPE, exact=exact, edge=full)
        assert torch.equal(a, got["out"]) and got["d_edge"].shape == (full.shape[0] - CUT, heads)


# 2 + 7. split depth (63 forward chunks, 10 transposed ones), run to run, short rows equal between modes
@pytest.mark.parametrize("heads,channels", GR.DEEP_SHAPES, ids=[f"{h}x{c}" for h, c in GR.DEEP_SHAPES])
def test_split_depth_and_run_to_run(dev, heads, channels):
    g = _graph(dev, "deep")
    sp, tsp = g.split.cpu(), G.transpose(g).split.cpu()
    assert sp[sp[:, 0] == GR.HUB_DST, 2].tolist() == [63] and tsp[tsp[:, 0] == GR.HUB_SRC, 2].tolist() == [10]
    x = AR.inputs("deep", heads, channels)
    got = {}
    for exact in (False, True):
        got[exact] = _run(dev, g, x, heads, channels, exact, True)
        _check(f"deep {heads}x{channels} exact={exact}", got[exact], _ref("deep", heads, channels, True))
        again = _run(dev, g, x, heads, channels, exact, True)
        assert all(torch.equal(got[exact][k], again[k]) for k in again), "not the same bits from run to run"
    short = g.deg.long() < GR.SPLIT_LEN
    assert 1 < int(short.sum()) < g.n_dst
    for k in ("out", "d_adst"):
        assert torch.equal(got[False][k][short], got[True][k][short]), k


# 4. the layer's layout: h_src, a_src, a_dst as column views of one table
@pytest.mark.parametrize("heads,channels", [(8, 16), (3, 12)], ids=["8x16", "3x12"])
def test_strided_inputs(dev, heads, channels):
    src, dst, n_src, n_dst = GR.make_graph("small")
    sq = (src, dst % n_src, n_src, n_src)  # square, so that one table serves both sides
    g = _graph(dev, "small_square", sq)
    x = AR.inputs("small", heads, channels)
    hc, H = heads * channels, heads
    a_dst = torch.cat([x["a_dst"], x["a_dst"][: n_src - n_dst]])
    table = torch.cat([x["h_src"], x["a_src"], a_dst, torch.zeros(n_src, -(hc + 2 * H) % 4)], 1).to(dev)
    outs = []
    for cols in (lambda t: t, lambda t: t.contiguous()):
        t = table.clone().requires_grad_(True)
        out = kops.gat_aggregate(g, cols(t[:, :hc]), cols(t[:, hc:hc + H]), cols(t[:, hc + H:hc + 2 * H]), heads,
                                 channels, GR.SLOPE)
        out.backward(torch.ones_like(out))
        outs.append((out.detach(), t.grad))
    assert table.stride(0) != hc
    for (a, b), what in zip(zip(*outs), ("out", "d table")):
        assert GR.ratio(a, b, b) <= 1.0, what


# 5. the max: one source outweighs HUB_DST's row by e^200 wherever its edge sits
@pytest.mark.parametrize("exact", [False, True], ids=["split", "exact"])
@pytest.mark.parametrize("pos", list(GR.DOMINANT_POS))
def test_dominant_edge_is_the_row(dev, pos, exact):
    heads, channels = 8, 16
    g = _graph(dev, ("dominant", pos), GR.dominant_graph(GR.DOMINANT_POS[pos]))
    x = AR.inputs("deep", heads, channels)
    a_src = x["a_src"].clone()
    a_src[GR.DOMINANT_SRC] = 200.0
    with torch.no_grad():
        out = kops.gat_aggregate(g, x["h_src"].to(dev), a_src.to(dev), x["a_dst"].to(dev), heads, channels,
                                 GR.SLOPE, exact=exact)
    assert bool(torch.isfinite(out).all())
    assert torch.equal(out[GR.HUB_DST], x["h_src"][GR.DOMINANT_SRC].to(dev))


# 6. attention dropout on the split path
def test_attention_dropout_split(dev):
    (heads, channels), p, seed = GR.DROPOUT_SHAPE, GR.DROPOUT_P, GR.DROPOUT_SEED
    g = _graph(dev, "deep")
    E = GR.make_graph("deep")[0].numel()
    mask = kops.dropout_mask(seed, p, torch.arange(E, dtype=torch.int32, device=dev), heads).cpu()
    x = AR.inputs("deep", heads, channels)
    got = _run(dev, g, x, heads, channels, False, True, dropout=p, seed=seed)
    _check("deep dropout", got, _ref("deep", heads, channels, True, mask=mask.double()))
    plain = _ref("deep", heads, channels, True)
    assert GR.ratio(got["out"], plain["out"], plain["out"]) > 100  # the mask was applied


# 8. the layer
NAMES = ("att_src", "att_dst", "final_bias", "att_edge", "linear_transform.kernel", "lin_edge.kernel")


def _layer_ref(v, W, edge_dim):
    """GATConv in float64 on float64 copies of the weights (autograd), PyG's order of operations."""
    cfg, H, C, f64 = v["cfg"], ER.LAYER_H, ER.LAYER_C, torch.float64
    W = {k: t.to(f64).requires_grad_(True) for k, t in W.items()}
    x, ea = v["x_j"].to(f64).requires_grad_(True), v["edge_attr"].to(f64).requires_grad_(True)
    src, dst, n = v["ei"][0], v["ei"][1], v["x_j"].shape[0]
    attr = ea
    if cfg["self_loops"]:
        attr = torch.cat([ea, ER.loop_attr_ref(ea, dst, n, cfg["fill"])])
        src, dst = torch.cat([src, torch.arange(n)]), torch.cat([dst, torch.arange(n)])
    h = (x @ W["linear_transform.kernel"]).view(n, H, C)
    s = ((h * W["att_dst"]).sum(-1)[dst] + (h * W["att_src"]).sum(-1)[src])
    if edge_dim:
        s = s + ((attr @ W["lin_edge.kernel"]).view(-1, H, C) * W["att_edge"]).sum(-1)
    s = torch.nn.functional.leaky_relu(s, cfg["slope"])
    mx = torch.full((n, H), float("-inf"), dtype=f64).scatter_reduce(0, dst[:, None].expand(-1, H), s, "amax")
    ex = torch.exp(s - mx[dst].detach())
    alpha = ex / (torch.zeros((n, H), dtype=f64).index_add(0, dst, ex)[dst] + 1e-16)
    out = torch.zeros((n, H, C), dtype=f64).index_add(0, dst, alpha[..., None] * h[src])
    out = out.reshape(n, H * C) if cfg["concat"] else out.mean(1)
    out = out + W["final_bias"]
    out.backward(v["gout"].to(f64))
    return {"out": out.detach(), "d_x": x.grad, "d_edge_attr": ea.grad if edge_dim else None,
            **{f"d_{k}": t.grad for k, t in W.items()}}


@pytest.mark.parametrize("edge_dim", [None, ER.LAYER_D], ids=["plain", "edge_dim"])
@pytest.mark.parametrize("case", ["mean", "concat_false"])
def test_layer_against_float64(dev, case, edge_dim):
    v = ER.layer_inputs(case)
    H, C = ER.LAYER_H, ER.LAYER_C
    layer = kgx.GATConv(C, heads=H, concat=v["cfg"]["concat"], negative_slope=0.2, add_self_loops=True,
                        edge_dim=edge_dim, fill_value="mean")
    assert kgx.GATConv.from_config(layer.get_config()).get_config() == layer.get_config()
    layer._build_device = dev
    layer.build([(None, ER.LAYER_F)])
    gen = torch.Generator().manual_seed(4242)
    W = {"att_src": ER.glorot((1, H, C), gen), "att_dst": ER.glorot((1, H, C), gen),
         "att_edge": ER.glorot((1, H, C), gen), "final_bias": v["weights"]["final_bias"],
         "linear_transform.kernel": v["weights"]["linear_transform.kernel"],
         "lin_edge.kernel": v["weights"]["lin_edge.kernel"]}
    names = [n for n in NAMES if edge_dim or "edge" not in n]
    params = dict(zip(names, layer.weights))
    assert len(layer.weights) == len(names)
    assert all(tuple(params[n].shape) == tuple(W[n].shape) for n in names), [tuple(w.shape) for w in layer.weights]
    layer.set_weights([W[n].numpy() for n in names])
    x, ea = v["x_j"].to(dev).requires_grad_(True), v["edge_attr"].to(dev).requires_grad_(True)
    out = layer([x, v["ei"].to(dev)], edge_attr=ea if edge_dim else None)
    out.backward(v["gout"].to(dev))
    got = {"out": out.detach(), "d_x": x.grad, "d_edge_attr": ea.grad if edge_dim else None,
           **{f"d_{n}": params[n].grad for n in names}}
    _check(f"layer {case} edge_dim={edge_dim}", got, _layer_ref(v, {n: W[n] for n in names}, edge_dim),
           ratios=ER.layer_ratios)
