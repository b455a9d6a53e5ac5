"""float64 restatement of the softmax aggregation (kgx_softmax_aggr / kgx_softmax_aggr_backward,
ops.softmax_aggregate),

    m_e = msg(x[j] + e_ij)      out[i] = sum_{j->i} softmax_{j->i}(temp * m_e) * m_e      (per channel),

from plain index arithmetic and closed-form gradients, with A = the sum of the magnitudes of each element's
per-edge contributions (the scale of the project's bound |got - ref| <= 1e-5 max(1, A), gine_ref.ratio), its
seeded inputs on the graphs of tests/gatv2_ref.py, and the float64 autograd restatement of GENConv that
tests/test_softmax_aggr_host.py and tests/test_gpu_softmax_aggr.py share."""

import functools

import torch

import gatv2_edge_ref as ER
import gatv2_ref as GR
from gine_ref import ratio

FORMS = {"node": (True, False, False), "node_edge_gen": (True, True, True), "by_edge": (False, True, False)}
EPS = 1e-7
LAYER_D = 5


@functools.lru_cache(maxsize=None)
def inputs(name, F):
    """Seeded fp32 inputs on make_graph(name): x [n_src, F], e [E, F], gout [n_dst, F] ~ N(0, 1); temp [F] ~ U[0.25, 2]."""
    src, _, n_src, n_dst = GR.make_graph(name)
    g = torch.Generator().manual_seed(41000 + 10 * F + (7 if name == "deep" else 0))
    rnd = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    return {"x": rnd(n_src, F), "e": rnd(src.numel(), F), "gout": rnd(n_dst, F),
            "temp": 0.25 + 1.75 * torch.rand(F, generator=g)}


def softmax64(x, e, temp, src, dst, n_dst, gout, gen=False, eps=EPS):
    """{out, d_x, d_e, d_t} and A_* of each; x or e may be None (not both), temp [F] or a scalar tensor."""
    f64 = torch.float64
    r = 0 if x is None else x.to(f64)[src]
    r = r if e is None else r + e.to(f64)
    m = r.clamp_min(0) + eps if gen else r
    temp, g = temp.to(f64), gout.to(f64)[dst]
    add = lambda idx, t, n: torch.zeros(n, t.shape[1], dtype=f64).index_add_(0, idx, t)  # noqa: E731
    s = temp * m
    mx = torch.full((n_dst, m.shape[1]), -float("inf"), dtype=f64).scatter_reduce(
        0, dst[:, None].expand(-1, m.shape[1]), s, "amax")
    w = torch.exp(s - mx[dst])
    p = w / add(dst, w, n_dst)[dst]
    out = add(dst, p * m, n_dst)
    dr = g * p * (1 + temp * (m - out[dst]))
    if gen:
        dr = dr * (r > 0)
    dt = g * p * m * (m - out[dst])
    ref = {"out": out, "A_out": add(dst, (p * m).abs(), n_dst), "d_e": dr, "A_e": dr.abs(),
           "d_t": dt.sum(0), "A_t": dt.abs().sum(0), "p": p}
    if x is not None:
        ref.update(d_x=add(src, dr, x.shape[0]), A_x=add(src, dr.abs(), x.shape[0]))
    return ref


def ratios(got, ref):
    """err / bound of out and of every gradient `got` has."""
    r = {"out": ratio(got["out"], ref["out"], ref["A_out"])}
    r.update({k: ratio(got[k], ref[k], ref["A_" + k[2:]]) for k in ("d_x", "d_e", "d_t") if got.get(k) is not None})
    return r


@functools.lru_cache(maxsize=None)
def reference(name, F, form):
    """softmax64 of inputs(name, F) on make_graph(name) in one of FORMS, computed once and shared (read-only)."""
    src, dst, _, n_dst = GR.make_graph(name)
    v, (has_x, has_e, gen) = inputs(name, F), FORMS[form]
    return softmax64(v["x"] if has_x else None, v["e"] if has_e else None, v["temp"], src, dst, n_dst, v["gout"], gen)


def run_op(kops, g, v, form, dev="cpu", **kw):
    """Forward + backward of ops.softmax_aggregate on `dev` in one of FORMS: {out, d_x, d_e, d_t}; kw may
    replace the inputs x, e, temp (tensors) and pass exact / fused."""
    has_x, has_e, gen = FORMS[form]
    t = {n: kw.pop(n, v[n]).detach().clone().to(dev).requires_grad_(True) for n in ("x", "e", "temp")}
    out = kops.softmax_aggregate(g, t["x"] if has_x else None, t["temp"], edge=t["e"] if has_e else None,
                                 message="gen" if gen else "identity", eps=EPS, **kw)
    out.backward(v["gout"].to(dev))
    return {"out": out.detach(), "d_x": t["x"].grad, "d_e": t["e"].grad, "d_t": t["temp"].grad}


# ---------------------------------------------------------------------------
# GENConv(norm=None, learn_t=True, bias=True) on gatv2_edge_ref.layer_graph
# ---------------------------------------------------------------------------
def layer_dims(f_in, f_out, edge_dim):
    """{weight name: shape} in the layer's own naming (attribute path under the layer)."""
    d = {"t": ()}
    for n, fi in (("lin_src", f_in), ("lin_dst", f_in), ("lin_edge", edge_dim)):
        if fi is not None and fi != f_out:
            d.update({n + ".kernel": (fi, f_out), n + ".bias": (f_out,)})
    d.update({"mlp.0.kernel": (f_out, 2 * f_out), "mlp.0.bias": (2 * f_out,), "mlp.1.kernel": (2 * f_out, f_out),
              "mlp.1.bias": (f_out,)})
    return d


@functools.lru_cache(maxsize=None)
def layer_inputs(f_in, f_out, edge_dim):
    g = torch.Generator().manual_seed(9400 + f_in)
    ei = ER.layer_graph(ER.LAYER_N)
    W = {n: (ER.glorot(s, g) if len(s) == 2 else 0.5 * torch.randn(s, generator=g) + (1.0 if n == "t" else 0.0))
         for n, s in layer_dims(f_in, f_out, edge_dim).items()}
    return {"x": torch.randn(ER.LAYER_N, f_in, generator=g), "ei": ei,
            "edge_attr": torch.randn(ei.shape[1], edge_dim, generator=g) if edge_dim else None, "weights": W,
            "gout": ER.COT * torch.randn(ER.LAYER_N, f_out, generator=g)}


@functools.lru_cache(maxsize=None)
def layer_ref(f_in, f_out, edge_dim):
    """GENConv in float64 autograd, PyG's order of operations: {out, d_x, d_edge_attr, d_<weight>}."""
    u, f64 = layer_inputs(f_in, f_out, edge_dim), torch.float64
    leaf = lambda t: t.detach().to(f64).requires_grad_(True)  # noqa: E731
    W, x = {n: leaf(t) for n, t in u["weights"].items()}, leaf(u["x"])
    ea = leaf(u["edge_attr"]) if edge_dim else None
    lin = lambda n, v: v @ W[n + ".kernel"] + W[n + ".bias"] if n + ".kernel" in W else v  # noqa: E731
    src, dst = u["ei"][0], u["ei"][1]
    r = lin("lin_src", x)[src]
    if edge_dim:
        r = r + lin("lin_edge", ea)
    m = torch.relu(r) + EPS
    alpha = torch.stack([torch.softmax(W["t"] * m[dst == i], 0).mul(m[dst == i]).sum(0) for i in range(x.shape[0])])
    h = alpha + lin("lin_dst", x)
    out = lin("mlp.1", torch.relu(lin("mlp.0", h)))
    out.backward(u["gout"].to(f64))
    return {"out": out.detach(), "d_x": x.grad, "d_edge_attr": ea.grad if edge_dim else None,
            **{f"d_{n}": t.grad for n, t in W.items()}}


def run_layer(dev, f_in, f_out, edge_dim):
    """The layer on `dev` with layer_inputs' weights: the quantities of layer_ref."""
    import keras_geometric_amd as kgx

    u = layer_inputs(f_in, f_out, edge_dim)
    layer = kgx.GENConv(f_in, f_out, learn_t=True, norm=None, bias=True, edge_dim=edge_dim)
    assert kgx.GENConv.from_config(layer.get_config()).get_config() == layer.get_config()
    layer._build_device = dev
    layer.build([(None, f_in)])
    params = dict(layer.named_parameters())
    assert set(params) == set(u["weights"]), sorted(params)
    with torch.no_grad():
        for n, p in params.items():
            p.copy_(u["weights"][n])
    x = u["x"].clone().to(dev).requires_grad_(True)
    ea = u["edge_attr"].clone().to(dev).requires_grad_(True) if edge_dim else None
    out = layer([x, u["ei"].to(dev)], edge_attr=ea)
    out.backward(u["gout"].to(dev))
    return {"out": out.detach(), "d_x": x.grad, "d_edge_attr": ea.grad if edge_dim else None,
            **{f"d_{n}": p.grad for n, p in params.items()}}
