"""float64 restatement of the gated sum (kgx_gated / kgx_gated_backward, ops.gated_aggregate),

    out[i] = sum_{j->i} sigmoid((k[i] + q[j]) + e_ij) * v[j] + root[i] + bias,

from plain index_add, with A = the sum of the magnitudes of each element's per-edge contributions (the
scale of the project's bound |got - ref| <= 1e-5 max(1, A), gine_ref.ratio), its seeded N(0, 1) inputs on
the graphs of tests/gatv2_ref.py, and the float64 autograd restatement of ResGatedGraphConv that
tests/test_gated_host.py and tests/test_gpu_gated.py share."""

import functools

import torch

import gatv2_edge_ref as ER
import gatv2_ref as GR
from gine_ref import ratio

GRADS = {"d_k": "k", "d_q": "q", "d_v": "v", "d_e": "e"}
LAYER_IN, LAYER_OUT, LAYER_D = 20, 24, 5
LAYER_WEIGHTS = ("final_bias", "lin_key.kernel", "lin_key.bias", "lin_query.kernel", "lin_query.bias",
                 "lin_value.kernel", "lin_value.bias", "lin_skip.kernel", "lin_edge.kernel")


def cpu_csr(src, dst, n_src, n_dst):
    """The CSR a stable build gives, as a host CSRGraph (no schedule: the composed form needs none)."""
    from keras_geometric_amd import graph as G

    order = torch.sort(dst, stable=True).indices
    deg = torch.bincount(dst, minlength=n_dst).to(torch.int32)
    rowptr = torch.zeros(n_dst + 1, dtype=torch.int32)
    rowptr[1:] = torch.cumsum(deg, 0)
    return G.CSRGraph(n_src=n_src, n_dst=n_dst, n_input_edges=src.numel(), kept=src.numel(),
                      max_degree=int(deg.max()), flags=0, rowptr=rowptr, col=src[order].to(torch.int32),
                      eid=order.to(torch.int32), deg=deg)


@functools.lru_cache(maxsize=None)
def inputs(name, F):
    """Seeded N(0, 1) fp32 inputs on make_graph(name): k, root, gout [n_dst, F]; q, v [n_src, F]; e [E, F]; bias [F]."""
    src, _, n_src, n_dst = GR.make_graph(name)
    g = torch.Generator().manual_seed(31000 + 10 * F + (7 if name == "deep" else 0))
    rnd = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    return {"k": rnd(n_dst, F), "q": rnd(n_src, F), "v": rnd(n_src, F), "e": rnd(src.numel(), F),
            "root": rnd(n_dst, F), "bias": rnd(F), "gout": rnd(n_dst, F)}


def gated64(k, q, v, e, root, bias, src, dst, n_dst, gout):
    """{out, d_k, d_q, d_v, d_e} and A_* of each; e, root, bias may be None."""
    k, q, v, gout = k.double(), q.double(), v.double(), gout.double()
    z = k[dst] + q[src]
    if e is not None:
        z = z + e.double()
    s = torch.sigmoid(z)
    m, dz, dv = s * v[src], gout[dst] * v[src] * s * (1 - s), s * gout[dst]
    add = lambda idx, t, n: torch.zeros(n, t.shape[1], dtype=torch.float64).index_add_(0, idx, t)  # noqa: E731
    n_src = q.shape[0]
    r = {"out": add(dst, m, n_dst), "A_out": add(dst, m.abs(), n_dst),
         "d_k": add(dst, dz, n_dst), "A_k": add(dst, dz.abs(), n_dst),
         "d_q": add(src, dz, n_src), "A_q": add(src, dz.abs(), n_src),
         "d_v": add(src, dv, n_src), "A_v": add(src, dv.abs(), n_src), "d_e": dz, "A_e": dz.abs()}
    for t in (root, bias):
        if t is not None:
            r["out"] = r["out"] + t.double()
            r["A_out"] = r["A_out"] + t.double().abs()
    return r


def ratios(got, ref):
    """err / bound of out and of every gradient `got` has."""
    r = {"out": ratio(got["out"], ref["out"], ref["A_out"])}
    r.update({k: ratio(got[k], ref[k], ref["A_" + a]) for k, a in GRADS.items() if got.get(k) is not None})
    return r


@functools.lru_cache(maxsize=None)
def reference(name, F, with_edge):
    """gated64 of inputs(name, F) on make_graph(name), computed once and shared (read-only)."""
    src, dst, _, n_dst = GR.make_graph(name)
    x = inputs(name, F)
    return gated64(x["k"], x["q"], x["v"], x["e"] if with_edge else None, x["root"], x["bias"], src, dst, n_dst,
                   x["gout"])


@functools.lru_cache(maxsize=None)
def layer_inputs():
    """x [40, 20], edge_index and edge_attr [E, 5] of gatv2_edge_ref.layer_graph, every weight of
    ResGatedGraphConv(24, edge_dim=5) by name, and the cotangent N(0, 1/16)."""
    g = torch.Generator().manual_seed(9300)
    ei = ER.layer_graph(ER.LAYER_N)
    fi, fo, d = LAYER_IN, LAYER_OUT, LAYER_D
    W = {n: (ER.glorot((d if "edge" in n else fi, fo), g) if n.endswith("kernel") else 0.5 * torch.randn(fo, generator=g))
         for n in LAYER_WEIGHTS}
    return {"x": torch.randn(ER.LAYER_N, fi, generator=g), "ei": ei, "edge_attr": torch.randn(ei.shape[1], d, generator=g),
            "weights": W, "gout": ER.COT * torch.randn(ER.LAYER_N, fo, generator=g)}


def layer_names(edge_dim, root_weight):
    return [n for n in LAYER_WEIGHTS if (edge_dim or "edge" not in n) and (root_weight or "skip" not in n)]


def layer_ref(edge_dim, root_weight):
    """ResGatedGraphConv in float64 autograd, PyG's order of operations: {out, d_x, d_edge_attr, d_<weight>}."""
    u, f64 = layer_inputs(), torch.float64
    W = {n: u["weights"][n].detach().to(f64).requires_grad_(True) for n in layer_names(edge_dim, root_weight)}
    x, ea = (u[n].detach().to(f64).requires_grad_(True) for n in ("x", "edge_attr"))
    src, dst = u["ei"][0], u["ei"][1]
    lin = lambda n: x @ W[f"lin_{n}.kernel"] + W[f"lin_{n}.bias"]  # noqa: E731
    z = lin("key")[dst] + lin("query")[src]
    if edge_dim:
        z = z + ea @ W["lin_edge.kernel"]
    out = torch.zeros((x.shape[0], LAYER_OUT), dtype=f64).index_add(0, dst, torch.sigmoid(z) * lin("value")[src])
    if root_weight:
        out = out + x @ W["lin_skip.kernel"]
    out = out + W["final_bias"]
    out.backward(u["gout"].to(f64))
    return {"out": out.detach(), "d_x": x.grad, "d_edge_attr": ea.grad if edge_dim else None,
            **{f"d_{n}": t.grad for n, t in W.items()}}


def run_layer(dev, edge_dim, root_weight):
    """The layer on `dev` with layer_inputs' weights: the quantities of layer_ref."""
    import keras_geometric_amd as kgx

    u = layer_inputs()
    layer = kgx.ResGatedGraphConv(LAYER_OUT, edge_dim=edge_dim, root_weight=root_weight)
    assert kgx.ResGatedGraphConv.from_config(layer.get_config()).get_config() == layer.get_config()
    layer._build_device = dev
    layer.build([(None, LAYER_IN)])
    names = layer_names(edge_dim, root_weight)
    params = dict(zip(names, layer.weights))
    assert len(layer.weights) == len(names)
    assert all(tuple(params[n].shape) == tuple(u["weights"][n].shape) for n in names), [tuple(w.shape) for w in layer.weights]
    layer.set_weights([u["weights"][n].numpy() for n in names])
    x, ea = (u[n].clone().to(dev).requires_grad_(True) for n in ("x", "edge_attr"))
    out = layer([x, u["ei"].to(dev)], edge_attr=ea if edge_dim else None)
    out.backward(u["gout"].to(dev))
    return {"out": out.detach(), "d_x": x.grad, "d_edge_attr": ea.grad if edge_dim else None,
            **{f"d_{n}": params[n].grad for n in names}}
