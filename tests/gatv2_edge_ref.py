"""Plain restatement of the GATv2 attention aggregation with edge features
(kops.gatv2_aggregate(edge=...), kgx_gatv2_edge) for its tests (test
infrastructure, imported by tests only; runs on the CPU at any dtype).

`gatv2_edge_ref` is tests/gatv2_ref.py's gatv2_ref with z = (h_i + h_j) + e in
the place of h_i + h_j: PyG's GATv2Conv message passing with edge_dim on the
reference's shared-weight layer, in the reference's order (gather, add, leaky
ReLU, score, segment max, exp, segment sum + 1e-10, divide, optional dropout
mask, index_add of alpha * h_j, + bias), on given h_src, h_dst and projected
edge rows e [E, H*C] in input-edge order.  The edge row enters the score only.

`gatv2_edge_grads64` is its float64 autograd on per-edge leaves, as
gatv2_ref.gatv2_grads64(per_edge=True): the gathered h_j, h_i, the expanded att
and e are leaf tensors, so no formula of the kernel is restated.  An edge row
has one use, so A_e = |d e|; A_src, A_dst and A_att sum the magnitudes of the
per-edge contributions as before.

The module also owns the seeded edge table the CPU and GPU modules share, and
the layer-level restatement of GATv2Conv(edge_dim=...).
"""

from __future__ import annotations

import functools
import math

import torch

import gatv2_ref as GR
from gatv2_ref import ratio


@functools.lru_cache(maxsize=None)
def make_edge(name: str, heads: int, channels: int):
    """Seeded fp32 edge table e ~ N(0, 1) of [E, H*C] for make_graph(name), input-edge order."""
    src = GR.make_graph(name)[0]
    g = torch.Generator().manual_seed(77000 + 1000 * heads + channels + (7 if name == "deep" else 0))
    return torch.randn(src.numel(), heads * channels, generator=g)


def gatv2_edge_ref(h_src, h_dst, att, bias, e, src, dst, n_dst, heads, channels, slope, mask=None, per_edge=False):
    """out [n_dst, heads*channels] in the dtype of h_src; with per_edge=True
    (out, (h_j, h_i, att_e, e_e)), the four being leaf tensors of shape [E, H, C]."""
    H, C = heads, channels
    src, dst = src.long(), dst.long()
    E = src.numel()
    dt = h_src.dtype
    h_j = h_src.reshape(-1, H, C)[src]
    h_i = h_dst.reshape(-1, H, C)[dst]
    att_e = att.reshape(1, H, C)
    e_e = e.reshape(-1, H, C)
    if per_edge:
        h_j = h_j.detach().clone().requires_grad_(True)
        h_i = h_i.detach().clone().requires_grad_(True)
        att_e = att_e.expand(E, H, C).detach().clone().requires_grad_(True)
        e_e = e_e.detach().clone().requires_grad_(True)
    z = (h_i + h_j) + e_e
    z = torch.where(z > 0, z, slope * z)
    s = (z * att_e).sum(-1)  # [E, H]
    idx = dst[:, None].expand(-1, H)
    mx = torch.full((n_dst, H), float("-inf"), dtype=dt).scatter_reduce(0, idx, s, "amax", include_self=True)
    ex = torch.exp(s - mx[dst])
    ssum = torch.zeros((n_dst, H), dtype=dt).index_add(0, dst, ex)
    alpha = ex / (ssum[dst] + 1e-10)
    if mask is not None:
        alpha = alpha * mask.to(dt)
    out = torch.zeros((n_dst, H, C), dtype=dt).index_add(0, dst, alpha[..., None] * h_j).reshape(n_dst, H * C)
    if bias is not None:
        out = out + bias
    return (out, (h_j, h_i, att_e, e_e)) if per_edge else out


def gatv2_edge_grads(dtype, h_src, h_dst, att, bias, e, src, dst, n_dst, heads, channels, slope, gout, mask=None):
    """Plain autograd of gatv2_edge_ref at `dtype`: {out, d_src, d_dst, d_att, d_e}."""
    hs, hd, a, b, ee = (t.detach().to(dtype).clone().requires_grad_(True) for t in (h_src, h_dst, att, bias, e))
    out = gatv2_edge_ref(hs, hd, a, b, ee, src, dst, n_dst, heads, channels, slope, mask=mask)
    out.backward(gout.to(dtype))
    return {"out": out.detach(), "d_src": hs.grad, "d_dst": hd.grad, "d_att": a.grad.reshape(-1), "d_e": ee.grad}


def gatv2_edge_grads64(h_src, h_dst, att, bias, e, src, dst, n_dst, heads, channels, slope, gout, mask=None):
    """float64 reference: {out, d_src, d_dst, d_att, d_e, A_src, A_dst, A_att, A_e}."""
    H, C = heads, channels
    src, dst = src.long(), dst.long()
    f64 = torch.float64
    b64 = None if bias is None else bias.to(f64)
    out, (h_j, h_i, att_e, e_e) = gatv2_edge_ref(h_src.to(f64), h_dst.to(f64), att.to(f64), b64, e.to(f64), src, dst,
                                                 n_dst, H, C, slope, mask=mask, per_edge=True)
    out.backward(gout.to(f64))
    n_src, E = h_src.shape[0], src.numel()

    def rows(n, index, t):
        return torch.zeros((n, H, C), dtype=f64).index_add(0, index, t).reshape(n, H * C)

    return {
        "out": out.detach(),
        "d_src": rows(n_src, src, h_j.grad),
        "d_dst": rows(n_dst, dst, h_i.grad),
        "d_att": att_e.grad.sum(0).reshape(-1),
        "d_e": e_e.grad.reshape(E, H * C),
        "A_src": rows(n_src, src, h_j.grad.abs()),
        "A_dst": rows(n_dst, dst, h_i.grad.abs()),
        "A_att": att_e.grad.abs().sum(0).reshape(-1),
        "A_e": e_e.grad.abs().reshape(E, H * C),
    }


@functools.lru_cache(maxsize=None)
def reference(name: str, heads: int, channels: int):
    """gatv2_edge_grads64 of GR.make_inputs + make_edge on make_graph(name) with
    bias 0 (empty rows are exact zeros), computed once and shared (treat as read-only)."""
    src, dst, _, n_dst = GR.make_graph(name)
    x = GR.make_inputs(name, heads, channels)
    return gatv2_edge_grads64(x["h_src"], x["h_dst"], x["att"], None, make_edge(name, heads, channels), src, dst,
                              n_dst, heads, channels, GR.SLOPE, x["gout"])


KEYS = ("out", "d_src", "d_dst", "d_att", "d_e")


def ratios(got: dict, ref: dict) -> dict:
    """err / bound per quantity: out against 1e-5 max(1, |ref|), the gradients
    that `got` has against 1e-5 max(1, A)."""
    r = {"out": ratio(got["out"], ref["out"], ref["out"])}
    for key, a in (("d_src", "A_src"), ("d_dst", "A_dst"), ("d_att", "A_att"), ("d_e", "A_e")):
        if key in got:
            r[key] = ratio(got[key], ref[key], ref[a])
    return r


# ---------------------------------------------------------------------------
# Layer level: GATv2Conv(edge_dim=...) restated with the layer's weights
# ---------------------------------------------------------------------------
def loop_attr_ref(edge_attr, dst, n, fill):
    """[n, edge_dim]: the edge_attr row of the loop added to every node, PyG's
    add_self_loops(fill_value=...): "mean" / "add" over the input edges into the
    node (0 without one), a float, or an [edge_dim] tensor."""
    D = edge_attr.shape[1]
    if isinstance(fill, str):
        tot = torch.zeros((n, D), dtype=edge_attr.dtype).index_add(0, dst.long(), edge_attr)
        if fill == "add":
            return tot
        assert fill == "mean"
        cnt = torch.bincount(dst.long(), minlength=n).to(edge_attr.dtype).clamp_min(1.0)
        return tot / cnt[:, None]
    if isinstance(fill, torch.Tensor):
        return fill.to(edge_attr.dtype).reshape(1, D).expand(n, D)
    return torch.full((n, D), float(fill), dtype=edge_attr.dtype)


def layer_ref(dtype, weights: dict, cfg: dict, x_i, x_j, edge_attr, src, dst, gout):
    """GATv2Conv with edge_dim at `dtype` on the given weights ({name: tensor}:
    linear_transform.kernel, att, final_bias (optional), lin_edge.kernel); cfg:
    heads, channels, concat, slope, self_loops, fill.  x_j is x_i on a square
    graph.  Input self loops stay ordinary edges (the documented deviation from
    PyG).  Returns {out, d_x_i, d_x_j (None on a square graph), d_edge_attr,
    d_<weight name>..., margin}; margin is min |z| over the leaky-ReLU inputs: an
    fp32 evaluation takes the same branches when its error in z is below it."""
    H, C = cfg["heads"], cfg["channels"]
    W = {n: w.detach().to(dtype).cpu().clone().requires_grad_(True) for n, w in weights.items()}
    square = x_j is x_i
    xi = x_i.detach().to(dtype).cpu().clone().requires_grad_(True)
    xj = xi if square else x_j.detach().to(dtype).cpu().clone().requires_grad_(True)
    ea = edge_attr.detach().to(dtype).cpu().clone().requires_grad_(True)
    src, dst = src.long().cpu(), dst.long().cpu()
    n = xi.shape[0]
    attr = ea
    if cfg["self_loops"]:
        assert square
        fill = cfg["fill"]
        fill = fill.detach().to(dtype).cpu() if isinstance(fill, torch.Tensor) else fill
        attr = torch.cat([ea, loop_attr_ref(ea, dst, n, fill)], 0)
        loops = torch.arange(n)
        src, dst = torch.cat([src, loops]), torch.cat([dst, loops])
    h_dst = xi @ W["linear_transform.kernel"]
    h_src = h_dst if square else xj @ W["linear_transform.kernel"]
    eps = attr @ W["lin_edge.kernel"]
    bias = W.get("final_bias")
    out = gatv2_edge_ref(h_src, h_dst, W["att"], bias if cfg["concat"] else None, eps, src, dst, n, H, C,
                         cfg["slope"])
    if not cfg["concat"]:
        out = out.reshape(n, H, C).mean(1)
        if bias is not None:
            out = out + bias
    out.backward(gout.to(dtype).cpu())
    z = (h_dst.reshape(-1, H, C)[dst] + h_src.reshape(-1, H, C)[src]) + eps.reshape(-1, H, C)
    return {"out": out.detach(), "d_x_i": xi.grad, "d_x_j": None if square else xj.grad, "d_edge_attr": ea.grad,
            "margin": float(z.detach().abs().min()), **{f"d_{k}": w.grad for k, w in W.items()}}


# The layer cases the CPU and the GPU module share: GATv2Conv(edge_dim=5, heads=4, output_dim=8)
LAYER_H, LAYER_C, LAYER_F, LAYER_D, LAYER_N = 4, 8, 12, 5, 40
LAYER_CASES = {
    "mean": dict(concat=True, self_loops=True, fill="mean"),
    "add": dict(concat=True, self_loops=True, fill="add"),
    "float": dict(concat=True, self_loops=True, fill=0.5),
    "tensor": dict(concat=True, self_loops=True, fill=torch.tensor([1.0, -2.0, 3.0, 0.5, 0.0])),
    "noloops": dict(concat=True, self_loops=False, fill="mean"),
    "concat_false": dict(concat=False, self_loops=True, fill="mean"),
    "bipartite": dict(concat=True, self_loops=False, fill="mean", n_dst=30),
}
COT = 0.25  # cotangent N(0, 1/16), as tests/test_gpu_transformer_conv_edge.py


@functools.lru_cache(maxsize=None)
def layer_inputs(case: str):
    """Seeded fp32 inputs and weights of a layer case: x (x_i [n_dst, F] and x_j [n, F]
    for the bipartite case, else one x), edge_index, edge_attr, the weights in the
    layer's order (att, final_bias, linear_transform.kernel, lin_edge.kernel) and
    the cotangent."""
    cfg = LAYER_CASES[case]
    H, C, F, D, n = LAYER_H, LAYER_C, LAYER_F, LAYER_D, LAYER_N
    g = torch.Generator().manual_seed(8100 + list(LAYER_CASES).index(case))
    ei = layer_graph(n)
    n_dst = cfg.get("n_dst", n)
    if n_dst != n:
        ei = torch.stack([ei[0], ei[1] % n_dst])
    x_j = torch.randn(n, F, generator=g)
    x_i = torch.randn(n_dst, F, generator=g) if n_dst != n else x_j
    od = H * C if cfg["concat"] else C
    return {
        "x_i": x_i, "x_j": x_j, "ei": ei, "edge_attr": torch.randn(ei.shape[1], D, generator=g),
        "weights": {"att": glorot((1, H, C), g), "final_bias": 0.5 * torch.randn(od, generator=g),
                    "linear_transform.kernel": glorot((F, H * C), g), "lin_edge.kernel": glorot((D, H * C), g)},
        "gout": COT * torch.randn(n_dst, od, generator=g),
        "cfg": dict(heads=H, channels=C, concat=cfg["concat"], slope=0.2, self_loops=cfg["self_loops"],
                    fill=cfg["fill"]),
    }


@functools.lru_cache(maxsize=None)
def layer_reference(case: str):
    """layer_ref in float64 on layer_inputs(case), computed once and shared (read-only)."""
    v = layer_inputs(case)
    return layer_ref(torch.float64, v["weights"], v["cfg"], v["x_i"], v["x_j"], v["edge_attr"], v["ei"][0],
                     v["ei"][1], v["gout"])


def layer_ratios(got: dict, ref: dict, tol: float = 1e-5) -> dict:
    """err / bound per quantity of `got`, bound tol * max(1, |ref|)."""
    return {k: ratio(v, ref[k], ref[k]) * (GR.TOL / tol) for k, v in got.items() if v is not None}


def layer_graph(n=40, e=300, seed=57):
    """Seeded [2, E] int64 on n nodes, E = e + 40: multi-edges, a few input self
    loops, node 0 without in-edges, node 5 a small hub."""
    import numpy as np

    rng = np.random.default_rng(seed)
    src = np.concatenate([rng.integers(0, n, e), rng.integers(0, n, 36), np.array([7, 7, 9, 11])])
    dst = np.concatenate([rng.integers(1, n, e), np.full(36, 5), np.array([7, 7, 9, 11])])
    return torch.from_numpy(np.stack([src, dst])).long()


def glorot(shape, generator):
    fi, fo = (shape[-2], shape[-1]) if len(shape) > 1 else (shape[0], shape[0])
    lim = math.sqrt(6.0 / (fi + fo))
    return (torch.rand(shape, generator=generator) * 2 - 1) * lim
