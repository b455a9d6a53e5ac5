"""Plain restatement of the dot-product graph attention with edge features
(kops.dot_attention(edge=...), kgx_dot_attention_edge) for its tests (test
infrastructure, imported by tests only; runs on the CPU at any dtype).

`dot_attention_edge_ref` is tests/dot_attention_ref.py's dot_attention_ref with
k_j + e and v_j + e in the place of k_j and v_j: PyG's TransformerConv message
passing with edge_dim, on given q, k, v and projected edge rows e [E, H*C] in
input-edge order.

`dot_attention_edge_grads64` is its float64 autograd on per-edge leaves, as
dot_attention_ref.dot_attention_grads64: the gathered q_i, k_j, v_j are leaves,
and the two uses of e (in the score and in the message) are two separate
leaves, so next to d e = d e_score + d e_value it returns

    A_e = |d e_score| + |d e_value|,

the scale of the bound |got - ref| <= 1e-5 * max(1, A_e) for d e (an edge row
has one contribution per use; A_q, A_k, A_v sum over edges as before).

The module also owns the seeded edge table the CPU and GPU modules share.
"""

from __future__ import annotations

import functools
import math

import torch

import dot_attention_ref as DR
from dot_attention_ref import ratio


@functools.lru_cache(maxsize=None)
def make_edge(name: str, heads: int, channels: int):
    """Seeded fp32 edge table e ~ N(0, 1) of [E, H*C] for make_graph(name), input-edge order."""
    src = DR.make_graph(name)[0]
    g = torch.Generator().manual_seed(99000 + 1000 * heads + channels + (7 if name == "deep" else 0))
    return torch.randn(src.numel(), heads * channels, generator=g)


def dot_attention_edge_ref(q, k, v, e, src, dst, n_dst, heads, channels, scale=None, mask=None, per_edge=False):
    """out [n_dst, heads*channels] in the dtype of q; with per_edge=True
    (out, (q_i, k_j, v_j, e_s, e_v)), leaf tensors of shape [E, H, C]; e_s is
    the use of e in the score, e_v the one in the message."""
    H, C = heads, channels
    scale = 1.0 / math.sqrt(C) if scale is None else scale
    src, dst = src.long(), dst.long()
    dt = q.dtype
    q_i = q.reshape(-1, H, C)[dst]
    k_j = k.reshape(-1, H, C)[src]
    v_j = v.reshape(-1, H, C)[src]
    e_s = e_v = e.reshape(-1, H, C)
    if per_edge:
        q_i, k_j, v_j, e_s, e_v = (t.detach().clone().requires_grad_(True) for t in (q_i, k_j, v_j, e_s, e_v))
    s = (q_i * (k_j + e_s)).sum(-1) * scale  # [E, H]
    idx = dst[:, None].expand(-1, H)
    mx = torch.full((n_dst, H), float("-inf"), dtype=dt).scatter_reduce(0, idx, s.detach(), "amax",
                                                                         include_self=True)
    ex = torch.exp(s - mx[dst])
    ssum = torch.zeros((n_dst, H), dtype=dt).index_add(0, dst, ex)
    alpha = ex / ssum[dst]
    if mask is not None:
        alpha = alpha * mask.to(dt)
    out = torch.zeros((n_dst, H, C), dtype=dt).index_add(0, dst, alpha[..., None] * (v_j + e_v))
    out = out.reshape(n_dst, H * C)
    return (out, (q_i, k_j, v_j, e_s, e_v)) if per_edge else out


def dot_attention_edge_grads(dtype, q, k, v, e, src, dst, n_dst, heads, channels, gout, scale=None, mask=None):
    """Plain autograd of dot_attention_edge_ref at `dtype`: {out, d_q, d_k, d_v, d_e}."""
    q, k, v, e = (t.detach().to(dtype).clone().requires_grad_(True) for t in (q, k, v, e))
    out = dot_attention_edge_ref(q, k, v, e, src, dst, n_dst, heads, channels, scale=scale, mask=mask)
    out.backward(gout.to(dtype))
    return {"out": out.detach(), "d_q": q.grad, "d_k": k.grad, "d_v": v.grad, "d_e": e.grad}


def dot_attention_edge_grads64(q, k, v, e, src, dst, n_dst, heads, channels, gout, scale=None, mask=None):
    """float64 reference: {out, d_q, d_k, d_v, d_e, A_q, A_k, A_v, A_e}."""
    H, C = heads, channels
    src, dst = src.long(), dst.long()
    f64 = torch.float64
    out, (q_i, k_j, v_j, e_s, e_v) = dot_attention_edge_ref(q.to(f64), k.to(f64), v.to(f64), e.to(f64), src, dst,
                                                            n_dst, H, C, scale=scale, mask=mask, per_edge=True)
    out.backward(gout.to(f64))
    n_src, E = k.shape[0], src.numel()

    def rows(n, index, t):
        return torch.zeros((n, H, C), dtype=f64).index_add(0, index, t).reshape(n, H * C)

    return {
        "out": out.detach(),
        "d_q": rows(n_dst, dst, q_i.grad),
        "d_k": rows(n_src, src, k_j.grad),
        "d_v": rows(n_src, src, v_j.grad),
        "d_e": (e_s.grad + e_v.grad).reshape(E, H * C),
        "A_q": rows(n_dst, dst, q_i.grad.abs()),
        "A_k": rows(n_src, src, k_j.grad.abs()),
        "A_v": rows(n_src, src, v_j.grad.abs()),
        "A_e": (e_s.grad.abs() + e_v.grad.abs()).reshape(E, H * C),
    }


@functools.lru_cache(maxsize=None)
def reference(name: str, heads: int, channels: int):
    """dot_attention_edge_grads64 of DR.make_inputs + make_edge on make_graph(name),
    computed once and shared (treat as read-only)."""
    src, dst, _, n_dst = DR.make_graph(name)
    x = DR.make_inputs(name, heads, channels)
    return dot_attention_edge_grads64(x["q"], x["k"], x["v"], make_edge(name, heads, channels), src, dst, n_dst,
                                      heads, channels, x["gout"])


def expanded(k, v, e, src, heads, channels):
    """The graph with one source per edge: (k', v', src') = (k[src] + e, v[src] + e, arange(E)),
    on which the attention without edge features is the attention with them."""
    src = src.long()
    return k[src] + e, v[src] + e, torch.arange(src.numel())


def ratios(got: dict, ref: dict) -> dict:
    """err / bound per quantity: out against 1e-5 max(1, |ref|), the gradients
    that `got` has against 1e-5 max(1, A)."""
    r = {"out": ratio(got["out"], ref["out"], ref["out"])}
    for key, a in (("d_q", "A_q"), ("d_k", "A_k"), ("d_v", "A_v"), ("d_e", "A_e")):
        if key in got:
            r[key] = ratio(got[key], ref[key], ref[a])
    return r


# ---------------------------------------------------------------------------
# Layer level: TransformerConv(edge_dim=...) restated in float64 with the layer's weights
# ---------------------------------------------------------------------------
LAYER_NAMES = ("lin_query", "lin_key", "lin_value", "lin_skip", "lin_beta", "lin_edge")


def layer_ref(dtype, weights: dict, cfg: dict, x_i, x_j, edge_attr, src, dst, gout):
    """PyG's TransformerConv with edge_dim at `dtype` on the given weights
    ({name: tensor}); cfg: heads, channels, concat, root_weight, beta.
    Returns (out, {name: grad}, d edge_attr)."""
    H, C = cfg["heads"], cfg["channels"]
    W = {n: w.detach().to(dtype).clone().requires_grad_(True) for n, w in weights.items()}
    x_i, x_j = x_i.detach().to(dtype).cpu(), x_j.detach().to(dtype).cpu()
    ea = edge_attr.detach().to(dtype).cpu().clone().requires_grad_(True)

    def lin(name, x):
        y = x @ W[f"{name}.kernel"]
        return y + W[f"{name}.bias"] if f"{name}.bias" in W else y

    n = x_i.shape[0]
    out = dot_attention_edge_ref(lin("lin_query", x_i), lin("lin_key", x_j), lin("lin_value", x_j),
                                 lin("lin_edge", ea), src, dst, n, H, C)
    if not cfg["concat"]:
        out = out.reshape(n, H, C).mean(1)
    if cfg["root_weight"]:
        r = lin("lin_skip", x_i)
        if cfg["beta"]:
            b = torch.sigmoid(torch.cat([out, r, out - r], -1) @ W["lin_beta.kernel"])
            out = b * r + (1 - b) * out
        else:
            out = out + r
    out.backward(gout.to(dtype).cpu())
    return out.detach(), {n: w.grad for n, w in W.items()}, ea.grad


def square_graph(n=64, e=500, seed=31):
    """tests/test_gpu_transformer_conv.py's graph: seeded [2, E] int64 on n nodes, E = e + 60:
    multi-edges, node 0 without in-edges, node 5 a small hub."""
    import numpy as np

    rng = np.random.default_rng(seed)
    src = np.concatenate([rng.integers(0, n, e), rng.integers(0, n, 60)])
    dst = np.concatenate([rng.integers(1, n, e), np.full(60, 5)])
    return torch.from_numpy(np.stack([src, dst])).long()


def layer_weights(seed: int, cfg: dict, f_dst: int, f_src: int, edge_dim: int, use_bias: bool = True) -> dict:
    """Weights as the GPU module leaves the layer's: glorot-uniform kernels, N(0, 1/4) biases."""
    H, C = cfg["heads"], cfg["channels"]
    hc = H * C
    od = hc if cfg["concat"] else C
    g = torch.Generator().manual_seed(seed)
    shapes = {"lin_query": (f_dst, hc), "lin_key": (f_src, hc), "lin_value": (f_src, hc)}
    if cfg["root_weight"]:
        shapes["lin_skip"] = (f_dst, od)
        if cfg["beta"]:
            shapes["lin_beta"] = (3 * od, 1)
    shapes["lin_edge"] = (edge_dim, hc)
    W = {}
    for lin in LAYER_NAMES:
        if lin not in shapes:
            continue
        fi, fo = shapes[lin]
        lim = math.sqrt(6.0 / (fi + fo))
        W[f"{lin}.kernel"] = (torch.rand(fi, fo, generator=g) * 2 - 1) * lim
        if use_bias and lin not in ("lin_beta", "lin_edge"):
            W[f"{lin}.bias"] = 0.5 * torch.randn(fo, generator=g)
    return W
