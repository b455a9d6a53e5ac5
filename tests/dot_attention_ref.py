"""Plain restatement of the dot-product graph attention (kops.dot_attention,
kgx_dot_attention) for its tests (test infrastructure, imported by tests only;
runs on the CPU at any dtype).

`dot_attention_ref` is PyG's TransformerConv message passing without edge
features, on given q, k, v: gather, per-head dot, scatter_reduce amax, exp,
index_add, divide (no epsilon), optional attention dropout mask, index_add of
alpha * v_j.  Edges are taken in input order; graphs may be bipartite and have
empty rows, whose exp(s - max) never exists and whose output row is zero.

`dot_attention_grads64` is its float64 autograd.  The gathered q_i, k_j and
v_j are leaf tensors, so their .grad are the per-edge contributions to d q,
d k and d v: no formula of the kernel is restated.  Next to the gradients it
returns the sums of the contributions' magnitudes

    A_q = index_add(|d q_i|),  A_k = index_add(|d k_j|),  A_v = index_add(|d v_j|),

the scale of the bound a re-associated fp32 sum is held to,
|got - ref| <= 1e-5 * max(1, A), exactly as gatv2_ref.gatv2_grads64.

The module also owns what the CPU and GPU test modules share: the graphs
(gatv2_ref.make_graph's, reused by import), the (heads, channels) list with
the lane layout kgx_dot_attention gives each pair (gatv2_ref.fwd_layout, the
Python mirror of the forward rule), and the seeded inputs.
"""

from __future__ import annotations

import functools
import math

import torch

import gatv2_ref as GR
from gatv2_ref import DOMINANT_POS, HUB_DST, HUB_SRC, SPLIT_LEN, dominant_graph, make_graph, ratio  # noqa: F401

TOL = 1e-5

# (heads, channels): (K, LH) = channels per lane and lanes per head, as csrc/kgx_attn_layout.h's
# attn_pick_k gives them for aligned contiguous inputs (one rule for the forward and both backward passes)
LAYOUTS = {
    (8, 16): (8, 2),
    (8, 64): (8, 8),
    (8, 128): (16, 8),
    (4, 256): (16, 16),
    (1, 64): (8, 8),
    (3, 12): (4, 4),  # padding sub-lane (LH 4 for 3 pieces) and a padding head
    (2, 7): (1, 8),  # scalar loads, padding sub-lane
    (3, 6): (2, 4),  # row stride 18: not a multiple of 4, float2 loads, padding sub-lane and head
}
SHAPES = [(8, 16), (8, 64), (8, 128), (4, 256), (1, 64), (3, 12), (2, 7)]  # the headroom / lane-layout list
ODD_SHAPES = [(3, 12), (2, 7), (3, 6)]
DEEP_SHAPES = [(8, 16), (8, 64)]
DROPOUT_SHAPE, DROPOUT_P, DROPOUT_SEED = (4, 8), 0.25, 20251
DOMINANT_SHAPES = [(8, 16), (3, 12)]
DOMINANT_SRC = GR.DOMINANT_SRC
DOMINANT_GAP = 30.0  # the dominant edge's score exceeds every other of its row by about this much


layout = GR.fwd_layout  # (K, LH) of kgx_dot_attention and kgx_dot_attention_backward, or None


@functools.lru_cache(maxsize=None)
def make_inputs(name: str, heads: int, channels: int):
    """Seeded fp32 inputs of a (graph, shape) pair: q, k, v and grad_out ~ N(0, 1)."""
    _, _, n_src, n_dst = make_graph(name)
    g = torch.Generator().manual_seed(77000 + 1000 * heads + channels + (7 if name == "deep" else 0))
    hc = heads * channels
    return {
        "q": torch.randn(n_dst, hc, generator=g),
        "k": torch.randn(n_src, hc, generator=g),
        "v": torch.randn(n_src, hc, generator=g),
        "gout": torch.randn(n_dst, hc, generator=g),
    }


@functools.lru_cache(maxsize=None)
def dominant_inputs(heads: int, channels: int):
    """Inputs of the rescale / merge case on gatv2_ref.dominant_graph: q, k ~
    N(0, 1) except the constant rows q[HUB_DST] = 1 and k[DOMINANT_SRC] =
    DOMINANT_GAP / sqrt(C): at scale 1/sqrt(C) the dominant score is
    DOMINANT_GAP in every head, the others of the row are sum_c k_jc / sqrt(C)
    ~ N(0, 1) (the CPU module checks the gap).  exp(-30) ~ 1e-13 does not
    underflow, so the running sums are really rescaled."""
    _, _, n_src, n_dst = make_graph("deep")
    g = torch.Generator().manual_seed(88000 + 100 * heads + channels)
    hc = heads * channels
    q = torch.randn(n_dst, hc, generator=g)
    k = torch.randn(n_src, hc, generator=g)
    v = torch.randn(n_src, hc, generator=g)
    q[HUB_DST] = 1.0
    k[DOMINANT_SRC] = DOMINANT_GAP / math.sqrt(channels)
    return {"q": q, "k": k, "v": v, "gout": torch.randn(n_dst, hc, generator=g)}


def dot_attention_ref(q, k, v, src, dst, n_dst, heads, channels, scale=None, mask=None, per_edge=False):
    """out [n_dst, heads*channels] in the dtype of q; with per_edge=True
    (out, (q_i, k_j, v_j)), the three being leaf tensors of shape [E, H, C]."""
    H, C = heads, channels
    scale = 1.0 / math.sqrt(C) if scale is None else scale
    src, dst = src.long(), dst.long()
    dt = q.dtype
    q_i = q.reshape(-1, H, C)[dst]
    k_j = k.reshape(-1, H, C)[src]
    v_j = v.reshape(-1, H, C)[src]
    if per_edge:
        q_i, k_j, v_j = (t.detach().clone().requires_grad_(True) for t in (q_i, k_j, v_j))
    s = (q_i * k_j).sum(-1) * scale  # [E, H]
    idx = dst[:, None].expand(-1, H)
    mx = torch.full((n_dst, H), float("-inf"), dtype=dt).scatter_reduce(0, idx, s.detach(), "amax",
                                                                         include_self=True)
    ex = torch.exp(s - mx[dst])
    ssum = torch.zeros((n_dst, H), dtype=dt).index_add(0, dst, ex)
    alpha = ex / ssum[dst]
    if mask is not None:
        alpha = alpha * mask.to(dt)
    out = torch.zeros((n_dst, H, C), dtype=dt).index_add(0, dst, alpha[..., None] * v_j).reshape(n_dst, H * C)
    return (out, (q_i, k_j, v_j)) if per_edge else out


def dot_attention_grads(dtype, q, k, v, src, dst, n_dst, heads, channels, gout, scale=None, mask=None):
    """Plain autograd of dot_attention_ref at `dtype`: {out, d_q, d_k, d_v}."""
    q, k, v = (t.detach().to(dtype).clone().requires_grad_(True) for t in (q, k, v))
    out = dot_attention_ref(q, k, v, src, dst, n_dst, heads, channels, scale=scale, mask=mask)
    out.backward(gout.to(dtype))
    return {"out": out.detach(), "d_q": q.grad, "d_k": k.grad, "d_v": v.grad}


def dot_attention_grads64(q, k, v, src, dst, n_dst, heads, channels, gout, scale=None, mask=None):
    """float64 reference: {out, d_q, d_k, d_v, A_q, A_k, A_v}, gradients summed
    from the per-edge leaves, A_* the sums of their magnitudes."""
    H, C = heads, channels
    src, dst = src.long(), dst.long()
    f64 = torch.float64
    out, (q_i, k_j, v_j) = dot_attention_ref(q.to(f64), k.to(f64), v.to(f64), src, dst, n_dst, H, C, scale=scale,
                                             mask=mask, per_edge=True)
    out.backward(gout.to(f64))
    n_src = k.shape[0]

    def rows(n, index, t):
        return torch.zeros((n, H, C), dtype=f64).index_add(0, index, t).reshape(n, H * C)

    return {
        "out": out.detach(),
        "d_q": rows(n_dst, dst, q_i.grad),
        "d_k": rows(n_src, src, k_j.grad),
        "d_v": rows(n_src, src, v_j.grad),
        "A_q": rows(n_dst, dst, q_i.grad.abs()),
        "A_k": rows(n_src, src, k_j.grad.abs()),
        "A_v": rows(n_src, src, v_j.grad.abs()),
    }


@functools.lru_cache(maxsize=None)
def reference(name: str, heads: int, channels: int):
    """dot_attention_grads64 of make_inputs(name, heads, channels) on
    make_graph(name), computed once and shared (treat as read-only)."""
    src, dst, _, n_dst = make_graph(name)
    x = make_inputs(name, heads, channels)
    return dot_attention_grads64(x["q"], x["k"], x["v"], src, dst, n_dst, heads, channels, x["gout"])


def ratios(got: dict, ref: dict) -> dict:
    """err / bound per quantity: out against 1e-5 max(1, |ref|), the gradients
    that `got` has against 1e-5 max(1, A)."""
    r = {"out": ratio(got["out"], ref["out"], ref["out"])}
    for key, a in (("d_q", "A_q"), ("d_k", "A_k"), ("d_v", "A_v")):
        if key in got:
            r[key] = ratio(got[key], ref[key], ref[a])
    return r
