"""Plain restatement of the GATv2 attention aggregation for the op-level tests
(test infrastructure, imported by tests only; runs on the CPU at any dtype).

`gatv2_ref` is `kops.gatv2_aggregate` on given h_src / h_dst, in the
reference's order (gatv2_conv.py:241-352): gather, leaky ReLU, score, segment
max, exp, segment sum + 1e-10, divide, optional attention dropout mask,
index_add of alpha * h_j, + bias.  Edges are taken in input order, graphs may
be bipartite (n_src != n_dst) and have empty rows.

`gatv2_grads64` is its float64 autograd.  With per_edge=True the gathered
h_j, h_i and an att expanded to [E, H, C] are leaf tensors, so their .grad
are the per-edge contributions to d h_src, d h_dst and d att: no formula of
the kernel is restated.  Next to the gradients it returns the sums of the
contributions' magnitudes,

    A_src = index_add(|d h_j|),  A_dst = index_add(|d h_i|),  A_att = sum_e |d att_e|,

the scale of the bound a re-associated fp32 sum is held to here,
|got - ref| <= 1e-5 * max(1, A) (tests/test_gpu_backward.py,
assert_tol_scaled): split hub rows, the transposed pass and the atomics of
d att all sum these terms in another order than the reference.

The module also owns what the CPU and the GPU test module must share: the two
bipartite graphs, the (heads, channels) list with the lane layout the two
rules of csrc/kgx_attn_layout.h give each pair, a Python mirror of those rules
(held equal to the C++ by tests/test_attn_layout_host.py), and the seeded
inputs.
"""

from __future__ import annotations

import functools

import numpy as np
import torch

SLOPE = 0.2
TOL = 1e-5
SPLIT_LEN = 16  # forward graphs are built with split_len=16
HUB_DST, HUB_SRC = 3, 7

# name: (n_src, n_dst, random edges, edges into HUB_DST, edges out of HUB_SRC, seed)
GRAPHS = {
    "small": (60, 50, 600, 300, 600, 101),
    "deep": (500, 400, 6000, 1000, 2500, 102),
}

# (heads, channels): (forward K, backward K) = channels per lane, as kgx_gatv2 and
# kgx_gatv2_backward pick them for aligned contiguous inputs (fwd_layout / bwd_layout
# below mirror the rules); the remarks name what each pair is in the list for
LAYOUTS = {
    (8, 16): (8, 2),
    (8, 32): (8, 4),
    (8, 64): (8, 8),
    (8, 128): (16, 16),
    (4, 256): (16, 16),  # backward LH 16
    (2, 64): (8, 2),  # backward LH 32
    (1, 64): (8, 1),  # backward LH 64
    (3, 12): (4, 1),  # forward: padding sub-lane and padding head
    (5, 24): (8, 4),  # backward: padding lanes and heads
    (16, 4): (4, 1),  # forward LH 1
    (2, 6): (2, 1),  # forward fallback 2
    (3, 6): (2, 1),  # row stride not a multiple of 4
    (2, 7): (1, 1),
}
SHAPES = list(LAYOUTS)
DEEP_SHAPES = [(8, 16), (8, 64)]
DROPOUT_SHAPE, DROPOUT_P, DROPOUT_SEED = (4, 8), 0.25, 20241
DOMINANT_SHAPES = [(8, 16), (3, 12)]
DOMINANT_SRC = 11
# position of the dominant edge in destination HUB_DST's row of `deep` (1000 edges, 63 chunks of 16):
# first slot, slot 17 (second chunk), a slot in chunk 40 (past the fix-up's first batch of 16), last slot
DOMINANT_POS = {"first": 0, "slot17": 17, "chunk40": 40 * SPLIT_LEN + 5, "last": 999}


def _np2(v: int) -> int:
    return 1 << (max(int(v), 1) - 1).bit_length()


def fwd_layout(heads: int, channels: int, ld: int | None = None, aligned: int = 16):
    """(K, LH) of the forward rule (attn_pick_k: kgx_gatv2, kgx_dot_attention and
    kgx_dot_attention_backward) for tensors whose pointers are `aligned`-byte
    aligned and whose leading dimensions are all multiples of gcd(ld, 4) (ld
    defaults to heads * channels), or None for an unsupported shape (more than
    64 lanes per row)."""
    ld = heads * channels if ld is None else ld
    if ld % 4 == 0 and aligned % 16 == 0:
        for k in (8, 4, 16):
            if channels % k == 0 and heads * _np2(channels // k) <= 64:
                return k, _np2(channels // k)
    k = 2 if (channels % 2 == 0 and ld % 2 == 0 and aligned % 8 == 0) else 1
    lh = _np2((channels + k - 1) // k)
    return (k, lh) if heads * lh <= 64 else None


def bwd_layout(heads: int, channels: int, ld: int | None = None, aligned: int = 16):
    """(K, LH) of kgx_gatv2_backward (attn_pick_k_smallest) under the same conditions."""
    ld = heads * channels if ld is None else ld
    for k in (1, 2, 4, 8, 16):
        if channels % k or ld % min(k, 4) or aligned % (4 * min(k, 4)):
            continue
        if heads * _np2(channels // k) <= 64:
            return k, _np2(channels // k)
    return None


def group_lanes(heads: int, layout):
    """G, the lanes of a row's group, of a (K, LH) layout."""
    return _np2(heads * layout[1])


@functools.lru_cache(maxsize=None)
def make_graph(name: str):
    """(src, dst, n_src, n_dst): int64 COO in input order.  Bipartite, no self
    loops in any sense (sources and destinations are different node sets),
    multi-edges, destination 0 with no in-edge, the last source with no
    out-edge, HUB_DST / HUB_SRC with exactly the listed hub degrees (the random
    edges avoid both)."""
    n_src, n_dst, n_rand, n_in, n_out, seed = GRAPHS[name]
    rng = np.random.default_rng(seed)
    src_pool = np.array([j for j in range(n_src - 1) if j != HUB_SRC])
    dst_pool = np.array([i for i in range(1, n_dst) if i != HUB_DST])
    src = np.concatenate([rng.choice(src_pool, n_rand), rng.choice(src_pool, n_in), np.full(n_out, HUB_SRC)])
    dst = np.concatenate([rng.choice(dst_pool, n_rand), np.full(n_in, HUB_DST), rng.choice(dst_pool, n_out)])
    perm = rng.permutation(src.size)
    return torch.from_numpy(src[perm]).long(), torch.from_numpy(dst[perm]).long(), n_src, n_dst


def dominant_graph(pos: int):
    """`deep` with source DOMINANT_SRC appearing exactly once in HUB_DST's row,
    as the pos-th of its edges in input order (= CSR order: the build is stable)."""
    src, dst, n_src, n_dst = make_graph("deep")
    src = src.clone()
    row = torch.nonzero(dst == HUB_DST).flatten()
    other = row[src[row] == DOMINANT_SRC]
    src[other] = DOMINANT_SRC + 1
    src[row[pos]] = DOMINANT_SRC
    return src, dst, n_src, n_dst


@functools.lru_cache(maxsize=None)
def make_inputs(name: str, heads: int, channels: int):
    """Seeded fp32 inputs of a (graph, shape) pair: h ~ N(0,1), att ~ 0.3 N(0,1),
    bias and grad_out ~ N(0,1)."""
    _, _, n_src, n_dst = make_graph(name)
    g = torch.Generator().manual_seed(1000 * heads + channels + (7 if name == "deep" else 0))
    hc = heads * channels
    return {
        "h_src": torch.randn(n_src, hc, generator=g),
        "h_dst": torch.randn(n_dst, hc, generator=g),
        "att": 0.3 * torch.randn(heads, channels, generator=g),
        "bias": torch.randn(hc, generator=g),
        "gout": torch.randn(n_dst, hc, generator=g),
    }


@functools.lru_cache(maxsize=None)
def dominant_inputs(heads: int, channels: int):
    """Inputs of the rescale / merge case on dominant_graph: strictly positive
    att (>= 0.5) and source row DOMINANT_SRC at +100 in every channel, so its
    score exceeds every other by far more than fp32 expf's underflow."""
    _, _, n_src, n_dst = make_graph("deep")
    g = torch.Generator().manual_seed(5000 + 100 * heads + channels)
    hc = heads * channels
    h_src = torch.randn(n_src, hc, generator=g)
    h_src[DOMINANT_SRC] = 100.0
    return {
        "h_src": h_src,
        "h_dst": torch.randn(n_dst, hc, generator=g),
        "att": torch.randn(heads, channels, generator=g).abs() + 0.5,
    }


def gatv2_ref(h_src, h_dst, att, bias, src, dst, n_dst, heads, channels, slope, mask=None, per_edge=False):
    """out [n_dst, heads*channels] in the dtype of h_src; with per_edge=True
    (out, (h_j, h_i, att_e)), the three being leaf tensors of shape [E, H, C]."""
    H, C = heads, channels
    src, dst = src.long(), dst.long()
    E = src.numel()
    dt = h_src.dtype
    h_j = h_src.reshape(-1, H, C)[src]
    h_i = h_dst.reshape(-1, H, C)[dst]
    att_e = att.reshape(1, H, C)
    if per_edge:
        h_j = h_j.detach().clone().requires_grad_(True)
        h_i = h_i.detach().clone().requires_grad_(True)
        att_e = att_e.expand(E, H, C).detach().clone().requires_grad_(True)
    z = h_i + h_j
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
    return (out, (h_j, h_i, att_e)) if per_edge else out


def gatv2_grads(dtype, h_src, h_dst, att, bias, src, dst, n_dst, heads, channels, slope, gout, mask=None):
    """Plain autograd of gatv2_ref at `dtype`: {out, d_src, d_dst, d_att, d_bias}."""
    hs, hd, a, b = (t.detach().to(dtype).clone().requires_grad_(True) for t in (h_src, h_dst, att, bias))
    out = gatv2_ref(hs, hd, a, b, src, dst, n_dst, heads, channels, slope, mask=mask)
    out.backward(gout.to(dtype))
    return {"out": out.detach(), "d_src": hs.grad, "d_dst": hd.grad, "d_att": a.grad.reshape(-1), "d_bias": b.grad}


def gatv2_grads64(h_src, h_dst, att, bias, src, dst, n_dst, heads, channels, slope, gout, mask=None):
    """float64 reference: {out, d_src, d_dst, d_att, d_bias, A_src, A_dst, A_att},
    gradients summed from the per-edge leaves, A_* the sums of their magnitudes."""
    H, C = heads, channels
    src, dst = src.long(), dst.long()
    f64 = torch.float64
    b64 = None if bias is None else bias.to(f64)
    out, (h_j, h_i, att_e) = gatv2_ref(h_src.to(f64), h_dst.to(f64), att.to(f64), b64, src, dst, n_dst, H, C,
                                       slope, mask=mask, per_edge=True)
    out.backward(gout.to(f64))
    n_src = h_src.shape[0]

    def rows(n, index, t):
        return torch.zeros((n, H, C), dtype=f64).index_add(0, index, t).reshape(n, H * C)

    return {
        "out": out.detach(),
        "d_src": rows(n_src, src, h_j.grad),
        "d_dst": rows(n_dst, dst, h_i.grad),
        "d_att": att_e.grad.sum(0).reshape(-1),
        "d_bias": gout.to(f64).sum(0),
        "A_src": rows(n_src, src, h_j.grad.abs()),
        "A_dst": rows(n_dst, dst, h_i.grad.abs()),
        "A_att": att_e.grad.abs().sum(0).reshape(-1),
    }


@functools.lru_cache(maxsize=None)
def reference(name: str, heads: int, channels: int):
    """gatv2_grads64 of make_inputs(name, heads, channels) on make_graph(name),
    computed once and shared (treat as read-only)."""
    src, dst, _, n_dst = make_graph(name)
    x = make_inputs(name, heads, channels)
    return gatv2_grads64(x["h_src"], x["h_dst"], x["att"], x["bias"], src, dst, n_dst, heads, channels, SLOPE,
                         x["gout"])


def ratio(got, ref, scale) -> float:
    """max |got - ref| / (TOL * max(1, scale)); a NaN anywhere gives inf."""
    got, ref, scale = (t.detach().cpu().to(torch.float64) for t in (got, ref, scale))
    r = (got - ref).abs() / (TOL * scale.abs().clamp_min(1.0))
    return float("inf") if bool(torch.isnan(r).any()) else float(r.max())


def ratios(got: dict, ref: dict) -> dict:
    """err / bound per quantity: out against 1e-5 max(1, |ref|), the gradients
    that `got` has against 1e-5 max(1, A)."""
    r = {"out": ratio(got["out"], ref["out"], ref["out"])}
    for k, a in (("d_src", "A_src"), ("d_dst", "A_dst"), ("d_att", "A_att")):
        if k in got:
            r[k] = ratio(got[k], ref[k], ref[a])
    return r
