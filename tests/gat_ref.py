"""Plain float64 restatement of the GAT attention aggregation (PyG's GATConv
after its linear maps) for tests/test_gpu_gat.py and tests/test_gat_host.py:

    z_e = (a_dst[i] + a_src[j]) + a_edge[e]    s_e = leaky_relu(z_e)
    alpha_e = exp(s_e - max_i) / (sum_i + 1e-16)   out[i] = sum_e alpha_e mask_e h_src[j_e] (+ bias)

Edges in input order.  The gathered h_j, a_src[j], a_dst[i] and a_edge are
per-edge leaf tensors, so their .grad are the per-edge contributions and A_* the
sums of their magnitudes (the scale of the bound, as tests/gatv2_ref.py).  The
leaky-ReLU branch is taken from the fp32 value of z by the same two adds, so the
kink cannot flip between this reference and a kernel that forms z that way.
Graphs, hub ids and the ratio come from tests/gatv2_ref.py.
"""

from __future__ import annotations

import functools

import torch

import gatv2_ref as GR


@functools.lru_cache(maxsize=None)
def inputs(name: str, heads: int, channels: int):
    """gatv2_ref.make_inputs' h_src, bias and gout plus seeded scalar tables: a_src, a_dst ~ N(0,1) and
    a_edge ~ 0.5 N(0,1) with one row per input edge."""
    x = GR.make_inputs(name, heads, channels)
    src, _, n_src, n_dst = GR.make_graph(name)
    g = torch.Generator().manual_seed(77000 + 100 * heads + channels + (7 if name == "deep" else 0))
    return {"h_src": x["h_src"], "bias": x["bias"], "gout": x["gout"],
            "a_src": torch.randn(n_src, heads, generator=g), "a_dst": torch.randn(n_dst, heads, generator=g),
            "a_edge": 0.5 * torch.randn(src.numel(), heads, generator=g)}


def gat_grads64(h_src, a_src, a_dst, a_edge, bias, src, dst, n_dst, heads, channels, slope, gout, mask=None):
    """a_edge: None or [n_e <= E, H] in input order (edges past it carry 0).  Returns {out, d_src, d_asrc,
    d_adst, d_edge [n_e, H], d_bias, A_src, A_asrc, A_adst, A_edge}."""
    H, C, f64 = heads, channels, torch.float64
    src, dst, E, n_src = src.long(), dst.long(), src.numel(), h_src.shape[0]
    ae32 = torch.zeros((E, H))
    if a_edge is not None:
        ae32[: a_edge.shape[0]] = a_edge
    pos = ((a_dst.float()[dst] + a_src.float()[src]) + ae32) > 0  # the fp32 z of the two adds decides the branch
    h_j = h_src.to(f64).reshape(-1, H, C)[src].clone().requires_grad_(True)
    as_j, ad_i, ae = (t.to(f64).clone().requires_grad_(True) for t in (a_src[src], a_dst[dst], ae32))
    z = (ad_i + as_j) + ae
    s = torch.where(pos, z, slope * z)
    mx = torch.full((n_dst, H), float("-inf"), dtype=f64).scatter_reduce(0, dst[:, None].expand(-1, H), s, "amax")
    ex = torch.exp(s - mx[dst])
    alpha = ex / (torch.zeros((n_dst, H), dtype=f64).index_add(0, dst, ex)[dst] + 1e-16)
    if mask is not None:
        alpha = alpha * mask.to(f64)
    out = torch.zeros((n_dst, H, C), dtype=f64).index_add(0, dst, alpha[..., None] * h_j).reshape(n_dst, H * C)
    if bias is not None:
        out = out + bias.to(f64)
    out.backward(gout.to(f64))

    def rows(n, index, t):
        return torch.zeros((n,) + t.shape[1:], dtype=f64).index_add(0, index, t).reshape(n, -1)

    n_e = 0 if a_edge is None else a_edge.shape[0]
    return {"out": out.detach(), "d_bias": gout.to(f64).sum(0),
            "d_src": rows(n_src, src, h_j.grad), "A_src": rows(n_src, src, h_j.grad.abs()),
            "d_asrc": rows(n_src, src, as_j.grad), "A_asrc": rows(n_src, src, as_j.grad.abs()),
            "d_adst": rows(n_dst, dst, ad_i.grad), "A_adst": rows(n_dst, dst, ad_i.grad.abs()),
            "d_edge": ae.grad[:n_e], "A_edge": ae.grad[:n_e].abs()}


def ratios(got: dict, ref: dict) -> dict:
    """err / bound: out against 1e-5 max(1, |ref|), each gradient `got` has against 1e-5 max(1, A)."""
    r = {"out": GR.ratio(got["out"], ref["out"], ref["out"])}
    for k in ("src", "asrc", "adst", "edge"):
        if got.get(f"d_{k}") is not None:
            r[f"d_{k}"] = GR.ratio(got[f"d_{k}"], ref[f"d_{k}"], ref[f"A_{k}"])
    return r
