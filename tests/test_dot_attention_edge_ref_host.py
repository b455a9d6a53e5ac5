"""The restatement of the dot-product attention with edge features
(tests/dot_attention_edge_ref.py) pinned on the CPU:

  * on the expanded graph -- one source per edge, k' = k[src] + e, v' = v[src]
    + e, src' = arange(E) -- the EXISTING dot_attention_ref (itself pinned to
    scaled_dot_product_attention by tests/test_dot_attention_ref_host.py) gives
    the same fp32 bits;
  * e = 0 is dot_attention_ref;
  * its fp32 run stays within 0.5 of every bound the GPU module holds the
    kernels to, against its float64 run, on that module's inputs: a condition
    of those bounds, asserted (largest here: out 0.13, d q 0.19, d k 0.08,
    d v 0.05, d e 0.11, all at 8 x 64 on `deep`);
  * the layer-level restatement (TransformerConv with edge_dim) in fp32 stays
    within 0.5 of the layer bound |got - ref| <= 1e-5 max(1, |ref|) at the
    cotangent N(0, 1/16) of tests/test_gpu_transformer_conv.py, five seeds,
    every configuration of tests/test_gpu_transformer_conv_edge.py (largest
    here: lin_edge.kernel 0.17, d edge_attr 0.02, lin_beta.kernel 0.18), so
    lin_edge.kernel and d edge_attr are held to the plain layer bound there.
"""

from __future__ import annotations

import pytest
import torch

import dot_attention_edge_ref as ER
import dot_attention_ref as DR

_LANE_SHAPES = DR.SHAPES + [(3, 6)]
_CASES = [("small", h, c) for h, c in _LANE_SHAPES] + [("deep", h, c) for h, c in DR.DEEP_SHAPES]
_IDS = [f"{n}-{h}x{c}" for n, h, c in _CASES]


def _inputs(name, heads, channels):
    src, dst, _, n_dst = DR.make_graph(name)
    return DR.make_inputs(name, heads, channels), ER.make_edge(name, heads, channels), src, dst, n_dst


@pytest.mark.parametrize("name,heads,channels", _CASES, ids=_IDS)
def test_equals_the_no_edge_restatement_on_the_expanded_graph(name, heads, channels):
    x, e, src, dst, n_dst = _inputs(name, heads, channels)
    got = ER.dot_attention_edge_ref(x["q"], x["k"], x["v"], e, src, dst, n_dst, heads, channels)
    k2, v2, src2 = ER.expanded(x["k"], x["v"], e, src, heads, channels)
    want = DR.dot_attention_ref(x["q"], k2, v2, src2, dst, n_dst, heads, channels)
    assert got.dtype == torch.float32 and torch.equal(got, want)


@pytest.mark.parametrize("name,heads,channels", [("small", 8, 16), ("small", 3, 6), ("deep", 8, 64)])
def test_zero_edge_table_is_the_no_edge_restatement(name, heads, channels):
    x, e, src, dst, n_dst = _inputs(name, heads, channels)
    got = ER.dot_attention_edge_ref(x["q"], x["k"], x["v"], torch.zeros_like(e), src, dst, n_dst, heads, channels)
    assert torch.equal(got, DR.dot_attention_ref(x["q"], x["k"], x["v"], src, dst, n_dst, heads, channels))


def test_float64_reference_sums_its_per_edge_leaves():
    """d e of the per-edge reference is plain float64 autograd's; A_e bounds it."""
    x, e, src, dst, n_dst = _inputs("small", 3, 12)
    ref = ER.reference("small", 3, 12)
    plain = ER.dot_attention_edge_grads(torch.float64, x["q"], x["k"], x["v"], e, src, dst, n_dst, 3, 12, x["gout"])
    for key in ("out", "d_q", "d_k", "d_v", "d_e"):
        assert torch.allclose(ref[key], plain[key], rtol=1e-12, atol=1e-12), key
    assert bool((ref["A_e"] >= ref["d_e"].abs() - 1e-12).all())


_WORST: dict = {}


@pytest.mark.parametrize("name,heads,channels", _CASES, ids=_IDS)
def test_fp32_restatement_is_within_half_of_the_bounds(name, heads, channels):
    x, e, src, dst, n_dst = _inputs(name, heads, channels)
    got = ER.dot_attention_edge_grads(torch.float32, x["q"], x["k"], x["v"], e, src, dst, n_dst, heads, channels,
                                      x["gout"])
    r = ER.ratios(got, ER.reference(name, heads, channels))
    for k, v in r.items():
        _WORST[k] = max(_WORST.get(k, 0.0), v)
    msg = f"{name} {heads}x{channels}: fp32 err / bound " + ", ".join(f"{k} {v:.3f}" for k, v in r.items())
    print(msg + " | worst so far " + ", ".join(f"{k} {v:.3f}" for k, v in _WORST.items()))
    assert set(r) == {"out", "d_q", "d_k", "d_v", "d_e"}
    assert all(v <= 0.5 for v in r.values()), msg


# ---------------------------------------------------------------------------
# layer level
# ---------------------------------------------------------------------------
LAYER_CASES = {
    "concat": (dict(heads=4, channels=16, concat=True, root_weight=True, beta=False), 8),
    "mean": (dict(heads=4, channels=16, concat=False, root_weight=True, beta=False), 8),
    "beta": (dict(heads=4, channels=16, concat=True, root_weight=True, beta=True), 8),
    "noroot": (dict(heads=4, channels=16, concat=True, root_weight=False, beta=False), 8),
    "edge-dim-3": (dict(heads=4, channels=16, concat=True, root_weight=True, beta=False), 3),
    "hc256": (dict(heads=4, channels=64, concat=True, root_weight=True, beta=True), 8),
}
F_IN, COT, TOL = 16, 0.25, 1e-5  # tests/test_gpu_transformer_conv.py


def _layer_ratio(got, ref):
    got, ref = got.double(), ref.double()
    return float(((got - ref).abs() / (TOL * ref.abs().clamp_min(1.0))).max())


@pytest.mark.parametrize("case", list(LAYER_CASES))
def test_layer_restatement_fp32_is_within_half_of_the_layer_bound(case):
    cfg, edge_dim = LAYER_CASES[case]
    ei = ER.square_graph()
    assert ei.shape == (2, 560)
    od = cfg["heads"] * cfg["channels"] if cfg["concat"] else cfg["channels"]
    worst = {}
    for seed in range(5):
        g = torch.Generator().manual_seed(1000 + seed)
        x = torch.randn(64, F_IN, generator=g)
        ea = torch.randn(ei.shape[1], edge_dim, generator=g)
        W = ER.layer_weights(seed, cfg, F_IN, F_IN, edge_dim)
        gout = COT * torch.randn(64, od, generator=g)
        o64, g64, e64 = ER.layer_ref(torch.float64, W, cfg, x, x, ea, ei[0], ei[1], gout)
        o32, g32, e32 = ER.layer_ref(torch.float32, W, cfg, x, x, ea, ei[0], ei[1], gout)
        r = {"out": _layer_ratio(o32, o64), "d edge_attr": _layer_ratio(e32, e64)}
        r.update({n: _layer_ratio(g32[n], g64[n]) for n in g64})
        assert "lin_edge.kernel" in r and bool(g64["lin_edge.kernel"].any()) and bool(e64.any())
        for k, v in r.items():
            worst[k] = max(worst.get(k, 0.0), v)
    msg = f"{case}: fp32 err / layer bound over five seeds " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items())
    print(msg)
    assert all(v <= 0.5 for v in worst.values()), msg
