"""The dot-product attention restatement of tests/dot_attention_ref.py, checked
on the CPU: pinned against torch's scaled_dot_product_attention, its dispatch
mirror's table, the headroom the fp32 restatement leaves under the bounds the
GPU module holds the kernels to, and the premises of the GPU cases.  Also the
device-free part of TransformerConv: export and config round trip.

Headroom (fp32 restatement against float64, standard-normal q, k, v and
grad_out at scale 1/sqrt(C), both graphs): largest err / bound 0.10 for out
and 0.15 for the gradients (d q 0.15, d k 0.11, d v 0.09) on the inputs of
dot_attention_ref.make_inputs; the GPU module's bounds are the same ones.
"""

from __future__ import annotations

import math

import pytest
import torch

import dot_attention_ref as DR

HEADROOM = 0.5


def test_restatement_equals_sdpa_on_a_simple_graph():
    """Independent pin: on a simple graph (no multi-edges, every destination
    with an in-edge) the restatement is dense attention under the boolean
    adjacency mask."""
    n, H, C = 40, 4, 8
    g = torch.Generator().manual_seed(4040)
    adj = torch.rand(n, n, generator=g) < 0.15  # adj[i, j]: edge j -> i
    adj[torch.arange(n), torch.randint(0, n, (n,), generator=g)] = True  # every destination has an in-edge
    dst, src = torch.nonzero(adj, as_tuple=True)
    perm = torch.randperm(dst.numel(), generator=g)  # input order is not CSR order
    src, dst = src[perm], dst[perm]
    assert int(adj.sum(1).min()) >= 1 and torch.unique(src * n + dst).numel() == src.numel()
    q, k, v = (torch.randn(n, H * C, generator=g, dtype=torch.float64) for _ in range(3))
    got = DR.dot_attention_ref(q, k, v, src, dst, n, H, C)

    def heads_first(t):
        return t.reshape(n, H, C).permute(1, 0, 2)[None]  # [1, H, n, C]

    want = torch.nn.functional.scaled_dot_product_attention(heads_first(q), heads_first(k), heads_first(v),
                                                            attn_mask=adj[None, None])
    want = want[0].permute(1, 0, 2).reshape(n, H * C)
    assert want.dtype == torch.float64
    assert float((got - want).abs().max()) <= 1e-12


def test_dispatch_mirror_table():
    for (h, c), want in DR.LAYOUTS.items():
        assert DR.layout(h, c) == want, (h, c)
    assert set(DR.SHAPES) | set(DR.ODD_SHAPES) == set(DR.LAYOUTS)
    # more than 64 lanes per row at the widest K: unsupported
    assert DR.layout(16, 128) is None and DR.layout(64, 33) is None
    # 16 x 64 fits at K = 16 with float4 loads, and only then
    assert DR.layout(16, 64) == (16, 4) and DR.layout(16, 64, aligned=4) is None
    # k and v as the column halves of one [n, 2 H C] tensor keep the float4 layout when H C % 4 == 0
    assert DR.layout(8, 16, ld=256) == (8, 2) and DR.layout(3, 6, ld=36, aligned=8) == (2, 4)


def _headroom_cases():
    for name in ("small", "deep"):
        for h, c in DR.SHAPES:
            yield name, h, c
    yield "small", 3, 6  # the shape added for the scalar / float2 paths


@pytest.mark.parametrize("name,heads,channels", list(_headroom_cases()),
                         ids=[f"{n}-{h}x{c}" for n, h, c in _headroom_cases()])
def test_fp32_restatement_headroom(name, heads, channels):
    """The fp32 run of the restatement stays within HEADROOM of the bounds on
    every shape the GPU module uses, so the bounds are not the kernels' own error."""
    src, dst, _, n_dst = DR.make_graph(name)
    x = DR.make_inputs(name, heads, channels)
    ref = DR.reference(name, heads, channels)
    got = DR.dot_attention_grads(torch.float32, x["q"], x["k"], x["v"], src, dst, n_dst, heads, channels, x["gout"])
    r = DR.ratios(got, ref)
    print(f"{name} {heads}x{channels}: fp32 restatement err / bound " + ", ".join(f"{k} {v:.3f}" for k, v in r.items()))
    assert all(v <= HEADROOM for v in r.values()), r


def test_empty_rows_in_the_restatement():
    src, dst, n_src, n_dst = DR.make_graph("small")
    assert not bool((dst == 0).any()) and not bool((src == n_src - 1).any())
    ref = DR.reference("small", 8, 16)
    assert not bool(ref["out"][0].any()) and not bool(ref["d_q"][0].any())
    assert not bool(ref["d_k"][n_src - 1].any()) and not bool(ref["d_v"][n_src - 1].any())
    for v in ref.values():
        assert bool(torch.isfinite(v).all())


@pytest.mark.parametrize("heads,channels", DR.DOMINANT_SHAPES)
def test_dominant_edge_premise(heads, channels):
    """The dominant edge's score exceeds every other score of the hub row by about DOMINANT_GAP."""
    x = DR.dominant_inputs(heads, channels)
    src, dst, _, _ = DR.dominant_graph(DR.DOMINANT_POS["slot17"])
    row = torch.nonzero(dst == DR.HUB_DST).flatten()
    assert row.numel() == 1000 and int((src[row] == DR.DOMINANT_SRC).sum()) == 1
    q = x["q"].double().reshape(-1, heads, channels)[DR.HUB_DST]
    k = x["k"].double().reshape(-1, heads, channels)[src[row]]
    s = (q[None] * k).sum(-1) / math.sqrt(channels)  # [1000, H]
    dom = src[row] == DR.DOMINANT_SRC
    assert float((s[dom] - DR.DOMINANT_GAP).abs().max()) < 1e-4
    gap = s[dom].min() - s[~dom].max()
    assert DR.DOMINANT_GAP - 6 < float(gap) < DR.DOMINANT_GAP + 6


def test_transformer_conv_is_exported_and_config_round_trips():
    import keras_geometric_amd as kgx
    from keras_geometric_amd import layers

    assert "TransformerConv" in kgx.__all__ and "TransformerConv" in layers.__all__
    assert kgx.TransformerConv is layers.TransformerConv
    layer = kgx.TransformerConv(16, heads=4, concat=False, beta=True, dropout=0.25, root_weight=True,
                                use_bias=False, name="tc")
    cfg = layer.get_config()
    for key, want in (("output_dim", 16), ("heads", 4), ("concat", False), ("beta", True), ("dropout", 0.25),
                      ("root_weight", True), ("use_bias", False), ("name", "tc")):
        assert cfg[key] == want, key
    again = kgx.TransformerConv.from_config(cfg)
    assert again.get_config() == cfg
    assert not again.built  # no device was needed
    with pytest.raises(ValueError):
        kgx.TransformerConv(8, dropout=1.0)
