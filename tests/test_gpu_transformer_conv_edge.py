"""TransformerConv(edge_dim=...) on the GPU against the float64 restatement of
PyG's TransformerConv with edge features (dot_attention_edge_ref.layer_ref)
that uses the layer's own weights:

    eps = edge_attr W_e                                   lin_edge, no bias
    out = dot_attention_edge_ref(q, k, v, eps)            k_j + eps_e, v_j + eps_e
    then the skip / beta terms of tests/test_gpu_transformer_conv.py

The graph (64 nodes, 560 edges), the F_IN = 16 inputs, the cotangent N(0, 1/16)
and the bound |got - ref| <= 1e-5 * max(1, |ref|) are that module's.  Forward,
every parameter gradient (lin_edge.kernel included) and d edge_attr are
checked; tests/test_dot_attention_edge_ref_host.py asserts that the fp32 run of
the restatement stays within 0.5 of this bound for all of them.  The largest
err / bound this module printed on an MI355X is 0.50 (d lin_beta at H*C = 256, a
parameter upstream of the edge path); lin_edge.kernel stayed at or below 0.16
and d edge_attr at or below 0.011.
"""

from __future__ import annotations

import numpy as np
import pytest
import torch

import dot_attention_edge_ref as ER
import dot_attention_ref as DR
import keras_geometric_amd as kgx
from keras_geometric_amd import ops as kops

pytestmark = pytest.mark.gpu

TOL = 1e-5
F_IN = 16
COT = 0.25
_WORST = [0.0]


def _randomise(layer, seed):
    """Glorot kernels as built; biases (zeros as built) reseeded so no term is trivial."""
    g = torch.Generator().manual_seed(seed)
    ws = [w if w.ndim == 2 else 0.5 * torch.randn(w.shape, generator=g).numpy() for w in layer.get_weights()]
    layer.set_weights(ws)


def _names(layer):
    names = []
    for lin in ER.LAYER_NAMES:
        d = getattr(layer, lin)
        if d is not None:
            names += [f"{lin}.kernel"] + ([f"{lin}.bias"] if d.use_bias else [])
    return names


def _ratio(got, ref):
    got, ref = got.detach().double().cpu(), ref.double()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    r = ((got - ref).abs() / (TOL * ref.abs().clamp_min(1.0)))
    return float("inf") if bool(torch.isnan(r).any()) else float(r.max())


def _check_layer(label, layer, make_inputs, x_i, x_j, edge_attr, src, dst, seed=3):
    """make_inputs(edge_attr leaf on the device) -> (inputs, kwargs) of the layer call."""
    ea = edge_attr.to(x_i.device).requires_grad_(True)
    inputs, kwargs = make_inputs(ea)
    with torch.no_grad():
        layer(inputs, **kwargs)  # build
    _randomise(layer, seed)
    for p in layer.parameters():
        p.grad = None
    out = layer(inputs, **kwargs)
    g = torch.Generator().manual_seed(seed + 1)
    gout = COT * torch.randn(out.shape, generator=g)
    out.backward(gout.to(out.device))
    names = _names(layer)
    assert names[-1] == "lin_edge.kernel" and len(names) == len(layer.weights)
    W = {n: torch.from_numpy(w) for n, w in zip(names, layer.get_weights())}
    cfg = dict(heads=layer.heads, channels=layer.output_dim, concat=layer.concat, root_weight=layer.root_weight,
               beta=layer.beta)
    ref, grads, d_ea = ER.layer_ref(torch.float64, W, cfg, x_i, x_j, edge_attr, src, dst, gout)
    r = {"out": _ratio(out, ref), "d edge_attr": _ratio(ea.grad, d_ea)}
    for name, p in zip(names, layer.weights):
        assert p.grad is not None, name
        r[name] = _ratio(p.grad, grads[name])
    assert bool(grads["lin_edge.kernel"].any()) and bool(d_ea.any())
    _WORST[0] = max(_WORST[0], max(r.values()))
    msg = f"{label}: err / bound " + ", ".join(f"{k} {v:.3f}" for k, v in r.items())
    print(msg + f" | worst so far {_WORST[0]:.3f}")
    assert all(v <= 1.0 for v in r.values()), msg
    return out


def _square(dev, edge_dim, seed):
    ei = ER.square_graph()
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(64, F_IN, generator=g).to(dev)
    ea = torch.randn(ei.shape[1], edge_dim, generator=g)
    return ei, x, ea


CONFIGS = {
    "concat": dict(heads=4, concat=True),
    "mean": dict(heads=4, concat=False),
    "beta": dict(heads=4, beta=True),
    "noroot": dict(heads=4, root_weight=False),
}


@pytest.mark.parametrize("name", list(CONFIGS))
def test_configurations(dev, name):
    ei, x, ea = _square(dev, 8, 21)
    layer = kgx.TransformerConv(16, edge_dim=8, **CONFIGS[name])
    out = _check_layer(name, layer, lambda e: ([x, ei.to(dev)], dict(edge_attr=e)), x, x, ea, ei[0], ei[1])
    assert out.shape == (64, layer._out_dim())
    assert layer.lin_edge.kernel.shape == (8, 64) and layer.lin_edge.bias is None
    assert kops.dense_supported(ea.to(dev), layer.lin_edge.kernel)


def test_edge_dim_not_a_multiple_of_four(dev):
    ei, x, ea = _square(dev, 3, 22)
    layer = kgx.TransformerConv(16, heads=4, edge_dim=3)
    _check_layer("edge_dim 3", layer, lambda e: ([x, ei.to(dev)], dict(edge_attr=e)), x, x, ea, ei[0], ei[1])
    assert not kops.dense_supported(ea.to(dev), layer.lin_edge.kernel)  # lin_edge went through torch's GEMM


def test_wide_heads(dev):
    """H * C = 256: 16 channels per lane."""
    ei, x, ea = _square(dev, 8, 23)
    layer = kgx.TransformerConv(64, heads=4, beta=True, edge_dim=8)
    _check_layer("H*C 256", layer, lambda e: ([x, ei.to(dev)], dict(edge_attr=e)), x, x, ea, ei[0], ei[1])


def test_pair_input_on_a_bipartite_graph(dev):
    src, dst, n_src, n_dst = DR.make_graph("small")
    g = torch.Generator().manual_seed(24)
    x_i, x_j = torch.randn(n_dst, F_IN, generator=g).to(dev), torch.randn(n_src, 24, generator=g).to(dev)
    ea = torch.randn(src.numel(), 8, generator=g)
    layer = kgx.TransformerConv(16, heads=4, beta=True, edge_dim=8)
    ei = torch.stack([src, dst]).to(dev)
    out = _check_layer("pair", layer, lambda e: ([(x_i, x_j), ei], dict(edge_attr=e)), x_i, x_j, ea, src, dst)
    assert out.shape == (n_dst, 64)


def test_sampled_block(dev):
    n, E = 300, 3000
    rng = np.random.default_rng(17)
    ei = torch.from_numpy(np.stack([rng.integers(0, n, E), rng.integers(0, n, E)]).astype(np.int32)).to(dev)
    sampler = kgx.NeighborSampler(ei, n, [4, 3], seed=5)
    blocks = sampler.sample_blocks(torch.arange(40, dtype=torch.int32, device=dev), epoch=1)
    blk = blocks[0]
    assert blk.n_src > blk.n_dst > 0 and blk.edge_index.shape[1] > 0
    g = torch.Generator().manual_seed(25)
    x = torch.randn(blk.n_src, F_IN, generator=g).to(dev)
    ea_full = torch.randn(E, 8, generator=g)
    ea = ea_full[blk.edge_ids.long().cpu()]  # one row per block edge, in the block's edge order
    layer = kgx.TransformerConv(16, heads=4, edge_dim=8)
    le = blk.edge_index.long().cpu()
    out = _check_layer("block", layer, lambda e: ([x, blk], dict(edge_attr=e)), x[: blk.n_dst], x, ea, le[0], le[1])
    assert out.shape == (blk.n_dst, 64)
    with pytest.raises(ValueError, match="edge_attr"):
        layer([x, blk], edge_attr=ea_full.to(dev))


def test_three_element_input_list(dev):
    ei, x, ea = _square(dev, 8, 26)
    layer = kgx.TransformerConv(16, heads=4, edge_dim=8)
    out = _check_layer("list", layer, lambda e: ([x, ei.to(dev), e], {}), x, x, ea, ei[0], ei[1])
    with torch.no_grad():
        assert torch.equal(layer([x, ei.to(dev)], edge_attr=ea.to(dev)), out)


def test_config_round_trip(dev):
    ei, x, ea = _square(dev, 8, 27)
    ei, ea = ei.to(dev), ea.to(dev)
    layer = kgx.TransformerConv(16, heads=4, concat=False, beta=True, dropout=0.1, edge_dim=8)
    with torch.no_grad():
        y = layer([x, ei], edge_attr=ea)
        cfg = layer.get_config()
        assert cfg["edge_dim"] == 8
        again = kgx.TransformerConv.from_config(cfg)
        assert again.get_config() == cfg
        again([x, ei, ea])
        again.set_weights(layer.get_weights())
        assert torch.equal(again([x, ei, ea]), y)
    # a layer without edge_dim keeps its weights' names and order, and says so in its config
    plain = kgx.TransformerConv(16, heads=4, beta=True)
    plain([x, ei])
    assert plain.get_config()["edge_dim"] is None and plain.lin_edge is None
    assert [tuple(w.shape) for w in plain.get_weights()] == [
        (16, 64), (64,), (16, 64), (64,), (16, 64), (64,), (16, 64), (64,), (192, 1)]


def test_edge_attr_errors(dev):
    ei, x, ea = _square(dev, 8, 28)
    ei, ea = ei.to(dev), ea.to(dev)
    layer = kgx.TransformerConv(16, heads=4, edge_dim=8)
    with pytest.raises(ValueError, match="edge_attr"):
        layer([x, ei])  # missing
    with pytest.raises(ValueError, match="edge_attr"):
        layer([x, ei], edge_attr=ea[:, :7])  # wrong width
    with pytest.raises(ValueError, match="edge_attr"):
        layer([x, ei, ea[:-1]])  # wrong row count
    plain = kgx.TransformerConv(16, heads=4)
    with pytest.raises(NotImplementedError, match="edge"):
        plain([x, ei], edge_attr=ea)
    with pytest.raises(NotImplementedError, match="edge"):
        plain([x, ei, ea])
