"""TransformerConv on the GPU against a float64 restatement of PyG's
TransformerConv (no edge features) that uses the layer's own weights:

    q = x_i W_q + b_q,  k = x_j W_k + b_k,  v = x_j W_v + b_v
    out = dot_attention_ref(q, k, v)           heads concatenated, or their mean
    r = x_i W_s + b_s                          root_weight
    out = b r + (1 - b) out,  b = sigmoid([out, r, out - r] w_b)      beta
    out = out + r                              root_weight without beta

Forward and every parameter gradient are held to the layer-level bound of
tests/test_gpu_layers.py (assert_tol): |got - ref| <= 1e-5 * max(1, |ref|).
Inputs are standard normal with 16 features, glorot kernels and N(0, 1/4)
biases.  The cotangent is N(0, 1/16): with a unit cotangent the fp32 run of
the restatement itself reaches 0.68 of the bound for d lin_beta (the gate's
logit gradient sums gout * (r - out) over every output column, and the sum
over the nodes reaches 20-30, where the bound is relative), and the layer
measured 0.89 there; at 1/16 the fp32 restatement stays at or below 0.21 for
every parameter at H*C = 64 and 256 (five seeds).  The largest err / bound this
module printed on an MI355X is 0.21 (d lin_beta, H*C = 256).
"""

from __future__ import annotations

import numpy as np
import pytest
import torch

import dot_attention_ref as DR
import keras_geometric_amd as kgx
from keras_geometric_amd import _native as nat

pytestmark = pytest.mark.gpu

TOL = 1e-5  # tests/test_gpu_layers.py assert_tol
F_IN = 16
COT = 0.25  # cotangent ~ N(0, 1/16), see the module docstring
_WORST = [0.0]


def _square_graph(n=64, e=500, seed=31):
    """Seeded [2, E] int64 graph on n nodes: multi-edges, node 0 without in-edges, node 5 a small hub."""
    rng = np.random.default_rng(seed)
    src = np.concatenate([rng.integers(0, n, e), rng.integers(0, n, 60)])
    dst = np.concatenate([rng.integers(1, n, e), np.full(60, 5)])
    return torch.from_numpy(np.stack([src, dst])).long()


def _randomise(layer, seed):
    """Glorot kernels as built; biases (zeros as built) and everything else reseeded so no term is trivial."""
    g = torch.Generator().manual_seed(seed)
    ws = [w if w.ndim == 2 else 0.5 * torch.randn(w.shape, generator=g).numpy() for w in layer.get_weights()]
    layer.set_weights(ws)


def _names(layer):
    names = []
    for lin in ("lin_query", "lin_key", "lin_value", "lin_skip", "lin_beta"):
        d = getattr(layer, lin)
        if d is not None:
            names += [f"{lin}.kernel"] + ([f"{lin}.bias"] if d.use_bias else [])
    return names


def _reference(layer, x_i, x_j, src, dst, gout):
    """float64 restatement with the layer's weights: (out, {name: grad})."""
    H, C = layer.heads, layer.output_dim
    W = {n: torch.from_numpy(w).double().requires_grad_(True) for n, w in zip(_names(layer), layer.get_weights())}
    assert len(W) == len(layer.get_weights())
    x_i, x_j = x_i.double().cpu(), x_j.double().cpu()

    def lin(name, x):
        y = x @ W[f"{name}.kernel"]
        return y + W[f"{name}.bias"] if f"{name}.bias" in W else y

    n = x_i.shape[0]
    out = DR.dot_attention_ref(lin("lin_query", x_i), lin("lin_key", x_j), lin("lin_value", x_j), src, dst, n, H, C)
    if not layer.concat:
        out = out.reshape(n, H, C).mean(1)
    if layer.root_weight:
        r = lin("lin_skip", x_i)
        if layer.beta:
            b = torch.sigmoid(torch.cat([out, r, out - r], -1) @ W["lin_beta.kernel"])
            out = b * r + (1 - b) * out
        else:
            out = out + r
    out.backward(gout.double().cpu())
    return out.detach(), {n: w.grad for n, w in W.items()}


def _ratio(got, ref):
    got, ref = got.detach().double().cpu(), ref.double()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    r = ((got - ref).abs() / (TOL * ref.abs().clamp_min(1.0)))
    return float("inf") if bool(torch.isnan(r).any()) else float(r.max())


def _check_layer(label, layer, inputs, x_i, x_j, src, dst, seed=3):
    layer(inputs)  # build
    _randomise(layer, seed)
    for p in layer.parameters():
        p.grad = None
    out = layer(inputs)
    g = torch.Generator().manual_seed(seed + 1)
    gout = COT * torch.randn(out.shape, generator=g)
    out.backward(gout.to(out.device))
    ref, grads = _reference(layer, x_i, x_j, src, dst, gout)
    r = {"out": _ratio(out, ref)}
    for name, p in zip(_names(layer), layer.weights):
        assert p.grad is not None, name
        r[name] = _ratio(p.grad, grads[name])
    _WORST[0] = max(_WORST[0], max(r.values()))
    msg = f"{label}: err / bound " + ", ".join(f"{k} {v:.3f}" for k, v in r.items())
    print(msg + f" | worst so far {_WORST[0]:.3f}")
    assert all(v <= 1.0 for v in r.values()), msg
    return out


CONFIGS = {
    "concat": dict(heads=4, concat=True),
    "mean": dict(heads=4, concat=False),
    "noroot": dict(heads=4, root_weight=False),
    "beta": dict(heads=4, beta=True),
    "beta-mean": dict(heads=4, concat=False, beta=True),
    "nobias": dict(heads=4, use_bias=False, beta=True),
    "one-head": dict(heads=1),
}


@pytest.mark.parametrize("name", list(CONFIGS))
def test_configurations_single_dense_path(dev, name):
    """H * C = 64: key and value come from one kgx_dense with [W_k | W_v]."""
    ei = _square_graph()
    x = torch.randn(64, F_IN, generator=torch.Generator().manual_seed(11)).to(dev)
    layer = kgx.TransformerConv(64 // CONFIGS[name]["heads"], **CONFIGS[name])
    out = _check_layer(name, layer, [x, ei.to(dev)], x, x, ei[0], ei[1])
    assert out.shape == (64, layer._out_dim())
    k, v = layer._key_value(x)
    assert k.untyped_storage().data_ptr() == v.untyped_storage().data_ptr() and k.stride(0) == 128
    if not layer.root_weight:
        assert not bool(out[0].any())  # node 0 has no in-edge and no skip term


@pytest.mark.parametrize("beta", [False, True], ids=["plain", "beta"])
def test_two_call_path(dev, beta):
    """H * C = 256: [W_k | W_v] would be 512 columns, past KGX_DENSE_MAX_N; two transforms."""
    ei = _square_graph()
    x = torch.randn(64, F_IN, generator=torch.Generator().manual_seed(12)).to(dev)
    layer = kgx.TransformerConv(64, heads=4, beta=beta)
    assert 2 * 256 > nat.DENSE_MAX_N
    _check_layer("two-call", layer, [x, ei.to(dev)], x, x, ei[0], ei[1])
    k, v = layer._key_value(x)
    assert k.untyped_storage().data_ptr() != v.untyped_storage().data_ptr() and k.is_contiguous()


def test_pair_input_on_a_bipartite_graph(dev):
    src, dst, n_src, n_dst = DR.make_graph("small")
    g = torch.Generator().manual_seed(13)
    x_i, x_j = torch.randn(n_dst, F_IN, generator=g).to(dev), torch.randn(n_src, 24, generator=g).to(dev)
    layer = kgx.TransformerConv(16, heads=4, beta=True)
    ei = torch.stack([src, dst]).to(dev)
    out = _check_layer("pair", layer, [(x_i, x_j), ei], x_i, x_j, src, dst)
    assert out.shape == (n_dst, 64)
    assert layer.lin_query.kernel.shape[0] == F_IN and layer.lin_key.kernel.shape[0] == 24


def test_sampled_block(dev):
    n = 300
    rng = np.random.default_rng(17)
    ei = torch.from_numpy(np.stack([rng.integers(0, n, 3000), rng.integers(0, n, 3000)]).astype(np.int32)).to(dev)
    sampler = kgx.NeighborSampler(ei, n, [4, 3], seed=5)
    blocks = sampler.sample_blocks(torch.arange(40, dtype=torch.int32, device=dev), epoch=1)
    blk = blocks[0]
    assert blk.n_src > blk.n_dst > 0 and blk.edge_index.shape[1] > 0
    x = torch.randn(blk.n_src, F_IN, generator=torch.Generator().manual_seed(14)).to(dev)
    layer = kgx.TransformerConv(16, heads=4)
    le = blk.edge_index.long().cpu()
    out = _check_layer("block", layer, [x, blk], x[: blk.n_dst], x, le[0], le[1])
    assert out.shape == (blk.n_dst, 64)
    with pytest.raises(ValueError, match="n_src"):
        layer([x[:-1], blk])


def test_attention_dropout_only_in_training(dev):
    ei = _square_graph().to(dev)
    x = torch.randn(64, F_IN, generator=torch.Generator().manual_seed(15)).to(dev)
    layer = kgx.TransformerConv(16, heads=4, dropout=0.5, root_weight=False)
    with torch.no_grad():
        a, b = layer([x, ei]), layer([x, ei], training=False)
        c = layer([x, ei], training=True)
    assert torch.equal(a, b)
    assert bool(torch.isfinite(c).all()) and not torch.equal(a, c)


def test_config_round_trip_and_edge_attr(dev):
    ei = _square_graph().to(dev)
    x = torch.randn(64, F_IN, generator=torch.Generator().manual_seed(16)).to(dev)
    layer = kgx.TransformerConv(16, heads=4, concat=False, beta=True, dropout=0.1)
    y = layer([x, ei])
    again = kgx.TransformerConv.from_config(layer.get_config())
    assert again.get_config() == layer.get_config()
    again([x, ei])
    again.set_weights(layer.get_weights())
    assert torch.equal(again([x, ei]), y)
    ea = torch.zeros(ei.shape[1], 3, device=dev)
    with pytest.raises(NotImplementedError, match="edge"):
        layer([x, ei], edge_attr=ea)
    with pytest.raises(NotImplementedError, match="edge"):
        layer([x, ei, ea])
