"""Link prediction end to end on the GPU: DotProductDecoder on an EdgeBatch and
on an edge_index, its config round trip, and one tiny training step (SAGEConv
encoder on a sampled subgraph, decoder, BCE with logits) whose gradients are
finite and bit-identical over two runs from the same seeds.
"""

import dataclasses

import numpy as np
import pytest
import torch

import edge_dot_ref as ER
import keras_geometric_amd as kgx
from keras_geometric_amd import layers, sampling

pytestmark = pytest.mark.gpu
T = torch.from_numpy
N, E, F = 200, 1200, 24


def _np(t):
    return t.detach().cpu().numpy()


@pytest.fixture(scope="module")
def data():
    rng = np.random.default_rng(13)
    ei = np.stack([rng.integers(0, N, E), rng.integers(0, N, E)]).astype(np.int32)
    x = rng.standard_normal((N, F)).astype(np.float32)
    return ei, x


def _within_bound(got, z_dst, z_src, a, b):
    s64, mag = ER.edge_dot(z_dst, z_src, a, b)
    return (np.abs(_np(got).astype(np.float64).reshape(s64.shape) - s64) <= ER.bound(z_dst.shape[1], mag)).all()


def test_decoder_on_edge_batch(dev, data):
    ei, x = data
    z = T(x).to(dev)
    batch = sampling.NegativeSampler(T(ei).to(dev), N, 4, seed=1).sample(np.arange(0, 300, 3, dtype=np.int32))
    dec = layers.DotProductDecoder()
    s = dec([z, batch])
    assert s.shape == (100, 5) and batch.fallbacks() >= 0
    assert _within_bound(s, x, x, _np(batch.a_idx), _np(batch.b_idx))
    # a pair (z_dst, z_src), and the logistic output
    x2 = np.random.default_rng(1).standard_normal((N, F)).astype(np.float32)
    s2 = dec([(z, T(x2).to(dev)), batch])
    assert _within_bound(s2, x, x2, _np(batch.a_idx), _np(batch.b_idx))
    p = layers.DotProductDecoder(sigmoid=True)([z, batch])
    assert torch.equal(p, torch.sigmoid(s))


def test_decoder_on_edge_index(dev, data):
    ei, x = data
    z = T(x).to(dev)
    dei = T(ei).to(dev)
    s = kgx.DotProductDecoder()([z, dei])
    assert s.shape == (E,)
    assert _within_bound(s, x, x, ei[1], ei[0])  # score of (s -> d) = z[d] . z[s], in input-edge order
    assert torch.equal(s, kgx.ops.edge_dot(z, z, dei[1], dei[0]))


def test_decoder_config_round_trip():
    dec = layers.DotProductDecoder(sigmoid=True, name="scores")
    cfg = dec.get_config()
    assert cfg["sigmoid"] is True and cfg["name"] == "scores"
    again = layers.DotProductDecoder.from_config(cfg)
    assert again.sigmoid is True and again.get_config() == cfg
    assert layers.DotProductDecoder().get_config()["sigmoid"] is False


def _step(dev, ei, x):
    layers.set_random_seed(5)
    dei = T(ei).to(dev)
    neg = sampling.NegativeSampler(dei, N, 4, seed=2)
    nbr = sampling.NeighborSampler(dei, N, fanouts=[5], seed=2)
    batch = neg.sample(np.arange(10, 74, dtype=np.int32), epoch=1)
    nodes, a_loc, b_loc = batch.relabel()
    sub = nbr.sample(nodes, epoch=1)
    enc = layers.SAGEConv(16)
    h = enc([sub.gather(T(x).to(dev)), sub.edge_index])[: sub.n_seeds]
    local = dataclasses.replace(batch, a_idx=a_loc, b_idx=b_loc)  # shares batch.extras: the cache is keyed
    logits = layers.DotProductDecoder()([h, local])
    loss = torch.nn.functional.binary_cross_entropy_with_logits(logits, batch.labels)
    loss.backward()
    assert batch.fallbacks() == 0
    return float(loss.detach()), [_np(p.grad) for p in enc.parameters()]


def test_tiny_training_step_is_deterministic(dev, data):
    ei, x = data
    loss1, g1 = _step(dev, ei, x)
    loss2, g2 = _step(dev, ei, x)
    assert np.isfinite(loss1) and loss1 == loss2
    assert len(g1) >= 2
    assert any(np.abs(a).max() > 0 for a in g1)
    for a, b in zip(g1, g2):
        assert np.isfinite(a).all()
        assert np.array_equal(a.view(np.int32), b.view(np.int32))
