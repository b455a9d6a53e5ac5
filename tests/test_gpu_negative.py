"""kgx_negative_edges / NegativeSampler against the numpy restatement (GPU).

The outputs are integers and a pure function of the arguments, so every check
is exact equality with tests/negative_ref.py (itself checked on the CPU by
tests/test_negative_host.py), the fallback and bad-row counters included.
"""

import numpy as np
import pytest
import torch

import negative_ref as NR
from keras_geometric_amd import sampling

pytestmark = pytest.mark.gpu
T = torch.from_numpy

GRAPHS = {"uniform": NR.uniform_graph, "fallback": NR.fallback_graph, "mixed": NR.mixed_graph}


def _np(t):
    return t.detach().cpu().numpy()


def _positives(name, ei, n):
    """(a, keys): destinations and keys of the positives; keys differ from arange."""
    rng = np.random.default_rng(21)
    if name == "mixed":
        ids = rng.permutation(ei.shape[1])[:120]
        a = ei[1][ids].astype(np.int32)
        a[7], a[8] = n, -3  # destinations out of range
        return a, (ids * 7 - 100).astype(np.int32)  # negative keys too
    a = np.zeros(200, np.int32)
    a[150:] = rng.integers(0, n, 50)
    return a, rng.integers(-2**31, 2**31 - 1, 200).astype(np.int32)


@pytest.mark.parametrize("flags", [(True, True), (True, False), (False, True), (False, False)])
@pytest.mark.parametrize("Q", [1, 5])
@pytest.mark.parametrize("name", list(GRAPHS))
def test_equals_restatement(dev, name, Q, flags):
    no_self, reject = flags
    ei, n = GRAPHS[name]()
    rowptr, col = NR.sorted_csr(ei, n)
    a, keys = _positives(name, ei, n)
    kw = dict(max_tries=16 if name == "uniform" else 8, no_self=no_self, reject_edges=reject)
    want, want_stats = NR.negative_edges(rowptr, col, n, n, a, keys, Q, 99, **kw)
    out, stats = sampling.negative_edges(T(rowptr).to(dev), T(col).to(dev), n, n, T(a).to(dev), T(keys).to(dev), Q,
                                         99, **kw)
    assert np.array_equal(_np(out), want)
    assert _np(stats).tolist() == want_stats
    if name == "fallback" and reject:
        assert want_stats[0] > 0
    if name == "mixed":
        assert want_stats[1] == 2
    # ld_out > Q: written in place into columns 1.. of a wider array, the rest untouched
    wide = torch.full((a.shape[0], Q + 3), -7, dtype=torch.int32, device=dev)
    sampling.negative_edges(T(rowptr).to(dev), T(col).to(dev), n, n, T(a).to(dev), T(keys).to(dev), Q, 99,
                            out=wide[:, 1:1 + Q], **kw)
    w = _np(wide)
    assert np.array_equal(w[:, 1:1 + Q], want) and (w[:, 0] == -7).all() and (w[:, 1 + Q:] == -7).all()


def test_empty_batch(dev):
    ei, n = NR.mixed_graph()
    rowptr, col = NR.sorted_csr(ei, n)
    e = torch.empty(0, dtype=torch.int32, device=dev)
    out, stats = sampling.negative_edges(T(rowptr).to(dev), T(col).to(dev), n, n, e, e, 4, 1)
    assert out.shape == (0, 4) and _np(stats).tolist() == [0, 0]


def test_negative_sampler_batches(dev):
    ei, n = NR.mixed_graph()
    rowptr, col = NR.sorted_csr(ei, n)
    s = sampling.NegativeSampler(T(ei).to(dev), n, 5, seed=3, max_tries=16)
    assert np.array_equal(_np(s.col_sorted), col) and np.array_equal(_np(s.graph.rowptr), rowptr)
    ids1 = np.array([5, 300, 17, 42, 399, 0], np.int32)
    ids2 = np.array([42, 8, 5], np.int32)
    b1, b2 = s.sample(ids1), s.sample(T(ids2).to(dev))
    assert b1.a_idx.shape == (6,) and b1.b_idx.shape == (6, 6) and b1.labels.shape == (6, 6)
    assert np.array_equal(_np(b1.a_idx), ei[1][ids1]) and np.array_equal(_np(b1.b_idx[:, 0]), ei[0][ids1])
    lab = _np(b1.labels)
    assert (lab[:, 0] == 1).all() and (lab[:, 1:] == 0).all()
    # the restatement, keyed on the input edge id under epoch_seed(seed, epoch)
    want, want_stats = NR.negative_edges(rowptr, col, n, n, ei[1][ids1], ids1, 5, sampling.epoch_seed(3, 0),
                                         max_tries=16)
    assert np.array_equal(_np(b1.b_idx[:, 1:]), want) and b1.fallbacks() == want_stats[0]
    # a positive draws the same negatives in another batch, at another position
    n1, n2 = _np(b1.b_idx), _np(b2.b_idx)
    assert np.array_equal(n1[3], n2[0]) and np.array_equal(n1[0], n2[2])
    # ... and others at another epoch
    e1 = _np(s.sample(ids1, epoch=1).b_idx)
    assert np.array_equal(e1[:, 0], n1[:, 0]) and not np.array_equal(e1[:, 1:], n1[:, 1:])
    assert np.array_equal(e1, _np(s.sample(ids1, epoch=1).b_idx))
    # relabel: distinct ascending node ids and positions in them
    nodes, a_loc, b_loc = b1.relabel()
    nodes = _np(nodes)
    assert np.array_equal(nodes, np.unique(np.concatenate([_np(b1.a_idx), n1.reshape(-1)])))
    assert np.array_equal(nodes[_np(a_loc)], _np(b1.a_idx)) and np.array_equal(nodes[_np(b_loc)], n1)
    # an edge id out of range: no fault, -1 indices, reported when the counters are read
    bad = s.sample(np.array([1, 400, -1], np.int32))
    assert _np(bad.a_idx).tolist()[1:] == [-1, -1] and (_np(bad.b_idx)[1:] == -1).all()
    with pytest.raises(IndexError, match="edge id"):
        bad.fallbacks()
    assert s.sample(np.empty(0, np.int32)).b_idx.shape == (0, 6)
