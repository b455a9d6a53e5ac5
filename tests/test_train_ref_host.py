"""tests/train_ref.py (the class graph and the float64 training-step reference
of tests/test_gpu_train_step.py) checked on the CPU: the recipe's class
counts, `grads` against float32 autograd through the oracle's GCN and GIN
forwards, and fused_ref.reference unchanged by returning its aggregate."""

import numpy as np
import pytest
import torch

import fused_ref
import train_ref
from oracle import reference as R
from oracle.rmat import rmat_edges, scale_for
from test_fused_ref_host import _case

T = torch.from_numpy


def test_class_graph_seed0_counts():
    src, dst = train_ref.class_graph(0)
    N = train_ref.CLASS_N
    assert src.size == dst.size == 73142
    want = {"hub": 2, "main": 1400, "short": 1400, "two": 4400, "one": 4400, "zero": 686}
    assert train_ref.class_counts(np.bincount(dst, minlength=N)) == want
    assert train_ref.class_counts(np.bincount(src, minlength=N)) == want
    pairs = set(zip(src.tolist(), dst.tolist()))
    assert len(pairs) == 72163
    assert sum((d, s) in pairs for s, d in pairs) == 33  # not symmetric: a missing transposition shows
    # in-degrees follow the node id, out-degrees do not
    assert np.bincount(dst, minlength=N)[:2].tolist() == [1061, 517]
    assert np.bincount(src, minlength=N)[:2].tolist() != [1061, 517]


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_class_graph_reaches_every_class(seed):
    """Both directions: hub rows past the default chunk length (256), main and
    short rows, and a degree <= 2 tail of >= 4096 rows (tiny._MIN_ROWS) with
    and without self loops; without them it holds degrees 2, 1 and 0."""
    from keras_geometric_amd import tiny

    src, dst = train_ref.class_graph(seed)
    N = train_ref.CLASS_N
    for ends in (dst, src):
        deg = np.bincount(ends, minlength=N)
        c = train_ref.class_counts(deg)
        assert c["hub"] >= 1 and c["main"] >= 1 and c["short"] >= 1
        assert min(c["two"], c["one"], c["zero"]) >= 1
        assert c["two"] + c["one"] + c["zero"] >= tiny._MIN_ROWS
        looped = train_ref.class_counts(deg + 1)
        assert looped["hub"] >= 1 and looped["short"] >= 1
        assert looped["two"] + looped["one"] >= tiny._MIN_ROWS and looped["zero"] == 0


def _small(seed=3, N=300, E=2600):
    s, d = rmat_edges(seed, scale_for(N), N, 0, E)
    return s.astype(np.int32), d.astype(np.int32), N


def _tensors(N, F, FO, seed):
    rng = np.random.default_rng(seed)
    x = T(rng.standard_normal((N, F)).astype(np.float32))
    W = T((rng.standard_normal((F, FO)) * 0.3).astype(np.float32))
    b = T(rng.standard_normal(FO).astype(np.float32))
    dOut = T(rng.standard_normal((N, FO)).astype(np.float32))
    return x, W, b, dOut


def _close(got, ref, mag, what):
    err = float(((got.double() - ref).abs() / mag.clamp_min(1.0)).max())
    assert err <= 1e-5, f"{what}: {err:.3g}"


@pytest.mark.parametrize("loops,norm", [(True, True), (False, False), (False, True)])
def test_grads_match_gcn_autograd(loops, norm):
    s, d, N = _small()
    x, W, b, dOut = _tensors(N, 16, 12, 5)
    g = train_ref.host_graph(s, d, N, loops, norm)
    ref, mag = train_ref.grads(g, x, W, b, dOut, "sum", norm)
    xr, Wr, br = (t.clone().requires_grad_(True) for t in (x, W, b))
    y = R.gcn_forward(xr, T(np.stack([s, d])), Wr, br, loops, norm)
    y.backward(dOut)
    _close(y.detach(), ref.y, mag.y, "y")
    _close(xr.grad, ref.dx, mag.dx, "dx")
    _close(Wr.grad, ref.dW, mag.dW, "dW")
    _close(br.grad, ref.db, mag.db, "db")
    assert bool((mag.y >= ref.y.abs() * (1 - 1e-12)).all()) and bool((mag.dx >= ref.dx.abs() * (1 - 1e-12)).all())
    assert bool((mag.dW >= ref.dW.abs() * (1 - 1e-12)).all())


@pytest.mark.parametrize("aggr", ["sum", "mean", "max", "min"])
def test_grads_match_gin_autograd(aggr):
    s, d, N = _small(seed=4)
    x, W, b, dOut = _tensors(N, 16, 12, 6)
    g = train_ref.host_graph(s, d, N, False, False)
    scale = float(np.float32(1.25))
    ref, mag = train_ref.grads(g, x, W, b, dOut, aggr, False, pre_gin=True, gin_scale=scale)
    xr, Wr, br = (t.clone().requires_grad_(True) for t in (x, W, b))
    ei = T(np.stack([s, d]))
    P = R.gin_aggregate_update_input(xr, ei, aggr, eps=0.25)
    y = R.gin_forward(xr, ei, [(Wr, br, None)], aggr, eps=0.25)
    y.backward(dOut)
    _close(P.detach(), ref.P, mag.P, "P")
    _close(y.detach(), ref.y, mag.y, "y")
    _close(xr.grad, ref.dx, mag.dx, "dx")
    _close(Wr.grad, ref.dW, mag.dW, "dW")
    _close(br.grad, ref.db, mag.db, "db")
    # the fp32 restatement the GPU tests compare max / min rows and short sums with bitwise
    a32, exact = train_ref.aggregate32(g, x, aggr, False, True, scale)
    assert torch.equal(a32[exact], P.detach()[exact])
    assert bool(exact.all()) == (aggr in ("max", "min")) and (aggr == "mean" or bool(exact.any()))


def test_grads_bias_none_and_rows():
    s, d, N = _small(seed=6)
    x, W, b, dOut = _tensors(N, 8, 8, 7)
    g = train_ref.host_graph(s, d, N, True, True)
    ref, mag = train_ref.grads(g, x, W, None, dOut, "sum", True)
    assert ref.db is None and mag.db is None
    full, _ = train_ref.grads(g, x, W, b, dOut, "sum", True)
    assert torch.equal(full.dx, ref.dx) and torch.equal(full.dW, ref.dW) and torch.equal(full.P, ref.P)
    torch.testing.assert_close(full.db, dOut.double().sum(0), rtol=1e-14, atol=0)


@pytest.mark.parametrize("red", ["sum", "mean", "max", "min"])
@pytest.mark.parametrize("weighted", [False, True])
def test_reference_unchanged_by_returning_the_aggregate(red, weighted):
    """fused_ref.reference's (y, scale) on test_fused_ref_host's case: the same
    bits with and without with_agg, in one chunk or several, and the returned
    aggregate is the one the product was taken of."""
    ei, g, x, W, b = _case()
    gin = red == "sum"
    y, scale = fused_ref.reference(g, x, W, red, weighted, b, pre_gin=gin, gin_scale=1.5, chunk_edges=997)
    y2, scale2, a, aa = fused_ref.reference(g, x, W, red, weighted, b, pre_gin=gin, gin_scale=1.5, chunk_edges=997,
                                            with_agg=True)
    assert torch.equal(y, y2) and torch.equal(scale, scale2)
    assert a.shape == (g.n_dst, x.shape[1]) and a.dtype == torch.float64
    torch.testing.assert_close(a @ W.double() + b.double(), y, rtol=1e-13, atol=1e-13)
    torch.testing.assert_close(aa @ W.double().abs() + b.double().abs(), scale, rtol=1e-13, atol=1e-13)
    assert bool((aa >= a.abs() * (1 - 1e-12)).all())
    # and it is train_ref's P (independent code: autograd-friendly, whole graph at once)
    ref, mag = train_ref.grads(g, x, W, b, torch.ones_like(y, dtype=torch.float32), red, weighted, gin, 1.5)
    # (its weighted messages are float64 products, fused_ref's the fp32 ones: 2^-24 of |terms| apart)
    assert float(((ref.P - a).abs() / aa.clamp_min(1.0)).max()) <= 1e-7
    assert float(((ref.y - y).abs() / scale.clamp_min(1.0)).max()) <= 1e-7
