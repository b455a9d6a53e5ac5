"""AttentionPooling / Set2Set on the GPU against a float64 restatement of the
reference arithmetic (attention_pooling.py:130-217, :381-414), fed with the
layer's own get_weights().  Bar: |a - b| <= 1e-5 * max(1, |b|).

The restatements are the reference's call() line by line on torch float64:
Dense = x @ kernel + bias, softmax over axis 0, the sum over axis 0, and
keras.layers.LSTMCell (gates i, f, c, o).  torch autograd through them is the
reference's gradient.
"""

import functools

import numpy as np
import pytest
import torch

from keras_geometric_amd import AttentionPooling, GCNConv, Set2Set, set_random_seed

pytestmark = pytest.mark.gpu

T = torch.from_numpy


def assert_bar(a, b, what=""):
    a = a.detach().cpu().double().numpy() if isinstance(a, torch.Tensor) else np.asarray(a, dtype=np.float64)
    b = b.detach().cpu().double().numpy() if isinstance(b, torch.Tensor) else np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape, f"{what}: shape {a.shape} vs {b.shape}"
    err = np.abs(a - b) / np.maximum(1.0, np.abs(b))
    worst = float(err.max()) if err.size else 0.0
    print(f"{what} max scaled err {worst:.3e}")
    assert worst <= 1e-5, f"{what}: max scaled err {worst:.3g}"


# -- float64 restatements -----------------------------------------------------
def ref_attention_pooling(x, w):
    k1, b1, k2, b2 = w
    scores = torch.tanh(x @ k1 + b1) @ k2 + b2  # [N, 1]
    weights = torch.softmax(scores, dim=0)
    return (weights * x).sum(0, keepdim=True)


def ref_set2set(x, w, steps):
    kernel, recurrent, bias, ak, ab = w
    n, u = x.shape[0], recurrent.shape[0]
    h = torch.zeros((1, u), dtype=x.dtype)
    c = torch.zeros((1, u), dtype=x.dtype)

    def attend(h):
        scores = torch.tanh(torch.cat([x, h.expand(n, u)], dim=-1) @ ak + ab)
        return (torch.softmax(scores, dim=0) * x).sum(0, keepdim=True)

    for _ in range(steps):
        z = attend(h) @ kernel + h @ recurrent + bias
        zi, zf, zc, zo = torch.split(z, u, dim=-1)
        c = torch.sigmoid(zf) * c + torch.sigmoid(zi) * torch.tanh(zc)
        h = torch.sigmoid(zo) * torch.tanh(c)
    return torch.cat([h, attend(h)], dim=-1)


def ref_gcn(x, ei, kernel, bias):
    """GCNConv (gcn_conv.py:233-272, utils/main.py:8-33) in the dtype of x."""
    n = x.shape[0]
    loops = torch.arange(n)
    src, dst = torch.cat([ei[0].long(), loops]), torch.cat([ei[1].long(), loops])
    deg = torch.zeros(n, dtype=x.dtype).index_add(0, dst, torch.ones(dst.numel(), dtype=x.dtype))
    dinv = (deg + 1e-12) ** -0.5
    msg = (x[src] @ kernel) * (dinv[dst] * dinv[src]).unsqueeze(1)
    return torch.zeros((n, kernel.shape[1]), dtype=x.dtype).index_add(0, dst, msg) + bias


def w64(layer):
    return [T(a).double() for a in layer.get_weights()]


@functools.lru_cache(maxsize=None)
def features(n, f, seed=0):
    return np.random.default_rng(seed).standard_normal((n, f)).astype(np.float32)


# -- AttentionPooling ---------------------------------------------------------
@pytest.mark.parametrize("n,f,dim", [(25, 64, 32), (5000, 128, None)])
def test_attention_pooling(dev, n, f, dim):
    set_random_seed(1)
    x = features(n, f)
    layer = AttentionPooling(attention_dim=dim)
    assert layer.attention_dense is None and layer.attention_score is None
    out = layer(T(x).to(dev))
    assert layer.attention_dense is not None and layer.attention_score is not None and layer.dropout_layer is None
    assert out.shape == (1, f)
    w = layer.get_weights()
    d = dim or f
    assert [a.shape for a in w] == [(f, d), (d,), (d, 1), (1,)]  # transform kernel, bias, score kernel, bias
    assert_bar(out, ref_attention_pooling(T(x).double(), w64(layer)), f"AttentionPooling ({n}, {f})")
    # numpy input, as the reference's tests pass it
    assert torch.equal(layer(x), out)


# -- Set2Set ------------------------------------------------------------------
@pytest.mark.parametrize("n,f,kw", [(25, 64, dict(output_dim=16, processing_steps=2)),
                                     (5000, 100, dict(output_dim=32, lstm_units=24, processing_steps=3))])
def test_set2set(dev, n, f, kw):
    set_random_seed(2)
    x = features(n, f, 1)
    layer = Set2Set(**kw)
    assert layer.lstm_cell is None and layer.attention_dense is None
    out = layer(T(x).to(dev))
    u = layer.lstm_units
    assert layer.lstm_cell is not None and layer.attention_dense is not None and layer.dropout_layer is None
    assert out.shape == (1, u + f)
    w = layer.get_weights()
    # LSTM kernel, recurrent kernel, bias, then attention kernel, bias
    assert [a.shape for a in w] == [(f, 4 * u), (u, 4 * u), (4 * u,), (f + u, 1), (1,)]
    assert (w[2][u:2 * u] == 1).all() and (w[2][:u] == 0).all() and (w[2][2 * u:] == 0).all()  # unit forget bias
    np.testing.assert_allclose(w[1] @ w[1].T, np.eye(u), atol=1e-5)  # orthogonal recurrent kernel
    assert_bar(out, ref_set2set(T(x).double(), w64(layer), layer.processing_steps), f"Set2Set ({n}, {f})")


def test_set_weights_round_trip(dev):
    set_random_seed(3)
    x = T(features(25, 64, 2)).to(dev)
    for make in (lambda: AttentionPooling(attention_dim=32), lambda: Set2Set(output_dim=16, processing_steps=2)):
        a, b = make(), make()
        ya, yb = a(x), b(x)
        assert not torch.equal(ya, yb)  # different initial weights
        b.set_weights(a.get_weights())
        for wa, wb in zip(a.get_weights(), b.get_weights()):
            assert np.array_equal(wa, wb)
        assert torch.equal(b(x), ya)
        a.set_weights(a.get_weights())
        assert torch.equal(a(x), ya)
        with pytest.raises(ValueError):
            b.set_weights(a.get_weights()[:-1])


# -- batched ------------------------------------------------------------------
GRAPH_SIZES = [30, 45, 0, 25, 1, 700]


@pytest.mark.parametrize("make", [lambda: AttentionPooling(attention_dim=32),
                                  lambda: Set2Set(output_dim=16, processing_steps=2)],
                         ids=["AttentionPooling", "Set2Set"])
@pytest.mark.parametrize("shuffled", [False, True], ids=["sorted", "shuffled"])
def test_batched_equals_per_graph(dev, make, shuffled):
    set_random_seed(4)
    batch = np.repeat(np.arange(len(GRAPH_SIZES)), GRAPH_SIZES).astype(np.int32)
    if shuffled:
        batch = batch[np.random.default_rng(3).permutation(batch.size)]
    x = T(features(batch.size, 64, 3)).to(dev)
    layer = make()
    out = layer([x, T(batch).to(dev)])
    width = layer.compute_output_shape((batch.size, 64))[1]
    assert out.shape == (len(GRAPH_SIZES), width)
    for gid, size in enumerate(GRAPH_SIZES):
        if size == 0:
            continue  # an empty graph has no single-graph call to compare with; its pooled part is the empty sum
        single = layer(x[T(batch == gid).to(dev)])
        assert_bar(out[gid:gid + 1], single.double(), f"graph {gid} ({size} nodes)")
    assert (out[2, -64:] == 0).all()  # the empty graph pools to the zero row


# -- training -----------------------------------------------------------------
def _edges(n, e, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(0, n, (2, e)).astype(np.int32)


def test_training_gcn_attention_pooling(dev):
    set_random_seed(5)
    n, f = 300, 16
    x, ei = features(n, f, 4), _edges(n, 2400, 5)
    lw = np.random.default_rng(6).standard_normal((1, 32)).astype(np.float32)
    conv, pool = GCNConv(32), AttentionPooling()
    xd = T(x).to(dev).requires_grad_(True)
    out = pool(conv([xd, T(ei).to(dev)]), training=True)
    (out * T(lw).to(dev)).sum().backward()
    xr = T(x).double().requires_grad_(True)
    wr = [t.requires_grad_(True) for t in w64(conv) + w64(pool)]
    ref = ref_attention_pooling(ref_gcn(xr, T(ei), wr[0], wr[1]), wr[2:])
    (ref * T(lw).double()).sum().backward()
    assert_bar(out, ref, "GCNConv -> AttentionPooling")
    assert_bar(xd.grad, xr.grad, "d x")
    for p, r, name in zip(conv.weights + pool.weights, wr, ["gcn kernel", "gcn bias", "transform kernel",
                                                           "transform bias", "score kernel", "score bias"]):
        # (the score bias: softmax is shift-invariant, so both gradients are rounding noise around 0)
        assert_bar(p.grad, r.grad, f"d {name}")


def test_training_set2set(dev):
    set_random_seed(6)
    n, f = 300, 64
    x = features(n, f, 7)
    layer = Set2Set(output_dim=16, processing_steps=2)
    lw = np.random.default_rng(8).standard_normal((1, 16 + f)).astype(np.float32)
    xd = T(x).to(dev).requires_grad_(True)
    out = layer(xd, training=True)
    (out * T(lw).to(dev)).sum().backward()
    xr = T(x).double().requires_grad_(True)
    wr = [t.requires_grad_(True) for t in w64(layer)]
    ref = ref_set2set(xr, wr, 2)
    (ref * T(lw).double()).sum().backward()
    assert_bar(out, ref, "Set2Set training forward")
    assert_bar(xd.grad, xr.grad, "d x")
    for p, r, name in zip(layer.weights, wr, ["lstm kernel", "recurrent kernel", "lstm bias", "attention kernel",
                                              "attention bias"]):
        assert_bar(p.grad, r.grad, f"d {name}")


# -- dropout ------------------------------------------------------------------
@pytest.mark.parametrize("make", [lambda p: AttentionPooling(attention_dim=32, dropout=p),
                                  lambda p: Set2Set(output_dim=16, processing_steps=2, dropout=p)],
                         ids=["AttentionPooling", "Set2Set"])
def test_dropout(dev, make):
    set_random_seed(7)
    x = T(features(200, 64, 9)).to(dev)
    plain, dropped = make(0.0), make(0.5)
    y = plain(x)
    assert plain.dropout_layer is None
    assert torch.equal(plain(x, training=True), y)  # p = 0: training is eval, bit for bit
    dropped(x)
    assert dropped.dropout_layer is not None
    dropped.set_weights(plain.get_weights())
    assert torch.equal(dropped(x, training=False), y)  # eval ignores dropout
    assert torch.equal(dropped(x), y)
    torch.manual_seed(0)
    z = dropped(x, training=True)
    assert z.shape == y.shape and torch.isfinite(z).all()
    assert not torch.equal(z, y)
