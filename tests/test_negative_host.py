"""Link prediction without a GPU: the negative sampler's numpy restatement
(tests/negative_ref.py) is deterministic, position independent, uniform over
the admissible sources and honest about its fallbacks; both entry points
refuse bad arguments before any device call; kgx::edge_dot has a fake kernel;
and the backward identity of edge_dot is the gradient of the composed form.
"""

import ctypes

import numpy as np
import pytest
import torch

import edge_dot_ref as ER
import negative_ref as NR


def _draw(graph, a, keys, Q, seed, **kw):
    ei, n = graph
    rowptr, col = NR.sorted_csr(ei, n)
    return NR.negative_edges(rowptr, col, n, n, a, keys, Q, seed, **kw)


def _edge_set(ei):
    return set(zip(ei[0].tolist(), ei[1].tolist()))


def test_restatement_is_deterministic_and_position_independent():
    g = NR.mixed_graph()
    ei, n = g
    rng = np.random.default_rng(0)
    ids = rng.permutation(ei.shape[1])[:150].astype(np.int32)
    a = ei[1][ids]
    out, stats = _draw(g, a, ids, 5, 42)
    out2, stats2 = _draw(g, a, ids, 5, 42)
    assert np.array_equal(out, out2) and stats == stats2
    perm = rng.permutation(150)
    outp, statsp = _draw(g, a[perm], ids[perm], 5, 42)
    assert np.array_equal(outp, out[perm]) and statsp == stats
    # a positive alone draws what it drew in the batch; Q only appends columns
    one, _ = _draw(g, a[17:18], ids[17:18], 5, 42)
    assert np.array_equal(one[0], out[17])
    assert np.array_equal(_draw(g, a, ids, 2, 42)[0], out[:, :2])
    assert not np.array_equal(_draw(g, a, ids, 5, 43)[0], out)


@pytest.mark.parametrize("no_self", [True, False])
def test_outputs_are_not_edges(no_self):
    g = NR.mixed_graph()
    ei, n = g
    ids = np.arange(ei.shape[1], dtype=np.int32)
    a = ei[1].astype(np.int64)
    out, stats = _draw(g, a, ids, 4, 7, max_tries=64, no_self=no_self)
    assert stats == [0, 0]  # 64 tries against rows of at most ~20 of 80 sources: (21/80)^64 ~ 1e-37
    edges = _edge_set(ei)
    assert out.min() >= 0 and out.max() < n
    for p in range(out.shape[0]):
        for c in out[p]:
            assert (int(c), int(a[p])) not in edges
            assert not (no_self and c == a[p])
    if not no_self:  # self pairs that are not edges can be drawn
        assert (out == a[:, None]).any()


def test_uniform_over_admissible_sources():
    g = NR.uniform_graph()
    P, Q = 4000, 5
    keys = np.arange(P, dtype=np.int32) * 3 + 1
    a = np.zeros(P, np.int64)
    out, stats = _draw(g, a, keys, Q, 2024, max_tries=16)
    # per try 17 of 64 candidates are rejected: all 16 rejected with probability (17/64)^16 = 6e-10
    assert stats == [0, 0]
    assert np.array_equal(out, _draw(g, a, keys, Q, 2024, max_tries=16)[0])
    admissible = np.arange(17, 64)
    assert np.isin(out, admissible).all()
    freq = np.bincount(out.reshape(-1), minlength=64)[17:] / float(P * Q)
    # 20 000 draws: 5 binomial standard deviations of p = 1/47 are 5 sqrt(p (1 - p) / 20000) = 0.0051
    assert np.abs(freq - 1.0 / 47).max() <= 0.0051, freq


def test_fallback_path():
    g = NR.fallback_graph(free=7)
    P, Q = 500, 4
    keys = np.arange(P, dtype=np.int32)
    out, stats = _draw(g, np.zeros(P, np.int64), keys, Q, 5, max_tries=8)
    fell, bad = stats
    assert bad == 0 and fell > 0
    assert 0.5 < fell / (P * Q) < 0.7  # (15/16)^8 = 0.597
    assert int((out != 7).sum()) == fell  # a fallback holds the last (rejected) candidate
    assert out.min() >= 0 and out.max() < 16
    # a destination out of range: counted once per positive, outputs -1, nothing drawn
    out2, stats2 = _draw(g, np.array([0, 16, -1]), keys[:3], Q, 5)
    assert stats2[1] == 2 and (out2[1:] == -1).all() and np.array_equal(out2[0], _draw(g, [0], keys[:1], Q, 5)[0][0])


# ---------------------------------------------------------------------------
# the library, without a device
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from keras_geometric_amd import _native

    return _native.lib()


PTR = ctypes.c_void_p(16)


def test_edge_dot_argument_errors(lib):
    def call(n_a=4, ld_a=8, n_b=4, ld_b=8, F=8, P=3, K=2, ld_out=2, xa=PTR, a_idx=PTR, out=PTR):
        return lib.kgx_edge_dot(xa, n_a, ld_a, PTR, n_b, ld_b, F, a_idx, PTR, P, K, None, out, ld_out, None, None)

    assert call(K=0) == 1 and b"K must be >= 1" in lib.kgx_last_error()
    assert call(ld_a=7) == 1 and b"leading dimension" in lib.kgx_last_error()
    assert call(ld_b=7) == 1
    assert call(ld_out=1) == 1 and b"ld_out" in lib.kgx_last_error()
    assert call(P=-1) == 1 and call(F=-1, ld_a=0) == 1 and call(n_a=-1) == 1
    assert call(P=1 << 20, K=1 << 11, ld_out=1 << 11) == 1 and b"int32" in lib.kgx_last_error()
    assert call(xa=None) == 1 and b"null" in lib.kgx_last_error()
    assert call(a_idx=None) == 1 and call(out=None) == 1
    assert call(n_a=0) == 1 and b"empty table" in lib.kgx_last_error()
    assert call(P=0, xa=None, a_idx=None, out=None) == 0  # nothing to do, nothing touched


def test_negative_edges_argument_errors(lib):
    def call(Q=2, max_tries=8, n_src=10, n_dst=10, P=3, ld_out=2, flags=3, rowptr=PTR, a=PTR, stats=PTR):
        return lib.kgx_negative_edges(rowptr, PTR, n_dst, n_src, a, PTR, P, Q, 1, max_tries, flags, PTR, ld_out,
                                      stats, None)

    assert call(Q=0) == 1 and b"Q must be >= 1" in lib.kgx_last_error()
    assert call(max_tries=0) == 1 and call(max_tries=65) == 1 and b"max_tries" in lib.kgx_last_error()
    assert call(n_src=0) == 1 and b"n_src" in lib.kgx_last_error()
    assert call(P=-1) == 1 and call(n_dst=-1) == 1
    assert call(ld_out=1) == 1 and b"ld_out" in lib.kgx_last_error()
    assert call(flags=4) == 1 and b"flags" in lib.kgx_last_error()
    assert call(a=None) == 1 and call(stats=None) == 1 and b"null" in lib.kgx_last_error()
    assert call(rowptr=None) == 1 and b"KGX_NEG_REJECT_EDGES" in lib.kgx_last_error()
    assert call(P=0, a=None, stats=None) == 0


def test_edge_dot_fake_kernel():
    import keras_geometric_amd  # noqa: F401  (registers torch.ops.kgx.*)

    m = dict(device="meta")
    xa, xb = torch.empty(9, 12, **m), torch.empty(5, 12, **m)
    a_idx = torch.empty(7, dtype=torch.int32, **m)
    b_idx = torch.empty(7, 3, dtype=torch.int32, **m)
    bad = torch.empty(1, dtype=torch.int32, **m)
    out = torch.ops.kgx.edge_dot(xa, xb, a_idx, b_idx, None, bad)
    assert out.shape == (7, 3) and out.dtype == torch.float32 and out.device.type == "meta"
    out = torch.ops.kgx.edge_dot(xa, xa, a_idx, b_idx[:, :1], a_idx, bad)
    assert out.shape == (7, 1)


@pytest.mark.parametrize("same", [False, True])
def test_backward_identity_matches_autograd(same):
    g = torch.Generator().manual_seed(1)
    n_a, n_b, F, P, K = 9, 9 if same else 6, 5, 40, 3
    xa = torch.randn(n_a, F, generator=g, dtype=torch.float64, requires_grad=True)
    xb = xa if same else torch.randn(n_b, F, generator=g, dtype=torch.float64, requires_grad=True)
    a_idx = torch.randint(0, n_a, (P,), generator=g, dtype=torch.int32)
    a_idx[:20] = 2  # a hub
    b_idx = torch.randint(0, n_b, (P, K), generator=g, dtype=torch.int32)
    D = torch.randn(P, K, generator=g, dtype=torch.float64)
    (ER.composed(xa, xb, a_idx, b_idx) * D).sum().backward()
    g_xa, g_xb = ER.backward_identity(xa.detach(), xb.detach(), a_idx, b_idx, D)
    if same:
        assert torch.allclose(xa.grad, g_xa + g_xb, rtol=1e-12, atol=1e-12)
    else:
        assert torch.allclose(xa.grad, g_xa, rtol=1e-12, atol=1e-12)
        assert torch.allclose(xb.grad, g_xb, rtol=1e-12, atol=1e-12)
    # the float64 restatement of the forward agrees with the composed form
    s, _ = ER.edge_dot(xa.detach().numpy(), xb.detach().numpy(), a_idx.numpy(), b_idx.numpy())
    assert np.allclose(s, ER.composed(xa, xb, a_idx, b_idx).detach().numpy(), rtol=1e-12, atol=1e-12)
