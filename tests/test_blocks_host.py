"""Sampled blocks without a device (CPU): the structure sample_blocks relies on,
on the numpy restatement, and kgx_block_csr's boundary.

* The sampler's merged edge list is sorted by destination, the edges of hops
  0..h are a prefix of it with dst < P_h and src < P_{h+1}, and every row's
  edges lie in one hop (so rowptr / deg of an inner block are prefix views).
* A float64 2-layer mean-SAGE over the blocks equals the same model over the
  merged subgraph at the seed rows.
* kgx_block_csr / kgx_block_workspace_bytes are declared, exported and bound,
  Block / SampledBlocks are public, and every argument error is reported as
  KGX_ERR_ARG from dummy pointers: no device call is reached.
"""

import ctypes
import re
from pathlib import Path

import numpy as np
import pytest

import blocks_ref as BR
import sampling_ref as SR

ROOT = Path(__file__).resolve().parents[1]
N, E = 2000, 20000
P = ctypes.c_void_p(256)  # a dummy non-null pointer: never dereferenced before the argument checks pass


@pytest.fixture(scope="module")
def graph():
    """2000 nodes, 20000 edges, skewed in-degrees, at least 8 nodes without in-edges."""
    rng = np.random.default_rng(5)
    dst = np.minimum((rng.pareto(1.2, E) * 40).astype(np.int64), N - 9)  # ids N-8.. get no in-edges
    dst = rng.permutation(N - 8)[dst]
    src = rng.integers(0, N, E)
    ei = np.stack([src, dst]).astype(np.int32)
    csr = SR.build_csr(ei, N)
    deg = np.diff(csr[0])
    zero = np.where(deg == 0)[0]
    assert len(zero) >= 8 and (deg > 5).sum() >= 50
    rest = rng.permutation(np.setdiff1d(np.arange(N), zero[:8]))[: 257 - 8]
    seeds = rng.permutation(np.concatenate([zero[:8], rest])).astype(np.int32)
    return {"csr": csr, "deg": deg, "seeds": seeds, "zero": zero.astype(np.int32)}


def _cases(graph):
    big = graph["seeds"][graph["deg"][graph["seeds"]] > 5]
    return [
        ([5, 3], graph["seeds"]), ([4, 3, 2], graph["seeds"]), ([-1, 2], graph["seeds"]), ([3], graph["seeds"]),
        ([5, 3], big[:1]),               # a one-seed batch
        ([5, 3], graph["zero"][:8]),     # zero-degree seeds only: hop 1 never runs
    ]


@pytest.mark.parametrize("case", range(6))
def test_prefix_and_sortedness(graph, case):
    fanouts, seeds = _cases(graph)[case]
    L = len(fanouts)
    sub = SR.sample_subgraph(graph["csr"], seeds, fanouts, seed=21, epoch=2)
    src, dst = sub["edge_index"].astype(np.int64)
    assert (np.diff(dst) >= 0).all(), "the merged edge list is not sorted by destination"
    Pn = BR.node_prefix(sub, L)
    assert Pn[0] == len(seeds) and Pn[-1] == len(sub["node_ids"]) and len(Pn) == L + 1
    bounds = BR.block_bounds(sub, L)
    assert len(bounds) == L
    for layer, (n_src, n_dst, e) in enumerate(bounds):
        assert (n_src, n_dst) == (Pn[L - layer], Pn[L - 1 - layer])
        assert (dst[:e] < n_dst).all() and (dst[e:] >= n_dst).all()  # a prefix, and the whole of it
        assert (src[:e] < n_src).all() and (src[:e] >= 0).all()
        if layer + 1 < L:
            assert bounds[layer + 1][0] == n_dst  # the shapes chain
        # rowptr / deg of this block are a prefix of the outermost block's
        rowptr0, deg0 = BR.forward_csr(dst, bounds[0][1])
        rowptr, deg = BR.forward_csr(dst[:e], n_dst)
        assert np.array_equal(rowptr, rowptr0[: n_dst + 1]) and np.array_equal(deg, deg0[:n_dst])
        # the transposed CSR lists every source's edges in ascending position
        t_rowptr, t_deg, t_col, t_eid = BR.transposed_csr(src[:e], dst[:e], n_src)
        assert t_rowptr[-1] == e and np.array_equal(np.sort(t_eid), np.arange(e))
        assert np.array_equal(t_col, dst[:e][t_eid]) and np.array_equal(np.repeat(np.arange(n_src), t_deg), src[:e][t_eid])
        for j in np.where(t_deg > 1)[0][:50]:
            assert (np.diff(t_eid[t_rowptr[j]: t_rowptr[j + 1]]) > 0).all()
    assert bounds[-1][1] == len(seeds) and bounds[0][2] == len(dst)
    if case == 5:
        assert sub["hop_node_counts"] == [8, 0] and bounds == [(8, 8, 0), (8, 8, 0)]


def test_two_layer_mean_sage_over_blocks_equals_the_merged_subgraph(graph):
    """float64, F 36 -> 20 -> 12.  Row i < n_dst of a block sums the same terms in
    the same order as the merged graph's row i; the matrix products may block
    differently, so the bar is 1e-12 scaled (a 36-term float64 dot product is
    exact to about 36 * 2.2e-16 of its terms' magnitude)."""
    sub = SR.sample_subgraph(graph["csr"], graph["seeds"], [5, 3], seed=4, epoch=1)
    rng = np.random.default_rng(9)
    n_sub = len(sub["node_ids"])
    x = rng.standard_normal((n_sub, 36))
    Ws = [(rng.standard_normal((36, 20)) / 6, rng.standard_normal((36, 20)) / 6, rng.standard_normal(20) / 6),
          (rng.standard_normal((20, 12)) / 4, rng.standard_normal((20, 12)) / 4, rng.standard_normal(12) / 4)]
    src, dst = sub["edge_index"]
    h = x
    for W_self, W_neigh, b in Ws:
        h = BR.sage_mean_layer(h, src, dst, n_sub, W_self, W_neigh, b)
    merged = h[: sub["n_seeds"]]
    h = x
    for (n_src, n_dst, e), (W_self, W_neigh, b) in zip(BR.block_bounds(sub, 2), Ws):
        assert h.shape[0] == n_src
        h = BR.sage_mean_layer(h, src[:e], dst[:e], n_dst, W_self, W_neigh, b)
    assert h.shape == merged.shape == (sub["n_seeds"], 12)
    err = (np.abs(h - merged) / np.maximum(np.abs(merged), 1.0)).max()
    assert err <= 1e-12, err
    assert np.abs(merged).max() > 0.1  # not a comparison of zeros


# ---------------------------------------------------------------------------
# the C-ABI boundary
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from keras_geometric_amd import _native

    return _native.lib()


def _block(lib, *, src=P, dst=P, E=12, n_src=9, n_dst=4, rowptr=P, deg=P, t_rowptr=P, t_deg=P, t_col=P, t_eid=P,
           ws=P, ws_bytes=1 << 30, info=True):
    buf = (ctypes.c_int64 * 4)() if info else None
    return lib.kgx_block_csr(src, dst, E, n_src, n_dst, rowptr, deg, t_rowptr, t_deg, t_col, t_eid, ws, ws_bytes,
                             buf, None)


def test_declared_exported_bound_and_public(lib):
    import keras_geometric_amd as kgx
    from keras_geometric_amd import _native

    header = (ROOT / "include" / "kgx.h").read_text()
    for name in ("kgx_block_workspace_bytes", "kgx_block_csr"):
        assert re.search(rf"^int {name}\(", header, flags=re.M), name
        assert hasattr(lib, name), name
        assert name in _native.exported_symbols(), name
    assert "Block" in kgx.__all__ and "SampledBlocks" in kgx.__all__
    assert kgx.SampledBlocks is kgx.sampling.SampledBlocks and kgx.Block is kgx.sampling.Block
    assert hasattr(kgx.NeighborSampler, "sample_blocks")


@pytest.mark.parametrize("kw, word", [
    (dict(E=-1), b"negative"), (dict(n_src=-1), b"negative"), (dict(n_dst=-1), b"negative"),
    (dict(E=1 << 31), b"int32"), (dict(n_src=(1 << 31) - 1), b"int32"),
    (dict(src=None), b"null"), (dict(dst=None), b"null"), (dict(t_rowptr=None), b"null"),
    (dict(t_deg=None), b"null"), (dict(t_col=None), b"null"), (dict(t_eid=None), b"null"),
    (dict(info=False), b"null"),
    (dict(rowptr=None), b"together"), (dict(deg=None), b"together"),
    (dict(ws=None), b"workspace"), (dict(ws_bytes=16), b"workspace"),
])
def test_block_csr_argument_errors_without_device(lib, kw, word):
    assert _block(lib, **kw) == 1
    assert word in lib.kgx_last_error().lower()


def test_block_workspace_sizes(lib):
    def ws(e, n):
        b = ctypes.c_size_t(0)
        assert lib.kgx_block_workspace_bytes(e, n, ctypes.byref(b)) == 0
        return b.value

    by_e = [ws(e, 50_000) for e in (0, 1, 1000, 150_000, 10_000_000)]
    assert by_e[0] > 0 and by_e == sorted(by_e) and by_e[-1] >= 16 * 10_000_000
    assert lib.kgx_block_workspace_bytes(4, 4, None) == 1
    assert lib.kgx_block_workspace_bytes(-1, 4, ctypes.byref(ctypes.c_size_t(0))) == 1
    assert lib.kgx_block_workspace_bytes(4, -1, ctypes.byref(ctypes.c_size_t(0))) == 1
