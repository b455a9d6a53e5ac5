"""The neighbour sampler's boundary and its numpy restatement, without a device (CPU).

* kgx_sample_neighbors / kgx_relabel_frontier and their workspace functions are
  declared, exported and bound; NeighborSampler is public.
* Every argument error include/kgx.h lists is reported as KGX_ERR_ARG with a
  message, from null or dummy pointers: no device call is reached.
* tests/sampling_ref.py (what the GPU tests compare against, exactly): its
  permutation is a bijection of [0, d), and the first-k selection is uniform
  over the slots of a row.
"""

import ctypes
import re
from pathlib import Path

import numpy as np
import pytest

import sampling_ref as SR

ROOT = Path(__file__).resolve().parents[1]
NAMES = ["kgx_sample_workspace_bytes", "kgx_sample_neighbors", "kgx_relabel_workspace_bytes",
         "kgx_relabel_frontier"]
P = ctypes.c_void_p(256)  # a dummy non-null pointer: never dereferenced before the argument checks pass


@pytest.fixture(scope="module")
def lib():
    from keras_geometric_amd import _native

    return _native.lib()


def _sample(lib, *, rowptr=P, col=P, eid=P, n_rows=10, seeds=P, n_seeds=4, fanout=3, out_rowptr=P, out_src=P,
            out_eid=P, cap=12, ws=P, ws_bytes=1 << 30, info=True):
    buf = (ctypes.c_int64 * 4)() if info else None
    return lib.kgx_sample_neighbors(rowptr, col, eid, n_rows, seeds, n_seeds, fanout, 7, 0, out_rowptr, out_src,
                                    out_eid, cap, ws, ws_bytes, buf, None)


def _relabel(lib, *, nodes=P, n_known=4, frontier=P, n_f=4, out_rowptr=P, out_src=P, n_edges=12, node_map=P,
             n_nodes=10, new_nodes=P, src_local=P, dst_local=P, ws=P, ws_bytes=1 << 30, info=True):
    buf = (ctypes.c_int64 * 4)() if info else None
    return lib.kgx_relabel_frontier(nodes, n_known, frontier, n_f, out_rowptr, out_src, n_edges, node_map, n_nodes,
                                    new_nodes, src_local, dst_local, ws, ws_bytes, buf, None)


def test_declared_exported_bound_and_public(lib):
    import keras_geometric_amd as kgx
    from keras_geometric_amd import _native

    header = (ROOT / "include" / "kgx.h").read_text()
    for name in NAMES:
        assert re.search(rf"^int {name}\(", header, flags=re.M), name
        assert hasattr(lib, name), name
        assert name in _native.exported_symbols(), name
    assert "NeighborSampler" in kgx.__all__ and "SampledSubgraph" in kgx.__all__
    assert kgx.NeighborSampler is kgx.sampling.NeighborSampler
    assert lib.kgx_version() == 2


@pytest.mark.parametrize("kw, word", [
    (dict(fanout=0), b"fanout"),
    (dict(fanout=-2), b"fanout"),
    (dict(n_seeds=-1), b"negative"),
    (dict(n_seeds=1 << 20, fanout=1 << 11, cap=(1 << 31) - 1), b"int32"),  # n_seeds * fanout = 2^31
    (dict(cap=11), b"cap"),
    (dict(rowptr=None), b"null"), (dict(col=None), b"null"), (dict(eid=None), b"null"),
    (dict(seeds=None), b"null"), (dict(out_rowptr=None), b"null"), (dict(out_src=None), b"null"),
    (dict(out_eid=None), b"null"), (dict(info=False), b"null"),
    (dict(ws=None), b"workspace"), (dict(ws_bytes=16), b"workspace"),
])
def test_sample_argument_errors_without_device(lib, kw, word):
    assert _sample(lib, **kw) == 1
    assert word in lib.kgx_last_error().lower()


@pytest.mark.parametrize("kw, word", [
    (dict(n_known=-1), b"negative"), (dict(n_edges=-1), b"negative"), (dict(n_f=-1), b"negative"),
    (dict(n_known=1 << 30, n_edges=1 << 30), b"int32"),
    (dict(n_f=0), b"frontier"),
    (dict(nodes=None), b"null"), (dict(frontier=None), b"null"), (dict(out_rowptr=None), b"null"),
    (dict(out_src=None), b"null"), (dict(node_map=None), b"null"), (dict(new_nodes=None), b"null"),
    (dict(src_local=None), b"null"), (dict(dst_local=None), b"null"), (dict(info=False), b"null"),
    (dict(ws=None), b"workspace"), (dict(ws_bytes=16), b"workspace"),
])
def test_relabel_argument_errors_without_device(lib, kw, word):
    assert _relabel(lib, **kw) == 1
    assert word in lib.kgx_last_error().lower()


def test_empty_calls_are_ok_and_launch_nothing(lib):
    info = (ctypes.c_int64 * 4)(9, 9, 9, 9)
    assert lib.kgx_sample_neighbors(None, None, None, 10, None, 0, 3, 7, 0, None, None, None, 0, None, 0, info,
                                    None) == 0
    assert list(info) == [0, 0, 0, 0]
    assert lib.kgx_sample_neighbors(None, None, None, 10, None, 0, -1, 7, 0, None, None, None, 0, None, 0, None,
                                    None) == 0
    assert lib.kgx_relabel_frontier(None, 0, None, 0, None, None, 0, None, 10, None, None, None, None, 0, info,
                                    None) == 0


def test_workspace_sizes_positive_and_monotone(lib):
    def sample_ws(n):
        b = ctypes.c_size_t(0)
        assert lib.kgx_sample_workspace_bytes(n, ctypes.byref(b)) == 0
        return b.value

    def relabel_ws(e, n):
        b = ctypes.c_size_t(0)
        assert lib.kgx_relabel_workspace_bytes(e, n, ctypes.byref(b)) == 0
        return b.value

    sizes = [sample_ws(n) for n in (0, 1, 257, 1024, 100_000, 10_000_000)]
    assert sizes[0] > 0 and sizes == sorted(sizes) and sizes[-1] >= 4 * 10_000_001
    by_e = [relabel_ws(e, 2_000_000) for e in (0, 1, 1000, 150_000, 10_000_000)]
    assert by_e[0] > 0 and by_e == sorted(by_e) and by_e[-1] >= 16 * 10_000_000
    by_n = [relabel_ws(150_000, n) for n in (1, 1000, 1 << 20, 1 << 30)]
    assert by_n == sorted(by_n)
    assert lib.kgx_sample_workspace_bytes(4, None) == 1
    assert lib.kgx_sample_workspace_bytes(-1, ctypes.byref(ctypes.c_size_t(0))) == 1
    assert lib.kgx_relabel_workspace_bytes(-1, 4, ctypes.byref(ctypes.c_size_t(0))) == 1


def test_half_width_keeps_the_superset_below_4d():
    for d in list(range(2, 300)) + [1 << 16, (1 << 16) + 1, 70001, (1 << 31) - 1]:
        hb = SR.half_bits(d)
        assert d <= 1 << (2 * hb) < 4 * d, d
    assert SR.half_bits(2) == 1 and SR.half_bits(8) == 2 and SR.half_bits(9) == 2 and SR.half_bits(70001) == 9


NODE_IDS = [0, 1, 2, 12345, 1_999_999, (1 << 31) - 2]


@pytest.mark.parametrize("d", list(range(2, 301)))
def test_permutation_is_a_bijection_small(d):
    keys = SR.row_keys(SR.hop_stream(5, 1), NODE_IDS)[:, None, :]
    y = SR.perm(np.arange(d, dtype=np.uint64)[None, :], keys, d)
    assert y.shape == (len(NODE_IDS), d)
    assert (np.sort(y, axis=1) == np.arange(d, dtype=np.uint64)).all()


@pytest.mark.parametrize("d", [1 << 16, (1 << 16) + 1, 70001])
def test_permutation_is_a_bijection_large(d):
    keys = SR.row_keys(SR.hop_stream(5, 0), NODE_IDS[:3])[:, None, :]
    y = SR.perm(np.arange(d, dtype=np.uint64)[None, :], keys, d)
    assert (np.sort(y, axis=1) == np.arange(d, dtype=np.uint64)).all()


def test_row_slots_follow_the_take_all_rule():
    assert SR.row_slots(3, 0, 11, 0, 5).tolist() == []
    assert SR.row_slots(3, 0, 11, 5, 5).tolist() == [0, 1, 2, 3, 4]
    assert SR.row_slots(3, 0, 11, 70001, -1).tolist() == list(range(70001))
    s = SR.row_slots(3, 0, 11, 6, 5)
    assert len(s) == 5 and len(set(s.tolist())) == 5 and s.min() >= 0 and s.max() < 6
    # a prefix property: k draws are the first k of k + 1 draws (both below the degree)
    assert SR.row_slots(3, 2, 11, 40, 7).tolist() == SR.row_slots(3, 2, 11, 40, 8).tolist()[:7]
    # the keys depend on seed, hop and row
    base = SR.row_slots(3, 0, 11, 1000, 10).tolist()
    assert base != SR.row_slots(4, 0, 11, 1000, 10).tolist()
    assert base != SR.row_slots(3, 1, 11, 1000, 10).tolist()
    assert base != SR.row_slots(3, 0, 12, 1000, 10).tolist()
    assert SR.epoch_seed(0, 0) != SR.epoch_seed(0, 1) != SR.epoch_seed(1, 0)


def test_epoch_seed_matches_the_package():
    from keras_geometric_amd import sampling

    for seed, epoch in [(0, 0), (0, 1), (123456789, 77), ((1 << 64) - 1, 3)]:
        assert sampling.epoch_seed(seed, epoch) == SR.epoch_seed(seed, epoch)


def test_first_k_selection_is_uniform_over_slots():
    """d = 10, k = 3 over 20 000 node ids at one fixed seed: each slot is chosen
    with frequency 0.3 +- 5 binomial standard deviations, 5 * sqrt(0.3 * 0.7 /
    20000) = 0.0162."""
    n, d, k = 20_000, 10, 3
    keys = SR.row_keys(SR.hop_stream(SR.epoch_seed(2024, 0), 0), np.arange(n))[:, None, :]
    y = SR.perm(np.arange(k, dtype=np.uint64)[None, :], keys, d)
    assert (np.sort(y, axis=1)[:, 1:] != np.sort(y, axis=1)[:, :-1]).all()  # distinct within a row
    freq = np.bincount(y.reshape(-1).astype(np.int64), minlength=d) / n
    print("slot frequencies", freq)
    bound = 5 * np.sqrt(0.3 * 0.7 / n)
    assert abs(bound - 0.0162) < 1e-4
    assert (np.abs(freq - 0.3) <= bound).all(), freq
