"""Host logic of the sliced fused launch (slice.py, kgx_slice_grid, kgx_slice_class):
which launches ask for a sliced schedule, the grid of a sliced launch and its
fall-back, and the source-class hash.  No GPU."""

import pytest

from keras_geometric_amd import _native as nat
from keras_geometric_amd import slice as S

NS = dict(have_items=True, two_tables=False, reduce=nat.SUM, f_in=128, f_out=128, n_edges=110_000_000, T=128, C=8)


def _wanted(**kw):
    return S.slice_wanted(**{**NS, "mode": None, "default_on": True, **kw})


def test_default_rule_slices_large_sums_only():
    assert _wanted()
    assert not _wanted(default_on=False)           # the rule's switch
    assert not _wanted(n_edges=11_000_000)         # C2: small graphs keep the plain schedule
    assert not _wanted(mode=False)                 # KGX_FUSED_SLICE=0
    assert _wanted(mode=True, default_on=False, n_edges=1000)  # KGX_FUSED_SLICE=1: any size


@pytest.mark.parametrize("kw", [
    dict(have_items=False),            # EXACT mode: no schedule
    dict(two_tables=True),             # the sharded passes' x2
    dict(reduce=nat.MEAN), dict(reduce=nat.MAX), dict(reduce=nat.MIN),
    dict(f_in=100), dict(f_in=256), dict(f_out=100), dict(f_out=0),
    dict(C=3), dict(C=16), dict(T=0),
])
def test_unsupported_launches_never_slice(kw):
    assert not _wanted(mode=True, **kw)


@pytest.mark.parametrize("val,mode", [(None, None), ("", None), ("0", False), ("false", False), ("1", True)])
def test_env_mode(monkeypatch, val, mode):
    if val is None:
        monkeypatch.delenv("KGX_FUSED_SLICE", raising=False)
    else:
        monkeypatch.setenv("KGX_FUSED_SLICE", val)
    assert S.env_mode() is mode


def test_env_params(monkeypatch):
    for k in ("KGX_FUSED_SLICE_T", "KGX_FUSED_SLICE_C", "KGX_FUSED_SLICE_HEAD"):
        monkeypatch.delenv(k, raising=False)
    assert S.env_params() == (S.DEFAULT_T, S.DEFAULT_C, S.DEFAULT_HEAD_SHARE)
    monkeypatch.setenv("KGX_FUSED_SLICE_T", "256")
    monkeypatch.setenv("KGX_FUSED_SLICE_C", "4")
    monkeypatch.setenv("KGX_FUSED_SLICE_HEAD", "1.5")
    assert S.env_params() == (256, 4, 1.0)


def test_effective_threshold_keeps_hub_rows_sliced():
    assert S.effective_threshold(128, 2048) == 128
    assert S.effective_threshold(4096, 2048) == 2048  # today's hub rows are always sliced
    assert S.effective_threshold(128, 0) == 128       # a graph that never splits


@pytest.mark.parametrize("resident,tiles,C,grid", [
    (384, 10_000, 8, 384),   # the CU-split head: 2 blocks on each of 192 CUs
    (372, 10_000, 8, 368),   # a shared GPU's 31 / 32: rounded down to a multiple of 8
    (512, 3, 8, 24),         # short lists: one block per tile
    (512, 3, 4, 12),
    (7, 100, 8, 0),          # fewer resident blocks than lists: the unsliced launch
    (3, 100, 4, 0),
    (8, 100, 8, 8),
    (512, 0, 8, 0),
    (512, 10, 0, 0),
])
def test_grid_is_a_multiple_of_the_lists_or_falls_back(resident, tiles, C, grid):
    got = nat.lib().kgx_slice_grid(resident, tiles, C)
    assert got == grid
    assert C <= 0 or got % C == 0


@pytest.mark.parametrize("C", [4, 8])
def test_class_hash_matches_the_library_and_mixes_strides(C):
    L = nat.lib()
    ids = list(range(0, 4096)) + [2**31 - 1, 10_000_000, 123_456_789]
    for c in ids:
        assert L.kgx_slice_class(c, C) == S.slice_class(c, C)
        assert 0 <= S.slice_class(c, C) < C
    # not col % C: ids with one residue (a strided user numbering) still spread over every class
    for stride in (C, 64, 1024):
        seen = {S.slice_class(c, C) for c in range(0, 4096 * stride, stride)}
        assert seen == set(range(C))
