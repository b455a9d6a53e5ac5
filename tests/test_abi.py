"""The C-ABI library loads and exports every entry point include/kgx.h declares (CPU)."""

import ctypes
import re
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
HEADER = ROOT / "include" / "kgx.h"


def declared_symbols():
    text = HEADER.read_text()
    return sorted(set(re.findall(r"^\s*(?:int|const char\*)\s+(kgx_\w+)\s*\(", text, flags=re.M)))


@pytest.fixture(scope="module")
def lib():
    from keras_geometric_amd import _native

    return _native.lib()


def test_header_declares_entry_points():
    syms = declared_symbols()
    assert "kgx_spmm" in syms and "kgx_csr_build" in syms and "kgx_gatv2" in syms
    assert len(syms) >= 13


def test_every_declared_symbol_is_exported(lib):
    missing = [s for s in declared_symbols() if not hasattr(lib, s)]
    assert not missing, f"libkgx.so lacks {missing}"


def test_binding_covers_header(lib):
    from keras_geometric_amd import _native

    assert set(declared_symbols()) <= set(_native.exported_symbols())


def test_version_and_error_channel(lib):
    assert lib.kgx_version() == 2
    rc = lib.kgx_spmm(99, 0, None, None, 1, None, 0, None, 0, None, None, None, 1, 1, None, 1, None, None, 0,
                      1.0, None, 0.0, 0, None, None)
    assert rc == 1  # KGX_ERR_ARG, no device touched
    assert b"unknown reduce" in lib.kgx_last_error()


def test_argument_validation_without_device(lib):
    from keras_geometric_amd import _native as nat

    # split_len not a power of two
    assert lib.kgx_schedule_build(ctypes.c_void_p(16), 4, 3, None, None, 0, None, None, 0, None, None) == 1
    assert b"power of two" in lib.kgx_last_error()
    # self loops need a square graph
    rc = lib.kgx_csr_build(None, None, 0, 3, 4, nat.CSR_SELF_LOOPS, None, None, None, None, None, None, None, 0,
                           None, None)
    assert rc == 1
    # unsupported GAT shape (too many lanes per row) is reported, not launched
    rc = lib.kgx_gatv2(ctypes.c_void_p(16), ctypes.c_void_p(16), 1, None, 0, None, 0, ctypes.c_void_p(16),
                       ctypes.c_void_p(16), ctypes.c_void_p(16), 64 * 33, ctypes.c_void_p(16), 64, 33, 0.2,
                       ctypes.c_void_p(16), 64 * 33, None, None, None, None, 0.0, 0, None)
    assert rc == 4
    # message dropout only for sums, p in [0, 1)
    rc = lib.kgx_spmm(2, 0, ctypes.c_void_p(16), ctypes.c_void_p(16), 1, None, 0, None, 0, ctypes.c_void_p(16), None,
                      ctypes.c_void_p(16), 4, 4, ctypes.c_void_p(16), 4, None, None, 0, 1.0, ctypes.c_void_p(16), 0.5,
                      1, None, None)
    assert rc == 1 and b"dropout" in lib.kgx_last_error()
    # backward of max/min only; fused accumulate flag validation
    assert lib.kgx_spmm_max_backward(0, 0, None, 0, None, None, 0, 0, None, 0, None, 0, None) == 1
    assert lib.kgx_spmm_max_backward_w(0, 0, None, 0, None, None, None, 0, 0, None, 0, None, 0, None) == 1
    # the unguarded (raw) extreme has no weighted form
    assert lib.kgx_spmm_max_backward_w(nat.MAX, 1, None, 0, None, ctypes.c_void_p(16), None, 0, 0, None, 0, None, 0,
                                       None) == 4
    # rmat argument checks
    assert lib.kgx_rmat_edges(0, 4, 100, 1, 1, 1, 0, 10, None, None, None) == 1


# the rungs the argument structs replaced: eight entry points above the positional kgx_spmm / kgx_spmm_gemm
REMOVED = ([f"kgx_spmm_ex{rung}" for rung in ("", 2)] + [f"kgx_spmm_gemm_ex{rung}" for rung in ("", 2, 3, 4)]
           + [f"kgx_spmm_gemm_f256{rung}" for rung in ("", "_ex")])
RUNS = (("kgx_spmm_run", "SpmmArgs"), ("kgx_spmm_gemm_run", "FusedArgs"), ("kgx_spmm_gemm_f256_run", "FusedArgs"))


def _args(nat, struct, **fields):
    """A zeroed argument struct with its struct_size and `fields` set."""
    cls = getattr(nat, struct)
    return cls(struct_size=ctypes.sizeof(cls), **fields)


@pytest.mark.parametrize("entry,struct", RUNS)
def test_run_rejects_null_and_foreign_struct(lib, entry, struct):
    from keras_geometric_amd import _native as nat

    assert getattr(lib, entry)(None, None) == 1
    a = _args(nat, struct)
    a.struct_size += 8
    assert getattr(lib, entry)(ctypes.byref(a), None) == 1
    assert b"struct_size" in lib.kgx_last_error()


def test_run_argument_validation_without_device(lib):
    from keras_geometric_amd import _native as nat

    p = 16  # a dummy non-null, 16-byte aligned address: every call fails before any device work
    assert lib.kgx_spmm_run(ctypes.byref(_args(nat, "SpmmArgs", reduce=99)), None) == 1
    assert b"unknown reduce" in lib.kgx_last_error()
    # the gather-reduce has no tiny-record path
    assert lib.kgx_spmm_run(ctypes.byref(_args(nat, "SpmmArgs", work=nat.Work(tiny_pack=p))), None) == 1
    assert b"tiny_pack" in lib.kgx_last_error()
    assert lib.kgx_spmm_run(ctypes.byref(_args(nat, "SpmmArgs", work=nat.Work(items=p, n_items=4, n_short_end=3))),
                            None) == 1
    assert b"n_short_end" in lib.kgx_last_error()
    # the 256-wide kernels have no sliced schedule
    assert lib.kgx_spmm_gemm_f256_run(ctypes.byref(_args(nat, "FusedArgs", slice=nat.Slice(n_classes=4))), None) == 1
    assert b"n_classes" in lib.kgx_last_error()
    # a complete sliced schedule with a second table: unsupported, as before the structs
    sliced = _args(nat, "FusedArgs", work=nat.Work(items=p, n_items=4, n_long_items=4, n_short_end=4), x2=p,
                   partials=p, slice=nat.Slice(items=p, lists=p, n_classes=4, tiles=1, idx=p, split=p, n_split=1))
    assert lib.kgx_spmm_gemm_run(ctypes.byref(sliced), None) == 4
    assert b"sliced schedule" in lib.kgx_last_error()


def test_the_ex_ladder_is_gone(lib):
    from keras_geometric_amd import _native

    for name in REMOVED:
        assert not hasattr(lib, name), name
        assert name not in _native.exported_symbols()


def test_library_refuses_cpu_tensors():
    import torch

    from keras_geometric_amd import _native as nat

    with pytest.raises(RuntimeError, match="no CPU path"):
        nat.require_device(torch.zeros(3))
