"""Fused multi-aggregation, list aggregators and PNAConv without a device (CPU).

* kgx_multi_aggr / kgx_multi_aggr_partials_floats are declared, exported and
  bound; kgx_version() is 2.
* Every argument error is KGX_ERR_ARG before any device work: the CSR / table
  pointers are dummy addresses and `out` is a sentinel-filled host buffer that
  must come back untouched.
* The partial-state size for every class of reducer subset.
* MultiAggregator / MessagePassing / PNAConv name validation and get_config.
* tests/multi_aggr_ref.py's float64 restatement equals oracle.reference.aggregate
  block for block (to fp32 rounding), and its concatenation keeps the order.
"""

import ctypes
import re
from pathlib import Path

import numpy as np
import pytest
import torch

import multi_aggr_ref as MR

ROOT = Path(__file__).resolve().parents[1]
P = ctypes.c_void_p(256)  # a dummy non-null pointer: never dereferenced before the argument checks pass
SUM, MEAN, MAX, MIN, STD = range(5)
SENTINEL = -123.5


@pytest.fixture(scope="module")
def lib():
    from keras_geometric_amd import _native

    return _native.lib()


def _ints(ids):
    return (ctypes.c_int * max(len(ids), 1))(*ids)


def _call(lib, *, reduces=(MEAN, MAX, MIN, STD), n_red=None, null_reduces=False, rowptr=P, rows=P, n_rows=7,
          items=None, n_items=0, split=None, n_split=0, idx=P, table=P, ld_table=8, F=8, out=True, ld_out=None,
          partials=None, partials_floats=0):
    """kgx_multi_aggr on dummy pointers; returns (status, out buffer untouched?)."""
    n_red = len(reduces) if n_red is None else n_red
    ld_out = max(n_red, 1) * max(F, 0) if ld_out is None else ld_out
    buf = np.full(7 * 5 * 8 + 64, SENTINEL, dtype=np.float32)
    rc = lib.kgx_multi_aggr(
        n_red, None if null_reduces else _ints(list(reduces)), rowptr, rows, n_rows, items, n_items, split, n_split,
        idx, table, ld_table, F, ctypes.c_void_p(buf.ctypes.data) if out else None, ld_out, partials, partials_floats,
        None)
    return rc, bool((buf == SENTINEL).all())


def test_declared_exported_bound_and_version(lib):
    import keras_geometric_amd as kgx
    from keras_geometric_amd import _native

    header = (ROOT / "include" / "kgx.h").read_text()
    for name in ("kgx_multi_aggr", "kgx_multi_aggr_partials_floats"):
        assert re.search(rf"^int {name}\(", header, flags=re.M), name
        assert hasattr(lib, name), name
        assert name in _native.exported_symbols(), name
    assert lib.kgx_version() == 2
    assert "PNAConv" in kgx.__all__ and kgx.PNAConv is kgx.layers.PNAConv
    assert "MultiAggregator" in kgx.layers.__all__
    assert callable(kgx.ops.multi_aggregate)


@pytest.mark.parametrize("kw, word", [
    (dict(null_reduces=True), b"null"), (dict(rowptr=None), b"null"), (dict(rows=None), b"null"),
    (dict(idx=None), b"null"), (dict(table=None), b"null"), (dict(out=False), b"null"),
    (dict(reduces=(), n_red=0), b"n_red"), (dict(reduces=(0, 1, 2, 3, 4), n_red=6), b"n_red"),
    (dict(reduces=(MEAN, 5)), b"unknown or repeated"), (dict(reduces=(MEAN, -1)), b"unknown or repeated"),
    (dict(reduces=(MAX, MEAN, MAX)), b"unknown or repeated"),
    (dict(n_rows=-1), b"negative"), (dict(F=-1), b"negative"), (dict(items=P, n_items=-1), b"negative"),
    (dict(items=P, n_items=3, split=P, n_split=-1), b"negative"), (dict(partials_floats=-1), b"negative"),
    (dict(ld_out=31), b"ld_out"),            # 4 blocks of 8 need 32
    (dict(ld_table=7), b"leading dimension"), (dict(ld_table=1 << 31), b"leading dimension"),
    (dict(items=P, n_items=9, split=None, n_split=2, partials=P, partials_floats=1 << 20), b"split"),
    (dict(items=P, n_items=9, split=P, n_split=2, partials=None, partials_floats=0), b"split"),
    # two split rows need at least two slots of 4 * 8 + 4 floats
    (dict(items=P, n_items=9, split=P, n_split=2, partials=P, partials_floats=2 * 36 - 1), b"too small"),
])
def test_argument_errors_without_device(lib, kw, word):
    rc, untouched = _call(lib, **kw)
    assert rc == 1, lib.kgx_last_error()
    assert word in lib.kgx_last_error().lower(), lib.kgx_last_error()
    assert untouched


def test_empty_work_is_ok_without_device(lib):
    """n_rows == 0 and F == 0 return KGX_OK after the checks, before any device work."""
    assert _call(lib, n_rows=0) == (0, True)
    assert _call(lib, F=0, ld_table=0) == (0, True)


@pytest.mark.parametrize("names, sections, tail", [
    (["sum"], 1, 0), (["mean"], 1, 0), (["sum", "mean"], 1, 0),          # one shared sum section
    (["max"], 1, 0), (["min"], 1, 0), (["max", "min"], 2, 0),
    (["mean", "max"], 2, 0), (["sum", "max", "min"], 3, 0),
    (["std"], 2, 4), (["mean", "std"], 2, 4), (["max", "std"], 3, 4),     # std: sum + M2 + the chunk length
    (MR.PNA_FOUR, 4, 4), (MR.ALL_FIVE, 4, 4),
])
def test_partials_floats(lib, names, sections, tail):
    from keras_geometric_amd import _native, ops

    ids = [_native.REDUCE_IDS[n] for n in names]
    for n_slots, F in [(0, 8), (1, 1), (7, 100), (1000, 260)]:
        v = ctypes.c_int64(-1)
        assert lib.kgx_multi_aggr_partials_floats(len(ids), _ints(ids), n_slots, F, ctypes.byref(v)) == 0
        assert v.value == n_slots * (sections * F + tail)
        assert ops.multi_aggr_partials_floats(names, n_slots, F) == v.value
    v = ctypes.c_int64(-1)
    assert lib.kgx_multi_aggr_partials_floats(len(ids), _ints(ids), -1, 8, ctypes.byref(v)) == 1
    assert lib.kgx_multi_aggr_partials_floats(len(ids), _ints(ids), 1, 8, None) == 1
    assert lib.kgx_multi_aggr_partials_floats(2, _ints([1, 1]), 1, 8, ctypes.byref(v)) == 1
    assert v.value == -1


def test_gathers_in_flight_rule():
    """The row degrees of the boundary graph bracket the kernel's U at every tested F."""
    from keras_geometric_amd import ops

    assert [ops.multi_aggr_gathers(F) for F in (1, 3, 4, 100, 128, 256, 260, 512, 516)] == [6, 6, 6, 6, 6, 6, 4, 4, 2]
    for F in (1, 3, 4, 100, 128, 260):
        U = ops.multi_aggr_gathers(F)
        assert {U - 1, U, U + 1, 2 * U + 1} <= set(MR.BOUNDARY_DEGREES)


def test_multi_aggregator_validation_and_name():
    from keras_geometric_amd.layers import AggregatorFactory, MultiAggregator

    a = AggregatorFactory.create_multi(["mean", "max", "std"])
    assert isinstance(a, MultiAggregator) and a.name == "mean+max+std" and a.names == ["mean", "max", "std"]
    with pytest.raises(ValueError, match=r"Invalid aggregator: median\. Available aggregators: \['mean', 'max', "
                                         r"'sum', 'min', 'std'\]"):
        MultiAggregator(["mean", "median"])
    with pytest.raises(ValueError, match="at least one"):
        MultiAggregator([])
    with pytest.raises(ValueError, match="repeated"):
        MultiAggregator(["max", "mean", "max"])
    assert list(AggregatorFactory._AGGREGATORS) == ["mean", "max", "sum", "min", "std"]  # registry unchanged


def test_ops_reducer_list_validation():
    from keras_geometric_amd import ops

    assert ops._reduce_list(["std", "sum"]) == [4, 0] and ops._reduce_list("max") == [2]
    for bad in ([], ["sum", "sum"], ["sum", "median"], [0, 5], ["sum", "mean", "max", "min", "std", "sum"]):
        with pytest.raises(ValueError):
            ops._reduce_list(bad)


def test_message_passing_list_config():
    from keras_geometric_amd.layers import MessagePassing, MultiAggregator

    mp = MessagePassing(aggregator=["mean", "max"], exact=True)
    assert isinstance(mp._aggregator, MultiAggregator) and mp.aggregator_name == "mean+max"
    assert mp.get_config()["aggregator"] == ["mean", "max"]
    assert mp.compute_output_shape([(None, 8), (2, None)]) == (None, 16)
    assert MessagePassing(aggregator=("std", "min")).get_config()["aggregator"] == ["std", "min"]
    assert MessagePassing(aggregator="sum").get_config()["aggregator"] == "sum"  # the string path as before
    with pytest.raises(ValueError, match="Invalid aggregator: nope"):
        MessagePassing(aggregator=["mean", "nope"])


def test_pna_validation_and_config():
    from keras_geometric_amd import PNAConv

    layer = PNAConv(16)
    cfg = layer.get_config()
    assert cfg["aggregators"] == ["mean", "max", "min", "std"]
    assert cfg["scalers"] == ["identity", "amplification", "attenuation"]
    assert cfg["delta"] is None and cfg["output_dim"] == 16 and cfg["root_weight"] and cfg["use_bias"]
    assert cfg["activation"] is None and "aggregator" not in cfg
    again = PNAConv(**cfg)
    assert again.get_config() == cfg
    cfg2 = PNAConv(4, aggregators=["sum", "std"], scalers=["attenuation"], delta=1.25, root_weight=False,
                   activation="relu", exact=True).get_config()
    assert (cfg2["aggregators"], cfg2["scalers"], cfg2["delta"], cfg2["root_weight"], cfg2["activation"],
            cfg2["exact"]) == (["sum", "std"], ["attenuation"], 1.25, False, "relu", True)
    with pytest.raises(ValueError, match="Invalid aggregator: var"):
        PNAConv(8, aggregators=["mean", "var"])
    with pytest.raises(ValueError, match="Invalid scaler: linear"):
        PNAConv(8, scalers=["identity", "linear"])
    with pytest.raises(ValueError):
        PNAConv(8, aggregators=[])
    with pytest.raises(ValueError):
        PNAConv(8, scalers=[])
    with pytest.raises(ValueError):
        PNAConv(8, scalers=["identity", "identity"])
    from keras_geometric_amd.layers import pna_conv

    assert "no reference counterpart" in pna_conv.__doc__


def test_average_log_degree_matches_float64():
    from keras_geometric_amd import PNAConv

    src, dst, degs = MR.boundary_graph()
    n = len(degs)
    want = float(np.log(degs.astype(np.float64) + 1.0).mean())
    assert abs(MR.average_log_degree_f64(dst, n) - want) < 1e-12
    assert abs(PNAConv.average_log_degree(np.stack([src, dst]), n) - want) < 1e-12
    assert abs(PNAConv.average_log_degree(torch.as_tensor(np.stack([src, dst]).T.copy()), n) - want) < 1e-12


def test_restatement_equals_the_oracle_block_for_block():
    """float64 restatement vs oracle.reference.aggregate (fp32) on the boundary graph:
    column block k of the concatenation is aggregator names[k]."""
    from keras_geometric_amd.layers import MultiAggregator

    src, dst, degs = MR.boundary_graph()
    n = len(degs)
    x = MR.features(n, 5)
    msg = x[torch.as_tensor(src).long()]
    tgt = torch.as_tensor(dst)
    for names in (MR.ALL_FIVE, MR.PNA_FOUR, ["std", "min", "sum", "max", "mean"], ["max", "std"]):
        names = MultiAggregator(names).names  # the block order is the aggregator's own list
        ref = MR.blocks_reference(names, msg, tgt, n)
        f64 = MR.multi_aggregate_f64(names, msg, tgt, n)
        assert ref.shape == f64.shape == (n, 5 * len(names))
        for k, name in enumerate(names):
            blk = slice(5 * k, 5 * k + 5)
            assert torch.equal(ref[:, blk], MR.R.aggregate(name, msg, tgt, n)), name
            assert MR.scaled_err(ref[:, blk], f64[:, blk]) <= 1e-5, name
    # empty rows give 0 in every block; a one-edge row has std 0
    assert torch.equal(f64[0], torch.zeros_like(f64[0])) and degs[0] == 0


def test_restatement_gradient_conventions():
    """sum / mean / max / min gradients against hand values; std's count <= 1 rows give NaN."""
    from keras_geometric_amd.layers import MultiAggregator

    assert MultiAggregator(["sum", "std"]).reduce == "std"  # the take() rule of the std path applies
    msg = torch.tensor([[1.0], [3.0], [3.0], [7.0]], dtype=torch.float64, requires_grad=True)
    tgt = torch.tensor([0, 0, 0, 1])
    def grad(name):
        return torch.autograd.grad(MR.aggregate_f64(name, msg, tgt, 3).sum(), msg)[0].flatten()

    assert grad("sum").tolist() == [1, 1, 1, 1] and grad("mean").tolist() == [1 / 3, 1 / 3, 1 / 3, 1]
    assert grad("max").tolist() == [0, 0.5, 0.5, 1] and grad("min").tolist() == [1, 0, 0, 1]  # ties share evenly
    gd = grad("std")
    assert torch.isnan(gd[3]) and torch.isfinite(gd[:3]).all()
    # in the concatenation the one-message row is NaN whatever the cotangent: 0 * sqrt'(0)
    out = MR.multi_aggregate_f64(["sum", "std"], msg, tgt, 3)
    assert torch.isnan(torch.autograd.grad(out[:, 0].sum(), msg)[0][3])
