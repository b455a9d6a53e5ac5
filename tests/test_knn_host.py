"""CPU-only checks for the k-NN graph build: tests/knn_ref.py against a brute-force float64 sort, the composed (CPU)
form of knn_graph against it, the exports, and the argument errors of the Python functions and of kgx_knn."""

from __future__ import annotations

import ctypes

import numpy as np
import pytest
import torch

import keras_geometric_amd as kgx
import knn_ref as R
from keras_geometric_amd import _native as nat

SEG = R.offsets(R.SIZES)
N = int(SEG[-1])
BAD, DESC, BIG = np.array([0, 41], np.int32), np.array([0, 50, 40], np.int32), np.array([0, 2**30], np.int32)


def test_restatement_against_brute_force():
    x = R.lattice(N, 3, 3)
    d2 = R.dist2_f64(x, x)
    assert np.array_equal(d2.astype(np.float32), R.dist2_f32(x, x))  # lattice: both forms are exact
    nbr, dist = R.knn_table(d2, SEG, SEG, 5, True)
    for i in range(N):
        s = np.searchsorted(SEG, i, side="right") - 1
        want = sorted((d2[i, c], c) for c in range(SEG[s], SEG[s + 1]) if c != i)[:5]
        assert [c for _, c in want] == [c for c in nbr[i] if c >= 0]
        assert [d for d, _ in want] == [d for d in dist[i] if d < np.inf]
    assert (nbr[0] == -1).all() and np.isinf(dist[0]).all()  # the segment of one point


@pytest.mark.parametrize("loop", [False, True])
def test_cpu_knn_graph_equals_restatement(loop):
    x = R.lattice(N, 3, 3)
    nbr, _ = R.knn_table(R.dist2_f32(x, x), SEG, SEG, 5, not loop)
    src, dst = R.edges_of(nbr)
    ei = kgx.knn_graph(torch.from_numpy(x), 5, torch.from_numpy(R.batch_of(R.SIZES)), loop=loop)
    assert ei.dtype == torch.int32 and np.array_equal(ei.numpy(), np.stack([src, dst]))


def test_exports_and_python_argument_errors():
    for name in ("knn", "knn_graph", "knn_csr", "knn_supported", "EdgeConv", "DynamicEdgeConv"):
        assert name in kgx.__all__ and hasattr(kgx, name)
    assert kgx.knn_supported(256, 64) and not kgx.knn_supported(257, 8) and not kgx.knn_supported(3, 65)
    x = torch.zeros(6, 3)
    with pytest.raises(ValueError, match="sorted"):
        kgx.knn_graph(x, 2, torch.tensor([0, 1, 0, 1, 1, 1]))
    for exc, call in ((ValueError, lambda: kgx.knn(x, torch.zeros(4, 2), 2)), (ValueError, lambda: kgx.knn_graph(x, 0)),
                      (TypeError, lambda: kgx.knn_graph(x.double(), 2)), (ValueError, lambda: kgx.EdgeConv(8, aggregator="std"))):
        with pytest.raises(exc):
            call()
    layer = kgx.DynamicEdgeConv(8, k=4, hidden=[6], aggregator="mean", activation="leaky_relu", name="dec")
    assert kgx.DynamicEdgeConv.from_config(layer.get_config()).get_config() == layer.get_config()
    assert kgx.EdgeConv(8).commuted and not layer.commuted and not kgx.EdgeConv(8, activation="gelu").commuted
    relu = lambda t: t * t  # noqa: E731  (a user callable is judged by identity, never by its name)
    relu.__name__ = "relu"
    assert not kgx.EdgeConv(8, activation=relu).commuted and kgx.EdgeConv(8, activation=torch.relu).commuted
    nbr, d2 = kgx.knn(torch.tensor([[0.0, 0.0], [1.0, 1.0]]), torch.zeros(1, 2), 2, [0, 0], torch.tensor([0]),
                      return_dist=True)  # a list and a tensor batch together; d2 = 2 exactly, not sqrt(2) squared
    assert nbr.tolist() == [[0, 1]] and d2.tolist() == [[0.0, 2.0]]


def _call(**kw):
    seg = np.array([0, 40], np.int32)
    a = dict(struct_size=ctypes.sizeof(nat.KnnArgs), x=16, ld_x=3, P=40, y=16, ld_y=3, Q=40, D=3, k=4, seg_x=seg.ctypes.data,
             seg_y=seg.ctypes.data, S=1, exclude_self=0, nbr=16, ld_nbr=4, dist2=None, ld_dist2=4, workspace=16,
             workspace_bytes=1 << 20)  # valid but for its (never read) pointers: only what a case changes is wrong
    a.update({key: v.ctypes.data if isinstance(v, np.ndarray) else v for key, v in kw.items()})
    return nat.lib().kgx_knn(ctypes.byref(nat.KnnArgs(**a)), None)


@pytest.mark.parametrize("kw,text", [
    (dict(struct_size=8), b"struct_size"), (dict(k=0), b"k = 0"), (dict(k=65), b"k = 65"), (dict(D=0), b"D = 0"),
    (dict(D=257), b"D = 257"), (dict(ld_x=2), b"leading dimension"), (dict(ld_nbr=3), b"leading dimension"),
    (dict(dist2=16, ld_dist2=3), b"leading dimension"), (dict(nbr=None), b"null pointer (x, y, nbr)"),
    (dict(x=None), b"null pointer (x, y, nbr)"), (dict(seg_y=None), b"null pointer (seg_x, seg_y)"),
    (dict(seg_x=BAD), b"ascend"), (dict(seg_x=DESC, seg_y=DESC, S=2), b"ascend"),
    (dict(Q=2**30, P=2**30, k=2, seg_x=BIG, seg_y=BIG), b"Q k"), (dict(workspace_bytes=0), b"workspace"),
])
def test_c_argument_errors_before_any_device_call(kw, text):
    assert _call(**kw) == nat.KGX_ERR_ARG
    assert text in nat.lib().kgx_last_error()
    assert _call(Q=0, seg_y=np.array([0, 0], np.int32)) == nat.KGX_OK  # nothing launched: no device is needed
