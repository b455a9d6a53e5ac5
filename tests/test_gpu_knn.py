"""kgx_knn (torch.ops.kgx.knn, knn / knn_graph / knn_csr) and EdgeConv / DynamicEdgeConv against the
restatements of tests/knn_ref.py, on one fixture of segment sizes [1, 5, 6, 63, 64, 65, 130, 0, 17]: query
tiles of 64 that straddle segments, an empty segment, segments with fewer than k + 1 points.

Lattice inputs (integers in [-8, 8]) and the direct path (D <= 8) are compared bit for bit.  The MFMA path on
random inputs is held to the project's own bound B = 1e-5 * max(1, A), A = sum_d (y_d^2 + x_d^2 + 2 |y_d x_d|),
for every query.  Layers: 1e-5 * max(1, max |ref|) per tensor against the float64 literal form.

Largest err / bound seen (MI355X, all cases of this module):
  dist2 against float64: 0.012 (D = 9), 0.017 (D = 40), 0.021 (D = 64), 0.039 (D = 256); no returned neighbour lies
  beyond the float64 k-th smallest distance (slack 0.000 of 2 B)
  layers, worst tensor: 0.056 (one hidden layer, max, EdgeConv); 0.013 - 0.020 on the other paths
"""

from __future__ import annotations

import ctypes
import dataclasses
import functools

import numpy as np
import pytest
import torch

import keras_geometric_amd as kgx
import knn_ref as R
from keras_geometric_amd import _native as nat
from keras_geometric_amd import graph as G

gpu = pytest.mark.gpu
SEG, SEG_Y = R.offsets(R.SIZES), R.offsets(R.SIZES_Y)
N, DEV = int(SEG[-1]), "cuda"


@functools.lru_cache(maxsize=None)
def _points(D, kind, n=N):
    if kind == "lattice":
        return R.lattice(n, D, D)
    return np.random.default_rng(100 + D).standard_normal((n, D)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _table(D, kind, bipartite=False):
    """The restatement's distance table: the direct path's fp32 arithmetic, float64 for the MFMA path."""
    x = _points(D, kind)
    y = _points(D, kind, int(SEG_Y[-1]))[::-1].copy() if bipartite else x
    return R.dist2_f32(y, x) if D <= 8 else R.dist2_f64(y, x)


def _knn(x, y, k, seg_x, seg_y, excl):
    nbr, d = torch.ops.kgx.knn(torch.from_numpy(x).to(DEV), torch.from_numpy(y).to(DEV), torch.from_numpy(seg_x),
                               torch.from_numpy(seg_y), k, excl, True)
    return nbr.cpu().numpy(), d.cpu().numpy()


@gpu
@pytest.mark.parametrize("excl", [True, False])
@pytest.mark.parametrize("k", [1, 5, 16, 64])
@pytest.mark.parametrize("D", [1, 3, 8, 9, 32, 33, 64, 256])
def test_lattice_exact(D, k, excl):
    x = _points(D, "lattice")
    ref_n, ref_d = R.knn_table(_table(D, "lattice"), SEG, SEG, k, excl)
    nbr, d = _knn(x, x, k, SEG, SEG, excl)
    assert np.array_equal(nbr, ref_n) and np.array_equal(d.view(np.int32), ref_d.astype(np.float32).view(np.int32))


@gpu
@pytest.mark.parametrize("D", [3, 33])
def test_bipartite_exact(D):
    x, y = _points(D, "lattice"), _points(D, "lattice", int(SEG_Y[-1]))[::-1].copy()
    ref_n, ref_d = R.knn_table(_table(D, "lattice", True), SEG, SEG_Y, 5, False)
    nbr, d = _knn(x, y, 5, SEG, SEG_Y, False)
    assert np.array_equal(nbr, ref_n) and np.array_equal(d.view(np.int32), ref_d.astype(np.float32).view(np.int32))
    pub = kgx.knn(torch.from_numpy(x).to(DEV), torch.from_numpy(y).to(DEV), 5, torch.from_numpy(R.batch_of(R.SIZES)).to(DEV),
                  torch.from_numpy(R.batch_of(R.SIZES_Y)).to(DEV))
    assert np.array_equal(pub.cpu().numpy(), ref_n)


@gpu
def test_ld_nbr_view_leaves_other_columns():
    x = torch.from_numpy(_points(9, "lattice")).to(DEV)
    wide = torch.full((N, 8), 77, dtype=torch.int32, device=DEV)
    n = ctypes.c_size_t(0)
    nat.check(nat.lib().kgx_knn_workspace_bytes(N, N, 9, len(SEG) - 1, ctypes.byref(n)), "ws")
    ws = torch.empty(n.value, dtype=torch.uint8, device=DEV)
    a = nat.KnnArgs(struct_size=ctypes.sizeof(nat.KnnArgs), x=x.data_ptr(), ld_x=9, P=N, y=x.data_ptr(), ld_y=9, Q=N, D=9, k=5,
                    seg_x=SEG.ctypes.data, seg_y=SEG.ctypes.data, S=len(SEG) - 1, exclude_self=1, nbr=wide.data_ptr(),
                    ld_nbr=8, dist2=None, ld_dist2=0, workspace=ws.data_ptr(), workspace_bytes=n.value)
    nat.check(nat.lib().kgx_knn(ctypes.byref(a), nat.stream(x.device)), "kgx_knn")
    got = wide.cpu().numpy()
    assert np.array_equal(got[:, :5], R.knn_table(_table(9, "lattice"), SEG, SEG, 5, True)[0]) and (got[:, 5:] == 77).all()


@gpu
@pytest.mark.parametrize("D", [1, 3, 8])
def test_random_direct_path_bit_equal(D):
    x = _points(D, "random")
    ref_n, ref_d = R.knn_table(_table(D, "random"), SEG, SEG, 16, True)
    nbr, d = _knn(x, x, 16, SEG, SEG, True)
    assert np.array_equal(nbr, ref_n) and np.array_equal(d.view(np.int32), ref_d.astype(np.float32).view(np.int32))


@gpu
@pytest.mark.parametrize("D", [9, 40, 64, 256])
def test_random_mfma_path_within_bound(D):
    k, x = 16, _points(D, "random")
    d64 = _table(D, "random")
    ax, n2 = np.abs(x.astype(np.float64)), (x.astype(np.float64) ** 2).sum(1)
    B = 1e-5 * np.maximum(1.0, n2[:, None] + n2[None, :] + 2.0 * ax @ ax.T)
    ref_n, ref_d = R.knn_table(d64, SEG, SEG, k, True)
    nbr, d = _knn(x, x, k, SEG, SEG, True)
    assert np.array_equal(_knn(x, x, k, SEG, SEG, True)[0], nbr)  # the same bits from run to run
    ok, safe, rows = nbr >= 0, np.maximum(nbr, 0), np.arange(N)[:, None]
    seg = np.searchsorted(SEG, np.arange(N), side="right") - 1
    assert np.array_equal(ok, ref_n >= 0) and np.isinf(d[~ok]).all()  # min(k, segment size - 1) for every query
    assert ((nbr >= SEG[seg][:, None]) & (nbr < SEG[seg + 1][:, None]) & (nbr != rows))[ok].all()
    srt = np.sort(np.where(ok, nbr, -1 - np.arange(k)[None, :]), axis=1)
    assert (srt[:, 1:] != srt[:, :-1]).all()  # distinct
    assert (d[:, 1:] >= d[:, :-1]).all() and (nbr[:, 1:] > nbr[:, :-1])[(d[:, 1:] == d[:, :-1]) & ok[:, 1:]].all()
    true_d, bound = d64[rows, safe], B[rows, safe]
    err = np.where(ok, np.abs(d - true_d) / bound, 0.0).max()
    kth = np.where(ok, ref_d, -np.inf).max(axis=1, keepdims=True)  # the float64 k-th (or last) smallest
    slack = np.where(ok, (true_d - kth) / (2.0 * bound), 0.0).max()
    print(f"D = {D}: dist2 err / bound {err:.3f}, (d64 - kth) / 2 bound {slack:.3f}")
    assert err <= 1.0 and slack <= 1.0


@gpu
@pytest.mark.parametrize("D", [3, 40])
def test_empty_queries_and_nan_rows(D):
    x = _points(D, "random").copy()
    x[70] = np.nan
    nbr, d = _knn(x, x, 5, SEG, SEG, True)
    assert not (nbr == 70).any() and (nbr[70] == -1).all() and np.isinf(d[70]).all()
    assert (nbr[[69, 71]] >= 0).all()
    nbr, d = _knn(x, x[:0], 5, SEG, np.zeros_like(SEG), False)
    assert nbr.shape == (0, 5) and d.shape == (0, 5)


@gpu
def test_knn_csr_and_its_transpose():
    x = _points(3, "lattice")
    ref_n, _ = R.knn_table(_table(3, "lattice"), SEG, SEG, 5, True)
    g = kgx.knn_csr(torch.from_numpy(x).to(DEV), 5, torch.from_numpy(R.batch_of(R.SIZES)).to(DEV))
    src, _ = R.edges_of(ref_n)
    assert np.array_equal(g.rowptr.cpu().numpy(), np.concatenate([[0], np.cumsum((ref_n >= 0).sum(1))]))
    assert np.array_equal(g.col.cpu().numpy(), src) and g.kept == src.size
    t, want = g.extras["T"], G.transpose(dataclasses.replace(g, extras={}))
    for name in ("rowptr", "col", "eid", "deg"):
        assert torch.equal(getattr(t, name), getattr(want, name)), name


_ACT = {"relu": torch.relu, "leaky_relu": lambda t: torch.nn.functional.leaky_relu(t, 0.2)}


def _layer_run(layer, inputs, weights):
    x = inputs[0].clone().requires_grad_(True)
    layer([x, inputs[1]])  # lazy build
    layer.set_weights(weights)
    layer.zero_grad(set_to_none=True)
    out = layer([x, inputs[1]])
    out.backward(torch.from_numpy(_gout(out.shape[1])).to(DEV))
    return [out.detach(), x.grad] + [w.grad for w in layer.weights]


def _gout(H):
    return np.random.default_rng(7).standard_normal((N, H)).astype(np.float32)


@gpu
@pytest.mark.parametrize("dynamic", [False, True])
@pytest.mark.parametrize("hidden,act,aggr", [(None, "relu", "max"), (None, "leaky_relu", "max"), ([12], "relu", "max"),
                                             (None, "relu", "mean")])
def test_edge_conv_layers(hidden, act, aggr, dynamic):
    F, H, k = 8, 16, 5
    pos = _points(F if dynamic else 3, "lattice")  # the graph's coordinates: exact, so the graph is the restatement's
    assert len(np.unique(pos, axis=0)) == N or not dynamic  # no duplicate feature rows: no tie in a max's gradient
    feats = pos if dynamic else _points(F, "random")
    src, dst = R.edges_of(R.knn_table(_table(pos.shape[1], "lattice"), SEG, SEG, k, True)[0])
    rng = np.random.default_rng(11)
    widths = [2 * F] + (hidden or []) + [H]
    layers = [(0.3 * rng.standard_normal((a, b)).astype(np.float32), 0.3 * rng.standard_normal(b).astype(np.float32))
              for a, b in zip(widths[:-1], widths[1:])]
    ref_out, ref_dx, ref_dw = R.edge_conv64(feats, layers, src, dst, aggr, _ACT[act], _gout(H))
    batch = torch.from_numpy(R.batch_of(R.SIZES)).to(DEV)
    kw, xt = dict(hidden=hidden, activation=act, aggregator=aggr), torch.from_numpy(feats).to(DEV)
    if dynamic:
        layer, inputs = kgx.DynamicEdgeConv(H, k, **kw), [xt, batch]
    else:
        layer, inputs = kgx.EdgeConv(H, **kw), [xt, kgx.knn_graph(torch.from_numpy(pos).to(DEV), k, batch)]
    assert layer.commuted == (hidden is None and aggr == "max")
    weights = [a for pair in layers for a in pair]
    got = _layer_run(layer, inputs, weights)
    worst = 0.0
    for name, g, r in zip(["out", "dx"] + ["dw"] * len(ref_dw), got, [ref_out, ref_dx] + ref_dw):
        ratio = np.abs(g.cpu().numpy() - r).max() / (1e-5 * max(1.0, np.abs(r).max()))
        worst = max(worst, ratio)
        assert ratio <= 1.0, (name, ratio)
    assert not got[0][0].any()  # the segment of one point: a node without neighbours gives 0
    if layer.commuted:  # against the composed path directly, at twice the bound
        layer.commuted = False
        for g, c, r in zip(got, _layer_run(layer, inputs, weights), [ref_out, ref_dx] + ref_dw):
            assert (g - c).abs().max().item() <= 2e-5 * max(1.0, np.abs(r).max())
    print(f"hidden {hidden} {act} {aggr} dynamic {dynamic}: err / bound {worst:.3f}")
