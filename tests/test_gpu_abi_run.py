"""The struct entry points against the positional ones and the Python layer (GPU).

kgx_spmm / kgx_spmm_gemm are the minimal positional bindings; each must equal
kgx_spmm_run / kgx_spmm_gemm_run given the equivalent struct, and a
kgx_fused_args filled by hand with the graph's real short-row boundary, tiny
records and sliced schedule must equal kops.aggregate_transform on the same
graph.  Every path here is deterministic (ordered fix-up, no atomics), so the
comparisons are torch.equal.

The graph is R-MAT seed 8 at 3000 nodes / 40000 edges with self loops and
split_len 16: 557 rows of in-degree >= 16 (split), 860 of degree 3..7 (the
short-row items past n_long) and 1218 of degree <= 2 (the tiny records).
"""

import ctypes

import numpy as np
import pytest
import torch

from keras_geometric_amd import _native as nat
from keras_geometric_amd import graph as G
from keras_geometric_amd import ops as kops
from keras_geometric_amd import slice as S
from keras_geometric_amd import tiny
from oracle.rmat import rmat_edges, scale_for

pytestmark = pytest.mark.gpu
N = 3000


@pytest.fixture(scope="module")
def graph(dev):
    s, d = rmat_edges(8, scale_for(N), N, 0, 40000)
    ei = torch.from_numpy(np.ascontiguousarray(np.stack([s, d]))).to(dev)
    g = G.build_csr(ei[0].contiguous(), ei[1].contiguous(), N, N, n_features=128, self_loops=True, gcn_norm=True,
                    split_len=16)
    assert g.n_split > 0  # hub rows: partials and the fix-up
    assert 0 < g.n_long < g.n_items  # short-row items past n_long
    deg = g.rowptr[1:] - g.rowptr[:-1]
    assert int((deg <= 2).sum()) > 0  # the degree <= 2 tail
    # its packed records at this size too (by default a tail under 4096 rows stays on the short-row
    # kernel); cached on g, so kops.aggregate_transform launches with them as well
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(tiny, "_MIN_ROWS", 1)
        assert tiny.tiny_pack(g, refresh=True)[0] is not None
    return g


def _tensors(dev, F_in, F_out, seed):
    gen = torch.Generator(device="cpu").manual_seed(seed)
    x = torch.randn(N, F_in, generator=gen).to(dev)
    W = (torch.randn(F_in, F_out, generator=gen) / F_in ** 0.5).to(dev)
    b = torch.randn(F_out, generator=gen).to(dev)
    return x, W, b


def _fused_args(work, reduce, x, W, b, out, partials):
    return nat.FusedArgs(
        struct_size=ctypes.sizeof(nat.FusedArgs), reduce=reduce, work=work, x=nat.addr(x), ld_x=x.stride(0),
        F_in=x.shape[1], W=nat.addr(W), F_out=W.shape[1], bias=nat.addr(b), gin_scale=1.0, out=nat.addr(out),
        ld_out=out.stride(0), partials=nat.addr(partials))


@pytest.mark.parametrize("F", [12, 128])
def test_positional_spmm_equals_run(dev, graph, F):
    g = graph
    x, _, _ = _tensors(dev, F, 4, F)
    b = torch.randn(F, generator=torch.Generator(device="cpu").manual_seed(1)).to(dev)
    partials = torch.empty((g.n_slots, F), device=dev)
    out_p, out_r = torch.full((N, F), float("nan"), device=dev), torch.full((N, F), float("nan"), device=dev)
    L = nat.lib()
    nat.check(L.kgx_spmm(nat.SUM, nat.EPI_BIAS, nat.ptr(g.rowptr), nat.ptr(g.rows), N, nat.ptr(g.items), g.n_items,
                         nat.ptr(g.split), g.n_split, nat.ptr(g.col), nat.ptr(g.w), nat.ptr(x), x.stride(0), F,
                         nat.ptr(out_p), out_p.stride(0), nat.ptr(b), None, 0, 1.0, None, 0.0, 0, nat.ptr(partials),
                         nat.stream(dev)), "kgx_spmm")
    a = nat.SpmmArgs(
        struct_size=ctypes.sizeof(nat.SpmmArgs), reduce=nat.SUM, epilogue=nat.EPI_BIAS,
        work=nat.work(g.rowptr, g.rows, g.items, g.split, g.col, g.w, g.n_items),
        table=nat.addr(x), ld_table=x.stride(0), F=F, out=nat.addr(out_r), ld_out=out_r.stride(0), bias=nat.addr(b),
        gin_scale=1.0, partials=nat.addr(partials))
    nat.check(L.kgx_spmm_run(ctypes.byref(a), nat.stream(dev)), "kgx_spmm_run")
    assert not torch.isnan(out_p).any()
    assert torch.equal(out_p, out_r)


@pytest.mark.parametrize("reduce,weighted", [(nat.SUM, True), (nat.MAX, False)])
def test_positional_spmm_gemm_equals_run(dev, graph, reduce, weighted):
    g = graph
    x, W, b = _tensors(dev, 128, 16, 2)
    w = g.w if weighted else None
    partials = torch.empty((g.n_slots, 128), device=dev)
    out_p, out_r = torch.full((N, 16), float("nan"), device=dev), torch.full((N, 16), float("nan"), device=dev)
    L = nat.lib()
    nat.check(L.kgx_spmm_gemm(reduce, nat.ptr(g.rowptr), nat.ptr(g.rows), N, nat.ptr(g.items), g.n_items,
                              nat.ptr(g.split), g.n_split, nat.ptr(g.col), nat.ptr(w), nat.ptr(x), x.stride(0), 128,
                              nat.ptr(W), 16, nat.ptr(b), 0, 1.0, nat.ptr(out_p), out_p.stride(0), nat.ptr(partials),
                              None, 0, nat.stream(dev)), "kgx_spmm_gemm")
    work = nat.work(g.rowptr, g.rows, g.items, g.split, g.col, w, g.n_items)  # n_long = n_short_end = n_items
    a = _fused_args(work, reduce, x, W, b, out_r, partials)
    nat.check(L.kgx_spmm_gemm_run(ctypes.byref(a), nat.stream(dev)), "kgx_spmm_gemm_run")
    assert not torch.isnan(out_p).any()
    assert torch.equal(out_p, out_r)


@pytest.mark.parametrize("sliced", [False, True])
def test_run_with_the_whole_work_list_equals_aggregate_transform(dev, graph, monkeypatch, sliced):
    """n_long, the tiny records and (sliced) the source-class lists, as ops.py passes them."""
    g = graph
    x, W, b = _tensors(dev, 128, 32, 3)
    T, C, share = S.env_params()
    sl = None
    if sliced:
        monkeypatch.setenv("KGX_FUSED_SLICE", "1")  # this graph is below the default rule's size
        sl = S.sliced_schedule(g, T, C, share, force=True)
        assert sl is not None and sl.n_long == g.n_long
    else:
        monkeypatch.setenv("KGX_FUSED_SLICE", "0")
    ref = kops.aggregate_transform(g, x, W, "sum", weighted=True, bias=b)
    if sliced:
        assert S.sliced_schedule(g, T, C, share) is sl  # the op found the same cached lists
    tpack, tw, n_se, n_tiny2 = tiny.tiny_pack(g)
    assert g.n_long <= n_se < g.n_items
    slots = max(g.n_slots, sl.n_slots if sl is not None else 0)
    partials = torch.empty((slots, 128), device=dev)
    out = torch.full_like(ref, float("nan"))
    a = _fused_args(nat.work(g.rowptr, g.rows, g.items, g.split, g.col, g.w, g.n_long, n_se, tpack, tw, n_tiny2),
                    nat.SUM, x, W, b, out, partials)
    if sl is not None:
        a.slice = nat.Slice(items=nat.addr(sl.items), lists=nat.addr(sl.lists), n_classes=sl.C, tiles=sl.tiles,
                            idx=nat.addr(sl.col), w=nat.addr(sl.w), split=nat.addr(sl.fix), n_split=sl.n_rows,
                            head_short_end=min(sl.head_short_end, n_se))
    nat.check(nat.lib().kgx_spmm_gemm_run(ctypes.byref(a), nat.stream(dev)), "kgx_spmm_gemm_run")
    assert torch.equal(out, ref)
