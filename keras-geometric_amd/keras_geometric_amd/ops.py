"""PyTorch-ROCm operator registration of the kgx C-ABI (torch.ops.kgx.*).

Each op is a `torch.library.custom_op` whose implementation calls straight into
libkgx.so on torch's current HIP stream, with a fake (meta) kernel so that
torch.compile / symbolic tracing sees shapes without running the GPU.

  kgx::spmm   fused gather -> message -> segment {sum,mean,max,min,std} -> epilogue
  kgx::multi_aggr  several of those reducers from one gather, blocks concatenated
  kgx::gatv2  fused GATv2 attention aggregation (optionally with projected edge rows in the score)
  kgx::dot_attention  fused dot-product (query / key / value) attention aggregation
  kgx::softmax_pool  fused segment softmax + weighted sum (attention readouts)
  kgx::edge_dot  edge scores from node rows (link prediction)
  kgx::gather_rows, kgx::scatter_f32   row movement helpers
"""

from __future__ import annotations

import ctypes
import os
import threading
from typing import List, Optional

import torch

from . import _native as nat
from .graph import CSRGraph


def _f32c(t: Optional[torch.Tensor]) -> Optional[torch.Tensor]:
    if t is None:
        return None
    if t.dtype != torch.float32:
        raise TypeError(f"kgx kernels compute in fp32; got {t.dtype}")
    return t.contiguous()


_EXACT_DYN = __import__("os").environ.get("KGX_EXACT_DYN", "1") != "0"


def _spmm_launch(out, reduce, epilogue, table, table2, rowptr, rows, items, split, idx, w, n_slots, n_long, bias,
                 xroot, gin_scale, counters=None, drop_key=None, drop_p=0.0, drop_seed=0):
    """One kgx_spmm_run into out [n_dst > 0, F > 0]: the split rows' partials and
    the kgx_spmm_args by field name (table2: sources >= table.shape[0] are its rows)."""
    F = table.shape[1]
    partials = None
    if items is not None and split is not None and split.shape[0] > 0 and reduce != nat.STD:
        partials = torch.empty((n_slots, F), dtype=torch.float32, device=out.device)
    a = nat.SpmmArgs(
        struct_size=ctypes.sizeof(nat.SpmmArgs), reduce=reduce, epilogue=epilogue,
        work=nat.work(rowptr, rows, items, split, idx, w, n_long),
        table=nat.addr(table), ld_table=table.stride(0), table2=nat.addr(table2),
        n_table1=table.shape[0] if table2 is not None else 0, F=F,
        out=nat.addr(out), ld_out=out.stride(0),
        bias=nat.addr(bias), xroot=nat.addr(xroot), ld_x=xroot.stride(0) if xroot is not None else 0,
        gin_scale=float(gin_scale), drop_p=float(drop_p),
        drop_key=nat.addr(drop_key) if drop_p > 0 else None, drop_seed=int(drop_seed) & (2**64 - 1),
        partials=nat.addr(partials), counters=nat.addr(counters),
    )
    nat.check(nat.lib().kgx_spmm_run(ctypes.byref(a), nat.stream(out.device)), "kgx_spmm")


@torch.library.custom_op("kgx::spmm", mutates_args=())
def spmm(
    table: torch.Tensor,
    rowptr: torch.Tensor,
    rows: torch.Tensor,
    items: Optional[torch.Tensor],
    split: Optional[torch.Tensor],
    idx: torch.Tensor,
    w: Optional[torch.Tensor],
    n_slots: int,
    reduce: int,
    epilogue: int,
    bias: Optional[torch.Tensor],
    xroot: Optional[torch.Tensor],
    gin_scale: float,
    drop_key: Optional[torch.Tensor] = None,
    drop_p: float = 0.0,
    drop_seed: int = 0,
    n_long: int = -1,
) -> torch.Tensor:
    table = _f32c(table)
    w, bias, xroot = _f32c(w), _f32c(bias), _f32c(xroot)
    dev = nat.require_device(table, rowptr, rows, idx, w, bias, xroot, items, split)
    n_dst = rowptr.numel() - 1
    F = table.shape[1]
    out = torch.empty((n_dst, F), dtype=torch.float32, device=dev)
    if n_dst == 0 or F == 0:
        return out
    if items is not None:  # EXACT mode (no items): n_long names the short suffix of the row list (or -1)
        n_long = items.shape[0] if n_long < 0 or n_long > items.shape[0] else n_long
    # EXACT mode: the hub-row kernel hands its items out dynamically (KGX_EXACT_DYN=0: static, A/B only)
    counters = (torch.zeros(2, dtype=torch.int32, device=dev)
                if items is None and reduce != nat.STD and _EXACT_DYN else None)
    _spmm_launch(out, reduce, epilogue, table, None, rowptr, rows, items, split, idx, w, n_slots, n_long, bias, xroot,
                 gin_scale, counters, drop_key, drop_p, drop_seed)
    return out


@spmm.register_fake
def _spmm_fake(table, rowptr, rows, items, split, idx, w, n_slots, reduce, epilogue, bias, xroot, gin_scale,
               drop_key=None, drop_p=0.0, drop_seed=0, n_long=-1):
    return table.new_empty((rowptr.shape[0] - 1, table.shape[1]))


@torch.library.custom_op("kgx::spmm_acc_", mutates_args=("out",))
def spmm_acc_(
    out: torch.Tensor,
    table: torch.Tensor,
    rowptr: torch.Tensor,
    rows: torch.Tensor,
    items: Optional[torch.Tensor],
    split: Optional[torch.Tensor],
    idx: torch.Tensor,
    w: Optional[torch.Tensor],
    n_slots: int,
    n_long: int = -1,
    epilogue: int = 4,
    bias: Optional[torch.Tensor] = None,
    xroot: Optional[torch.Tensor] = None,
    gin_scale: float = 1.0,
    table2: Optional[torch.Tensor] = None,
) -> None:
    """out[i] += SUM_{e in row i} table[idx[e]] (* w[e]) in place (KGX_EPI_ACCUM,
    the default epilogue); any other epilogue overwrites the scheduled rows of
    out (and leaves the rest untouched).  table2: sources >= table.shape[0]
    are rows of table2 (two-table gathers, kgx_spmm_args.table2)."""
    table, w, bias, xroot, table2 = _f32c(table), _f32c(w), _f32c(bias), _f32c(xroot), _f32c(table2)
    nat.require_device(out, table, rowptr, rows, idx, w, items, split, bias, xroot, table2)
    if table2 is not None and (table2.dim() != 2 or table2.shape[1] != table.shape[1]
                               or (table2.shape[0] and table2.stride(0) != table.stride(0))):
        raise ValueError("spmm_acc_: table2 must have table's row width and leading dimension")
    n_dst = rowptr.numel() - 1
    F = table.shape[1]
    if out.dtype != torch.float32 or out.shape != (n_dst, F) or out.stride(1) != 1:
        raise ValueError(f"spmm_acc_: out must be float32 [{n_dst}, {F}] with unit column stride")
    if n_dst == 0 or F == 0:
        return
    n_items = 0 if items is None else items.shape[0]
    n_long = n_items if n_long < 0 or n_long > n_items else n_long
    _spmm_launch(out, nat.SUM, int(epilogue), table, table2, rowptr, rows, items, split, idx, w, n_slots, n_long, bias,
                 xroot, gin_scale)


@spmm_acc_.register_fake
def _spmm_acc_fake(out, table, rowptr, rows, items, split, idx, w, n_slots, n_long=-1, epilogue=4, bias=None,
                   xroot=None, gin_scale=1.0, table2=None):
    return None


def aggregate_accumulate(g: CSRGraph, table: torch.Tensor, out: torch.Tensor, *, weighted: bool = False,
                         epilogue: int = nat.EPI_ACCUM, bias: torch.Tensor | None = None,
                         xroot: torch.Tensor | None = None, gin_scale: float = 1.0,
                         table2: torch.Tensor | None = None) -> torch.Tensor:
    """out += (weighted) row sums of table rows over g, in place; forward only.
    Meant for accumulate-only graphs (graph.split_by_part), whose schedules skip
    the rows they add nothing to.  Another epilogue (NONE / BIAS / GIN)
    overwrites g's scheduled rows of out instead; table2 = second table for
    sources >= table.shape[0] (the sharded layers' merged halo pass)."""
    if _needs_grad(table, out, table2):
        raise NotImplementedError("aggregate_accumulate is a forward-only (no_grad) path")
    items, _, split, _, n_slots = g.work(False)
    w = g.w if weighted else None
    if weighted and w is None:
        raise ValueError("graph was built without edge weights")
    _timed(lambda: torch.ops.kgx.spmm_acc_(out, table, g.rowptr, g.rows, items, split, g.col, w, n_slots,
                                           g.n_long if items is not None else -1, int(epilogue), bias, xroot,
                                           float(gin_scale), table2))
    return out


# Launch hint (results unchanged): while set, fused launches leave 1/8 of the
# block slots free for a concurrent collective (distributed.py's own-source pass).
# Per host thread: ranks driven by threads of one process (tests, rehearsals)
# each enter and leave their own passes' contexts; a process-wide flag was left
# set by interleaved exits.
_SHARE = threading.local()


def _share_gpu() -> bool:
    return getattr(_SHARE, "on", False)


class sharing_gpu:
    def __enter__(self):
        self._old = _share_gpu()
        _SHARE.on = True

    def __exit__(self, *exc):
        _SHARE.on = self._old


_NOSPLIT = threading.local()


class _unsplit:
    """CU-split launches off inside (per host thread): the training backward's
    transposed pass.  There the split measured slower -- NS training step 21.40-21.62
    ms split against 20.69-20.79 one-stream, the dx pass 9.12-9.18 against 8.79-8.82
    (profiles/r06/train/split_ab/) -- while the inference forward gains from it.
    KGX_BWD_CU_SPLIT=1 keeps the split (measurement)."""

    def __enter__(self):
        self._old = getattr(_NOSPLIT, "on", False)
        _NOSPLIT.on = os.environ.get("KGX_BWD_CU_SPLIT") != "1"

    def __exit__(self, *exc):
        _NOSPLIT.on = self._old


def _tiny_abi(items, n_items, n_long, tpack, tw, n_short_end, n_tiny2):
    """(n_short_end, tiny_pack, tiny_w, n_tiny_deg2) of a fused launch's kgx_work."""
    if items is None or tpack is None or not (n_long <= n_short_end <= n_items):
        return n_items, None, None, 0
    from . import tiny

    if tpack.numel() != tiny.pack_numel(n_items - n_short_end, n_tiny2):
        raise ValueError(f"tiny records: {tpack.numel()} ints for a tail of {n_items - n_short_end} rows "
                         f"({n_tiny2} of degree 2) -- stale or foreign pack (tiny.py)")
    return n_short_end, tpack, tw, n_tiny2


F256 = 256  # F_in of kgx_spmm_gemm_f256_run (GINConv C4: 256 -> 256)
# layers take the 256-wide fused kernels by default: at C4 they beat the unfused
# pair (kgx_spmm + kgx_dense), 22.0 vs 24.5 ms; KGX_FUSED256=0 turns them off
_F256_DEFAULT = "1"


def _fused_args(reduce, flags, work, x, x2, W, bias, gin_scale, out, partials, agg) -> nat.FusedArgs:
    """The kgx_fused_args of one launch, unsliced; x2: second feature table for
    sources >= x.shape[0] (the sharded layers' merged halo passes; sums only)."""
    if x2 is not None and (x2.dim() != 2 or x2.shape[1] != x.shape[1]
                           or (x2.shape[0] and x2.stride(0) != x.stride(0))):
        raise ValueError(f"spmm_gemm: x2 {tuple(x2.shape)} must have x's row width and leading dimension")
    return nat.FusedArgs(
        struct_size=ctypes.sizeof(nat.FusedArgs), reduce=reduce, flags=flags, work=work,
        x=nat.addr(x), ld_x=x.stride(0), x2=nat.addr(x2), n_x1=x.shape[0] if x2 is not None else 0, F_in=x.shape[1],
        W=nat.addr(W), F_out=W.shape[1], bias=nat.addr(bias), gin_scale=float(gin_scale),
        out=nat.addr(out), ld_out=out.stride(0), partials=nat.addr(partials),
        agg_out=nat.addr(agg), ld_agg=agg.stride(0) if agg is not None else 0,
    )


def _f256_call(reduce, rowptr, rows, items, split, idx, w, x, x2, W, bias, flags, gin_scale, out, partials, agg,
               tpack=None, tw=None, n_short_end=-1, n_long=-1):
    """kgx_spmm_gemm_f256_run: the 256-wide fused kernels (main + the degree <= 2
    tail from the packed records), never sliced."""
    n_items = 0 if items is None else items.shape[0]
    n_se, tpack, tw, _ = _tiny_abi(items, n_items, 0, tpack, tw if w is not None else None, n_short_end, 0)
    work = nat.work(rowptr, rows, items, split, idx, w, n_long if items is not None and 0 <= n_long <= n_se else -1,
                    n_se, tpack, tw)
    a = _fused_args(reduce, flags, work, x, x2, W, bias, gin_scale, out, partials, agg)
    nat.check(nat.lib().kgx_spmm_gemm_f256_run(ctypes.byref(a), nat.stream(out.device)), "kgx_spmm_gemm_f256")


def _f256_cu_split(n_edges: int, n_tiny: int) -> bool:
    """Whether a 256-wide launch runs its degree <= 2 tail on 64 CUs beside the
    rest on the other 192 (KGX_FUSED_CU_SPLIT): when the modelled split time,
    max(head on 192 CUs, tail on 64) plus the measured 10 % interference, beats
    the one-stream sum by 3 %.  Per-unit costs from the C4 graph
    (profiles/r05/c4_cupart*.json: head 15.7 ms / 97M edges on 256 CUs, 17.9 on
    192; tail 5.63 ms / 7.46M rows on 256, 16.0 on 64).  Large launches only
    (>= 1M tail rows): the fork / join and the smaller grids cost more than they
    hide on small ones.  KGX_F256_CU_SPLIT: unset = this model (8 of every 32
    CUs for the tail), "0" = never, t > 0 = always, with t of every 32 CUs."""
    per32 = _per32_override("KGX_F256_CU_SPLIT")
    if per32 is not None:
        return n_tiny > 0 and per32 > 0
    if n_tiny < 1_000_000:
        return False
    head_e = max(n_edges - 2 * n_tiny, 0)
    t_seq = 1.62e-7 * head_e + 7.55e-7 * n_tiny
    t_split = 1.1 * max(1.85e-7 * head_e, 2.14e-6 * n_tiny)
    return t_split < 0.97 * t_seq


CU_SPLIT_LAUNCHES = 0  # launches that ran CU-split (KGX_FUSED_CU_SPLIT): bench.py reports it


def _per32_override(name: str):
    """A KGX_*_CU_SPLIT override parsed as the library parses it: None when
    unset, else the tail CUs per 32 -- an integer in 1..31, anything else 0
    (the library then runs unsplit)."""
    env = os.environ.get(name)
    if env is None:
        return None
    try:
        v = int(env.strip())
    except ValueError:
        return 0
    return v if 0 < v < 32 else 0


_DEVICE_SPLIT_OK: dict = {}


def _device_split_ok(dev: torch.device | None) -> bool:
    """The device has the layout the CU split was validated on (kgx_cu_split_supported:
    gfx950, 256 CUs, 8 XCDs); else its launches run unsplit and are not counted."""
    if dev is None:
        return True
    idx = dev.index if dev.index is not None else torch.cuda.current_device()
    ok = _DEVICE_SPLIT_OK.get(idx)
    if ok is None:
        ok = _DEVICE_SPLIT_OK[idx] = nat.lib().kgx_cu_split_supported(int(idx)) == 1
    return ok


def _split_allowed(dev: torch.device | None = None) -> bool:
    """CU-split launches stay off while a launch shares the GPU with an exchange
    (sharing_gpu: the sharded layers' passes beside RCCL and the packing), unless
    KGX_CU_SPLIT_SHARED=1 (measurement); off on a device whose layout is not the
    validated one, and for a tensor on another device than the current one (the
    library would run it unsplit)."""
    if _share_gpu() and os.environ.get("KGX_CU_SPLIT_SHARED") != "1":
        return False
    if getattr(_NOSPLIT, "on", False):
        return False
    if dev is not None and dev.type == "cuda" and dev.index is not None and dev.index != torch.cuda.current_device():
        return False
    return _device_split_ok(dev)


def _count_cu_split() -> None:
    global CU_SPLIT_LAUNCHES
    CU_SPLIT_LAUNCHES += 1


def _fused_cu_split(n_edges: int, n_tail_rows: int) -> bool:
    """Whether a 128-wide fused launch runs its short-row and tiny-record
    launches on 64 CUs beside spmm_gemm_kernel on the other 192
    (KGX_FUSED_CU_SPLIT): large schedules with a large tail only -- fitted on
    the north-star graph (profiles/r05/ns_cusplit*/: 8.62-8.69 against
    8.92-8.94 ms one-stream; main 8.29 ms on 192 CUs beside the tails' 8.61 on
    64).  KGX_FUSED_CU_SPLIT: unset = this rule, "0" = never, t > 0 = always,
    with t of every 32 CUs (only 8 measured well: see DESIGN.md §4)."""
    per32 = _per32_override("KGX_FUSED_CU_SPLIT")
    if per32 is not None:
        return n_tail_rows > 0 and per32 > 0
    return n_edges >= 50_000_000 and n_tail_rows >= 2_000_000


def _partial_width(x: torch.Tensor) -> int:
    """Floats per hub-chunk partial: the 256-wide kernels 256, kgx_spmm_gemm 128 (any F_in <= 128)."""
    return F256 if x.shape[1] == F256 else 128


def _fused_launch(out, agg, x, x2, rowptr, rows, items, split, idx, w, n_slots, reduce, W, bias, flags, gin_scale,
                  allow_split, n_long, tpack, tw, n_short_end, n_tiny2, dev, sl=None):
    """One fused aggregate -> transform launch into out (n_dst > 0 rows), and into
    agg, when given, the aggregated rows before the transform: the hub partials,
    the 256- / 128-wide dispatch, the CU-split decision and the native call.
    allow_split is off for the training forward's saved-aggregate launch: its
    tail launches also store the aggregated rows (the EXTRA instantiations), and
    split it measured slower (NS training step 23.1 -> 25.0 ms, profiles/r05/train/).
    sl: a slice.SlicedSchedule for the main kernel (kgx_fused_args.slice), or None."""
    n_items = 0 if items is None else items.shape[0]
    n_split = 0 if split is None else split.shape[0]
    if sl is not None and (items is None or x.shape[1] == F256 or x2 is not None):
        sl = None
    partials = None
    if items is not None and (n_split > 0 or sl is not None):
        # (the sliced launch falls back to the unsliced one when no grid fits: room for either schedule's slots)
        slots = max(n_slots if n_split > 0 else 0, sl.n_slots if sl is not None else 0)
        partials = torch.empty((slots, _partial_width(x)), dtype=torch.float32, device=dev)
    allow_split = allow_split and items is not None
    if x.shape[1] == F256:
        if tpack is not None and allow_split and _split_allowed(dev) and \
                _f256_cu_split(idx.numel(), n_items - (n_short_end if n_short_end >= 0 else n_items)):
            flags |= nat.FUSED_CU_SPLIT
            _count_cu_split()
        _f256_call(reduce, rowptr, rows, items, split, idx, w, x, x2, W, bias, flags, gin_scale, out, partials, agg,
                   tpack, tw, n_short_end, n_long)
        return
    n_long = n_items if n_long < 0 or n_long > n_items else n_long
    n_se, tpack, tw, n_tiny2 = _tiny_abi(items, n_items, n_long, tpack, tw if w is not None else None, n_short_end,
                                         n_tiny2)
    if allow_split and _split_allowed(dev) and _fused_cu_split(idx.numel(), n_items - n_long):
        flags |= nat.FUSED_CU_SPLIT
        _count_cu_split()
    if sl is not None and ((w is not None) != (sl.w is not None) or sl.n_long != n_long):
        sl = None  # (lists built without weights, or for another long-item boundary)
    a = _fused_args(reduce, flags, nat.work(rowptr, rows, items, split, idx, w, n_long, n_se, tpack, tw, n_tiny2),
                    x, x2, W, bias, gin_scale, out, partials, agg)
    if sl is not None:
        a.slice = nat.Slice(
            items=nat.addr(sl.items), lists=nat.addr(sl.lists), n_classes=sl.C, tiles=sl.tiles,
            idx=nat.addr(sl.col), w=nat.addr(sl.w), split=nat.addr(sl.fix), n_split=sl.n_rows,
            head_short_end=min(sl.head_short_end, n_se),
        )
    nat.check(nat.lib().kgx_spmm_gemm_run(ctypes.byref(a), nat.stream(dev)), "kgx_spmm_gemm")


def _spmm_gemm_impl(x, rowptr, rows, items, split, idx, w, n_slots, reduce, W, bias, pre_gin, gin_scale, save_agg,
                    relu=False, n_long=-1, tpack=None, tw=None, n_short_end=-1, n_tiny2=0, x2=None, sl=None):
    x, w, W, bias, x2 = _f32c(x), _f32c(w), _f32c(W), _f32c(bias), _f32c(x2)
    dev = nat.require_device(x, rowptr, rows, idx, w, W, bias, items, split, x2)
    n_dst = rowptr.numel() - 1
    out = torch.empty((n_dst, W.shape[1]), dtype=torch.float32, device=dev)
    agg = torch.empty((n_dst if save_agg else 0, x.shape[1]), dtype=torch.float32, device=dev)
    if n_dst == 0:
        return out, agg
    flags = int(pre_gin) | (nat.FUSED_SHARE_GPU if _share_gpu() else 0) | (nat.FUSED_RELU if relu else 0)
    _fused_launch(out, agg if save_agg else None, x, x2, rowptr, rows, items, split, idx, w, n_slots, reduce, W, bias,
                  flags, gin_scale, not save_agg, n_long, tpack, tw, n_short_end, n_tiny2, dev, sl)
    return out, agg


@torch.library.custom_op("kgx::spmm_gemm", mutates_args=())
def spmm_gemm(
    x: torch.Tensor,
    rowptr: torch.Tensor,
    rows: torch.Tensor,
    items: Optional[torch.Tensor],
    split: Optional[torch.Tensor],
    idx: torch.Tensor,
    w: Optional[torch.Tensor],
    n_slots: int,
    reduce: int,
    W: torch.Tensor,
    bias: Optional[torch.Tensor],
    pre_gin: bool,
    gin_scale: float,
    relu: bool = False,
    n_long: int = -1,
    tpack: Optional[torch.Tensor] = None,
    tw: Optional[torch.Tensor] = None,
    n_short_end: int = -1,
    n_tiny2: int = 0,
    x2: Optional[torch.Tensor] = None,
    sl_items: Optional[torch.Tensor] = None,
    sl_lists: Optional[torch.Tensor] = None,
    sl_idx: Optional[torch.Tensor] = None,
    sl_w: Optional[torch.Tensor] = None,
    sl_fix: Optional[torch.Tensor] = None,
    sl_slots: int = 0,
    sl_max_list: int = 0,
    sl_head_short_end: int = -1,
) -> torch.Tensor:
    """x2 (two-table gathers): sources >= x.shape[0] are rows of x2.
    sl_*: a sliced schedule for the main kernel (slice.SlicedSchedule's arrays, kgx_fused_args.slice)."""
    sl = None
    if sl_items is not None:
        from .slice import SlicedSchedule

        sl = SlicedSchedule(T=0, C=sl_lists.shape[0], split_len=0, n_rows=sl_fix.shape[0], n_edges=sl_idx.numel(),
                            n_items_s=0, n_long=n_long, col=sl_idx, w=sl_w, items=sl_items, lists=sl_lists,
                            fix=sl_fix, n_slots=sl_slots, max_list=sl_max_list, build_ms=0.0,
                            head_short_end=sl_head_short_end)
    return _spmm_gemm_impl(x, rowptr, rows, items, split, idx, w, n_slots, reduce, W, bias, pre_gin, gin_scale,
                           False, relu, n_long, tpack, tw, n_short_end, n_tiny2, x2, sl)[0]


@spmm_gemm.register_fake
def _spmm_gemm_fake(x, rowptr, rows, items, split, idx, w, n_slots, reduce, W, bias, pre_gin, gin_scale, relu=False,
                    n_long=-1, tpack=None, tw=None, n_short_end=-1, n_tiny2=0, x2=None, sl_items=None, sl_lists=None,
                    sl_idx=None, sl_w=None, sl_fix=None, sl_slots=0, sl_max_list=0, sl_head_short_end=-1):
    return x.new_empty((rowptr.shape[0] - 1, W.shape[1]))


@torch.library.custom_op("kgx::spmm_gemm_save", mutates_args=())
def spmm_gemm_save(
    x: torch.Tensor,
    rowptr: torch.Tensor,
    rows: torch.Tensor,
    items: Optional[torch.Tensor],
    split: Optional[torch.Tensor],
    idx: torch.Tensor,
    w: Optional[torch.Tensor],
    n_slots: int,
    reduce: int,
    W: torch.Tensor,
    bias: Optional[torch.Tensor],
    pre_gin: bool,
    gin_scale: float,
    n_long: int = -1,
    tpack: Optional[torch.Tensor] = None,
    tw: Optional[torch.Tensor] = None,
    n_short_end: int = -1,
    n_tiny2: int = 0,
) -> tuple[torch.Tensor, torch.Tensor]:
    """kgx::spmm_gemm that also returns the aggregated rows before the transform."""
    return _spmm_gemm_impl(x, rowptr, rows, items, split, idx, w, n_slots, reduce, W, bias, pre_gin, gin_scale, True,
                           False, n_long, tpack, tw, n_short_end, n_tiny2)


@spmm_gemm_save.register_fake
def _spmm_gemm_save_fake(x, rowptr, rows, items, split, idx, w, n_slots, reduce, W, bias, pre_gin, gin_scale,
                         n_long=-1, tpack=None, tw=None, n_short_end=-1, n_tiny2=0):
    n = rowptr.shape[0] - 1
    return x.new_empty((n, W.shape[1])), x.new_empty((n, x.shape[1]))


@torch.library.custom_op("kgx::spmm_gemm_acc_", mutates_args=("out",))
def spmm_gemm_acc_(
    out: torch.Tensor,
    x: torch.Tensor,
    rowptr: torch.Tensor,
    rows: torch.Tensor,
    items: Optional[torch.Tensor],
    split: Optional[torch.Tensor],
    idx: torch.Tensor,
    w: Optional[torch.Tensor],
    n_slots: int,
    reduce: int,
    W: torch.Tensor,
    bias: Optional[torch.Tensor],
    n_long: int = -1,
    tpack: Optional[torch.Tensor] = None,
    tw: Optional[torch.Tensor] = None,
    n_short_end: int = -1,
    n_tiny2: int = 0,
    x2: Optional[torch.Tensor] = None,
    accumulate: bool = True,
    flags: int = 0,
    gin_scale: float = 1.0,
) -> None:
    """out += bias + REDUCE(...) @ W (KGX_FUSED_ACCUMULATE), in place; with
    accumulate=False the scheduled rows of out are overwritten instead (and the
    rest left untouched): two launches over disjoint row sets fill one output.
    flags: KGX_FUSED_PRE_GIN / KGX_FUSED_RELU for an overwriting launch (the
    sharded GIN layer's passes: (1+eps) x_i + aggr -> Dense)."""
    x, w, W, bias, x2 = _f32c(x), _f32c(w), _f32c(W), _f32c(bias), _f32c(x2)
    dev = nat.require_device(out, x, rowptr, rows, idx, w, W, bias, items, split, x2)
    n_dst = rowptr.numel() - 1
    if out.dtype != torch.float32 or out.shape != (n_dst, W.shape[1]) or out.stride(1) != 1:
        raise ValueError(f"spmm_gemm_acc_: out must be float32 [{n_dst}, {W.shape[1]}] with unit column stride")
    if n_dst == 0:
        return
    flags |= (nat.FUSED_ACCUMULATE if accumulate else 0) | (nat.FUSED_SHARE_GPU if _share_gpu() else 0)
    _fused_launch(out, None, x, x2, rowptr, rows, items, split, idx, w, n_slots, reduce, W, bias, flags, gin_scale,
                  True, n_long, tpack, tw, n_short_end, n_tiny2, dev)


@spmm_gemm_acc_.register_fake
def _spmm_gemm_acc_fake(out, x, rowptr, rows, items, split, idx, w, n_slots, reduce, W, bias, n_long=-1, tpack=None,
                        tw=None, n_short_end=-1, n_tiny2=0, x2=None, accumulate=True, flags=0, gin_scale=1.0):
    return None


def fused_transform_supported(f_in: int, f_out: int, two_table: bool = False) -> bool:
    """Shapes kgx_spmm_gemm (F_in 128) and kgx_spmm_gemm_f256_run (F_in 256)
    implement, with one feature table or two (two_table: the sharded layers'
    merged halo passes, sum only; aggregate-then-transform is also only worth
    it when F_in <= F_out)."""
    import os

    if os.environ.get("KGX_FUSED", "1") in ("0", "false", "False"):
        return False
    if f_in == F256:
        return f_out == F256 and os.environ.get("KGX_FUSED256", _F256_DEFAULT) not in ("0", "false", "False")
    return f_in == 128 and f_out % 16 == 0 and 0 < f_out <= 128 and f_in <= f_out


def fused_sage_supported(f_in: int, f_out: int) -> bool:
    """SAGEConv's update through kgx_spmm_gemm (any F_in, F_out <= 128, multiples
    of 4): out = x W_self + b by kgx_dense, then out = relu?(out + REDUCE(x) W_neigh)
    in the fused aggregation's store, so the [N, F_in] aggregate is never
    written (C5: 2.45M x 100).  Opt-in (KGX_FUSED_SAGE=1): at C5 it measured
    slower than the two-step path -- the fused main kernel's W registers hold
    it at 4 waves per SIMD, and C5's 50-edge rows want spmm_kernel's gather
    depth.  KGX_FUSED=0 turns it off too."""
    import os

    if os.environ.get("KGX_FUSED", "1") in ("0", "false", "False"):
        return False
    if os.environ.get("KGX_FUSED_SAGE", "0") not in ("1", "true", "True"):
        return False
    return 0 < f_in <= 128 and f_in % 4 == 0 and 0 < f_out <= 128 and f_out % 4 == 0


def _sched_counts(items, split):
    """(n_items, n_split) of a schedule's lists, 0 for a list that is absent."""
    return (0 if items is None else items.shape[0]), (0 if split is None else split.shape[0])


def _attn_partials(dev, items, n_split, n_slots, heads, channels):
    """Chunk partials of the attention forwards, None without split rows: per
    slot [H*C acc | H m | H l], padded to whole float4s (attn_partial_ld in
    csrc/kgx_attn_layout.h; tests/test_attn_layout_host.py holds the two equal)."""
    if items is None or n_split == 0:
        return None
    return torch.empty((n_slots, (heads * channels + 2 * heads + 3) // 4 * 4), dtype=torch.float32, device=dev)


def _drop_args(drop_key, drop_p, drop_seed):
    """(key pointer, p, seed) as the C entry points take attention dropout: no key without dropout."""
    return (nat.ptr(drop_key) if drop_p > 0 else None), float(drop_p), int(drop_seed) & (2**64 - 1)


def _gatv2_impl(h_src, h_dst, rowptr, rows, items, split, col, att, heads, channels, negative_slope, bias,
                n_slots, save_stats, drop_key=None, drop_p=0.0, drop_seed=0, edge=None, edge_idx=None):
    h_src, h_dst, att, bias = _f32c(h_src), _f32c(h_dst), _f32c(att), _f32c(bias)
    HC = heads * channels
    if edge is not None:
        edge = _edge_table(edge, edge_idx, HC, col.numel(), "gatv2")
    else:
        edge_idx = None
    dev = nat.require_device(h_src, h_dst, rowptr, rows, col, att, bias, items, split, edge, edge_idx)
    n_dst = rowptr.numel() - 1
    out = torch.empty((n_dst, HC), dtype=torch.float32, device=dev)
    stats = torch.empty((n_dst if save_stats else 0, 2 * heads), dtype=torch.float32, device=dev)
    if n_dst == 0:
        return out, stats
    n_items, n_split = _sched_counts(items, split)
    partials = _attn_partials(dev, items, n_split, n_slots, heads, channels)
    if edge is None:
        nat.check(
            nat.lib().kgx_gatv2(
                nat.ptr(rowptr), nat.ptr(rows), n_dst, nat.ptr(items), n_items, nat.ptr(split), n_split,
                nat.ptr(col), nat.ptr(h_src), nat.ptr(h_dst), h_src.stride(0), nat.ptr(att), heads, channels,
                float(negative_slope), nat.ptr(out), out.stride(0), nat.ptr(bias), nat.ptr(partials),
                nat.ptr(stats) if save_stats else None, *_drop_args(drop_key, drop_p, drop_seed), nat.stream(dev),
            ),
            "kgx_gatv2",
        )
        return out, stats
    nat.check(
        nat.lib().kgx_gatv2_edge(
            nat.ptr(rowptr), nat.ptr(rows), n_dst, nat.ptr(items), n_items, nat.ptr(split), n_split,
            nat.ptr(col), nat.ptr(h_src), nat.ptr(h_dst), h_src.stride(0), nat.ptr(edge), _attn_ld(edge),
            edge.shape[0], nat.ptr(edge_idx), nat.ptr(att), heads, channels, float(negative_slope), nat.ptr(out),
            out.stride(0), nat.ptr(bias), nat.ptr(partials), nat.ptr(stats) if save_stats else None,
            *_drop_args(drop_key, drop_p, drop_seed), nat.stream(dev),
        ),
        "kgx_gatv2_edge",
    )
    return out, stats


@torch.library.custom_op("kgx::gatv2_save", mutates_args=())
def gatv2_save(
    h_src: torch.Tensor,
    h_dst: torch.Tensor,
    rowptr: torch.Tensor,
    rows: torch.Tensor,
    items: Optional[torch.Tensor],
    split: Optional[torch.Tensor],
    col: torch.Tensor,
    att: torch.Tensor,
    heads: int,
    channels: int,
    negative_slope: float,
    bias: Optional[torch.Tensor],
    n_slots: int,
    drop_key: Optional[torch.Tensor] = None,
    drop_p: float = 0.0,
    drop_seed: int = 0,
    edge: Optional[torch.Tensor] = None,
    edge_idx: Optional[torch.Tensor] = None,
) -> tuple[torch.Tensor, torch.Tensor]:
    """kgx::gatv2 that also returns the per-row softmax statistics [n, 2*heads]."""
    return _gatv2_impl(h_src, h_dst, rowptr, rows, items, split, col, att, heads, channels, negative_slope, bias,
                       n_slots, True, drop_key, drop_p, drop_seed, edge, edge_idx)


@gatv2_save.register_fake
def _gatv2_save_fake(h_src, h_dst, rowptr, rows, items, split, col, att, heads, channels, negative_slope, bias,
                     n_slots, drop_key=None, drop_p=0.0, drop_seed=0, edge=None, edge_idx=None):
    n = rowptr.shape[0] - 1
    return h_src.new_empty((n, heads * channels)), h_src.new_empty((n, 2 * heads))


@torch.library.custom_op("kgx::gatv2", mutates_args=())
def gatv2(
    h_src: torch.Tensor,
    h_dst: torch.Tensor,
    rowptr: torch.Tensor,
    rows: torch.Tensor,
    items: Optional[torch.Tensor],
    split: Optional[torch.Tensor],
    col: torch.Tensor,
    att: torch.Tensor,
    heads: int,
    channels: int,
    negative_slope: float,
    bias: Optional[torch.Tensor],
    n_slots: int,
    drop_key: Optional[torch.Tensor] = None,
    drop_p: float = 0.0,
    drop_seed: int = 0,
    edge: Optional[torch.Tensor] = None,
    edge_idx: Optional[torch.Tensor] = None,
) -> torch.Tensor:
    """Fused GATv2 attention aggregation (kgx_gatv2); with `edge` [n_e, heads*channels], row
    edge_idx[slot] (None: the slot) is added to h_dst[i] + h_src[j] in the score (kgx_gatv2_edge)."""
    return _gatv2_impl(h_src, h_dst, rowptr, rows, items, split, col, att, heads, channels, negative_slope, bias,
                       n_slots, False, drop_key, drop_p, drop_seed, edge, edge_idx)[0]


@gatv2.register_fake
def _gatv2_fake(h_src, h_dst, rowptr, rows, items, split, col, att, heads, channels, negative_slope, bias, n_slots,
                drop_key=None, drop_p=0.0, drop_seed=0, edge=None, edge_idx=None):
    return h_src.new_empty((rowptr.shape[0] - 1, heads * channels))


def _attn_table(t: torch.Tensor, width: int, what: str, op: str = "dot_attention") -> torch.Tensor:
    """A [n, heads*channels] fp32 table the attention kernels read in place:
    unit column stride, non-overlapping rows (a column half of a wider tensor
    passes through uncopied)."""
    if t.dtype != torch.float32:
        raise TypeError(f"kgx kernels compute in fp32; got {t.dtype}")
    if t.dim() != 2 or t.shape[1] != width:
        raise ValueError(f"{op}: {what} must be [n, {width}], got {tuple(t.shape)}")
    if (t.shape[1] > 1 and t.stride(1) != 1) or (t.shape[0] > 1 and t.stride(0) < t.shape[1]):
        return t.contiguous()
    return t


def _attn_ld(t: torch.Tensor) -> int:
    return t.stride(0) if t.shape[0] > 1 else max(t.shape[1], 1)


def _edge_table(edge, edge_idx, HC, n_slots_csr, op: str = "dot_attention"):
    """The edge table as the kernels read it: [n_e, heads*channels] in place; without
    edge_idx its rows are the CSR slots."""
    edge = _attn_table(edge, HC, "edge", op)
    if edge_idx is None and edge.shape[0] != n_slots_csr:
        raise ValueError(f"{op}: edge in CSR order must have {n_slots_csr} rows, got {edge.shape[0]}")
    if edge_idx is not None and (edge_idx.dtype != torch.int32 or edge_idx.numel() != n_slots_csr):
        raise ValueError(f"{op}: edge_idx must be int32 [{n_slots_csr}]")
    return edge


def gatv2_edge_backward_into(grad_e, grad_out, h_src, h_dst, att, bias, edge, out, stats, rowptr, rows, items, split,
                             col, n_slots, t_rowptr, t_rows, t_items, t_split, t_col, t_slot, t_slots, heads,
                             channels, negative_slope, edge_idx, t_edge_idx, drop_key=None, drop_p=0.0, drop_seed=0):
    """(grad_h_src, grad_h_dst, grad_att) of kgx::gatv2_save with an edge table, and
    d edge written into the rows of `grad_e` [n_e, heads*channels] (a row view of
    a wider tensor is written in place) that a kept slot names: the caller
    zeroes the others (kgx_gatv2_edge_backward)."""
    HC = heads * channels
    edge = _edge_table(edge, edge_idx, HC, col.numel(), "gatv2")
    if t_edge_idx.dtype != torch.int32 or t_edge_idx.numel() != t_col.numel():
        raise ValueError(f"gatv2: t_edge_idx must be int32 [{t_col.numel()}]")
    if (grad_e.dtype != torch.float32 or grad_e.shape != edge.shape
            or _attn_table(grad_e, HC, "grad_e", "gatv2") is not grad_e):
        raise ValueError(f"gatv2: grad_e must be fp32 {tuple(edge.shape)} with unit column stride, got "
                         f"{grad_e.dtype} {tuple(grad_e.shape)} strides {grad_e.stride()}")
    grad_out, h_src, h_dst, out, stats = (_f32c(t) for t in (grad_out, h_src, h_dst, out, stats))
    att, bias = _f32c(att.reshape(-1)), _f32c(bias)
    dev = nat.require_device(grad_out, h_src, h_dst, att, bias, edge, grad_e, out, stats, rowptr, rows, items, split,
                             col, t_rowptr, t_rows, t_items, t_split, t_col, t_slot, edge_idx, t_edge_idx, drop_key)
    n_dst, n_src = rowptr.numel() - 1, t_rowptr.numel() - 1
    g_src = torch.empty((n_src, HC), dtype=torch.float32, device=dev)
    g_dst = torch.empty((n_dst, HC), dtype=torch.float32, device=dev)
    g_att = torch.zeros(HC, dtype=torch.float32, device=dev)
    if n_dst == 0 and n_src == 0:
        return g_src, g_dst, g_att
    kept = col.numel()
    alpha = torch.empty((max(kept, 1), heads), dtype=torch.float32, device=dev)
    ds = torch.empty_like(alpha)
    partials = torch.empty((max(n_slots, t_slots, 1), HC), dtype=torch.float32, device=dev)
    n_items, n_split = _sched_counts(items, split)
    t_n_items, t_n_split = _sched_counts(t_items, t_split)
    nat.check(
        nat.lib().kgx_gatv2_edge_backward(
            nat.ptr(rowptr), nat.ptr(rows), n_dst, nat.ptr(items), n_items, nat.ptr(split), n_split, nat.ptr(col),
            nat.ptr(h_src), nat.ptr(h_dst), h_src.stride(0), nat.ptr(edge), _attn_ld(edge), edge.shape[0],
            nat.ptr(edge_idx), nat.ptr(att), heads, channels, float(negative_slope), nat.ptr(out), out.stride(0),
            nat.ptr(bias), nat.ptr(stats), nat.ptr(grad_out), grad_out.stride(0), nat.ptr(t_rowptr),
            nat.ptr(t_rows), n_src, nat.ptr(t_items), t_n_items, nat.ptr(t_split), t_n_split, nat.ptr(t_col),
            nat.ptr(t_slot), nat.ptr(t_edge_idx), nat.ptr(g_src), nat.ptr(g_dst), g_src.stride(0), nat.ptr(g_att),
            nat.ptr(grad_e), _attn_ld(grad_e), nat.ptr(alpha), nat.ptr(ds), nat.ptr(partials),
            *_drop_args(drop_key, drop_p, drop_seed), nat.stream(dev),
        ),
        "kgx_gatv2_edge_backward",
    )
    return g_src, g_dst, g_att


@torch.library.custom_op("kgx::gatv2_edge_backward", mutates_args=())
def gatv2_edge_backward(
    grad_out: torch.Tensor,
    h_src: torch.Tensor,
    h_dst: torch.Tensor,
    att: torch.Tensor,
    bias: Optional[torch.Tensor],
    edge: torch.Tensor,
    out: torch.Tensor,
    stats: torch.Tensor,
    rowptr: torch.Tensor,
    rows: torch.Tensor,
    items: Optional[torch.Tensor],
    split: Optional[torch.Tensor],
    col: torch.Tensor,
    n_slots: int,
    t_rowptr: torch.Tensor,
    t_rows: torch.Tensor,
    t_items: Optional[torch.Tensor],
    t_split: Optional[torch.Tensor],
    t_col: torch.Tensor,
    t_slot: torch.Tensor,
    t_slots: int,
    heads: int,
    channels: int,
    negative_slope: float,
    edge_idx: Optional[torch.Tensor],
    t_edge_idx: torch.Tensor,
    zero_grad_edge: bool,
    drop_key: Optional[torch.Tensor] = None,
    drop_p: float = 0.0,
    drop_seed: int = 0,
) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """(grad_h_src, grad_h_dst, grad_att [heads*channels], grad_edge) of kgx::gatv2_save with an
    edge table; zero_grad_edge: some row of `edge` belongs to no kept slot."""
    make = torch.zeros if zero_grad_edge or col.numel() == 0 else torch.empty
    g_e = make((edge.shape[0], heads * channels), dtype=torch.float32, device=edge.device)
    g_src, g_dst, g_att = gatv2_edge_backward_into(
        g_e, grad_out, h_src, h_dst, att, bias, edge, out, stats, rowptr, rows, items, split, col, n_slots, t_rowptr,
        t_rows, t_items, t_split, t_col, t_slot, t_slots, heads, channels, negative_slope, edge_idx, t_edge_idx,
        drop_key, drop_p, drop_seed)
    return g_src, g_dst, g_att, g_e


@gatv2_edge_backward.register_fake
def _gatv2_edge_backward_fake(grad_out, h_src, h_dst, att, bias, edge, out, stats, rowptr, rows, items, split, col,
                              n_slots, t_rowptr, t_rows, t_items, t_split, t_col, t_slot, t_slots, heads, channels,
                              negative_slope, edge_idx, t_edge_idx, zero_grad_edge, drop_key=None, drop_p=0.0,
                              drop_seed=0):
    hc = heads * channels
    return (h_src.new_empty((t_rowptr.shape[0] - 1, hc)), h_src.new_empty((rowptr.shape[0] - 1, hc)),
            h_src.new_empty((hc,)), h_src.new_empty((edge.shape[0], hc)))


def _dot_attention_impl(q, k, v, rowptr, rows, items, split, col, heads, channels, scale, n_slots, save_stats,
                        drop_key=None, drop_p=0.0, drop_seed=0, edge=None, edge_idx=None):
    HC = heads * channels
    q, k, v = _attn_table(q, HC, "q"), _attn_table(k, HC, "k"), _attn_table(v, HC, "v")
    if edge is not None:
        edge = _edge_table(edge, edge_idx, HC, col.numel())
    else:
        edge_idx = None
    dev = nat.require_device(q, k, v, rowptr, rows, col, items, split, drop_key, edge, edge_idx)
    n_dst = rowptr.numel() - 1
    if q.shape[0] != n_dst or k.shape[0] != v.shape[0]:
        raise ValueError(f"dot_attention: q has {q.shape[0]} rows for {n_dst} destinations, k {k.shape[0]} and v "
                         f"{v.shape[0]} rows")
    out = torch.empty((n_dst, HC), dtype=torch.float32, device=dev)
    stats = torch.empty((n_dst if save_stats else 0, 2 * heads), dtype=torch.float32, device=dev)
    if n_dst == 0:
        return out, stats
    n_items, n_split = _sched_counts(items, split)
    partials = _attn_partials(dev, items, n_split, n_slots, heads, channels)
    # no table: the entry point is kgx_dot_attention (which forwards to this one with these arguments)
    e_args = (None, 0, 0, None) if edge is None else (nat.ptr(edge), _attn_ld(edge), edge.shape[0], nat.ptr(edge_idx))
    nat.check(
        nat.lib().kgx_dot_attention_edge(
            nat.ptr(rowptr), nat.ptr(rows), n_dst, nat.ptr(items), n_items, nat.ptr(split), n_split, nat.ptr(col),
            nat.ptr(q), _attn_ld(q), nat.ptr(k), _attn_ld(k), nat.ptr(v), _attn_ld(v), *e_args, heads, channels,
            float(scale), nat.ptr(out), out.stride(0), nat.ptr(partials), nat.ptr(stats) if save_stats else None,
            *_drop_args(drop_key, drop_p, drop_seed), nat.stream(dev),
        ),
        "kgx_dot_attention",
    )
    return out, stats


@torch.library.custom_op("kgx::dot_attention_save", mutates_args=())
def dot_attention_save(
    q: torch.Tensor,
    k: torch.Tensor,
    v: torch.Tensor,
    rowptr: torch.Tensor,
    rows: torch.Tensor,
    items: Optional[torch.Tensor],
    split: Optional[torch.Tensor],
    col: torch.Tensor,
    heads: int,
    channels: int,
    scale: float,
    n_slots: int,
    drop_key: Optional[torch.Tensor] = None,
    drop_p: float = 0.0,
    drop_seed: int = 0,
    edge: Optional[torch.Tensor] = None,
    edge_idx: Optional[torch.Tensor] = None,
) -> tuple[torch.Tensor, torch.Tensor]:
    """kgx::dot_attention that also returns the per-row softmax statistics [n_dst, 2*heads]: (m, l)."""
    return _dot_attention_impl(q, k, v, rowptr, rows, items, split, col, heads, channels, scale, n_slots, True,
                               drop_key, drop_p, drop_seed, edge, edge_idx)


@dot_attention_save.register_fake
def _dot_attention_save_fake(q, k, v, rowptr, rows, items, split, col, heads, channels, scale, n_slots,
                             drop_key=None, drop_p=0.0, drop_seed=0, edge=None, edge_idx=None):
    n = rowptr.shape[0] - 1
    return q.new_empty((n, heads * channels)), q.new_empty((n, 2 * heads))


@torch.library.custom_op("kgx::dot_attention", mutates_args=())
def dot_attention_op(
    q: torch.Tensor,
    k: torch.Tensor,
    v: torch.Tensor,
    rowptr: torch.Tensor,
    rows: torch.Tensor,
    items: Optional[torch.Tensor],
    split: Optional[torch.Tensor],
    col: torch.Tensor,
    heads: int,
    channels: int,
    scale: float,
    n_slots: int,
    drop_key: Optional[torch.Tensor] = None,
    drop_p: float = 0.0,
    drop_seed: int = 0,
    edge: Optional[torch.Tensor] = None,
    edge_idx: Optional[torch.Tensor] = None,
) -> torch.Tensor:
    """out[i,h,:] = sum_e softmax_i(scale <q_i, k_j>_h)_e mask_e v[j_e,h,:] (kgx_dot_attention); with
    `edge` [n_e, heads*channels], row edge_idx[slot] (None: the slot) is added to k_j and to v_j
    (kgx_dot_attention_edge)."""
    return _dot_attention_impl(q, k, v, rowptr, rows, items, split, col, heads, channels, scale, n_slots, False,
                               drop_key, drop_p, drop_seed, edge, edge_idx)[0]


@dot_attention_op.register_fake
def _dot_attention_fake(q, k, v, rowptr, rows, items, split, col, heads, channels, scale, n_slots, drop_key=None,
                        drop_p=0.0, drop_seed=0, edge=None, edge_idx=None):
    return q.new_empty((rowptr.shape[0] - 1, heads * channels))


@torch.library.custom_op("kgx::dot_attention_backward", mutates_args=())
def dot_attention_backward(
    grad_out: torch.Tensor,
    q: torch.Tensor,
    k: torch.Tensor,
    v: torch.Tensor,
    out: torch.Tensor,
    stats: torch.Tensor,
    rowptr: torch.Tensor,
    rows: torch.Tensor,
    items: Optional[torch.Tensor],
    split: Optional[torch.Tensor],
    col: torch.Tensor,
    n_slots: int,
    t_rowptr: torch.Tensor,
    t_rows: torch.Tensor,
    t_items: Optional[torch.Tensor],
    t_split: Optional[torch.Tensor],
    t_col: torch.Tensor,
    t_key: torch.Tensor,
    t_slots: int,
    heads: int,
    channels: int,
    scale: float,
    drop_key: Optional[torch.Tensor] = None,
    drop_p: float = 0.0,
    drop_seed: int = 0,
) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """(grad_q, grad_k, grad_v) of kgx::dot_attention_save: a destination pass
    over the forward CSR and a source pass over the transposed one, both
    recomputing the probabilities from q, k and stats (kgx_dot_attention_backward)."""
    HC = heads * channels
    q, k, v = _attn_table(q, HC, "q"), _attn_table(k, HC, "k"), _attn_table(v, HC, "v")
    grad_out, out, stats = _f32c(grad_out), _f32c(out), _f32c(stats)
    dev = nat.require_device(grad_out, q, k, v, out, stats, rowptr, rows, items, split, col, t_rowptr, t_rows,
                             t_items, t_split, t_col, t_key, drop_key)
    n_dst, n_src = rowptr.numel() - 1, t_rowptr.numel() - 1
    g_q = torch.empty((n_dst, HC), dtype=torch.float32, device=dev)
    g_k = torch.empty((n_src, HC), dtype=torch.float32, device=dev)
    g_v = torch.empty((n_src, HC), dtype=torch.float32, device=dev)
    if col.numel() == 0 or n_dst == 0 or n_src == 0:
        return g_q.zero_(), g_k.zero_(), g_v.zero_()
    dsum = torch.empty((n_dst, heads), dtype=torch.float32, device=dev)
    n_items, n_split = _sched_counts(items, split)
    t_n_items, t_n_split = _sched_counts(t_items, t_split)
    partials = None
    if (items is not None and n_split > 0) or (t_items is not None and t_n_split > 0):
        partials = torch.empty((max(n_slots, t_slots, 1), 2 * HC), dtype=torch.float32, device=dev)
    nat.check(
        nat.lib().kgx_dot_attention_backward(
            nat.ptr(rowptr), nat.ptr(rows), n_dst, nat.ptr(items), n_items, nat.ptr(split), n_split, nat.ptr(col),
            nat.ptr(q), _attn_ld(q), nat.ptr(k), _attn_ld(k), nat.ptr(v), _attn_ld(v), heads, channels,
            float(scale), nat.ptr(out), out.stride(0), nat.ptr(stats), nat.ptr(grad_out), grad_out.stride(0),
            nat.ptr(t_rowptr), nat.ptr(t_rows), n_src, nat.ptr(t_items), t_n_items, nat.ptr(t_split), t_n_split,
            nat.ptr(t_col), nat.ptr(t_key), nat.ptr(g_q), g_q.stride(0), nat.ptr(g_k), g_k.stride(0),
            nat.ptr(g_v), g_v.stride(0), nat.ptr(dsum), nat.ptr(partials),
            *_drop_args(drop_key, drop_p, drop_seed), nat.stream(dev),
        ),
        "kgx_dot_attention_backward",
    )
    return g_q, g_k, g_v


@dot_attention_backward.register_fake
def _dot_attention_backward_fake(grad_out, q, k, v, out, stats, rowptr, rows, items, split, col, n_slots, t_rowptr,
                                 t_rows, t_items, t_split, t_col, t_key, t_slots, heads, channels, scale,
                                 drop_key=None, drop_p=0.0, drop_seed=0):
    hc = heads * channels
    return (q.new_empty((rowptr.shape[0] - 1, hc)), q.new_empty((t_rowptr.shape[0] - 1, hc)),
            q.new_empty((t_rowptr.shape[0] - 1, hc)))


def dot_attention_edge_backward_into(grad_e, grad_out, q, k, v, edge, out, stats, rowptr, rows, items, split, col,
                                     n_slots, t_rowptr, t_rows, t_items, t_split, t_col, t_key, t_slots, heads,
                                     channels, scale, edge_idx, t_edge_idx, drop_key=None, drop_p=0.0, drop_seed=0):
    """(grad_q, grad_k, grad_v) of kgx::dot_attention_save with an edge table, and
    d edge written into the rows of `grad_e` [n_e, heads*channels] (a row view of
    a wider tensor is written in place) that a kept slot names: the caller
    zeroes it when the graph dropped input edges (kgx_dot_attention_edge_backward)."""
    HC = heads * channels
    q, k, v = _attn_table(q, HC, "q"), _attn_table(k, HC, "k"), _attn_table(v, HC, "v")
    edge = _edge_table(edge, edge_idx, HC, col.numel())
    if t_edge_idx.dtype != torch.int32 or t_edge_idx.numel() != t_col.numel():
        raise ValueError(f"dot_attention: t_edge_idx must be int32 [{t_col.numel()}]")
    if grad_e.dtype != torch.float32 or grad_e.shape != edge.shape or _attn_table(grad_e, HC, "grad_e") is not grad_e:
        raise ValueError(f"dot_attention: grad_e must be fp32 {tuple(edge.shape)} with unit column stride, got "
                         f"{grad_e.dtype} {tuple(grad_e.shape)} strides {grad_e.stride()}")
    grad_out, out, stats = _f32c(grad_out), _f32c(out), _f32c(stats)
    dev = nat.require_device(grad_out, q, k, v, edge, grad_e, out, stats, rowptr, rows, items, split, col, t_rowptr,
                             t_rows, t_items, t_split, t_col, t_key, edge_idx, t_edge_idx, drop_key)
    n_dst, n_src = rowptr.numel() - 1, t_rowptr.numel() - 1
    g_q = torch.empty((n_dst, HC), dtype=torch.float32, device=dev)
    g_k = torch.empty((n_src, HC), dtype=torch.float32, device=dev)
    g_v = torch.empty((n_src, HC), dtype=torch.float32, device=dev)
    if col.numel() == 0 or n_dst == 0 or n_src == 0:
        return g_q.zero_(), g_k.zero_(), g_v.zero_()
    dsum = torch.empty((n_dst, heads), dtype=torch.float32, device=dev)
    n_items, n_split = _sched_counts(items, split)
    t_n_items, t_n_split = _sched_counts(t_items, t_split)
    partials = None
    if (items is not None and n_split > 0) or (t_items is not None and t_n_split > 0):
        partials = torch.empty((max(n_slots, t_slots, 1), 2 * HC), dtype=torch.float32, device=dev)
    nat.check(
        nat.lib().kgx_dot_attention_edge_backward(
            nat.ptr(rowptr), nat.ptr(rows), n_dst, nat.ptr(items), n_items, nat.ptr(split), n_split, nat.ptr(col),
            nat.ptr(q), _attn_ld(q), nat.ptr(k), _attn_ld(k), nat.ptr(v), _attn_ld(v), nat.ptr(edge),
            _attn_ld(edge), edge.shape[0], nat.ptr(edge_idx), heads, channels, float(scale), nat.ptr(out),
            out.stride(0), nat.ptr(stats), nat.ptr(grad_out), grad_out.stride(0),
            nat.ptr(t_rowptr), nat.ptr(t_rows), n_src, nat.ptr(t_items), t_n_items, nat.ptr(t_split), t_n_split,
            nat.ptr(t_col), nat.ptr(t_key), nat.ptr(t_edge_idx), nat.ptr(g_q), g_q.stride(0), nat.ptr(g_k),
            g_k.stride(0), nat.ptr(g_v), g_v.stride(0), nat.ptr(grad_e), _attn_ld(grad_e), nat.ptr(dsum),
            nat.ptr(partials), *_drop_args(drop_key, drop_p, drop_seed), nat.stream(dev),
        ),
        "kgx_dot_attention_edge_backward",
    )
    return g_q, g_k, g_v


@torch.library.custom_op("kgx::dot_attention_edge_backward", mutates_args=())
def dot_attention_edge_backward(
    grad_out: torch.Tensor,
    q: torch.Tensor,
    k: torch.Tensor,
    v: torch.Tensor,
    edge: torch.Tensor,
    out: torch.Tensor,
    stats: torch.Tensor,
    rowptr: torch.Tensor,
    rows: torch.Tensor,
    items: Optional[torch.Tensor],
    split: Optional[torch.Tensor],
    col: torch.Tensor,
    n_slots: int,
    t_rowptr: torch.Tensor,
    t_rows: torch.Tensor,
    t_items: Optional[torch.Tensor],
    t_split: Optional[torch.Tensor],
    t_col: torch.Tensor,
    t_key: torch.Tensor,
    t_slots: int,
    heads: int,
    channels: int,
    scale: float,
    edge_idx: Optional[torch.Tensor],
    t_edge_idx: torch.Tensor,
    zero_grad_edge: bool,
    drop_key: Optional[torch.Tensor] = None,
    drop_p: float = 0.0,
    drop_seed: int = 0,
) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """(grad_q, grad_k, grad_v, grad_edge) of kgx::dot_attention_save with an edge
    table; zero_grad_edge: some row of `edge` belongs to no kept slot."""
    make = torch.zeros if zero_grad_edge or col.numel() == 0 else torch.empty
    g_e = make((edge.shape[0], heads * channels), dtype=torch.float32, device=edge.device)
    g_q, g_k, g_v = dot_attention_edge_backward_into(
        g_e, grad_out, q, k, v, edge, out, stats, rowptr, rows, items, split, col, n_slots, t_rowptr, t_rows,
        t_items, t_split, t_col, t_key, t_slots, heads, channels, scale, edge_idx, t_edge_idx, drop_key, drop_p,
        drop_seed)
    return g_q, g_k, g_v, g_e


@dot_attention_edge_backward.register_fake
def _dot_attention_edge_backward_fake(grad_out, q, k, v, edge, out, stats, rowptr, rows, items, split, col, n_slots,
                                      t_rowptr, t_rows, t_items, t_split, t_col, t_key, t_slots, heads, channels,
                                      scale, edge_idx, t_edge_idx, zero_grad_edge, drop_key=None, drop_p=0.0,
                                      drop_seed=0):
    hc = heads * channels
    return (q.new_empty((rowptr.shape[0] - 1, hc)), q.new_empty((t_rowptr.shape[0] - 1, hc)),
            q.new_empty((t_rowptr.shape[0] - 1, hc)), q.new_empty((edge.shape[0], hc)))


@torch.library.custom_op("kgx::gather_rows", mutates_args=())
def gather_rows(table: torch.Tensor, rows: torch.Tensor) -> torch.Tensor:
    table = _f32c(table)
    dev = nat.require_device(table, rows)
    n, F = rows.numel(), table.shape[1]
    out = torch.empty((n, F), dtype=torch.float32, device=dev)
    nat.check(
        nat.lib().kgx_gather_rows(
            nat.ptr(table), table.stride(0), nat.ptr(rows.contiguous()), n, F, nat.ptr(out), out.stride(0),
            nat.stream(dev),
        ),
        "kgx_gather_rows",
    )
    return out


@gather_rows.register_fake
def _gather_rows_fake(table, rows):
    return table.new_empty((rows.shape[0], table.shape[1]))


@torch.library.custom_op("kgx::scatter_f32", mutates_args=())
def scatter_f32(values: torch.Tensor, perm: torch.Tensor, n_out: int) -> torch.Tensor:
    """out[perm[i]] = values[i]; positions not hit are zero."""
    values = _f32c(values)
    dev = nat.require_device(values, perm)
    out = torch.zeros(n_out, dtype=torch.float32, device=dev)
    nat.check(
        nat.lib().kgx_scatter_f32(nat.ptr(values), nat.ptr(perm.contiguous()), values.numel(), nat.ptr(out),
                                  nat.stream(dev)),
        "kgx_scatter_f32",
    )
    return out


@scatter_f32.register_fake
def _scatter_fake(values, perm, n_out):
    return values.new_empty((n_out,))


# ---------------------------------------------------------------------------
# graph-level helpers used by the layers
# ---------------------------------------------------------------------------
# When a list is installed here, every aggregation launch is bracketed by a
# pair of torch.cuda.Events recorded on the current stream — the stream the
# kernels are launched on — so a harness can time the kernels alone.
EVENT_SINK: list | None = None


def _timed(fn):
    if EVENT_SINK is None:
        return fn()
    start = torch.cuda.Event(enable_timing=True)
    end = torch.cuda.Event(enable_timing=True)
    start.record()
    out = fn()
    end.record()
    EVENT_SINK.append((start, end))
    return out

def _reduce_id(reduce) -> int:
    return nat.REDUCE_IDS[reduce] if isinstance(reduce, str) else int(reduce)


def _needs_grad(*ts) -> bool:
    return torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in ts)


def _exact_short(g, red) -> int:
    """EXACT mode's short-row suffix for kgx_spmm's n_long_items (graph.exact_short_start)."""
    from . import graph as G

    return -1 if red == nat.STD else G.exact_short_start(g)


def _aggregate_raw(g, table, red, weighted, by_edge, epilogue, bias, xroot, gin_scale, exact, drop_p=0.0,
                   drop_seed=0):
    items, _, split, _, n_slots = g.work(exact or red == nat.STD)
    idx = g.eid if by_edge else g.col
    w = g.w if weighted else None
    if weighted and w is None:
        raise ValueError("graph was built without GCN normalisation weights")
    if drop_p > 0 and red != nat.SUM:
        raise ValueError("message dropout is implemented for sum aggregation (GCNConv) only")
    return _timed(lambda: torch.ops.kgx.spmm(
        table, g.rowptr, g.rows, items, split, idx, w, n_slots, red, epilogue, bias, xroot, float(gin_scale),
        g.eid if drop_p > 0 else None, float(drop_p), int(drop_seed),
        g.n_long if items is not None else _exact_short(g, red),
    ))


def _reduce_backward(g: CSRGraph, red: int, weighted: bool, by_edge: bool, table: torch.Tensor | None,
                     grad_out: torch.Tensor, exact: bool, table_rows: int, raw: bool = False, drop_p: float = 0.0,
                     drop_seed: int = 0) -> torch.Tensor:
    """d loss / d table of REDUCE_{e in row} table[idx_e] (* w_e), given d loss / d out.

    sum / mean: the transposed aggregation (graph.transpose: each source row
    gathers the gradient rows of its edges' destinations, in input-edge order);
    max / min: kgx_spmm_max_backward (ties share evenly, +-inf rows pass
    nothing — torch scatter_reduce amax/amin under the reference's isinf guard;
    weighted: extreme and ties among the products, each share times w_e);
    by_edge (message tensors): each message receives its row's gradient."""
    from . import graph as G

    grad_out = grad_out.contiguous()
    if red == nat.STD:
        # std_i = sqrt(ssd_i / n_i) (0 where n_i <= 1), aggregators.py:182-228:
        #   d std_i / d m_e = (m_e - mean_i) / (n_i std_i)   (the mean's own path sums to 0)
        # so with A_i = g_i / (n_i std_i) (0 where n_i <= 1):
        #   grad m_e = A_i (m_e - mean_i);  grad x_j = x_j * (A^T A)_j - (A^T (A * mean))_j
        std = _aggregate_raw(g, table, nat.STD, False, by_edge, nat.EPI_NONE, None, None, 1.0, True)
        mean = _aggregate_raw(g, table, nat.MEAN, False, by_edge, nat.EPI_NONE, None, None, 1.0, True)
        # As torch autograd of the reference: the count <= 1 guard's where() sends 0 into
        # sqrt'(0) = inf, so rows with one message (and zero-variance rows) yield NaN.
        count = torch.clamp(g.deg, max=1 << 24).float().unsqueeze(1)
        A = grad_out / (torch.clamp(count, min=1e-8) * std)
        A = torch.where(count > 1, A, torch.full_like(A, float("nan")))
        if by_edge:
            rows = G.row_of_slot(g).long()
            gt = grad_out.new_zeros((table_rows, grad_out.shape[1]))
            gt.index_copy_(0, g.eid.long(), A.index_select(0, rows) * (table.index_select(0, g.eid.long())
                                                                       - mean.index_select(0, rows)))
            return gt
        t = G.transpose(g)
        sa = _aggregate_raw(t, A.contiguous(), nat.SUM, False, False, nat.EPI_NONE, None, None, 1.0, exact)
        sb = _aggregate_raw(t, (A * mean).contiguous(), nat.SUM, False, False, nat.EPI_NONE, None, None, 1.0, exact)
        return table * sa - sb
    if red in (nat.MAX, nat.MIN):
        table = table.contiguous()
        gt = torch.zeros_like(table)
        idx = g.eid if by_edge else g.col
        w = _f32c(g.w) if weighted else None  # the forward's messages were table[idx_e] * w_e
        if weighted and (w is None or w.numel() != idx.numel()):
            raise ValueError("graph was built without GCN normalisation weights")
        nat.check(
            nat.lib().kgx_spmm_max_backward_w(
                red, int(raw), nat.ptr(g.rowptr), g.n_dst, nat.ptr(idx), nat.ptr(w), nat.ptr(table),
                table.stride(0), table.shape[1], nat.ptr(grad_out), grad_out.stride(0), nat.ptr(gt), gt.stride(0),
                nat.stream(table.device),
            ),
            "kgx_spmm_max_backward",
        )
        return gt
    d = grad_out
    if red == nat.MEAN:  # forward: sum / max(count_f32, 1e-8) (aggregators.py:56-85)
        count = torch.clamp(g.deg, max=1 << 24).float()
        d = (grad_out / torch.clamp(count, min=1e-8).unsqueeze(1)).contiguous()
    if by_edge:
        vals = d.index_select(0, G.row_of_slot(g).long())
        if weighted:
            vals = vals * g.w.unsqueeze(1)
        gt = grad_out.new_zeros((table_rows, grad_out.shape[1]))
        gt.index_copy_(0, g.eid.long(), vals)
        return gt
    t = G.transpose(g)  # t.eid = input edge ids: the same dropout mask keys as the forward
    return _aggregate_raw(t, d, nat.SUM, weighted, False, nat.EPI_NONE, None, None, 1.0, exact, drop_p, drop_seed)


def dropout_mask(seed: int, p: float, keys: torch.Tensor, F: int) -> torch.Tensor:
    """The multipliers (0 or 1/(1-p)) kgx's message dropout applies: [len(keys), F]."""
    keys = keys.to(torch.int32).contiguous()
    out = torch.empty((keys.numel(), F), dtype=torch.float32, device=keys.device)
    nat.check(nat.lib().kgx_dropout_mask(int(seed) & (2**64 - 1), float(p), nat.ptr(keys), keys.numel(), F,
                                         nat.ptr(out), nat.stream(keys.device)), "kgx_dropout_mask")
    return out


class _AggregateFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, table, bias, xroot, g, red, weighted, by_edge, epilogue, gin_scale, exact, drop_p, drop_seed):
        ctx.g, ctx.red, ctx.weighted, ctx.by_edge = g, red, weighted, by_edge
        ctx.epilogue, ctx.gin_scale, ctx.exact = epilogue, gin_scale, exact
        ctx.drop_p, ctx.drop_seed = drop_p, drop_seed
        ctx.table_rows = table.shape[0]
        ctx.save_for_backward(table if red in (nat.MAX, nat.MIN, nat.STD) else None)
        return _aggregate_raw(g, table, red, weighted, by_edge, epilogue, bias, xroot, gin_scale, exact, drop_p,
                              drop_seed)

    @staticmethod
    def backward(ctx, grad_out):
        (table,) = ctx.saved_tensors
        g_table = g_bias = g_xroot = None
        if ctx.needs_input_grad[0]:
            g_table = _reduce_backward(ctx.g, ctx.red, ctx.weighted, ctx.by_edge, table, grad_out, ctx.exact,
                                       ctx.table_rows, raw=ctx.epilogue == nat.EPI_RAW, drop_p=ctx.drop_p,
                                       drop_seed=ctx.drop_seed)
        if ctx.needs_input_grad[1] and ctx.epilogue == nat.EPI_BIAS:
            g_bias = grad_out.sum(0)
        if ctx.needs_input_grad[2] and ctx.epilogue == nat.EPI_GIN:
            g_xroot = grad_out * ctx.gin_scale
        return g_table, g_bias, g_xroot, None, None, None, None, None, None, None, None, None


def aggregate(
    g: CSRGraph,
    table: torch.Tensor,
    reduce: str | int = "sum",
    *,
    weighted: bool = False,
    by_edge: bool = False,
    epilogue: int = nat.EPI_NONE,
    bias: torch.Tensor | None = None,
    xroot: torch.Tensor | None = None,
    gin_scale: float = 1.0,
    exact: bool = False,
    dropout: float = 0.0,
    seed: int = 0,
) -> torch.Tensor:
    """out[i] = EPI(REDUCE_{e in row i} table[idx[e]] * (w[e] if weighted)).

    by_edge=False gathers node rows through `col` (the fused propagate path);
    by_edge=True gathers rows of a per-edge message tensor through `eid`
    (the reference's Aggregator.aggregate(messages, target_idx, dim_size)).
    Differentiable in table, bias and xroot (sum, mean, max, min).  dropout > 0
    (sum only): every message element is kept with probability 1 - dropout and
    scaled by 1/(1 - dropout), the mask a function of (seed, input edge id,
    column) -- GCNConv's training-time message dropout (gcn_conv.py:237-242).
    """
    red = _reduce_id(reduce)
    if dropout and by_edge:
        raise ValueError("message dropout applies to gathered node rows, not to message tensors")
    if _needs_grad(table, bias, xroot):
        if weighted and epilogue == nat.EPI_RAW and red in (nat.MAX, nat.MIN) and table.requires_grad:
            # kgx_spmm_max_backward_w has no unguarded form: say so here, not in the middle of backward()
            raise NotImplementedError("aggregate: a weighted max / min with the raw (unguarded) epilogue is "
                                      "forward-only; differentiate the guarded form or drop the weights")
        return _AggregateFn.apply(table, bias, xroot, g, red, weighted, by_edge, epilogue, float(gin_scale), exact,
                                  float(dropout), int(seed))
    return _aggregate_raw(g, table, red, weighted, by_edge, epilogue, bias, xroot, gin_scale, exact, float(dropout),
                          int(seed))


# ---------------------------------------------------------------------------
# Fused multi-aggregation (kgx_multi_aggr): several reducers, one gather
# ---------------------------------------------------------------------------
def _reduce_list(reduces) -> list[int]:
    """Reducer names / ids -> 1..5 distinct kgx_reduce ids, in the caller's order."""
    if isinstance(reduces, (str, int)):
        reduces = [reduces]
    ids = []
    for r in reduces:
        if isinstance(r, str) and r not in nat.REDUCE_IDS:
            raise ValueError(f"multi_aggregate: unknown reducer {r!r}; available: {list(nat.REDUCE_IDS)}")
        ids.append(_reduce_id(r))
    if not 1 <= len(ids) <= 5 or len(set(ids)) != len(ids) or any(i < nat.SUM or i > nat.STD for i in ids):
        raise ValueError(f"multi_aggregate: 1..5 distinct reducers of {list(nat.REDUCE_IDS)} expected, got "
                         f"{list(reduces)}")
    return ids


def _c_ints(ids):
    return (ctypes.c_int * len(ids))(*ids)


def multi_aggr_partials_floats(reduces, n_slots: int, F: int) -> int:
    """Floats of split-row chunk state kgx_multi_aggr needs (kgx_multi_aggr_partials_floats)."""
    ids = _reduce_list(reduces)
    floats = ctypes.c_int64(0)
    nat.check(nat.lib().kgx_multi_aggr_partials_floats(len(ids), _c_ints(ids), int(n_slots), int(F),
                                                       ctypes.byref(floats)), "kgx_multi_aggr_partials_floats")
    return floats.value


def multi_aggr_gathers(F: int) -> int:
    """Neighbour rows kgx_multi_aggr keeps in flight per lane group for a contiguous
    [*, F] table (multi_aggr.hip's Gathers<NT>::U): also the longest row whose std
    second pass reuses the gathered registers.  Tests place row degrees around it."""
    vec = 4 if F % 4 == 0 else (2 if F % 2 == 0 else 1)
    cv = min(F, 256 * vec) // vec
    return 6 if cv <= 64 else (4 if cv <= 128 else 2)


@torch.library.custom_op("kgx::multi_aggr", mutates_args=())
def multi_aggr(
    table: torch.Tensor,
    rowptr: torch.Tensor,
    rows: torch.Tensor,
    items: Optional[torch.Tensor],
    split: Optional[torch.Tensor],
    idx: torch.Tensor,
    n_slots: int,
    reduces: List[int],
) -> torch.Tensor:
    """out[:, k*F:(k+1)*F] = reducer reduces[k] of the rows table[idx[e]] of every CSR row."""
    table = _f32c(table)
    dev = nat.require_device(table, rowptr, rows, idx, items, split)
    ids = _reduce_list(list(reduces))
    n_dst = rowptr.numel() - 1
    F = table.shape[1]
    out = torch.empty((n_dst, len(ids) * F), dtype=torch.float32, device=dev)
    if n_dst == 0 or F == 0:
        return out
    if idx.numel() == 0 or table.shape[0] == 0:  # no edges: every block of an empty row is 0
        return out.zero_()
    n_items = 0 if items is None else items.shape[0]
    n_split = 0 if split is None else split.shape[0]
    partials, floats = None, 0
    if items is not None and n_split > 0:
        floats = multi_aggr_partials_floats(ids, n_slots, F)
        partials = torch.empty(floats, dtype=torch.float32, device=dev)
    nat.check(
        nat.lib().kgx_multi_aggr(
            len(ids), _c_ints(ids), nat.ptr(rowptr), nat.ptr(rows), n_dst, nat.ptr(items), n_items,
            nat.ptr(split), n_split, nat.ptr(idx), nat.ptr(table), table.stride(0), F,
            nat.ptr(out), out.stride(0), nat.ptr(partials), floats, nat.stream(dev),
        ),
        "kgx_multi_aggr",
    )
    return out


@multi_aggr.register_fake
def _multi_aggr_fake(table, rowptr, rows, items, split, idx, n_slots, reduces):
    return table.new_empty((rowptr.shape[0] - 1, len(reduces) * table.shape[1]))


def _multi_aggregate_raw(g, table, ids, by_edge, exact):
    items, _, split, _, n_slots = g.work(exact)
    idx = g.eid if by_edge else g.col
    return _timed(lambda: torch.ops.kgx.multi_aggr(table, g.rowptr, g.rows, items, split, idx, n_slots, ids))


def _multi_backward(g: CSRGraph, ids: list[int], by_edge: bool, table: torch.Tensor, full: torch.Tensor,
                    full_ids: list[int], grad_out: torch.Tensor, exact: bool) -> torch.Tensor:
    """d loss / d table of multi_aggregate, from existing kernels and the saved
    forward blocks `full` (mean and std are not recomputed).  With n the clamped
    fp32 count, A = g_std / (n std) (NaN where n <= 1: _reduce_backward's convention)
    and D = g_sum + g_mean / n - A * mean:
        grad_x = T_sum(D) + x * T_sum(A)
    as ONE transposed kgx_spmm sum over the 2F-wide table [D | A]; max and min
    add kgx_spmm_max_backward passes into one zeroed buffer.  by_edge: every
    message receives its row's terms through row_of_slot, std's in the centred
    form A * (m_e - mean) of _reduce_backward's by-edge branch."""
    from . import graph as G

    F = table.shape[1]
    grad_out = grad_out.contiguous()

    def blk(t, id_list, red):
        k = id_list.index(red)
        return t[:, k * F:(k + 1) * F]

    count = torch.clamp(g.deg, max=1 << 24).float().unsqueeze(1)
    n = torch.clamp(count, min=1e-8)
    D = A = mean = None
    if nat.SUM in ids:
        D = blk(grad_out, ids, nat.SUM)
    if nat.MEAN in ids:
        d = blk(grad_out, ids, nat.MEAN) / n
        D = d if D is None else D + d
    if nat.STD in ids:
        A = blk(grad_out, ids, nat.STD) / (n * blk(full, full_ids, nat.STD))
        A = torch.where(count > 1, A, torch.full_like(A, float("nan")))
        mean = blk(full, full_ids, nat.MEAN)
        if not by_edge:  # per edge the centred form A * (m_e - mean) is applied instead
            d = A * mean
            D = -d if D is None else D - d
    gt = None
    if nat.MAX in ids or nat.MIN in ids:
        table = table.contiguous()
        gt = torch.zeros_like(table)
        idx = g.eid if by_edge else g.col
        for red in (nat.MAX, nat.MIN):
            if red not in ids:
                continue
            go = blk(grad_out, ids, red)
            nat.check(
                nat.lib().kgx_spmm_max_backward(
                    red, 0, nat.ptr(g.rowptr), g.n_dst, nat.ptr(idx), nat.ptr(table), table.stride(0), F,
                    nat.ptr(go), go.stride(0), nat.ptr(gt), gt.stride(0), nat.stream(table.device),
                ),
                "kgx_spmm_max_backward",
            )
    if D is None and A is None:
        return gt
    if by_edge:  # each message receives its row's terms, as _reduce_backward's by-edge branches
        rows = G.row_of_slot(g).long()
        eid = g.eid.long()
        vals = D.index_select(0, rows) if D is not None else None
        if A is not None:
            v = A.index_select(0, rows) * (table.index_select(0, eid) - mean.index_select(0, rows))
            vals = v if vals is None else vals + v
        lin = grad_out.new_zeros((table.shape[0], F))
        lin.index_copy_(0, eid, vals)
    else:
        t = G.transpose(g)
        DA = (torch.cat([D, A], dim=1) if A is not None else D).contiguous()
        S = _aggregate_raw(t, DA, nat.SUM, False, False, nat.EPI_NONE, None, None, 1.0, exact)
        lin = S[:, :F] + table * S[:, F:] if A is not None else S
    return lin if gt is None else gt.add_(lin)


class _MultiAggregateFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, table, g, ids, by_edge, exact):
        # std's gradient reads the row means: keep a mean block beside the requested ones
        full_ids = ids + [nat.MEAN] if nat.STD in ids and nat.MEAN not in ids else ids
        full = _multi_aggregate_raw(g, table, full_ids, by_edge, exact)
        ctx.g, ctx.ids, ctx.full_ids, ctx.by_edge, ctx.exact = g, ids, full_ids, by_edge, exact
        ctx.save_for_backward(table, full)
        if full_ids is ids:
            return full
        return full[:, : len(ids) * table.shape[1]].contiguous()

    @staticmethod
    def backward(ctx, grad_out):
        table, full = ctx.saved_tensors
        g_table = None
        if ctx.needs_input_grad[0]:
            g_table = _multi_backward(ctx.g, ctx.ids, ctx.by_edge, table, full, ctx.full_ids, grad_out, ctx.exact)
        return g_table, None, None, None, None


def multi_aggregate(g: CSRGraph, table: torch.Tensor, reduces, *, by_edge: bool = False,
                    exact: bool = False) -> torch.Tensor:
    """[n_dst, len(reduces) * F]: block k is reducer reduces[k] ("sum", "mean",
    "max", "min", "std" or their ids, each at most once) of table[idx[e]] over
    every row's edges, all from ONE gather of each neighbour row (kgx_multi_aggr)
    instead of one kgx_spmm launch per reducer.  by_edge as in aggregate().
    exact=True: every block bit-identical to aggregate(..., exact=True).
    Otherwise the schedule is used, std included: split hub rows fold their
    chunks' (sum, M2) pairwise in chunk order, deterministic but re-associated.
    Differentiable in table; the backward is composed from the existing kernels."""
    ids = _reduce_list(reduces)
    if _needs_grad(table):
        return _MultiAggregateFn.apply(table, g, ids, bool(by_edge), bool(exact))
    return _multi_aggregate_raw(g, table, ids, by_edge, exact)


def _tiny_of(g, items):
    """(tpack, tw, n_short_end, n_tiny2) for a fused launch over g's schedule
    (tiny.py: packed records of the degree <= 2 tail, built once per graph)."""
    if items is None:
        return None, None, -1, 0
    from . import tiny

    return tiny.tiny_pack(g)


def _slice_of(g, items, x, W, red, x2):
    """The sliced schedule's arguments of kgx::spmm_gemm for this launch (slice.py:
    built on the second forward over g), or the eight "none" values."""
    from . import slice as S

    none = (None, None, None, None, None, 0, 0, -1)
    T, C, share = S.env_params()
    if not S.slice_wanted(mode=S.env_mode(), default_on=S.DEFAULT_ON, have_items=items is not None,
                          two_tables=x2 is not None, reduce=red, f_in=x.shape[1], f_out=W.shape[1],
                          n_edges=int(g.col.numel()), T=T, C=C):
        return none
    if _share_gpu() or "accumulate_only" in g.extras or "restricted_of" in g.extras:
        return none  # the sharded layers' passes and restricted sub-schedules keep the plain schedule
    sl = S.sliced_schedule(g, T, C, share)
    if sl is None:
        return none
    return sl.items, sl.lists, sl.col, sl.w, sl.fix, sl.n_slots, sl.max_list, sl.head_short_end


def _aggregate_transform_raw(g, x, W, red, weighted, bias, pre_gin, gin_scale, exact, relu=False, x2=None,
                             allow_slice=True):
    items, _, split, _, n_slots = g.work(exact)
    w = g.w if weighted else None
    if weighted and w is None:
        raise ValueError("graph was built without GCN normalisation weights")
    sl = _slice_of(g, items if allow_slice else None, x, W, red, x2)
    if sl[0] is not None and not weighted:
        sl = sl[:3] + (None,) + sl[4:]
    return _timed(lambda: torch.ops.kgx.spmm_gemm(
        x, g.rowptr, g.rows, items, split, g.col, w, n_slots, red, W, bias, bool(pre_gin), float(gin_scale),
        bool(relu), g.n_long if items is not None else -1, *_tiny_of(g, items), x2, *sl
    ))


def gemm_tn(P: torch.Tensor, D: torch.Tensor, with_db: bool = False):
    """(P^T D, column sums of D or None) in one pass over P and D (kgx_gemm_tn:
    the bf16x3-split MFMA product over the node dimension, split-K over row
    ranges with partials summed in block order) -- the weight and bias
    gradients of a layer out = P W + b.  Device tensors only (the product path
    has no CPU fallback)."""
    P = P if P.stride(-1) == 1 else P.contiguous()
    D = D if D.stride(-1) == 1 else D.contiguous()
    dev = nat.require_device(P, D)
    if P.dtype != torch.float32 or D.dtype != torch.float32 or P.dim() != 2 or D.dim() != 2 or P.shape[0] != D.shape[0]:
        raise ValueError(f"gemm_tn: float32 [N, K] and [N, M] expected (got {tuple(P.shape)}, {tuple(D.shape)})")
    N, K, M = P.shape[0], P.shape[1], D.shape[1]
    dW = torch.empty((K, M), dtype=torch.float32, device=dev)
    db = torch.empty(M, dtype=torch.float32, device=dev) if with_db else None
    if K == 0 or M == 0:
        return dW, (db.zero_() if db is not None else None)
    L = nat.lib()
    nbytes = ctypes.c_size_t(0)
    nat.check(L.kgx_gemm_tn_workspace_bytes(N, K, M, ctypes.byref(nbytes)), "kgx_gemm_tn_workspace_bytes")
    ws = torch.empty(max(nbytes.value, 4), dtype=torch.uint8, device=dev)
    nat.check(L.kgx_gemm_tn(N, nat.ptr(P), P.stride(0), K, nat.ptr(D), D.stride(0), M, nat.ptr(dW), M, nat.ptr(db),
                            nat.ptr(ws), nbytes.value, nat.stream(dev)), "kgx_gemm_tn")
    return dW, db


class _AggregateTransformFn(torch.autograd.Function):
    """out = bias + PRE(A x) W.  Backward: P = PRE(A x) is recomputed (one
    aggregation launch) rather than kept from the forward; dW = P^T dOut,
    db = sum dOut, dx = A^T-backward(dOut W^T) (+ gin_scale dOut W^T)."""

    @staticmethod
    def forward(ctx, x, W, bias, g, red, weighted, pre_gin, gin_scale, exact):
        ctx.g, ctx.red, ctx.weighted, ctx.pre_gin, ctx.gin_scale, ctx.exact = g, red, weighted, pre_gin, gin_scale, exact
        items, _, split, _, n_slots = g.work(exact)
        w = g.w if weighted else None
        if ctx.needs_input_grad[1]:  # keep P = PRE(A x) for dW (one extra row store instead of a recompute)
            out, P = _timed(lambda: torch.ops.kgx.spmm_gemm_save(
                x, g.rowptr, g.rows, items, split, g.col, w, n_slots, red, W, bias, bool(pre_gin), float(gin_scale),
                g.n_long if items is not None else -1, *_tiny_of(g, items)))
        else:
            out = _aggregate_transform_raw(g, x, W, red, weighted, bias, pre_gin, gin_scale, exact)
            P = None
        ctx.save_for_backward(x if red in (nat.MAX, nat.MIN) else None, W, P)
        ctx.x_rows = x.shape[0]
        return out

    @staticmethod
    def backward(ctx, grad_out):
        from . import graph as G

        x, W, P = ctx.saved_tensors
        grad_out = grad_out.contiguous()
        g_x = g_W = g_b = None
        # dW / db (kgx_gemm_tn) beside the dx pass: the side stream waits for an event recorded
        # here, before dx is launched, and is forked after it, so dx's blocks are dispatched first;
        # W^T is copied before the event (queued after it, the small copy waited for the whole
        # dW pass: its waves found no registers free beside kgx_gemm_tn's, profiles/r06/train/)
        overlap = ctx.needs_input_grad[1] and ctx.needs_input_grad[0] and grad_out.is_cuda and _tn_overlap()
        W_t = W.t().contiguous() if ctx.needs_input_grad[0] else None  # before the fork: see above
        start = None
        if overlap:
            start = torch.cuda.Event()
            start.record()
        if not overlap and ctx.needs_input_grad[1]:  # dW = P^T dOut and db = colsum(dOut) in one pass
            g_W, g_b = gemm_tn(P, grad_out, with_db=ctx.needs_input_grad[2])
        elif not ctx.needs_input_grad[1] and ctx.needs_input_grad[2]:
            g_b = grad_out.sum(0)
        if ctx.needs_input_grad[0]:
            with _unsplit():  # the transposed pass one-stream (see _unsplit)
                f_out, f_in = W.shape[1], W.shape[0]
                if ctx.red in (nat.SUM, nat.MEAN) and not ctx.pre_gin and fused_transform_supported(f_out, f_in):
                    # dx = A^T (dOut W^T) = (A^T dOut) W^T: the same fused kernel on the transposed graph
                    d = grad_out
                    if ctx.red == nat.MEAN:
                        count = torch.clamp(ctx.g.deg, max=1 << 24).float()
                        d = (grad_out / torch.clamp(count, min=1e-8).unsqueeze(1)).contiguous()
                    t = G.transpose(ctx.g)
                    g_x = _aggregate_transform_raw(t, d, W_t, nat.SUM, ctx.weighted, None, False, 1.0, ctx.exact,
                                                   allow_slice=False)
                else:
                    dP = grad_out @ W_t
                    g_x = _reduce_backward(ctx.g, ctx.red, ctx.weighted, False, x, dP, ctx.exact, ctx.x_rows)
                    if ctx.pre_gin:
                        g_x = g_x + dP * ctx.gin_scale
        if overlap:
            cur = torch.cuda.current_stream(grad_out.device)
            side = _side_stream(grad_out.device)
            side.wait_event(start)
            with torch.cuda.stream(side):
                g_W, g_b = gemm_tn(P, grad_out, with_db=ctx.needs_input_grad[2])
            P.record_stream(side)
            grad_out.record_stream(side)
            cur.wait_stream(side)  # join: dW / db are ready before anything later on this stream
            for t_ in (g_W, g_b):
                if t_ is not None:
                    t_.record_stream(cur)
        return g_x, g_W, g_b, None, None, None, None, None, None


_SIDE_STREAMS: dict = {}


def _side_stream(dev: torch.device) -> torch.cuda.Stream:
    """One side stream per device for backward work that runs beside the main pass."""
    key = dev.index if dev.index is not None else torch.cuda.current_device()
    s = _SIDE_STREAMS.get(key)
    if s is None:
        s = _SIDE_STREAMS[key] = torch.cuda.Stream(device=dev)
    return s


def _tn_overlap() -> bool:
    """KGX_TN_OVERLAP (default 0): 1 runs the fused layers' dW / db pass (kgx_gemm_tn) on a side
    stream beside the dx pass of the same backward.  Off by default: both passes stream HBM, and
    side by side the dx pass's main kernel went 8.2 -> 13.9 ms for the 2.3 ms of dW it hid (NS
    training step 21.7 ms serial against 21.8-24.4 overlapped, profiles/r06/train/overlap.md)."""
    return os.environ.get("KGX_TN_OVERLAP", "0") not in ("0", "", "false", "False")


def aggregate_transform(
    g: CSRGraph,
    x: torch.Tensor,
    W: torch.Tensor,
    reduce: str | int = "sum",
    *,
    weighted: bool = False,
    bias: torch.Tensor | None = None,
    pre_gin: bool = False,
    gin_scale: float = 1.0,
    exact: bool = False,
    out: torch.Tensor | None = None,
    relu: bool = False,
    x2: torch.Tensor | None = None,
    accumulate: bool = True,
) -> torch.Tensor:
    """out = bias + PRE(REDUCE_{e in row} x[col_e] * w_e) @ W in one fused launch
    (out += ... in place when `out` is given, or, with accumulate=False, the
    graph's scheduled rows of `out` overwritten; relu=True applies max(., 0) in
    the kernel's store).  Differentiable in x, W, bias.  x2 (forward only): a
    second table, sources col >= x.shape[0] gather x2[col - x.shape[0]]
    (the sharded layers' own rows + received halo rows in one pass)."""
    red = _reduce_id(reduce)
    if x2 is not None and _needs_grad(x, x2, W, bias):
        raise NotImplementedError("aggregate_transform(x2=...) is a forward-only (no_grad) path")
    if out is not None:  # into `out`: a sum may be split over launches (the caller splits a row's edges);
        # a mean / max / min launch must cover each row's whole edge list
        if red != nat.SUM and (x2 is not None or x.shape[1] == F256):
            raise ValueError("aggregate_transform(out=...): two-table and 256-wide passes accumulate plain sums only")
        if accumulate and (pre_gin or (relu and x.shape[1] == F256)):
            raise ValueError("aggregate_transform(out=...): pre_gin (and relu at F_in 256) only with "
                             "accumulate=False (overwrite)")
        if _needs_grad(x, W, bias, out):
            raise NotImplementedError("aggregate_transform(out=...) is a forward-only (no_grad) path")
        items, _, split, _, n_slots = g.work(exact)
        w = g.w if weighted else None
        flags = (nat.FUSED_PRE_GIN if pre_gin else 0) | (nat.FUSED_RELU if relu else 0)
        _timed(lambda: torch.ops.kgx.spmm_gemm_acc_(out, x, g.rowptr, g.rows, items, split, g.col, w, n_slots, red,
                                                   W, bias, g.n_long if items is not None else -1,
                                                   *_tiny_of(g, items), x2, bool(accumulate), int(flags),
                                                   float(gin_scale)))
        return out
    if x2 is not None:
        return _aggregate_transform_raw(g, x, W, red, weighted, bias, pre_gin, gin_scale, exact, relu, x2)
    if _needs_grad(x, W, bias):
        y = _AggregateTransformFn.apply(x, W, bias, g, red, weighted, pre_gin, float(gin_scale), exact)
        return torch.relu(y) if relu else y
    return _aggregate_transform_raw(g, x, W, red, weighted, bias, pre_gin, gin_scale, exact, relu)


def _fwd_slot32(t):
    """int32 [kept] of a transposed graph: the forward CSR slot of each of its slots (cached on it)."""
    slot = t.extras.get("fwd_slot32")
    if slot is None:
        slot = t.extras["fwd_slot"].to(torch.int32)
        t.extras["fwd_slot32"] = slot
    return slot


def _gatv2_raw(g, h_src, h_dst, att, heads, channels, negative_slope, bias, exact, drop_p=0.0, drop_seed=0,
               edge=None, edge_order="input"):
    items, _, split, _, n_slots = g.work(exact)
    return _timed(lambda: torch.ops.kgx.gatv2(
        h_src, h_dst, g.rowptr, g.rows, items, split, g.col, att.reshape(-1), heads, channels,
        float(negative_slope), bias, n_slots, g.eid if drop_p > 0 else None, float(drop_p), int(drop_seed),
        edge, g.eid if edge is not None and edge_order == "input" else None,
    ))


class _GATv2Fn(torch.autograd.Function):
    """Autograd of the fused GATv2 aggregation: the forward keeps its output
    and per-row softmax statistics; kgx_gatv2_backward does one pass over the
    destination CSR (d h_dst, d att, per-edge alpha / ds, and d edge with an
    edge table) and pulls d h_src over the transposed CSR, both with hub rows
    split into chunks."""

    @staticmethod
    def forward(ctx, h_src, h_dst, att, bias, g, heads, channels, negative_slope, exact, drop_p, drop_seed,
                edge=None, edge_order="input"):
        ctx.g, ctx.heads, ctx.channels, ctx.slope, ctx.exact = g, heads, channels, float(negative_slope), exact
        ctx.drop_p, ctx.drop_seed, ctx.edge_order = drop_p, drop_seed, edge_order
        items, _, split, _, n_slots = g.work(exact)
        out, stats = _timed(lambda: torch.ops.kgx.gatv2_save(
            h_src, h_dst, g.rowptr, g.rows, items, split, g.col, att.reshape(-1), heads, channels,
            float(negative_slope), bias, n_slots, g.eid if drop_p > 0 else None, float(drop_p), int(drop_seed),
            edge, g.eid if edge is not None and edge_order == "input" else None,
        ))
        ctx.has_edge = edge is not None
        ctx.save_for_backward(h_src, h_dst, att, bias, out, stats, *((edge,) if ctx.has_edge else ()))
        return out

    @staticmethod
    def _backward_edge(ctx, grad_out):
        from . import graph as G

        h_src, h_dst, att, bias, out, stats, edge = ctx.saved_tensors
        g = ctx.g
        t = G.transpose(g)
        items, _, split, _, n_slots = g.work(ctx.exact)
        t_items, _, t_split, _, t_slots = t.work(ctx.exact)
        by_input = ctx.edge_order == "input"
        # input order: the rows of input edges the graph dropped belong to no kept slot and stay zero
        n_loops = g.n_dst if g.flags & nat.CSR_SELF_LOOPS else 0
        unwritten = by_input and g.kept - n_loops != g.n_input_edges
        g_src, g_dst, g_att, g_e = _timed(lambda: torch.ops.kgx.gatv2_edge_backward(
            grad_out, h_src, h_dst, att.reshape(-1), bias, edge, out, stats, g.rowptr, g.rows, items, split, g.col,
            n_slots, t.rowptr, t.rows, t_items, t_split, t.col, _fwd_slot32(t), t_slots, ctx.heads, ctx.channels,
            ctx.slope, g.eid if by_input else None, t.eid if by_input else _fwd_slot32(t), unwritten,
            g.eid if ctx.drop_p > 0 else None, float(ctx.drop_p), int(ctx.drop_seed),
        ))
        g_bias = grad_out.sum(0) if ctx.needs_input_grad[3] else None
        return (g_src, g_dst, g_att.view(att.shape), g_bias, None, None, None, None, None, None, None, g_e, None)

    @staticmethod
    def backward(ctx, grad_out):
        from . import graph as G

        if ctx.has_edge:
            return _GATv2Fn._backward_edge(ctx, grad_out)
        h_src, h_dst, att, bias, out, stats = ctx.saved_tensors
        g, H, C = ctx.g, ctx.heads, ctx.channels
        grad_out = grad_out.contiguous()
        h_src, h_dst = h_src.contiguous(), h_dst.contiguous()
        att_flat = att.reshape(-1).contiguous()
        t = G.transpose(g)
        items, _, split, _, n_slots = g.work(ctx.exact)
        t_items, _, t_split, _, t_slots = t.work(ctx.exact)
        dev = grad_out.device
        g_src = torch.empty((g.n_src, H * C), dtype=torch.float32, device=dev)
        g_dst = torch.empty((g.n_dst, H * C), dtype=torch.float32, device=dev)
        g_att = torch.zeros(H * C, dtype=torch.float32, device=dev)
        alpha = torch.empty((max(g.kept, 1), H), dtype=torch.float32, device=dev)
        ds = torch.empty_like(alpha)
        partials = torch.empty((max(n_slots, t_slots, 1), H * C), dtype=torch.float32, device=dev)
        slot = _fwd_slot32(t)
        n_items, n_split = _sched_counts(items, split)
        t_n_items, t_n_split = _sched_counts(t_items, t_split)
        nat.check(
            nat.lib().kgx_gatv2_backward(
                nat.ptr(g.rowptr), nat.ptr(g.rows), g.n_dst, nat.ptr(items), n_items, nat.ptr(split), n_split,
                nat.ptr(g.col), nat.ptr(h_src), nat.ptr(h_dst), h_src.stride(0), nat.ptr(att_flat), H, C,
                ctx.slope, nat.ptr(out), out.stride(0), nat.ptr(bias), nat.ptr(stats), nat.ptr(grad_out),
                grad_out.stride(0), nat.ptr(t.rowptr), nat.ptr(t.rows), g.n_src, nat.ptr(t_items), t_n_items,
                nat.ptr(t_split), t_n_split, nat.ptr(t.col), nat.ptr(slot), nat.ptr(g_src), nat.ptr(g_dst),
                g_src.stride(0), nat.ptr(g_att), nat.ptr(alpha), nat.ptr(ds), nat.ptr(partials),
                *_drop_args(g.eid, ctx.drop_p, ctx.drop_seed), nat.stream(dev),
            ),
            "kgx_gatv2_backward",
        )
        g_bias = grad_out.sum(0) if ctx.needs_input_grad[3] else None
        return g_src, g_dst, g_att.view(att.shape), g_bias, None, None, None, None, None, None, None, None, None


def gatv2_aggregate(
    g: CSRGraph,
    h_src: torch.Tensor,
    h_dst: torch.Tensor,
    att: torch.Tensor,
    heads: int,
    channels: int,
    negative_slope: float,
    bias: torch.Tensor | None = None,
    exact: bool = False,
    dropout: float = 0.0,
    seed: int = 0,
    edge: torch.Tensor | None = None,
    edge_order: str = "input",
) -> torch.Tensor:
    """Fused GATv2 attention aggregation; differentiable in h_src, h_dst, att, bias.
    dropout > 0: attention dropout of alpha per (edge, head), mask of (seed, input edge id, head).

    edge (PyG's edge_dim, already projected): one row per edge that is added to
    h_dst[i] + h_src[j] in the score (not to the message); differentiable too, and a
    column-slice view of a wider tensor is read in place.
    edge_order="input": [g.n_input_edges, heads*channels] in input-edge order; the
    self-loop slots a graph added carry no feature, unless the table has
    g.n_input_edges + g.n_dst rows, whose rows E + i are then the loop of node i
    (g.eid's loop id).  "csr": [g.kept, heads*channels] in CSR slot order, which
    the kernel streams."""
    if edge is not None:
        if edge_order not in ("input", "csr"):
            raise ValueError(f"gatv2: edge_order must be 'input' or 'csr', got {edge_order!r}")
        hc = heads * channels
        rows = [g.kept] if edge_order == "csr" else [g.n_input_edges]
        if edge_order == "input" and g.flags & nat.CSR_SELF_LOOPS:
            rows.append(g.n_input_edges + g.n_dst)
        if edge.dim() != 2 or edge.shape[0] not in rows or edge.shape[1] != hc:
            want = " or ".join(f"[{r}, {hc}]" for r in rows)
            raise ValueError(f"gatv2: edge in {edge_order} order must be {want}, got {tuple(edge.shape)}")
    if _needs_grad(h_src, h_dst, att, bias, edge):
        return _GATv2Fn.apply(h_src, h_dst, att, bias, g, heads, channels, negative_slope, exact, float(dropout),
                              int(seed), edge, edge_order)
    return _gatv2_raw(g, h_src, h_dst, att, heads, channels, negative_slope, bias, exact, float(dropout), int(seed),
                      edge, edge_order)


def _dot_attention_raw(g, q, k, v, heads, channels, scale, exact, drop_p=0.0, drop_seed=0, edge=None,
                       edge_order="input"):
    items, _, split, _, n_slots = g.work(exact)
    return _timed(lambda: torch.ops.kgx.dot_attention(
        q, k, v, g.rowptr, g.rows, items, split, g.col, heads, channels, float(scale), n_slots,
        g.eid if drop_p > 0 else None, float(drop_p), int(drop_seed),
        edge, g.eid if edge is not None and edge_order == "input" else None,
    ))


class _DotAttentionFn(torch.autograd.Function):
    """Autograd of the fused dot-product attention: the forward keeps its
    output and per-row softmax statistics; kgx_dot_attention_backward runs a
    destination pass (D, d q, and d edge with an edge table) over the forward
    CSR and a source pass (d k, d v) over the transposed CSR, both recomputing
    the probabilities, hub rows split into chunks, no atomics."""

    @staticmethod
    def forward(ctx, q, k, v, edge, g, heads, channels, scale, exact, drop_p, drop_seed, edge_order):
        ctx.g, ctx.heads, ctx.channels, ctx.scale, ctx.exact = g, heads, channels, float(scale), exact
        ctx.drop_p, ctx.drop_seed, ctx.edge_order = drop_p, drop_seed, edge_order
        items, _, split, _, n_slots = g.work(exact)
        out, stats = _timed(lambda: torch.ops.kgx.dot_attention_save(
            q, k, v, g.rowptr, g.rows, items, split, g.col, heads, channels, float(scale), n_slots,
            g.eid if drop_p > 0 else None, float(drop_p), int(drop_seed),
            edge, g.eid if edge is not None and edge_order == "input" else None,
        ))
        ctx.has_edge = edge is not None
        ctx.save_for_backward(q, k, v, out, stats, *((edge,) if ctx.has_edge else ()))
        return out

    @staticmethod
    def backward(ctx, grad_out):
        from . import graph as G

        q, k, v, out, stats = ctx.saved_tensors[:5]
        g = ctx.g
        t = G.transpose(g)
        items, _, split, _, n_slots = g.work(ctx.exact)
        t_items, _, t_split, _, t_slots = t.work(ctx.exact)
        drop = (g.eid if ctx.drop_p > 0 else None, float(ctx.drop_p), int(ctx.drop_seed))
        if not ctx.has_edge:
            g_q, g_k, g_v = _timed(lambda: torch.ops.kgx.dot_attention_backward(
                grad_out, q, k, v, out, stats, g.rowptr, g.rows, items, split, g.col, n_slots,
                t.rowptr, t.rows, t_items, t_split, t.col, t.eid, t_slots, ctx.heads, ctx.channels, ctx.scale, *drop,
            ))
            return g_q, g_k, g_v, None, None, None, None, None, None, None, None, None
        by_input = ctx.edge_order == "input"
        # input order: rows of edges the graph dropped, and none for its self-loop slots, stay zero
        dropped = by_input and (g.kept != g.n_input_edges or bool(g.flags & nat.CSR_SELF_LOOPS))
        g_q, g_k, g_v, g_e = _timed(lambda: torch.ops.kgx.dot_attention_edge_backward(
            grad_out, q, k, v, ctx.saved_tensors[5], out, stats, g.rowptr, g.rows, items, split, g.col, n_slots,
            t.rowptr, t.rows, t_items, t_split, t.col, t.eid, t_slots, ctx.heads, ctx.channels, ctx.scale,
            g.eid if by_input else None, t.eid if by_input else _fwd_slot32(t), dropped, *drop,
        ))
        return g_q, g_k, g_v, g_e, None, None, None, None, None, None, None, None


def dot_attention(
    g: CSRGraph,
    q: torch.Tensor,
    k: torch.Tensor,
    v: torch.Tensor,
    heads: int,
    channels: int,
    *,
    scale: float | None = None,
    exact: bool = False,
    dropout: float = 0.0,
    seed: int = 0,
    edge: torch.Tensor | None = None,
    edge_order: str = "input",
) -> torch.Tensor:
    """Fused dot-product graph attention (TransformerConv's message passing):
    out[i,h,:] = sum_{e: j_e -> i} softmax_i(scale <q_i, k_j>_h)_e v[j_e,h,:];
    q [n_dst, heads*channels], k and v [n_src, heads*channels] (row views of a
    wider tensor are read in place).  scale=None: 1/sqrt(channels).
    Differentiable in q, k and v.  dropout > 0: attention dropout of the
    normalised weight per (edge, head), mask of (seed, input edge id, head).

    edge (PyG's edge_dim, already projected): one row per edge that is added to
    k_j in the score and to v_j in the message; differentiable too.
    edge_order="input": [g.n_input_edges, heads*channels] in input-edge order
    (self-loop slots the graph added carry no feature); "csr": [g.kept,
    heads*channels] in CSR slot order, which the kernel streams."""
    import math

    scale = 1.0 / math.sqrt(channels) if scale is None else float(scale)
    if edge is not None:
        if edge_order not in ("input", "csr"):
            raise ValueError(f"dot_attention: edge_order must be 'input' or 'csr', got {edge_order!r}")
        rows = g.n_input_edges if edge_order == "input" else g.kept
        if edge.dim() != 2 or edge.shape[0] != rows or edge.shape[1] != heads * channels:
            raise ValueError(f"dot_attention: edge in {edge_order} order must be [{rows}, {heads * channels}], got "
                             f"{tuple(edge.shape)}")
    if _needs_grad(q, k, v, edge):
        return _DotAttentionFn.apply(q, k, v, edge, g, heads, channels, scale, exact, float(dropout), int(seed),
                                     edge_order)
    return _dot_attention_raw(g, q, k, v, heads, channels, scale, exact, float(dropout), int(seed), edge, edge_order)


# ---------------------------------------------------------------------------
# Dense node transform: kgx_dense (bf16x3-split MFMA, f32-accurate)
# ---------------------------------------------------------------------------
def _aligned16(t: torch.Tensor) -> torch.Tensor:
    """Contiguous fp32 rows on a 16-byte boundary (what kgx_dense's dwordx4 loads need)."""
    t = _f32c(t)
    return t if t.data_ptr() % 16 == 0 else t.clone()


def dense_supported(x0: torch.Tensor, W0: torch.Tensor, W1: torch.Tensor | None = None) -> bool:
    """Shapes kgx_dense implements: K0 + K1 <= 256, N <= 256, K0, K1 multiples of 4."""
    if not (x0.is_cuda and x0.dim() == 2 and W0.dim() == 2):
        return False
    k0, n = W0.shape
    k1 = 0 if W1 is None else W1.shape[0]
    return (0 < n <= nat.DENSE_MAX_N and k0 + k1 <= nat.DENSE_MAX_K and k0 % 4 == 0 and k1 % 4 == 0
            and (W1 is None or W1.shape[1] == n))


@torch.library.custom_op("kgx::dense", mutates_args=())
def dense_op(
    x0: torch.Tensor,
    W0: torch.Tensor,
    x1: Optional[torch.Tensor],
    W1: Optional[torch.Tensor],
    bias: Optional[torch.Tensor],
    relu: bool,
) -> torch.Tensor:
    x0, W0, bias = _aligned16(x0), _f32c(W0), _f32c(bias)
    x1 = None if x1 is None else _aligned16(x1)
    W1 = None if W1 is None else _f32c(W1)
    dev = nat.require_device(x0, W0, x1, W1, bias)
    M, N = x0.shape[0], W0.shape[1]
    if x1 is not None and x1.shape[0] != M:
        raise ValueError(f"kgx.dense: x1 has {x1.shape[0]} rows, x0 has {M}")
    out = torch.empty((M, N), dtype=torch.float32, device=dev)
    nat.check(
        nat.lib().kgx_dense(
            M, nat.ptr(x0), x0.stride(0), x0.shape[1], nat.ptr(W0),
            nat.ptr(x1), x1.stride(0) if x1 is not None else 0, x1.shape[1] if x1 is not None else 0, nat.ptr(W1),
            N, nat.ptr(bias), nat.DENSE_RELU if relu else 0, nat.ptr(out), out.stride(0), nat.stream(dev),
        ),
        "kgx_dense",
    )
    return out


@dense_op.register_fake
def _dense_fake(x0, W0, x1, W1, bias, relu):
    return x0.new_empty((x0.shape[0], W0.shape[1]))


def _matmul_t(g: torch.Tensor, W: torch.Tensor) -> torch.Tensor:
    """g @ W^T for the backward: the library fp32 GEMM, so gradients keep the
    reference autograd's fp32 GEMM numerics (kgx_dense is f32-accurate too,
    but its re-associated sums moved GIN's d/dx past the 1e-5 gradient bar
    on the toy graph of tests/test_gpu_backward.py)."""
    return g @ W.t()


class _DenseFn(torch.autograd.Function):
    """y = relu?(bias + x0 W0 + x1 W1).  Backward: dz = dy * (y > 0) for ReLU;
    dx_t = dz W_t^T (kgx_dense again), dW_t = x_t^T dz (split-K), db = sum dz."""

    @staticmethod
    def forward(ctx, x0, W0, x1, W1, bias, relu):
        y = torch.ops.kgx.dense(x0, W0, x1, W1, bias, relu)
        ctx.relu = relu
        ctx.save_for_backward(x0, W0, x1, W1, y if relu else None)
        return y

    @staticmethod
    def backward(ctx, grad):
        x0, W0, x1, W1, y = ctx.saved_tensors
        dz = grad.contiguous()
        if ctx.relu:
            dz = dz * (y > 0)
        g = [None] * 6
        if ctx.needs_input_grad[0]:
            g[0] = _matmul_t(dz, W0)
        if ctx.needs_input_grad[1]:  # dW0 = x0^T dz (+ db = colsum(dz) in the same pass, kgx_gemm_tn)
            g[1], g[4] = gemm_tn(x0, dz, with_db=ctx.needs_input_grad[4])
        if x1 is not None and ctx.needs_input_grad[2]:
            g[2] = _matmul_t(dz, W1)
        if x1 is not None and ctx.needs_input_grad[3]:
            g[3], _ = gemm_tn(x1, dz)
        if ctx.needs_input_grad[4] and g[4] is None:
            g[4] = dz.sum(0)
        return tuple(g)


def dense(
    x0: torch.Tensor,
    W0: torch.Tensor,
    bias: torch.Tensor | None = None,
    *,
    x1: torch.Tensor | None = None,
    W1: torch.Tensor | None = None,
    relu: bool = False,
) -> torch.Tensor:
    """relu?(bias + x0 @ W0 (+ x1 @ W1)) -- keras Dense / SAGEConv's two linear
    maps in one kgx_dense launch (differentiable).  Shapes kgx_dense does not
    implement (K > 256, N > 256, K % 4 != 0) run as the library GEMM
    (hipBLASLt) on the same device."""
    if (x1 is None) != (W1 is None):
        raise ValueError("dense: x1 and W1 go together")
    if dense_supported(x0, W0, W1):
        if _needs_grad(x0, W0, x1, W1, bias):
            return _DenseFn.apply(x0, W0, x1, W1, bias, bool(relu))
        return torch.ops.kgx.dense(x0, W0, x1, W1, bias, bool(relu))
    y = torch.addmm(bias, x0, W0) if bias is not None else x0 @ W0
    if x1 is not None:
        y = torch.addmm(y, x1, W1)
    return torch.relu(y) if relu else y


# ---------------------------------------------------------------------------
# Attention readouts: fused segment softmax + weighted sum (kgx_softmax_pool)
# ---------------------------------------------------------------------------
def _softmax_pool_impl(x, rowptr, rows, items, split, idx, s, score_u, score_c, tanh, n_slots, save):
    if x.dtype != torch.float32:
        raise TypeError(f"kgx kernels compute in fp32; got {x.dtype}")
    s, score_c = _f32c(s), _f32c(score_c)
    score_u = None if score_u is None else _aligned16(score_u)  # a misaligned u would cost the float4 lanes
    dev = nat.require_device(x, rowptr, rows, items, split, idx, s, score_u, score_c)
    n_seg = rowptr.numel() - 1
    N, F = x.shape
    fused = score_u is not None
    out = torch.empty((n_seg, F), dtype=torch.float32, device=dev)
    stats = torch.empty((n_seg if save else 0, 2), dtype=torch.float32, device=dev)
    # nodes in no segment keep score 0 (they pool nowhere and get zero gradient)
    s_out = torch.zeros(N if fused else 0, dtype=torch.float32, device=dev)
    if n_seg == 0:
        return out, stats, s_out
    n_items, n_split = _sched_counts(items, split)
    partials = None
    if items is not None and n_split > 0:
        partials = torch.empty((n_slots, F + 2), dtype=torch.float32, device=dev)
    nat.check(
        nat.lib().kgx_softmax_pool(
            nat.ptr(rowptr), nat.ptr(rows), n_seg, nat.ptr(items), n_items, nat.ptr(split), n_split,
            nat.ptr(idx), nat.ptr(x), x.stride(0) if N > 1 else max(x.stride(0), F), F,
            nat.ptr(s), nat.ptr(score_u), nat.ptr(score_c), nat.POOL_SCORE_TANH if (fused and tanh) else 0,
            nat.ptr(s_out) if fused else None, nat.ptr(out), out.stride(0),
            nat.ptr(stats) if save else None, nat.ptr(partials), nat.stream(dev),
        ),
        "kgx_softmax_pool",
    )
    return out, stats, s_out


@torch.library.custom_op("kgx::softmax_pool_save", mutates_args=())
def softmax_pool_save(
    x: torch.Tensor,
    rowptr: torch.Tensor,
    rows: torch.Tensor,
    items: Optional[torch.Tensor],
    split: Optional[torch.Tensor],
    idx: Optional[torch.Tensor],
    s: Optional[torch.Tensor],
    score_u: Optional[torch.Tensor],
    score_c: Optional[torch.Tensor],
    tanh: bool,
    n_slots: int,
) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """kgx::softmax_pool that also returns the per-segment softmax statistics
    [n_seg, 2] and, for fused scores, the scores [N] (empty for given ones)."""
    return _softmax_pool_impl(x, rowptr, rows, items, split, idx, s, score_u, score_c, tanh, n_slots, True)


@softmax_pool_save.register_fake
def _softmax_pool_save_fake(x, rowptr, rows, items, split, idx, s, score_u, score_c, tanh, n_slots):
    n = rowptr.shape[0] - 1
    return (x.new_empty((n, x.shape[1])), x.new_empty((n, 2)),
            x.new_empty((x.shape[0] if score_u is not None else 0,)))


@torch.library.custom_op("kgx::softmax_pool", mutates_args=())
def softmax_pool_op(
    x: torch.Tensor,
    rowptr: torch.Tensor,
    rows: torch.Tensor,
    items: Optional[torch.Tensor],
    split: Optional[torch.Tensor],
    idx: Optional[torch.Tensor],
    s: Optional[torch.Tensor],
    score_u: Optional[torch.Tensor],
    score_c: Optional[torch.Tensor],
    tanh: bool,
    n_slots: int,
) -> torch.Tensor:
    return _softmax_pool_impl(x, rowptr, rows, items, split, idx, s, score_u, score_c, tanh, n_slots, False)[0]


@softmax_pool_op.register_fake
def _softmax_pool_fake(x, rowptr, rows, items, split, idx, s, score_u, score_c, tanh, n_slots):
    return x.new_empty((rowptr.shape[0] - 1, x.shape[1]))


@torch.library.custom_op("kgx::softmax_pool_backward", mutates_args=())
def softmax_pool_backward(
    x: torch.Tensor,
    seg: Optional[torch.Tensor],
    s: torch.Tensor,
    stats: torch.Tensor,
    out: torch.Tensor,
    grad_out: torch.Tensor,
) -> tuple[torch.Tensor, torch.Tensor]:
    """(grad_x [N, F], grad_s [N]) of kgx::softmax_pool, one pass over x."""
    s, stats, out, grad_out = _f32c(s), _f32c(stats), _f32c(out), _f32c(grad_out)
    dev = nat.require_device(x, seg, s, stats, out, grad_out)
    N, F = x.shape
    grad_x = torch.empty((N, F), dtype=torch.float32, device=dev)
    grad_s = torch.empty(N, dtype=torch.float32, device=dev)
    nat.check(
        nat.lib().kgx_softmax_pool_backward(
            N, out.shape[0], nat.ptr(seg), nat.ptr(x), x.stride(0) if N > 1 else max(x.stride(0), F), F,
            nat.ptr(s), nat.ptr(stats), nat.ptr(out), out.stride(0), nat.ptr(grad_out), grad_out.stride(0),
            nat.ptr(grad_x), grad_x.stride(0), nat.ptr(grad_s), nat.stream(dev),
        ),
        "kgx_softmax_pool_backward",
    )
    return grad_x, grad_s


@softmax_pool_backward.register_fake
def _softmax_pool_backward_fake(x, seg, s, stats, out, grad_out):
    return x.new_empty(x.shape), x.new_empty((x.shape[0],))


def softmax_pool_supported(x: torch.Tensor) -> bool:
    """Inputs kgx_softmax_pool takes: fp32 rows of 1..256 features with unit
    column stride and a row stride that covers them (any row alignment: rows
    that are not 16-byte aligned take the kernel's scalar lanes)."""
    return (x.dim() == 2 and x.dtype == torch.float32 and 0 < x.shape[1] <= nat.POOL_MAX_F and x.stride(1) == 1
            and (x.shape[0] <= 1 or x.stride(0) >= x.shape[1]))


def _pool_args(g: CSRGraph):
    items, _, split, _, n_slots = g.work(False)
    return g.rowptr, g.rows, items, split, g.col, n_slots


def _segment_sum_1d(g: CSRGraph, v: torch.Tensor) -> torch.Tensor:
    """[n_seg]: per-segment sum of a per-node vector, in a fixed order."""
    if g.col is None:
        return v.sum().reshape(1)
    return aggregate(g, v.unsqueeze(1).contiguous(), "sum", exact=True).reshape(-1)


class _SoftmaxPoolFn(torch.autograd.Function):
    """Autograd of the fused softmax pooling.  The forward keeps out, the
    per-segment (max, denominator) and the scores; kgx_softmax_pool_backward
    gives (grad_x, grad_s) in one pass over x.  For fused scores s = act(x u +
    c[g]) the chain is finished with torch ops: dz = grad_s * act'(s),
    grad_x += dz (x) u, grad_u = x^T dz, grad_c = segment sum of dz."""

    @staticmethod
    def forward(ctx, x, s, score_u, score_c, g, tanh):
        from . import graph as G

        ctx.g, ctx.tanh, ctx.fused = g, bool(tanh), score_u is not None
        a = _pool_args(g)
        out, stats, s_out = _timed(lambda: torch.ops.kgx.softmax_pool_save(
            x, *a[:5], s, score_u, score_c, bool(tanh), a[5]))
        ctx.seg = G.segment_of_node(g)
        ctx.save_for_backward(x, s_out if ctx.fused else s, score_u, stats, out)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        x, s, score_u, stats, out = ctx.saved_tensors
        grad_x, grad_s = torch.ops.kgx.softmax_pool_backward(x, ctx.seg, s, stats, out, grad_out.contiguous())
        if not ctx.fused:
            return grad_x, grad_s, None, None, None, None
        dz = grad_s * (1.0 - s * s) if ctx.tanh else grad_s
        grad_u = grad_c = None
        if ctx.needs_input_grad[0]:
            grad_x.addcmul_(dz.unsqueeze(1), score_u.unsqueeze(0))
        if ctx.needs_input_grad[2]:
            grad_u = (x * dz.unsqueeze(1)).sum(0)  # a fixed-order column sum (bit-reproducible)
        if ctx.needs_input_grad[3]:
            grad_c = _segment_sum_1d(ctx.g, dz)
        return grad_x, None, grad_u, grad_c, None, None


def _softmax_pool_composed(g: CSRGraph, x, s, score_u, score_c, tanh):
    """The same pooling from torch ops (differentiable by torch autograd), for
    inputs kgx_softmax_pool rejects: F > 256 or a strided last dimension."""
    from . import graph as G

    seg = G.segment_of_node(g)
    n_seg = g.n_dst
    if seg is None:
        if s is None:
            z = x @ score_u + score_c[0]
            s = torch.tanh(z) if tanh else z
        w = torch.softmax(s, dim=0)
        return (w.unsqueeze(1) * x).sum(0, keepdim=True)
    keep = (seg >= 0).nonzero().reshape(-1)
    sg = seg[keep].long()
    xk = x[keep]
    if s is None:
        z = xk @ score_u + score_c[sg]
        sk = torch.tanh(z) if tanh else z
    else:
        sk = s[keep]
    m = torch.full((n_seg,), float("-inf"), dtype=x.dtype, device=x.device)
    m = m.scatter_reduce(0, sg, sk.detach(), "amax", include_self=True)
    e = torch.exp(sk - m[sg])
    den = torch.zeros(n_seg, dtype=x.dtype, device=x.device).index_add(0, sg, e)
    w = e / den[sg]
    return torch.zeros((n_seg, x.shape[1]), dtype=x.dtype, device=x.device).index_add(0, sg, w.unsqueeze(1) * xk)


def softmax_pool(
    g: CSRGraph,
    x: torch.Tensor,
    s: torch.Tensor | None = None,
    *,
    score_u: torch.Tensor | None = None,
    score_c: torch.Tensor | None = None,
    tanh: bool = False,
) -> torch.Tensor:
    """out[r, :] = sum_{i in segment r} softmax_r(s)_i * x[i, :] -> [g.n_dst, F].

    g: a segment CSR (layers.pooling.segment_graph / build_csr(segment_only=True)
    over a batch vector, col = node per slot) or graph.single_segment_graph.
    Scores are either given (`s` [N]) or fused: s_i = act(x_i . score_u +
    score_c[r]) with act = tanh when `tanh` (Set2Set's attention Dense),
    computed in the pooling kernel from the row it has loaded.  Differentiable
    in x, s, score_u, score_c.  F > 256 or a strided last dimension run as the
    composed torch form on the same device."""
    if (s is None) == (score_u is None):
        raise ValueError("softmax_pool: exactly one of s and score_u")
    if score_u is not None and score_c is None:
        raise ValueError("softmax_pool: score_u needs score_c")
    if tanh and score_u is None:
        raise ValueError("softmax_pool: tanh applies to fused scores (score_u) only")
    if x.dim() != 2 or x.shape[0] != g.n_src:
        raise ValueError(f"softmax_pool: x must be [{g.n_src}, F], got {tuple(x.shape)}")
    nat.require_device(x, s, score_u, score_c)
    if not softmax_pool_supported(x):
        return _softmax_pool_composed(g, x, s, score_u, score_c, tanh)
    if s is not None:
        s = s.reshape(-1)
    if score_u is not None:
        score_u, score_c = score_u.reshape(-1), score_c.reshape(-1)
    if _needs_grad(x, s, score_u, score_c):
        return _SoftmaxPoolFn.apply(x, s, score_u, score_c, g, bool(tanh))
    a = _pool_args(g)
    return _timed(lambda: torch.ops.kgx.softmax_pool(x, *a[:5], s, score_u, score_c, bool(tanh), a[5]))


# ---------------------------------------------------------------------------
# Edge scores for link prediction (kgx_edge_dot): node rows -> edge values
# ---------------------------------------------------------------------------
def _row_table(t: torch.Tensor, what: str) -> torch.Tensor:
    """A [n, F] fp32 table the kernel can read in place: unit column stride and
    rows that do not overlap (row views with ld > F pass through uncopied)."""
    if t.dtype != torch.float32:
        raise TypeError(f"kgx kernels compute in fp32; got {t.dtype}")
    if t.dim() != 2:
        raise ValueError(f"edge_dot: {what} must be [n, F], got {tuple(t.shape)}")
    if (t.shape[1] > 1 and t.stride(1) != 1) or (t.shape[0] > 1 and t.stride(0) < t.shape[1]):
        return t.contiguous()
    return t


def _ld(t: torch.Tensor) -> int:
    return t.stride(0) if t.shape[0] > 1 else max(t.shape[1], 1)


@torch.library.custom_op("kgx::edge_dot", mutates_args=("bad",))
def edge_dot_op(
    xa: torch.Tensor,
    xb: torch.Tensor,
    a_idx: torch.Tensor,
    b_idx: torch.Tensor,
    perm: Optional[torch.Tensor],
    bad: torch.Tensor,
) -> torch.Tensor:
    """out[p, k] = xa[a_idx[p]] . xb[b_idx[p, k]] (row p stored at perm[p] when
    given); `bad` (int32 [1]) counts the indices outside their table."""
    xa, xb = _row_table(xa, "xa"), _row_table(xb, "xb")
    dev = nat.require_device(xa, xb, a_idx, b_idx, perm, bad)
    if a_idx.dtype != torch.int32 or b_idx.dtype != torch.int32 or b_idx.dim() != 2:
        raise TypeError("kgx::edge_dot expects int32 a_idx [P] and b_idx [P, K]")
    if xa.shape[1] != xb.shape[1]:
        raise ValueError(f"edge_dot: feature widths differ ({xa.shape[1]} vs {xb.shape[1]})")
    P, K = b_idx.shape
    if a_idx.numel() != P or (perm is not None and perm.numel() != P):
        raise ValueError("edge_dot: a_idx, b_idx and perm disagree on P")
    out = torch.empty((P, K), dtype=torch.float32, device=dev)
    nat.check(
        nat.lib().kgx_edge_dot(
            nat.ptr(xa), xa.shape[0], _ld(xa), nat.ptr(xb), xb.shape[0], _ld(xb), xa.shape[1],
            nat.ptr(a_idx.contiguous()), nat.ptr(b_idx.contiguous()), P, K,
            nat.ptr(perm.contiguous()) if perm is not None else None, nat.ptr(out), out.stride(0) if P else K,
            nat.ptr(bad), nat.stream(dev),
        ),
        "kgx_edge_dot",
    )
    return out


@edge_dot_op.register_fake
def _edge_dot_fake(xa, xb, a_idx, b_idx, perm, bad):
    return xa.new_empty((b_idx.shape[0], b_idx.shape[1]))


def _weighted_sum(g: CSRGraph, table: torch.Tensor, w: torch.Tensor) -> torch.Tensor:
    """out[i] = sum_{slot s of row i} w[s] * table[col[s]] (kgx::spmm, per-call weights)."""
    items, _, split, _, n_slots = g.work(False)
    return _timed(lambda: torch.ops.kgx.spmm(
        table, g.rowptr, g.rows, items, split, g.col, w, n_slots, nat.SUM, nat.EPI_NONE, None, None, 1.0,
        None, 0.0, 0, g.n_long if items is not None else _exact_short(g, nat.SUM),
    ))


def edge_dot_pair_graph(a_idx: torch.Tensor, b_idx: torch.Tensor, n_a: int, n_b: int) -> CSRGraph:
    """The pair graph of an edge_dot call, for its backward: one row per xa row,
    one edge (b_idx[p, k] -> a_idx[p]) per score, input edge id p * K + k.  A
    pair with an index outside its table (a NaN score) is left out -- its
    destination becomes -1, which kgx_csr_build drops -- so it passes no
    gradient and a negative source never wraps to another row."""
    from . import graph as G

    K = b_idx.shape[1]
    src = b_idx.reshape(-1)
    dst = a_idx.repeat_interleave(K)
    bad = (src < 0) | (src >= n_b) | (dst < 0) | (dst >= n_a)
    return G.build_csr(src.masked_fill(bad, 0).contiguous(), dst.masked_fill(bad, -1).contiguous(), n_b, n_a)


class _EdgeDotFn(torch.autograd.Function):
    """Backward by existing deterministic kernels only: with D = d loss / d out,
        d xa[i] = sum_{pairs with a = i} D * xb[b]      (weighted kgx::spmm over the pair graph)
        d xb[j] = sum_{pairs with b = j} D * xa[a]      (the same over its graph.transpose)
    w = D in each CSR's slot order (eid: the pair's position in `out`).  A table
    passed as both xa and xb receives both, summed by autograd."""

    @staticmethod
    def forward(ctx, xa, xb, a_idx, b_idx, perm, bad, graph_of):
        ctx.graph_of = graph_of
        ctx.save_for_backward(xa, xb)
        return torch.ops.kgx.edge_dot(xa, xb, a_idx, b_idx, perm, bad)

    @staticmethod
    def backward(ctx, grad_out):
        from . import graph as G

        xa, xb = ctx.saved_tensors
        g = ctx.graph_of()
        d = grad_out.contiguous().reshape(-1)
        g_xa = g_xb = None
        if ctx.needs_input_grad[0]:
            g_xa = _weighted_sum(g, xb, d.index_select(0, g.eid.long()))
        if ctx.needs_input_grad[1]:
            t = G.transpose(g)
            g_xb = _weighted_sum(t, xa, d.index_select(0, t.eid.long()))
        return g_xa, g_xb, None, None, None, None, None


def _check_bad(bad: torch.Tensor, what: str) -> None:
    n = int(bad.item())
    if n:
        raise IndexError(f"{what}: {n} index(es) outside their table (their scores are NaN)")


def edge_dot(xa: torch.Tensor, xb: torch.Tensor, a_idx: torch.Tensor, b_idx: torch.Tensor, *, check: bool = True,
             cache: dict | None = None) -> torch.Tensor:
    """out[p, k] = xa[a_idx[p]] . xb[b_idx[p, k]] -> [P, K] ([P] for a 1-d b_idx).

    xa [n_a, F] and xb [n_b, F] are fp32 tables (row views are read in place)
    and may be the same tensor; a_idx [P] and b_idx [P, K] are node ids.  K = 1 +
    Q scores a positive and its Q negatives from one load of the xa row.  A
    score is a function of its two rows and F alone (bit-identical at every p,
    k, K and P).  An index outside its table gives a NaN score; check=True reads
    the kernel's counter back (one synchronise) and raises IndexError, check=
    False never synchronises.  Differentiable in xa and xb through weighted
    kgx::spmm sums over the pair graph and its transpose, both deterministic;
    the pair graph is built only when a gradient is asked for -- a build_csr
    and a graph.transpose per new index arrays, each with a host read-back, so
    a backward synchronises even with check=False -- and kept in `cache` (a
    dict, e.g. EdgeBatch.extras) when one is given, with the index arrays and
    table heights it was built for: other arrays or heights rebuild it.  A
    pair with an index outside its table is not in the pair graph and passes
    no gradient."""
    dev = nat.require_device(xa, xb, a_idx, b_idx)
    one_d = b_idx.dim() == 1
    a_idx = a_idx.to(torch.int32).reshape(-1).contiguous()
    b2 = (b_idx.unsqueeze(1) if one_d else b_idx).to(torch.int32).contiguous()
    if b2.dim() != 2 or b2.shape[0] != a_idx.numel() or b2.shape[1] < 1:
        raise ValueError(f"edge_dot: b_idx {tuple(b_idx.shape)} does not match a_idx {tuple(a_idx.shape)}")
    bad = torch.zeros(1, dtype=torch.int32, device=dev)
    if _needs_grad(xa, xb):
        n_a, n_b = xa.shape[0], xb.shape[0]

        # the cached graph belongs to these index arrays (kept alive beside it, so their
        # addresses cannot be handed out again) at these versions and table heights
        key = (n_a, n_b, a_idx.data_ptr(), tuple(a_idx.shape), a_idx._version,
               b2.data_ptr(), tuple(b2.shape), b2._version)

        def graph_of():
            hit = cache.get("pair_graph_key") if cache is not None else None
            if hit is not None and hit[0] == key and cache.get("pair_graph") is not None:
                return cache["pair_graph"]
            g = edge_dot_pair_graph(a_idx, b2, n_a, n_b)
            if cache is not None:
                cache["pair_graph"] = g
                cache["pair_graph_key"] = (key, a_idx, b2)
            return g

        out = _EdgeDotFn.apply(xa, xb, a_idx, b2, None, bad, graph_of)
    else:
        out = _timed(lambda: torch.ops.kgx.edge_dot(xa, xb, a_idx, b2, None, bad))
    if check:
        _check_bad(bad, "edge_dot")
    return out.reshape(-1) if one_d else out


def edge_dot_graph(g: CSRGraph, x_dst: torch.Tensor, x_src: torch.Tensor, *, check: bool = True) -> torch.Tensor:
    """Scores of the CSR's own edges, in input-edge order: out[e] = x_dst[dst_e] .
    x_src[src_e] -> [E].  The kernel walks the edges in CSR order (a_idx =
    row_of_slot(g), b_idx = g.col) and stores through perm = g.eid; the
    backward reuses g and its cached transpose.  A graph built with self loops
    is rejected (its extra slots are not input edges)."""
    from . import graph as G

    if g.flags & nat.CSR_SELF_LOOPS:
        raise ValueError("edge_dot_graph: the graph was built with self loops; score a graph of the input edges")
    if g.kept != g.n_input_edges:
        raise ValueError(f"edge_dot_graph: the CSR holds {g.kept} of {g.n_input_edges} input edges")
    if x_dst.dim() != 2 or x_src.dim() != 2 or x_dst.shape[0] != g.n_dst or x_src.shape[0] != g.n_src:
        raise ValueError(f"edge_dot_graph: expected x_dst [{g.n_dst}, F] and x_src [{g.n_src}, F], got "
                         f"{tuple(x_dst.shape)} and {tuple(x_src.shape)}")
    dev = nat.require_device(x_dst, x_src, g.rowptr)
    bad = torch.zeros(1, dtype=torch.int32, device=dev)
    args = (x_dst, x_src, G.row_of_slot(g), g.col.reshape(-1, 1), g.eid, bad)
    if _needs_grad(x_dst, x_src):
        out = _EdgeDotFn.apply(*args, lambda: g)
    else:
        out = _timed(lambda: torch.ops.kgx.edge_dot(*args))
    if check:
        _check_bad(bad, "edge_dot_graph")
    return out.reshape(-1)
