"""Sliced schedule of the fused aggregate -> transform launch (kgx_slice_build).

The fused GCN forward gathers most of its source rows from a few hot rows,
and every XCD's L2 holds its own copy of them.  A sliced schedule regroups
the edges of the rows of degree >= T (the split hub rows among them) by
SOURCE CLASS, a hash of the source id into [0, C), and gives the main kernel
C item lists, block b on list b % C -- with round-robin dispatch of blocks
over XCDs, one class per XCD (an affinity label: results never depend on
it).  Every sliced row becomes chunks that write partials; the fix-up kernel
combines them in slot order (class, then chunk) and applies W.

Built lazily, natively, on the second fused forward over the same graph, and
kept in g.extras beside g.items / g.split, which every other user of the
schedule keeps reading.  The CSR itself is untouched.
"""

from __future__ import annotations

import ctypes
import os
from dataclasses import dataclass
from typing import Optional

import torch

from . import _native as nat

DEFAULT_T = 256
DEFAULT_C = 8
# share of the short-row items (degree 3..7) a CU-split sliced launch runs on the
# head's CUs (behind the main kernel, by the short-row kernel) instead of the
# tail's: slicing shortens the head leg (profiles/r07)
DEFAULT_HEAD_SHARE = 0.0
# graphs below this many edges never slice by default (the fitted CU-split rule's size)
MIN_EDGES = 50_000_000
_EXTRAS_KEY = "fused_slice"
_USES_KEY = "fused_slice_uses"


@dataclass
class SlicedSchedule:
    T: int
    C: int
    split_len: int
    n_rows: int          # sliced rows: rows[0, n_rows) of the schedule order
    n_edges: int         # their edges
    n_items_s: int       # their items: items[0, n_items_s) of g.items
    n_long: int          # the long-item boundary the lists were built for
    col: torch.Tensor    # int32 [n_edges]   sources, row by row, grouped by class
    w: Optional[torch.Tensor]  # fp32 [n_edges] or None
    items: torch.Tensor  # int32 [n_items, 4]  the C lists back to back
    lists: torch.Tensor  # int32 [C, 4]  {first item, items, chunk items, 0}
    fix: torch.Tensor    # int32 [n_rows, 4]  {row, first slot, slots, degree}
    n_slots: int
    max_list: int        # items of the longest list
    build_ms: float
    head_short_end: int = -1  # short-row items [n_long, head_short_end) run on the head's CUs
    w_src: object = None  # the graph's weight tensor the copies were taken from

    @property
    def tiles(self) -> int:
        return (self.max_list + 15) // 16

    @property
    def device_bytes(self) -> int:
        return sum(t.numel() * t.element_size() for t in (self.col, self.w, self.items, self.lists, self.fix)
                   if t is not None)


def slice_class(col: int, C: int) -> int:
    """Source class of a source id (kgx_slice_class restated: top bits of a multiplicative hash)."""
    return (((int(col) * 0x9E3779B1) & 0xFFFFFFFF) * C) >> 32


def env_mode() -> Optional[bool]:
    """KGX_FUSED_SLICE: None when unset (the default rule), else on / off."""
    v = os.environ.get("KGX_FUSED_SLICE")
    if v is None or v.strip() == "":
        return None
    return v.strip() not in ("0", "false", "False")


def env_params() -> tuple[int, int, float]:
    """(T, C, head share) with the KGX_FUSED_SLICE_T / _C / _HEAD overrides of the sweep."""
    T = int(os.environ.get("KGX_FUSED_SLICE_T", DEFAULT_T))
    C = int(os.environ.get("KGX_FUSED_SLICE_C", DEFAULT_C))
    h = float(os.environ.get("KGX_FUSED_SLICE_HEAD", DEFAULT_HEAD_SHARE))
    return T, C, min(max(h, 0.0), 1.0)


def slice_wanted(*, mode: Optional[bool], default_on: bool, have_items: bool, two_tables: bool, reduce: int,
                 f_in: int, f_out: int, n_edges: int, T: int, C: int) -> bool:
    """Whether a fused launch asks for the sliced schedule: a pure function of
    the launch's shape and the KGX_FUSED_SLICE setting (mode: None = the
    default rule, which slices large graphs only when default_on).  Sums over
    one feature table at F_in 128, F_out % 16 == 0, through the schedule."""
    if mode is False or not have_items or two_tables:
        return False
    if reduce != nat.SUM or f_in != 128 or f_out % 16 != 0 or f_out <= 0 or f_out > 128:
        return False
    if C not in (4, 8) or T < 1:
        return False
    if mode is None:
        return default_on and n_edges >= MIN_EDGES
    return True


# The default rule's switch: on only where the sliced launch measured a clear
# gain at the north-star size (DESIGN.md §4 "Source-class slicing").
DEFAULT_ON = True


def effective_threshold(T: int, graph_split_len: int) -> int:
    """Rows of degree >= this are sliced: T, and never above the hub split's length
    (today's hub rows are always sliced)."""
    return min(T, graph_split_len) if graph_split_len > 0 else T


def build(g, T: int = DEFAULT_T, C: int = DEFAULT_C, split_len: Optional[int] = None) -> Optional[SlicedSchedule]:
    """The sliced schedule of g for (T, C), chunks of at most split_len edges
    (default: the graph's hub-split length), over the long items [0, g.n_long).
    None when no row reaches the threshold."""
    from .graph import default_split_len

    if g.items is None or g.n_items == 0 or g.rows is None:
        return None
    dev = g.device
    L = nat.lib()
    if split_len is None:
        split_len = g.split_len if g.split_len > 0 else default_split_len(g.kept)
    n_items = g.n_items
    n_long = g.n_long if 0 <= g.n_long <= n_items else n_items
    Te = effective_threshold(T, g.split_len)
    t0 = torch.cuda.Event(enable_timing=True)
    t1 = torch.cuda.Event(enable_timing=True)
    t0.record()
    ws16 = torch.empty(32, dtype=torch.uint8, device=dev)
    info = (ctypes.c_int64 * 4)()
    items = g.items if g.items.is_contiguous() else g.items.contiguous()
    nat.check(L.kgx_slice_count(nat.ptr(g.rowptr), g.n_dst, nat.ptr(items), n_long, Te, nat.ptr(ws16), info,
                                nat.stream(dev)), "kgx_slice_count")
    n_s, n_e, n_is = int(info[0]), int(info[1]), int(info[2])
    if n_s == 0 or n_e == 0:
        return None
    cap = n_e // split_len + n_s * C + (n_long - n_is)
    w = g.w
    col_s = torch.empty(n_e, dtype=torch.int32, device=dev)
    w_s = torch.empty(n_e, dtype=torch.float32, device=dev) if w is not None else None
    items_s = torch.empty((cap, 4), dtype=torch.int32, device=dev)
    lists = torch.empty((C, 4), dtype=torch.int32, device=dev)
    fix = torch.empty((n_s, 4), dtype=torch.int32, device=dev)
    nbytes = ctypes.c_size_t(0)
    nat.check(L.kgx_slice_workspace_bytes(n_s, n_e, C, ctypes.byref(nbytes)), "kgx_slice_workspace_bytes")
    ws = torch.empty(max(nbytes.value, 1), dtype=torch.uint8, device=dev)
    nat.check(L.kgx_slice_build(nat.ptr(g.rowptr), nat.ptr(g.col), nat.ptr(w), nat.ptr(g.rows), n_s, n_e,
                                nat.ptr(items), n_is, n_long, split_len, C, nat.ptr(col_s), nat.ptr(w_s),
                                nat.ptr(items_s), cap, nat.ptr(lists), nat.ptr(fix), nat.ptr(ws), nbytes.value,
                                info, nat.stream(dev)), "kgx_slice_build")
    t1.record()
    t1.synchronize()
    n_all, n_slots, max_list = int(info[0]), int(info[1]), int(info[2])
    return SlicedSchedule(T=T, C=C, split_len=split_len, n_rows=n_s, n_edges=n_e, n_items_s=n_is, n_long=n_long,
                          col=col_s, w=w_s, items=items_s[:n_all], lists=lists, fix=fix, n_slots=n_slots,
                          max_list=max_list, build_ms=t0.elapsed_time(t1), w_src=w)


def head_short_end(g, share: float) -> int:
    """End of the short-row items (degree 3..7) a CU-split sliced launch runs on
    the head's CUs: `share` of them, from g.n_long on, in whole 32-row tiles."""
    n_long = g.n_long if 0 <= g.n_long <= g.n_items else g.n_items
    if share <= 0.0:
        return n_long
    from . import tiny

    n_se = tiny.tiny_pack(g)[2]
    n_se = n_se if n_long <= n_se <= g.n_items else g.n_items
    return n_long + (int((n_se - n_long) * share) // 32) * 32


def sliced_schedule(g, T: int, C: int, share: float = 0.0, force: bool = False) -> Optional[SlicedSchedule]:
    """g's cached sliced schedule for (T, C, share), built on the SECOND request
    (force: now) -- a one-shot forward over a graph pays nothing.  Never built
    while the stream is being captured (the build syncs).  A weight tensor
    assigned after the build makes the copies stale: rebuilt."""
    key = (T, C, round(share, 6))
    hit = g.extras.get(_EXTRAS_KEY)
    if hit is not None and hit[0] == key and (hit[1] is None or hit[1].w_src is g.w):
        return hit[1]
    uses = g.extras.get(_USES_KEY, 0) + 1
    g.extras[_USES_KEY] = uses
    if not force and uses < 2:
        return None
    if torch.cuda.is_current_stream_capturing():
        return None
    s = build(g, T, C)
    if s is not None:
        s.head_short_end = head_short_end(g, share)
    g.extras[_EXTRAS_KEY] = (key, s)
    return s
