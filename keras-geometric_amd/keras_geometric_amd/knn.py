"""k-nearest-neighbour graphs from coordinates or features, on the device (kgx_knn).

    nbr = knn(x, y, k, batch_x, batch_y)            # PyG's bipartite knn: rows of x for every row of y
    edge_index = knn_graph(x, k, batch)             # PyG's knn_graph: row 0 the neighbour, row 1 the centre
    g = knn_csr(x, k, batch)                        # the same graph as a CSRGraph with its transpose

The kernel (csrc/knn.hip, include/kgx.h) never writes a distance table: a block of 64 queries walks
the points of its queries' segments tile by tile and keeps every query's k best in LDS.  D <= 8 is
evaluated directly in fp32 (bit for bit restatable, tests/knn_ref.py); 8 < D <= 256 takes the cross
term on bf16 MFMA with both operands split three ways.  Rows are ascending in (d2, index); a query
with fewer than k candidates is padded with -1 (and +inf); a candidate whose d2 is NaN or +inf is
never selected.  The indices are not differentiable: the op has no autograd formula.

Outside knn_supported (D > 256, k > 64) and for CPU tensors the functions take a composed form:
per segment and chunk of queries, the squared distances in the direct path's fp32 order and a stable
sort.  A batch vector is read back to the host once, whole (twice given, as by knn_graph: still once).
"""

from __future__ import annotations

import ctypes

import numpy as np
import torch

from . import _native as nat
from .graph import CSRGraph
from .sampling import _block_graph, block_csr

_CHUNK = 4096  # query rows per cdist call of the composed form


def knn_supported(D: int, k: int) -> bool:
    """Shapes knn.hip implements: D in [1, 256], k in [1, 64]."""
    return 1 <= D <= 256 and 1 <= k <= 64


def _check_batch(batch, n: int, what: str) -> torch.Tensor | None:
    if batch is None:
        return None
    if not isinstance(batch, torch.Tensor):
        batch = torch.as_tensor(np.asarray(batch))
    if batch.dim() != 1 or batch.numel() != n:
        raise ValueError(f"knn: {what} must be a 1-d vector of {n} segment ids, got shape {tuple(batch.shape)}")
    if batch.dtype.is_floating_point or batch.dtype.is_complex or batch.dtype == torch.bool:
        raise TypeError(f"knn: {what} must hold integer segment ids, got {batch.dtype}")
    return batch


def _offsets(batches: list, sizes: list) -> list:
    """Host int32 offsets [S + 1] of sorted batch vectors (None: one segment).  Every distinct batch
    vector is read back once, whole, whatever device it is on, and checked and counted on the host:
    one host synchronisation per vector, and one offset array for the vectors that are one object."""
    host = {id(b): b.detach().cpu().numpy() for b in batches if b is not None}
    S = 1
    for h in host.values():
        if h.size:
            if (h[1:] < h[:-1]).any():
                raise ValueError("knn: batch must be sorted ascending")
            if h[0] < 0:
                raise ValueError("knn: batch holds a negative segment id")
            S = max(S, int(h[-1]) + 1)
    ids = np.arange(S + 1)
    offs = {i: np.searchsorted(h, ids).astype(np.int32) for i, h in host.items()}  # rows with an id below s
    return [np.array([0] + [n] * S, dtype=np.int32) if b is None else offs[id(b)] for b, n in zip(batches, sizes)]


@torch.library.custom_op("kgx::knn", mutates_args=())
def knn_op(x: torch.Tensor, y: torch.Tensor, seg_x: torch.Tensor, seg_y: torch.Tensor, k: int, exclude_self: bool,
           return_dist: bool) -> tuple[torch.Tensor, torch.Tensor]:
    """(nbr int32 [Q, k], dist2 fp32 [Q, k] or [0, k]) of kgx_knn; seg_x / seg_y: CPU int32 offsets [S + 1]."""
    dev = nat.require_device(x, y)
    if x.stride(1) != 1:
        x = x.contiguous()
    if y.stride(1) != 1:
        y = y.contiguous()
    P, D = x.shape
    Q = y.shape[0]
    S = seg_x.numel() - 1
    nbr = torch.empty((Q, k), dtype=torch.int32, device=dev)
    dist2 = torch.empty((Q if return_dist else 0, k), dtype=torch.float32, device=dev)
    seg_x, seg_y = seg_x.contiguous(), seg_y.contiguous()
    L = nat.lib()
    n = ctypes.c_size_t(0)
    nat.check(L.kgx_knn_workspace_bytes(P, Q, D, S, ctypes.byref(n)), "kgx_knn_workspace_bytes")
    ws = torch.empty(max(n.value, 16), dtype=torch.uint8, device=dev)
    a = nat.KnnArgs(
        struct_size=ctypes.sizeof(nat.KnnArgs), x=nat.addr(x), ld_x=x.stride(0) if P > 1 else D, P=P,
        y=nat.addr(y), ld_y=y.stride(0) if Q > 1 else D, Q=Q, D=D, k=k,
        seg_x=seg_x.data_ptr(), seg_y=seg_y.data_ptr(), S=S, exclude_self=int(exclude_self),
        nbr=nat.addr(nbr), ld_nbr=k, dist2=nat.addr(dist2) if return_dist else None, ld_dist2=k,
        workspace=nat.addr(ws), workspace_bytes=ws.numel(),
    )
    nat.check(L.kgx_knn(ctypes.byref(a), nat.stream(dev)), "kgx_knn")
    return nbr, dist2


@knn_op.register_fake
def _knn_fake(x, y, seg_x, seg_y, k, exclude_self, return_dist):
    Q = y.shape[0]
    return x.new_empty((Q, k), dtype=torch.int32), x.new_empty((Q if return_dist else 0, k))


def _knn_composed(x, y, seg_x, seg_y, k: int, exclude_self: bool):
    """The same table from torch ops: per segment and chunk of queries, the squared differences summed
    column by column in the direct path's order (so dist2 is that path's fp32 value at every D) and a
    stable sort (ties to the lower index).  Writes a [chunk, segment] distance block at a time."""
    Q = y.shape[0]
    nbr = torch.full((Q, k), -1, dtype=torch.int32, device=y.device)
    dist2 = torch.full((Q, k), float("inf"), dtype=torch.float32, device=y.device)
    for s in range(len(seg_x) - 1):
        lo, hi = int(seg_x[s]), int(seg_x[s + 1])
        if hi == lo:
            continue
        xs = x[lo:hi]
        for q0 in range(int(seg_y[s]), int(seg_y[s + 1]), _CHUNK):
            q1 = min(q0 + _CHUNK, int(seg_y[s + 1]))
            d = torch.zeros((q1 - q0, hi - lo), dtype=torch.float32, device=y.device)
            for j in range(x.shape[1]):  # acc + t * t for d ascending, as the direct path rounds it
                t = y[q0:q1, j, None] - xs[None, :, j]
                d += t.mul_(t)
            if exclude_self:
                rows = torch.arange(q0, q1, device=y.device)
                own = (rows >= lo) & (rows < hi)
                d[torch.nonzero(own).squeeze(1), rows[own] - lo] = float("inf")
            d = torch.where(d < float("inf"), d, float("inf"))  # NaN and +inf: never selected
            val, idx = torch.sort(d, dim=1, stable=True)
            kk = min(k, hi - lo)
            val, idx = val[:, :kk], idx[:, :kk] + lo
            dist2[q0:q1, :kk] = val
            nbr[q0:q1, :kk] = torch.where(val < float("inf"), idx, -1).to(torch.int32)
    return nbr, dist2


def _knn_table(x, y, k, batch_x, batch_y, exclude_self: bool, return_dist: bool):
    for t, what in ((x, "x"), (y, "y")):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.float32:
            raise TypeError(f"knn: {what} must be an fp32 tensor, got {getattr(t, 'dtype', type(t))}")
        if t.dim() != 2:
            raise ValueError(f"knn: {what} must be [rows, D], got shape {tuple(t.shape)}")
    if x.shape[1] != y.shape[1] or x.shape[1] < 1:
        raise ValueError(f"knn: x has {x.shape[1]} columns and y {y.shape[1]} (equal and >= 1)")
    k = int(k)
    if k < 1:
        raise ValueError(f"knn: k must be >= 1, got {k}")
    shared = batch_y is batch_x and y.shape[0] == x.shape[0]  # knn_graph: one vector, checked and read back once
    batch_x = _check_batch(batch_x, x.shape[0], "batch_x")
    batch_y = batch_x if shared else _check_batch(batch_y, y.shape[0], "batch_y")
    seg_x, seg_y = _offsets([batch_x, batch_y], [x.shape[0], y.shape[0]])
    if x.is_cuda and knn_supported(x.shape[1], k):
        nbr, dist2 = torch.ops.kgx.knn(x.detach(), y.detach(), torch.from_numpy(seg_x), torch.from_numpy(seg_y), k,
                                       exclude_self, return_dist)
    else:
        with torch.no_grad():
            nbr, dist2 = _knn_composed(x, y, seg_x, seg_y, k, exclude_self)
    return (nbr, dist2) if return_dist else nbr


def knn(x: torch.Tensor, y: torch.Tensor, k: int, batch_x=None, batch_y=None, *, return_dist: bool = False):
    """For every row of y [Q, D] the k nearest rows of x [P, D] of the same segment: nbr int32 [Q, k]
    (and their squared distances with return_dist).  batch_x / batch_y: sorted segment ids, None = one
    segment.  ValueError for an unsorted batch, mismatched D or k < 1; TypeError for a non-fp32 table."""
    return _knn_table(x, y, k, batch_x, batch_y, False, return_dist)


def knn_graph(x: torch.Tensor, k: int, batch=None, loop: bool = False) -> torch.Tensor:
    """edge_index int32 [2, E] of the k-NN graph of x in PyG's convention: row 0 the neighbour (source),
    row 1 the centre (target); sorted by target, then by (d2, index).  loop=False leaves a point out of
    its own list (by index: a duplicate of it stays a neighbour)."""
    nbr = _knn_table(x, x, k, batch, batch, not loop, False)
    keep = nbr >= 0
    centre = torch.arange(nbr.shape[0], dtype=torch.int32, device=nbr.device)[:, None].expand_as(nbr)
    return torch.stack([nbr[keep], centre[keep]])


def knn_csr(x: torch.Tensor, k: int, batch=None, loop: bool = False, n_features: int = 128) -> CSRGraph:
    """knn_graph(x, k, batch, loop) as a CSRGraph over destination rows with its transposed graph in
    extras["T"].  The neighbour table is a destination CSR already, so nothing is sorted: the row
    pointers and the transpose come from kgx_block_csr.  Edge ids are the edges' positions in
    knn_graph's edge_index.  n_features sizes the schedules' hub chunks, as in the layers' graph cache."""
    src, dst = knn_graph(x, k, batch, loop)
    n = x.shape[0]
    (rowptr, deg), (t_rowptr, t_deg, t_col, t_eid), (max_in, max_out) = block_csr(src, dst, n, n)
    pos = torch.arange(src.numel(), dtype=torch.int32, device=src.device)
    g = _block_graph(n, n, src, pos, rowptr, deg, max_in, n_features)
    t = _block_graph(n, n, t_col, t_eid, t_rowptr, t_deg, max_out, n_features)
    t.extras["fwd_slot"] = t_eid.long()  # as graph.transpose leaves it
    g.extras["T"] = t
    return g
