"""float64 restatement of the fused training step for the GPU tests (test
infrastructure, imported by tests only).

    y = b + P W,  P = PRE(REDUCE_{e in CSR row i} x[col_e] * w_e)
    dW = P^T dOut,  db = colsum(dOut),  dx = d/dx <y, dOut>

`grads` computes all five in float64 with torch autograd straight from the
graph's CSR arrays (rowptr / col / w: one index_add_ / scatter_reduce_ per
reduction, no transposed graph, nothing from keras_geometric_amd.ops), and
once more on |x|, |W|, |b|, |dOut|: the value of the same computation over
|terms| bounds the error of any re-associated fp32 evaluation of it, which is
the scale every tolerance of tests/test_gpu_train_step.py is relative to
(1e-5 * max(1, scale), as fused_ref.check).

`class_graph` is the graph those tests run on: a numpy recipe that puts every
schedule class of the fused kernels (hub rows split into chunks, main rows,
the degree 3..7 short rows, the degree <= 2 records) into the graph AND its
transpose, and is not symmetric, so a missing or wrong transposition shows.
"""

from __future__ import annotations

from collections import namedtuple
from types import SimpleNamespace

import numpy as np
import torch

import fused_ref

Step = namedtuple("Step", "y P dx dW db")

HUBS = (1061, 517)  # 4 chunks of 256 + 37, 2 chunks + 5
N_MAIN, N_SHORT, N_TWO, N_ONE = 1400, 1400, 4400, 4400
CLASS_N = 12288


def class_graph(seed: int, N: int = CLASS_N):
    """(src, dst) int32 [E]: in-degrees by node id = the class multiset (hubs,
    8..64, 3..7, twos, ones, zeros), out-degrees the same multiset under a
    random permutation of the nodes, sources shuffled over the edges.
    Duplicate edges and the odd self edge stay."""
    rng = np.random.default_rng(seed)
    main = rng.integers(8, 65, N_MAIN)
    short = rng.integers(3, 8, N_SHORT)
    d_in = np.concatenate([np.array(HUBS), main, short, np.full(N_TWO, 2), np.full(N_ONE, 1)]).astype(np.int64)
    if d_in.size > N:
        raise ValueError(f"class_graph: N = {N} holds fewer nodes than the {d_in.size} with edges")
    d_in = np.concatenate([d_in, np.zeros(N - d_in.size, np.int64)])
    d_out = d_in[rng.permutation(N)]
    dst = np.repeat(np.arange(N), d_in)
    src = np.repeat(np.arange(N), d_out)
    rng.shuffle(src)
    return src.astype(np.int32), dst.astype(np.int32)


def class_counts(deg) -> dict:
    """Rows per schedule class of a degree vector (default chunk length 256)."""
    deg = np.asarray(deg)
    return {"hub": int((deg > 256).sum()), "main": int(((deg >= 8) & (deg <= 256)).sum()),
            "short": int(((deg >= 3) & (deg <= 7)).sum()), "two": int((deg == 2).sum()),
            "one": int((deg == 1).sum()), "zero": int((deg == 0).sum())}


def host_graph(src, dst, N: int, self_loops: bool, gcn_norm: bool):
    """The CSR the device build gives (rows by destination, input-edge order
    within a row, loops last; w = the reference's GCN edge norm), from the
    oracle on the host: an object with the fields `grads` reads."""
    from oracle import reference as R

    rowptr, col, eid, _ = R.csr_by_destination(np.asarray(src), np.asarray(dst), N, N, self_loops=self_loops)
    g = SimpleNamespace(rowptr=torch.from_numpy(rowptr), col=torch.from_numpy(col), n_dst=N, w=None, items=None)
    if gcn_norm:
        ei = torch.from_numpy(np.stack([src, dst]))
        if self_loops:
            ei = R.add_self_loops(ei, N)
        g.w = R.compute_gcn_normalization(ei, N)[torch.from_numpy(eid).long()].float().contiguous()
    return g


def forward64(g, x, W, b, red: str, weighted: bool, pre_gin: bool, gin_scale: float, select=None):
    """(y, P) in float64, differentiable in x, W, b (float64 leaves).  max / min
    select each row's extreme among the fp32 products of `select` (the fp32 x;
    what the kernels compare) and share the value evenly among equal winners
    (scatter_reduce amax's gradient; duplicate edges tie with themselves)."""
    n = g.n_dst
    rowptr, col = g.rowptr.long(), g.col.long()
    deg = rowptr[1:] - rowptr[:-1]
    seg = torch.repeat_interleave(torch.arange(n, device=x.device), deg, output_size=col.numel())
    w = g.w if weighted else None
    m = x[col]
    if w is not None:
        m = m * w.double()[:, None]
    F = x.shape[1]
    if red in ("sum", "mean"):
        a = torch.zeros((n, F), dtype=torch.float64, device=x.device).index_add(0, seg, m)
        if red == "mean":
            a = a / deg.to(torch.float32).clamp_min(1e-8).double()[:, None]
    else:
        m32 = select[col]
        if w is not None:
            m32 = m32 * w[:, None]
        init = float("-inf") if red == "max" else float("inf")
        ext = torch.full((n, F), init, dtype=torch.float32, device=x.device)
        ext.scatter_reduce_(0, seg[:, None].expand(-1, F), m32, "amax" if red == "max" else "amin", include_self=True)
        win = (m32 == ext[seg]) & ~torch.isinf(ext[seg])  # the isinf guard: such rows give 0 and pass no gradient
        cnt = torch.zeros((n, F), dtype=torch.float64, device=x.device).index_add_(0, seg, win.double())
        share = win.double() / cnt.clamp_min(1.0)[seg]
        a = torch.zeros((n, F), dtype=torch.float64, device=x.device).index_add(0, seg, m * share)
    P = gin_scale * x[:n] + a if pre_gin else a
    y = P @ W
    if b is not None:
        y = y + b
    return y, P


def _step(g, x, W, b, dOut, red, weighted, pre_gin, gin_scale, select):
    x64, W64 = x.double().requires_grad_(True), W.double().requires_grad_(True)
    b64 = b.double().requires_grad_(True) if b is not None else None
    y, P = forward64(g, x64, W64, b64, red, weighted, pre_gin, gin_scale, select)
    y.backward(dOut.double())
    return Step(y.detach(), P.detach(), x64.grad, W64.grad, b64.grad if b64 is not None else None)


def grads(g, x, W, b, dOut, red: str, weighted: bool, pre_gin: bool = False, gin_scale: float = 1.0):
    """(ref, mag): two Steps (y, P, dx, dW, db) of float64 tensors -- the training
    step of out = b + PRE(REDUCE(x)) W under the upstream gradient dOut, and the
    same step on |x|, |W|, |b|, |dOut| (|w| too) with a sum (a mean keeps its
    division by the count): an upper bound of every intermediate's |terms|."""
    ref = _step(g, x, W, b, dOut, red, weighted, pre_gin, gin_scale, x.float())
    ga = SimpleNamespace(rowptr=g.rowptr, col=g.col, n_dst=g.n_dst, w=g.w.abs() if weighted else None)
    mag = _step(ga, x.abs(), W.abs(), b.abs() if b is not None else None, dOut.abs(),
                red if red == "mean" else "sum", weighted, pre_gin, abs(gin_scale), None)
    return ref, mag


def aggregate32(g, x, red: str, weighted: bool, pre_gin: bool = False, gin_scale: float = 1.0):
    """(P32, exact_rows): the fp32 restatement of P in separate fp32 ops, and the
    bool [n] mask of the rows on which it has one possible rounding -- every
    row for max / min (fp32 products, amax / amin, the isinf guard: selection
    is exact), the rows of degree <= 2 for a sum (0 + m0 + m1 has one order);
    a mean's rows are not claimed."""
    n, F = g.n_dst, x.shape[1]
    rowptr, col = g.rowptr.long(), g.col.long()
    deg = rowptr[1:] - rowptr[:-1]
    m = x[col]
    if weighted:
        m = m * g.w[:, None]
    if red in ("max", "min"):
        seg = torch.repeat_interleave(torch.arange(n, device=x.device), deg, output_size=col.numel())
        a = torch.full((n, F), float("-inf") if red == "max" else float("inf"), dtype=torch.float32, device=x.device)
        a.scatter_reduce_(0, seg[:, None].expand(-1, F), m, "amax" if red == "max" else "amin", include_self=True)
        a = torch.where(torch.isinf(a), torch.zeros_like(a), a)
        exact = torch.ones(n, dtype=torch.bool, device=x.device)
    else:
        last = max(col.numel() - 1, 0)
        zero = torch.zeros((n, F), dtype=torch.float32, device=x.device)
        m0 = torch.where((deg > 0)[:, None], m[rowptr[:-1].clamp(max=last)], zero)
        m1 = torch.where((deg > 1)[:, None], m[(rowptr[:-1] + 1).clamp(max=last)], zero)
        a = (zero + m0) + m1
        exact = deg <= 2 if red == "sum" else torch.zeros(n, dtype=torch.bool, device=x.device)
    if pre_gin:
        a = torch.tensor(gin_scale, dtype=torch.float32, device=x.device) * x[:n] + a
    return a, exact


def poison(dev, *shapes, streams=(None,), limit: int = 512) -> None:
    """Fill the caching allocator's free blocks with NaN: for each shape, NaN
    tensors are allocated until the cache cannot serve one (no cached bytes
    left for it, or the allocation took fresh device memory: every cached
    block that could serve the shape is then held and filled), and all are
    freed.  The next torch.empty of these shapes reads NaN where no kernel
    stores, not the previous launch's (right) answer.  The allocator pools its
    blocks per stream: `streams` lists the streams whose pools are filled
    (None = the current one)."""
    for stream in streams:
        with torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream(dev)):
            for shape in shapes:
                held = []
                nbytes = 4 * int(np.prod(shape))
                before = torch.cuda.memory_reserved(dev)
                while len(held) < limit and before - torch.cuda.memory_allocated(dev) >= nbytes:
                    held.append(torch.full(tuple(shape), float("nan"), dtype=torch.float32, device=dev))
                    if torch.cuda.memory_reserved(dev) > before:
                        break
                del held


def assert_same(got, want, g, label: str) -> None:
    """Bitwise equality of two results of the same computation (NaN equal to
    NaN); a failure names the rows that differ and, for a per-row quantity
    ([g.n_dst, F]), their kernels in g's schedule (g None: a reduced quantity)."""
    if got.shape != want.shape:
        raise AssertionError(f"{label}: shape {tuple(got.shape)} != {tuple(want.shape)}")
    if got.dim() == 0:
        got, want = got.reshape(1), want.reshape(1)
    diff = (got != want) & ~(torch.isnan(got) & torch.isnan(want))
    if not bool(diff.any()):
        return
    bad = torch.nonzero(diff.reshape(diff.shape[0], -1).any(1)).flatten()
    first = bad[:8]
    own = f" on {fused_ref.owners(g, first)} kernels" if g is not None and got.dim() == 2 else ""
    i = int(first[0])
    j = int(torch.nonzero(diff.reshape(diff.shape[0], -1)[i]).flatten()[0])
    raise AssertionError(f"{label}: {bad.numel()} rows differ ({int(diff.sum())} entries), first {first.tolist()}{own}; "
                         f"row {i} entry {j}: got {float(got.reshape(got.shape[0], -1)[i, j]):.9g} "
                         f"want {float(want.reshape(want.shape[0], -1)[i, j]):.9g}")


def check_rows(got, g, ref, mag, label: str, tol: float = 1e-5) -> float:
    """A per-row quantity (y, P or dx: fp32 [n, F]) against float64 within
    tol * max(1, mag); a failure names the rows and their kernels in g's
    schedule (for dx: the transposed graph's).  Returns the max scaled error."""
    return fused_ref.check(got, g, (ref, mag), label, tol)


def check_dense(got, ref, mag, label: str, tol: float = 1e-5) -> float:
    """A reduced quantity (dW, db: sums over all rows) against float64 within
    tol * mag, kgx_gemm_tn's own bound (tests/test_gpu_gemm_tn.py)."""
    err = (got.double() - ref).abs() / mag.clamp_min(1e-30)
    mx = float(err.max())
    if not mx <= tol:  # NaN fails too
        i = int(torch.nan_to_num(err, nan=float("inf")).argmax())
        raise AssertionError(f"{label}: max scaled error {mx:.3g} > {tol} at flat index {i}: got "
                             f"{float(got.flatten()[i]):.7g} ref {float(ref.flatten()[i]):.7g}")
    return mx
