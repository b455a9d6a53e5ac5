"""numpy restatement of kgx_knn (include/kgx.h) and a float64 literal EdgeConv; imports nothing of the package."""

from __future__ import annotations

import numpy as np
import torch

SIZES = [1, 5, 6, 63, 64, 65, 130, 0, 17]  # tiles of 64 queries straddle segments; an empty one; two below k + 1
SIZES_Y = [3, 0, 20, 64, 1, 70, 5, 2, 9]   # the bipartite form's queries


def offsets(sizes) -> np.ndarray:
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)


def batch_of(sizes) -> np.ndarray:
    return np.repeat(np.arange(len(sizes)), sizes).astype(np.int64)


def lattice(n: int, D: int, seed: int) -> np.ndarray:
    """Integer coordinates in [-8, 8]: every product and sum is exact in bf16 and fp32, and ties abound."""
    return np.random.default_rng(seed).integers(-8, 9, size=(n, D)).astype(np.float32)


def dist2_f32(y: np.ndarray, x: np.ndarray) -> np.ndarray:
    """The direct path's arithmetic: acc = 0; for d ascending: t = y_d - x_d; acc = acc + t * t, in fp32."""
    acc = np.zeros((y.shape[0], x.shape[0]), np.float32)
    for d in range(x.shape[1]):
        t = y[:, None, d] - x[None, :, d]
        acc = acc + t * t
    return acc


def dist2_f64(y: np.ndarray, x: np.ndarray) -> np.ndarray:
    return ((y.astype(np.float64)[:, None, :] - x.astype(np.float64)[None, :, :]) ** 2).sum(-1)


def knn_table(d2: np.ndarray, seg_x, seg_y, k: int, exclude_self: bool):
    """(nbr int32 [Q, k], dist [Q, k]) from a full distance table: per segment, ascending in (d2, index);
    NaN and +inf are never selected; short rows are padded with -1 / +inf."""
    Q = d2.shape[0]
    nbr = np.full((Q, k), -1, np.int32)
    dist = np.full((Q, k), np.inf, d2.dtype)
    for s in range(len(seg_x) - 1):
        lo, hi, qlo, qhi = seg_x[s], seg_x[s + 1], seg_y[s], seg_y[s + 1]
        blk = d2[qlo:qhi, lo:hi].copy()
        if exclude_self:
            for i in range(max(qlo, lo), min(qhi, hi)):
                blk[i - qlo, i - lo] = np.inf
        blk[~(blk < np.inf)] = np.inf
        order = np.argsort(blk, axis=1, kind="stable")[:, :k]
        val = np.take_along_axis(blk, order, axis=1)
        kk = order.shape[1]
        dist[qlo:qhi, :kk] = val
        nbr[qlo:qhi, :kk] = np.where(val < np.inf, order + lo, -1)
    return nbr, dist


def edges_of(nbr: np.ndarray):
    keep = nbr >= 0  # knn_graph's order: by target, then by rank
    return nbr[keep].astype(np.int64), np.nonzero(keep)[0]


def edge_conv64(x, layers, src, dst, aggr: str, act, gout):
    """aggr_j MLP([x_i || x_j - x_i]) literally, per edge, in float64, with its gradients.
    layers: [(W, b), ...] numpy; act: a torch function.  A row without edges is 0."""
    xt = torch.tensor(x, dtype=torch.float64, requires_grad=True)
    ws = [(torch.tensor(W, dtype=torch.float64, requires_grad=True), torch.tensor(b, dtype=torch.float64, requires_grad=True))
          for W, b in layers]
    s, d = torch.as_tensor(src), torch.as_tensor(dst)
    h = torch.cat([xt[d], xt[s] - xt[d]], dim=1)
    for W, b in ws:
        h = act(h @ W + b)
    out = torch.zeros((x.shape[0], h.shape[1]), dtype=torch.float64)
    out = out.scatter_reduce(0, d[:, None].expand_as(h), h, {"max": "amax", "mean": "mean"}[aggr], include_self=False)
    out.backward(torch.tensor(gout, dtype=torch.float64))
    grads = [g.grad.numpy() for pair in ws for g in pair]
    return out.detach().numpy(), xt.grad.numpy(), grads
