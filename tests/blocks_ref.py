"""numpy restatement of the sampled blocks (NeighborSampler.sample_blocks,
kgx_block_csr) and of a SAGE layer over a bipartite block, in float64.

TEST INFRASTRUCTURE ONLY.  Everything is derived from the output of
sampling_ref.sample_subgraph: local ids are seeds first, then hop by hop, so
with P_h = sum(hop_node_counts[: h + 1]) the edges of hops 0..h are the edges
with dst < P_h, a prefix of the destination-sorted edge list.
"""

from __future__ import annotations

import numpy as np


def node_prefix(sub: dict, n_layers: int) -> list[int]:
    """[P_0, ..., P_L]: a hop that never ran adds no nodes."""
    counts = list(sub["hop_node_counts"]) + [0] * (n_layers + 1 - len(sub["hop_node_counts"]))
    return np.cumsum(counts).tolist()


def block_bounds(sub: dict, n_layers: int) -> list[tuple[int, int, int]]:
    """(n_src, n_dst, E_b) of every block, outermost first."""
    P = node_prefix(sub, n_layers)
    dst = np.asarray(sub["edge_index"][1], dtype=np.int64)
    out = []
    for layer in range(n_layers):
        h = n_layers - 1 - layer
        out.append((P[h + 1], P[h], int((dst < P[h]).sum())))
    return out


def forward_csr(dst: np.ndarray, n_dst: int):
    """(rowptr, deg) of destination-sorted edges; col = src and eid = arange."""
    deg = np.bincount(np.asarray(dst, dtype=np.int64), minlength=n_dst)[:n_dst]
    rowptr = np.zeros(n_dst + 1, dtype=np.int64)
    rowptr[1:] = np.cumsum(deg)
    return rowptr.astype(np.int32), deg.astype(np.int32)


def transposed_csr(src: np.ndarray, dst: np.ndarray, n_src: int):
    """(t_rowptr, t_deg, t_col, t_eid): source-major, edges of one source in ascending position."""
    src = np.asarray(src, dtype=np.int64)
    order = np.argsort(src, kind="stable")
    t_deg = np.bincount(src, minlength=n_src)[:n_src]
    t_rowptr = np.zeros(n_src + 1, dtype=np.int64)
    t_rowptr[1:] = np.cumsum(t_deg)
    return (t_rowptr.astype(np.int32), t_deg.astype(np.int32), np.asarray(dst)[order].astype(np.int32),
            order.astype(np.int32))


def sage_mean_layer(x, src, dst, n_dst, W_self, W_neigh, b, relu=True):
    """float64 relu?(x[:n_dst] W_self + mean_{e: dst = i} x[src_e] W_neigh + b); rows without edges aggregate 0."""
    x = np.asarray(x, dtype=np.float64)
    src, dst = np.asarray(src, dtype=np.int64), np.asarray(dst, dtype=np.int64)
    agg = np.zeros((n_dst, x.shape[1]))
    np.add.at(agg, dst, x[src])
    cnt = np.bincount(dst, minlength=n_dst)[:n_dst].astype(np.float64)
    agg /= np.maximum(cnt, 1.0)[:, None]
    out = x[:n_dst] @ W_self + agg @ W_neigh + b
    return np.maximum(out, 0.0) if relu else out
