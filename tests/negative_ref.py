"""numpy restatement of kgx_negative_edges (include/kgx.h), bit for bit in uint64.

Every output is a function of (seed, the positive's key, q, the destination's
sorted CSR row):
    ks   = splitmix64(seed ^ splitmix64(uint64(uint32(key))))
    rs   = splitmix64(ks + q)
    try t: r = splitmix64(rs + t), cand = ((r >> 32) * n_src) >> 32
and the first candidate that is neither the destination itself (no_self) nor
one of its in-neighbours (reject_edges) is taken; after max_tries rejections
the last candidate is, and it is counted as a fallback.
"""

import numpy as np

U64 = np.uint64


def splitmix64(z):
    """The mixing step on uint64 arrays (wrapping arithmetic)."""
    z = np.asarray(z, dtype=U64)
    with np.errstate(over="ignore"):
        z = z + U64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> U64(30))) * U64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> U64(27))) * U64(0x94D049BB133111EB)
    return z ^ (z >> U64(31))


def sorted_csr(edge_index, n_dst):
    """(rowptr [n_dst + 1], col_sorted [E]) of a [2, E] (src, dst) edge list: the
    destination CSR with every row ascending (duplicates kept)."""
    src, dst = np.asarray(edge_index[0], np.int64), np.asarray(edge_index[1], np.int64)
    order = np.lexsort((src, dst))
    rowptr = np.zeros(n_dst + 1, np.int32)
    np.cumsum(np.bincount(dst, minlength=n_dst), out=rowptr[1:])
    return rowptr, src[order].astype(np.int32)


def uniform_graph():
    """64 nodes; destination 0 has the 16 distinct in-neighbours 1..16 (so with
    no_self 17 of 64 candidates are rejected per try and 47 are admissible);
    a few other rows so that the CSR is not one row.  (edge_index, n)"""
    src = list(range(1, 17)) + [5, 9, 0, 63, 2]
    dst = [0] * 16 + [20, 20, 33, 63, 1]
    rng = np.random.default_rng(3)
    order = rng.permutation(len(src))  # input order is not CSR order
    return np.stack([np.array(src)[order], np.array(dst)[order]]).astype(np.int32), 64


def fallback_graph(free=7):
    """16 nodes; destination 0's row holds every source but `free`, itself
    included: 15 of 16 candidates are rejected per try.  (edge_index, n)"""
    src = [s for s in range(16) if s != free] + [3, 4]
    dst = [0] * 15 + [9, 9]
    return np.stack([np.array(src[::-1]), np.array(dst[::-1])]).astype(np.int32), 16


def mixed_graph():
    """80 nodes, 400 random edges with duplicates, self loops and empty rows
    (destinations are drawn from 50 of the nodes).  (edge_index, n)"""
    rng = np.random.default_rng(11)
    src = rng.integers(0, 80, 400)
    dst = rng.integers(0, 50, 400) + 10
    src[:40] = src[40:80]  # duplicated edges
    dst[:40] = dst[40:80]
    src[100:110] = dst[100:110]  # self loops
    return np.stack([src, dst]).astype(np.int32), 80


def negative_edges(rowptr, col_sorted, n_dst, n_src, a, keys, Q, seed, max_tries=8, no_self=True, reject_edges=True):
    """(out int32 [P, Q], [fallbacks, destinations out of range])."""
    a = np.asarray(a, np.int64)
    keys = np.asarray(keys, np.int32)
    P = a.shape[0]
    out = np.full((P, Q), -1, np.int32)
    row_ok = (a >= 0) & (a < n_dst)
    if P == 0:
        return out, [0, 0]
    rows = np.repeat(np.arange(n_dst, dtype=np.int64), np.diff(np.asarray(rowptr, np.int64)))
    edge_keys = rows * n_src + np.asarray(col_sorted, np.int64)[: rows.shape[0]]
    with np.errstate(over="ignore"):
        ks = splitmix64(U64(seed & (2**64 - 1)) ^ splitmix64(keys.astype(np.uint32).astype(U64)))
        rs = splitmix64(ks[:, None] + np.arange(Q, dtype=U64)[None, :])
    pending = np.repeat(row_ok[:, None], Q, axis=1)
    cand = np.full((P, Q), -1, np.int64)
    for t in range(max_tries):
        with np.errstate(over="ignore"):
            r = splitmix64(rs + U64(t))
        cand = (((r >> U64(32)) * U64(n_src)) >> U64(32)).astype(np.int64)
        rej = np.zeros((P, Q), bool)
        if no_self:
            rej |= cand == a[:, None]
        if reject_edges:
            rej |= np.isin(a[:, None] * n_src + cand, edge_keys)
        take = pending & ~rej
        out[take] = cand[take]
        pending &= rej
    out[pending] = cand[pending]
    return out, [int(pending.sum()), int((~row_ok).sum())]
