"""numpy restatement of the neighbour sampler (keras-geometric_amd/csrc/sampler.hip
and keras_geometric_amd/sampling.py), bit for bit.

TEST INFRASTRUCTURE ONLY.  All generator arithmetic is uint64 modulo 2^64, as
on the device (include/kgx.h, "Neighbour sampling"):

    hs     = splitmix64(seed ^ splitmix64(uint64(uint32(hop))))
    rs     = splitmix64(hs ^ uint64(row))
    key[i] = splitmix64(rs + i),  i = 0..3
    rot    = ((splitmix64(rs + 4) >> 32) * d) >> 32
    phi    = 4-round Feistel on 2 * hb bits, hb = ceil(ceil_log2(d) / 2),
             cycle-walked into [0, d)
    pi(t)  = (phi(t) + rot) mod d

A row of degree d > k takes CSR slots pi(0..k-1) in that order; a row of degree
d <= k (or k = -1) is taken whole in CSR order.  The epoch is mixed in on the
host: seed64 = splitmix64(splitmix64(seed) + epoch).
"""

from __future__ import annotations

import numpy as np

U = np.uint64


def splitmix64(z):
    z = np.asarray(z, dtype=np.uint64)
    with np.errstate(over="ignore"):
        z = z + U(0x9E3779B97F4A7C15)
        z = (z ^ (z >> U(30))) * U(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> U(27))) * U(0x94D049BB133111EB)
    return z ^ (z >> U(31))


def epoch_seed(seed: int, epoch: int) -> int:
    with np.errstate(over="ignore"):
        return int(splitmix64(splitmix64(U(seed & 0xFFFFFFFFFFFFFFFF)) + U(epoch)))


def hop_stream(seed: int, hop: int) -> np.uint64:
    return U(splitmix64(U(seed & 0xFFFFFFFFFFFFFFFF) ^ splitmix64(U(hop & 0xFFFFFFFF))))


def ceil_log2(d: int) -> int:
    return 0 if d <= 1 else int(d - 1).bit_length()


def half_bits(d: int) -> int:
    return (ceil_log2(d) + 1) // 2


def row_keys(hs, rows):
    """uint64 [len(rows), 5]: the four Feistel keys of every row, then the word its rotation comes from."""
    rows = np.asarray(rows, dtype=np.uint64)
    with np.errstate(over="ignore"):
        rs = splitmix64(U(hs) ^ rows)
        return np.stack([splitmix64(rs + U(i)) for i in range(5)], axis=-1)


def _feistel_once(x, keys, hb: int):
    """x: uint64 [...]; keys: uint64 [..., 5] broadcastable against x."""
    mask = U((1 << hb) - 1)
    L = x >> U(hb)
    R = x & mask
    for i in range(4):
        nl = R
        R = L ^ (splitmix64(keys[..., i] ^ R) & mask)
        L = nl
    return (L << U(hb)) | R


def perm(t, keys, d: int):
    """pi(t) on [0, d) for every (t, key row) pair (broadcast); d >= 2."""
    hb = half_bits(d)
    t = np.asarray(t, dtype=np.uint64)
    keys = np.asarray(keys, dtype=np.uint64)
    shape = np.broadcast_shapes(t.shape, keys.shape[:-1])
    y = np.broadcast_to(t, shape).copy()
    k = np.broadcast_to(keys, shape + (5,))
    y = _feistel_once(y, k, hb)
    bad = y >= U(d)
    while bad.any():
        y[bad] = _feistel_once(y[bad], k[bad], hb)
        bad = y >= U(d)
    rot = ((k[..., 4] >> U(32)) * U(d)) >> U(32)
    return (y + rot) % U(d)


def row_slots(seed: int, hop: int, row: int, d: int, k: int) -> np.ndarray:
    """The CSR slots (int64, relative to the row's start) row `row` of degree d draws."""
    if k < 0 or d <= k:
        return np.arange(d, dtype=np.int64)
    keys = row_keys(hop_stream(seed, hop), [row])[0]
    return perm(np.arange(k, dtype=np.uint64), keys, d).astype(np.int64)


def build_csr(edge_index: np.ndarray, n: int):
    """Stable CSR by destination (kgx_csr_build for ids in [0, n)): rowptr, col, eid."""
    src = np.asarray(edge_index[0], dtype=np.int64)
    dst = np.asarray(edge_index[1], dtype=np.int64)
    order = np.argsort(dst, kind="stable")
    rowptr = np.zeros(n + 1, dtype=np.int64)
    rowptr[1:] = np.cumsum(np.bincount(dst, minlength=n))
    return rowptr, src[order].astype(np.int32), order.astype(np.int32)


def sample_hop(csr, seeds, fanout: int, seed: int, hop: int):
    """kgx_sample_neighbors: (out_rowptr, out_src, out_eid) as int32."""
    rowptr, col, eid = csr
    seeds = np.asarray(seeds, dtype=np.int64)
    out_rowptr = np.zeros(len(seeds) + 1, dtype=np.int32)
    src, ids = [], []
    for i, r in enumerate(seeds):
        b = int(rowptr[r])
        d = int(rowptr[r + 1]) - b
        slots = b + row_slots(seed, hop, int(r), d, fanout)
        src.append(col[slots])
        ids.append(eid[slots])
        out_rowptr[i + 1] = out_rowptr[i] + len(slots)
    cat = lambda parts: np.concatenate(parts).astype(np.int32) if parts else np.zeros(0, np.int32)  # noqa: E731
    return out_rowptr, cat(src), cat(ids)


def relabel(nodes, frontier, out_rowptr, out_src):
    """kgx_relabel_frontier: (new_nodes, src_local, dst_local) as int32."""
    nodes = np.asarray(nodes, dtype=np.int64)
    local = {int(v): i for i, v in enumerate(nodes)}
    assert len(local) == len(nodes), "duplicate ids in nodes"
    new = np.array(sorted({int(s) for s in out_src} - set(local)), dtype=np.int32)
    for j, v in enumerate(new):
        local[int(v)] = len(nodes) + j
    src_local = np.array([local[int(s)] for s in out_src], dtype=np.int32)
    counts = np.diff(np.asarray(out_rowptr, dtype=np.int64))
    dst_local = np.repeat(np.array([local[int(f)] for f in frontier], dtype=np.int32), counts).astype(np.int32)
    return new, src_local, dst_local


def sample_subgraph(csr, seeds, fanouts, seed: int = 0, epoch: int = 0) -> dict:
    """NeighborSampler.sample: node_ids, edge_index [2, E_s], edge_ids, n_seeds, hop_node_counts."""
    nodes = np.asarray(seeds, dtype=np.int32)
    frontier = nodes
    seed64 = epoch_seed(seed, epoch)
    counts = [len(nodes)]
    srcs, dsts, eids = [], [], []
    for hop, k in enumerate(fanouts):
        if len(frontier) == 0:
            break
        out_rowptr, out_src, out_eid = sample_hop(csr, frontier, k, seed64, hop)
        new, s_l, d_l = relabel(nodes, frontier, out_rowptr, out_src)
        srcs.append(s_l)
        dsts.append(d_l)
        eids.append(out_eid)
        counts.append(len(new))
        nodes = np.concatenate([nodes, new]).astype(np.int32)
        frontier = new
    z = np.zeros(0, np.int32)
    return {
        "node_ids": nodes,
        "edge_index": np.stack([np.concatenate(srcs or [z]), np.concatenate(dsts or [z])]).astype(np.int32),
        "edge_ids": np.concatenate(eids or [z]).astype(np.int32),
        "n_seeds": len(seeds),
        "hop_node_counts": counts,
    }
