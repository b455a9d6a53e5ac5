"""Neighbour sampling for mini-batch GraphSAGE training, on the device.

`NeighborSampler` draws a fan-out sample around a batch of seed nodes
(kgx_sample_neighbors, one launch group per hop) and compacts it into a small
graph with local ids (kgx_relabel_frontier); the existing layers run on it,
with autograd, like on any other edge_index:

    sampler = NeighborSampler(edge_index, num_nodes, fanouts=[15, 10], seed=0)
    sub = sampler.sample(batch_ids, epoch=e)
    out = layer([sub.gather(x), sub.edge_index])[: sub.n_seeds]

A model of several layers takes the same sample as one bipartite Block per
layer (sample_blocks; kgx_block_csr), so that layer l computes only the rows
the layers after it read:

    blocks = sampler.sample_blocks(batch_ids, epoch=e)
    h = blocks.gather(x)
    for layer, blk in zip(layers, blocks):
        h = layer([h, blk])              # [blk.n_src, F] -> [blk.n_dst, F_out]

The reference has no sampler (it trains full-batch); the semantics are those of
PyG's NeighborLoader without replacement: hop 0 expands the seeds, hop h > 0
expands exactly the nodes hop h - 1 added, every node is expanded at most once.
The sample is counter based: a node's neighbours depend on (seed, epoch, hop,
the node's id) only, never on the batch around it (include/kgx.h states the
key derivation, tests/sampling_ref.py restates it in numpy).

For link prediction, `NegativeSampler` turns a batch of positive edges into an
`EdgeBatch` with Q corrupted sources each (kgx_negative_edges), keyed the same
way on the positive's input edge id (tests/negative_ref.py):

    neg = NegativeSampler(edge_index, num_nodes, num_negatives=4, seed=0)
    batch = neg.sample(edge_ids, epoch=e)         # a_idx [P], b_idx [P, 1 + Q], labels
    scores = DotProductDecoder()([z, batch])      # [P, 1 + Q], column 0 the positive
"""

from __future__ import annotations

import ctypes
from dataclasses import dataclass, field

import numpy as np
import torch

from . import _native as nat
from . import ops as kops
from .graph import Block, CSRGraph, _build_schedule, default_split_len
from .layers._edges import edge_index_tensor, graph_for

_M64 = (1 << 64) - 1


def splitmix64(z: int) -> int:
    """The generator's mixing step on a Python int (uint64 arithmetic)."""
    z = (z + 0x9E3779B97F4A7C15) & _M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
    return z ^ (z >> 31)


def epoch_seed(seed: int, epoch: int) -> int:
    """The 64-bit seed of one epoch: splitmix64(splitmix64(seed) + epoch) mod 2^64."""
    return splitmix64((splitmix64(int(seed) & _M64) + int(epoch)) & _M64)


def _ws(nbytes: int, dev: torch.device) -> torch.Tensor:
    return torch.empty(max(nbytes, 1), dtype=torch.uint8, device=dev)


def _seed_tensor(seeds, dev: torch.device) -> torch.Tensor:
    if not isinstance(seeds, torch.Tensor):
        seeds = torch.as_tensor(np.asarray(seeds))
    if seeds.dim() != 1:
        raise ValueError(f"seeds must be a 1-d list of node ids, got shape {tuple(seeds.shape)}")
    return seeds.to(device=dev, dtype=torch.int32).contiguous()


def sample_neighbors(g: CSRGraph, seeds: torch.Tensor, fanout: int, seed: int, hop: int = 0):
    """One hop of fan-out sampling over g's rows (kgx_sample_neighbors).

    Returns (rowptr [n_seeds + 1], src [E_s], eid [E_s]), int32 on g's device:
    row i lists min(deg(seeds[i]), fanout) in-edges of seeds[i] (all of them for
    fanout = -1) as global source ids and input edge ids."""
    dev = nat.require_device(g.rowptr, seeds)
    if seeds.dtype != torch.int32:
        raise TypeError("sample_neighbors expects int32 seeds")
    seeds = seeds.contiguous()
    n = int(seeds.numel())
    fanout = int(fanout)
    i32 = dict(dtype=torch.int32, device=dev)
    if n == 0 and (fanout >= 1 or fanout == -1):
        return torch.zeros(1, **i32), torch.empty(0, **i32), torch.empty(0, **i32)
    # fanout -1: the seeds' total degree, on the device (the call checks it against cap anyway)
    cap = n * fanout if fanout > 0 else (int(g.deg[seeds.long().clamp(0, max(g.n_dst - 1, 0))].sum()) if g.n_dst else 0)
    L = nat.lib()
    rowptr = torch.empty(n + 1, **i32)
    src = torch.empty(max(cap, 1), **i32)
    eid = torch.empty(max(cap, 1), **i32)
    nbytes = ctypes.c_size_t(0)
    nat.check(L.kgx_sample_workspace_bytes(n, ctypes.byref(nbytes)), "kgx_sample_workspace_bytes")
    ws = _ws(nbytes.value, dev)
    info = (ctypes.c_int64 * 4)()
    nat.check(
        L.kgx_sample_neighbors(
            nat.ptr(g.rowptr), nat.ptr(g.col), nat.ptr(g.eid), g.n_dst, nat.ptr(seeds), n, fanout,
            int(seed) & _M64, int(hop), nat.ptr(rowptr), nat.ptr(src), nat.ptr(eid), max(cap, 0),
            nat.ptr(ws), nbytes.value, info, nat.stream(dev),
        ),
        "kgx_sample_neighbors",
    )
    e = int(info[0])
    return rowptr, src[:e], eid[:e]


def relabel_frontier(nodes: torch.Tensor, frontier: torch.Tensor, rowptr: torch.Tensor, src: torch.Tensor,
                     node_map: torch.Tensor):
    """Local ids of one hop (kgx_relabel_frontier): (new_nodes, src_local,
    dst_local).  node_map: int32 [n_nodes], all -1 on entry and on return."""
    dev = nat.require_device(nodes, frontier, rowptr, src, node_map)
    n_known, n_f, e = int(nodes.numel()), int(frontier.numel()), int(src.numel())
    n_nodes = int(node_map.numel())
    i32 = dict(dtype=torch.int32, device=dev)
    new_nodes = torch.empty(max(e, 1), **i32)
    src_local = torch.empty(max(e, 1), **i32)
    dst_local = torch.empty(max(e, 1), **i32)
    L = nat.lib()
    nbytes = ctypes.c_size_t(0)
    nat.check(L.kgx_relabel_workspace_bytes(e, n_nodes, ctypes.byref(nbytes)), "kgx_relabel_workspace_bytes")
    ws = _ws(nbytes.value, dev)
    info = (ctypes.c_int64 * 4)()
    nat.check(
        L.kgx_relabel_frontier(
            nat.ptr(nodes), n_known, nat.ptr(frontier), n_f, nat.ptr(rowptr), nat.ptr(src), e,
            nat.ptr(node_map), n_nodes, nat.ptr(new_nodes), nat.ptr(src_local), nat.ptr(dst_local),
            nat.ptr(ws), nbytes.value, info, nat.stream(dev),
        ),
        "kgx_relabel_frontier",
    )
    return new_nodes[: int(info[0])], src_local[:e], dst_local[:e]


@dataclass
class SampledSubgraph:
    """A sampled mini-batch in local ids.

    node_ids         int32 [n_sub]   global ids; the seeds first, in the order given,
                                     then every hop's new nodes in ascending global id
    edge_index       int32 [2, E_s]  local (src, dst), the hops concatenated in hop order
    edge_ids         int32 [E_s]     input edge id of every sampled edge
    n_seeds          the first n_seeds local ids are the seeds
    hop_node_counts  [n_seeds, nodes added by hop 0, nodes added by hop 1, ...]
    """

    node_ids: torch.Tensor
    edge_index: torch.Tensor
    edge_ids: torch.Tensor
    n_seeds: int
    hop_node_counts: list = field(default_factory=list)

    def gather(self, x: torch.Tensor) -> torch.Tensor:
        """x[node_ids] (kgx_gather_rows): the batch's feature rows, local order."""
        return kops.gather_rows(x, self.node_ids)


def block_csr(src: torch.Tensor, dst: torch.Tensor, n_src: int, n_dst: int, forward: bool = True):
    """The CSR pair of a bipartite block whose edges are sorted by destination
    (kgx_block_csr).  Returns (rowptr [n_dst + 1], deg [n_dst]) -- (None, None)
    with forward=False --, (t_rowptr [n_src + 1], t_deg [n_src], t_col [E],
    t_eid [E]) and (max in-degree, max out-degree); all tensors int32.  The
    forward CSR's col is `src` and its eid the edge position.  ValueError for
    an unsorted dst, IndexError for an id out of range."""
    dev = nat.require_device(src, dst)
    if src.dtype != torch.int32 or dst.dtype != torch.int32:
        raise TypeError("block_csr expects int32 src / dst")
    src, dst = src.contiguous(), dst.contiguous()
    E = int(src.numel())
    if int(dst.numel()) != E:
        raise ValueError(f"src/dst length mismatch: {E} vs {dst.numel()}")
    n_src, n_dst = int(n_src), int(n_dst)
    i32 = dict(dtype=torch.int32, device=dev)
    rowptr = torch.empty(n_dst + 1, **i32) if forward else None
    deg = torch.empty(max(n_dst, 1), **i32) if forward else None
    t_rowptr = torch.empty(n_src + 1, **i32)
    t_deg = torch.empty(max(n_src, 1), **i32)
    t_col = torch.empty(max(E, 1), **i32)
    t_eid = torch.empty(max(E, 1), **i32)
    L = nat.lib()
    nbytes = ctypes.c_size_t(0)
    nat.check(L.kgx_block_workspace_bytes(E, n_src, ctypes.byref(nbytes)), "kgx_block_workspace_bytes")
    ws = _ws(nbytes.value, dev)
    info = (ctypes.c_int64 * 4)()
    nat.check(
        L.kgx_block_csr(
            nat.ptr(src), nat.ptr(dst), E, n_src, n_dst, nat.ptr(rowptr), nat.ptr(deg),
            nat.ptr(t_rowptr), nat.ptr(t_deg), nat.ptr(t_col), nat.ptr(t_eid),
            nat.ptr(ws), nbytes.value, info, nat.stream(dev),
        ),
        "kgx_block_csr",
    )
    fwd = (rowptr, deg[:n_dst]) if forward else (None, None)
    return fwd, (t_rowptr, t_deg[:n_src], t_col[:E], t_eid[:E]), (int(info[0]), int(info[1]))


@dataclass
class SampledBlocks:
    """A sampled mini-batch as one Block per layer, outermost first:

        h = blocks.gather(x)
        for layer, blk in zip(layers, blocks):
            h = layer([h, blk])          # [blk.n_src, F] -> [blk.n_dst, F_out]

    blocks[l].n_dst == blocks[l + 1].n_src, and the last block writes the seeds.
    node_ids, n_seeds and hop_node_counts are those of SampledSubgraph."""

    node_ids: torch.Tensor
    n_seeds: int
    hop_node_counts: list
    blocks: list

    def gather(self, x: torch.Tensor) -> torch.Tensor:
        """x[node_ids] (kgx_gather_rows): the outermost block's source rows."""
        return kops.gather_rows(x, self.node_ids)

    def __len__(self) -> int:
        return len(self.blocks)

    def __getitem__(self, i):
        return self.blocks[i]

    def __iter__(self):
        return iter(self.blocks)


def _block_graph(n_src: int, n_dst: int, col, eid, rowptr, deg, max_deg: int, n_features: int) -> CSRGraph:
    kept = int(col.numel())
    g = CSRGraph(n_src=n_src, n_dst=n_dst, n_input_edges=kept, kept=kept, max_degree=max_deg, flags=0,
                 rowptr=rowptr, col=col, eid=eid, deg=deg)
    _build_schedule(g, default_split_len(kept, n_features))
    return g


class NeighborSampler:
    """Fan-out neighbour sampler over one graph.

    fanouts: neighbours drawn per node and hop (-1: all of them).  The CSR by
    destination is built once, through the layers' graph cache (no self loops,
    no GCN norm), and the sampler owns the dense local-id map the relabel step
    uses (all -1 between calls)."""

    def __init__(self, edge_index, num_nodes: int, fanouts: list[int], seed: int = 0) -> None:
        fanouts = [int(k) for k in fanouts]
        if not fanouts or any(k == 0 or k < -1 for k in fanouts):
            raise ValueError(f"fanouts must be a non-empty list of k >= 1 or -1, got {fanouts}")
        self.num_nodes = int(num_nodes)
        self.fanouts = fanouts
        self.seed = int(seed)
        self._edge_index = edge_index  # the graph cache is keyed on the caller's object
        ei = edge_index_tensor(edge_index, None, allow_transpose=True)
        self.graph = graph_for(edge_index, ei, self.num_nodes, self.num_nodes)
        self._map = torch.full((max(self.num_nodes, 1),), -1, dtype=torch.int32, device=self.graph.device)

    @property
    def device(self) -> torch.device:
        return self.graph.device

    def sample(self, seeds, epoch: int = 0) -> SampledSubgraph:
        """One mini-batch around `seeds` (distinct node ids).  ValueError for
        duplicate seeds, IndexError for a seed outside [0, num_nodes)."""
        dev = self.device
        nodes = _seed_tensor(seeds, dev)
        n_seeds = int(nodes.numel())
        seed64 = epoch_seed(self.seed, epoch)
        frontier = nodes
        counts = [n_seeds]
        srcs, dsts, eids = [], [], []
        for hop, k in enumerate(self.fanouts):
            if frontier.numel() == 0:
                break
            rowptr, src, eid = sample_neighbors(self.graph, frontier, k, seed64, hop)
            new, src_l, dst_l = relabel_frontier(nodes, frontier, rowptr, src, self._map[: self.num_nodes])
            srcs.append(src_l)
            dsts.append(dst_l)
            eids.append(eid)
            counts.append(int(new.numel()))
            if new.numel():
                nodes = torch.cat([nodes, new])
            frontier = new
        i32 = dict(dtype=torch.int32, device=dev)
        if srcs:
            edge_index = torch.stack([torch.cat(srcs), torch.cat(dsts)])
            edge_ids = torch.cat(eids)
        else:
            edge_index, edge_ids = torch.empty((2, 0), **i32), torch.empty(0, **i32)
        return SampledSubgraph(node_ids=nodes, edge_index=edge_index, edge_ids=edge_ids, n_seeds=n_seeds,
                               hop_node_counts=counts)

    def sample_blocks(self, seeds, epoch: int = 0, n_features: int = 128) -> SampledBlocks:
        """The sample of `sample(seeds, epoch)` as one bipartite Block per layer.

        Local ids are given to the seeds first, then hop by hop, so with
        P_h = sum(hop_node_counts[: h + 1]) the edges of hops 0..h are a prefix
        of the edge list, sorted by destination, with destinations < P_h and
        sources < P_{h+1}: block l (outermost first) is the prefix of hops
        0..L-1-l with n_dst = P_{L-1-l}, n_src = P_{L-l}.  A hop that never ran
        (the frontier emptied) adds no nodes and no edges.  The forward CSR is
        computed once, for the outermost block; every block gets its own
        transposed CSR (kgx_block_csr) and its schedules.  n_features sizes the
        schedules' hub chunks, as in the layers' graph cache."""
        return self._blocks_of(*self._sample_hops(seeds, epoch), n_features=n_features)

    def _blocks_of(self, nodes, edge_index, edge_ids, counts, e_counts, n_features: int = 128) -> SampledBlocks:
        """The blocks of one _sample_hops draw (everything after the sample itself)."""
        L = len(self.fanouts)
        P = np.cumsum(counts + [0] * (L + 1 - len(counts))).tolist()  # P[h] = nodes before hop h runs
        Ep = np.cumsum(e_counts + [0] * (L - len(e_counts))).tolist()  # Ep[h] = edges of hops 0..h
        src, dst = edge_index[0], edge_index[1]
        pos = torch.arange(Ep[-1], dtype=torch.int32, device=self.device)
        blocks = []
        rowptr = deg = None
        for layer in range(L):
            h = L - 1 - layer
            n_dst, n_src, e = P[h], P[h + 1], Ep[h]
            fwd, (t_rowptr, t_deg, t_col, t_eid), (max_in, max_out) = block_csr(src[:e], dst[:e], n_src, n_dst,
                                                                               forward=layer == 0)
            if layer == 0:
                rowptr, deg = fwd
            g = _block_graph(n_src, n_dst, src[:e], pos[:e], rowptr[: n_dst + 1], deg[:n_dst], max_in, n_features)
            t = _block_graph(n_dst, n_src, t_col, t_eid, t_rowptr, t_deg, max_out, n_features)
            t.extras["fwd_slot"] = t_eid.long()  # as graph.transpose leaves it
            g.extras["T"] = t
            blocks.append(Block(n_src=n_src, n_dst=n_dst, edge_index=edge_index[:, :e], edge_ids=edge_ids[:e], graph=g))
        return SampledBlocks(node_ids=nodes, n_seeds=counts[0], hop_node_counts=counts, blocks=blocks)

    def _sample_hops(self, seeds, epoch: int):
        """sample()'s draw, with the edge count of every hop that ran:
        (node_ids, edge_index, edge_ids, hop_node_counts, hop_edge_counts)."""
        dev = self.device
        nodes = _seed_tensor(seeds, dev)
        seed64 = epoch_seed(self.seed, epoch)
        frontier = nodes
        counts, e_counts = [int(nodes.numel())], []
        srcs, dsts, eids = [], [], []
        for hop, k in enumerate(self.fanouts):
            if frontier.numel() == 0:
                break
            rowptr, src, eid = sample_neighbors(self.graph, frontier, k, seed64, hop)
            new, src_l, dst_l = relabel_frontier(nodes, frontier, rowptr, src, self._map[: self.num_nodes])
            srcs.append(src_l)
            dsts.append(dst_l)
            eids.append(eid)
            counts.append(int(new.numel()))
            e_counts.append(int(eid.numel()))
            if new.numel():
                nodes = torch.cat([nodes, new])
            frontier = new
        i32 = dict(dtype=torch.int32, device=dev)
        if srcs:
            edge_index = torch.stack([torch.cat(srcs), torch.cat(dsts)])
            edge_ids = torch.cat(eids)
        else:
            edge_index, edge_ids = torch.empty((2, 0), **i32), torch.empty(0, **i32)
        return nodes, edge_index, edge_ids, counts, e_counts


# ---------------------------------------------------------------------------
# Link prediction: positives with their negatives
# ---------------------------------------------------------------------------
def negative_edges(rowptr: torch.Tensor | None, col_sorted: torch.Tensor | None, n_dst: int, n_src: int,
                   a: torch.Tensor, keys: torch.Tensor, num_negatives: int, seed: int, *, max_tries: int = 8,
                   no_self: bool = True, reject_edges: bool = True, out: torch.Tensor | None = None,
                   stats: torch.Tensor | None = None):
    """Q corrupted sources for every positive (kgx_negative_edges): (out, stats).

    a [P]: the positives' destinations, keys [P]: their keys (input edge ids),
    both int32; rowptr / col_sorted: a destination CSR whose rows are sorted
    ascending.  out: int32 [P, >= Q] with unit column stride (a column slice of
    a wider index array is written in place), made [P, Q] when None.  stats:
    int32 [2] on the device, zeroed here when None: outputs that used up
    max_tries, and positives whose destination is outside [0, n_dst) (their
    outputs are -1).  Never synchronises."""
    dev = nat.require_device(a, keys, rowptr, col_sorted, out, stats)
    if a.dtype != torch.int32 or keys.dtype != torch.int32:
        raise TypeError("negative_edges expects int32 a / keys")
    a, keys = a.contiguous(), keys.contiguous()
    P, Q = int(a.numel()), int(num_negatives)
    if int(keys.numel()) != P:
        raise ValueError(f"a / keys length mismatch: {P} vs {keys.numel()}")
    if out is None:
        out = torch.empty((P, max(Q, 0)), dtype=torch.int32, device=dev)
    if out.dtype != torch.int32 or out.dim() != 2 or out.shape[0] != P or (out.shape[1] > 1 and out.stride(1) != 1):
        raise ValueError("negative_edges: out must be an int32 [P, >= Q] array with unit column stride")
    if stats is None:
        stats = torch.zeros(2, dtype=torch.int32, device=dev)
    flags = (nat.NEG_NO_SELF if no_self else 0) | (nat.NEG_REJECT_EDGES if reject_edges else 0)
    ld_out = out.stride(0) if P > 1 else max(out.shape[1], Q)
    nat.check(
        nat.lib().kgx_negative_edges(
            nat.ptr(rowptr), nat.ptr(col_sorted), int(n_dst), int(n_src), nat.ptr(a), nat.ptr(keys), P, Q,
            int(seed) & _M64, int(max_tries), flags, nat.ptr(out), ld_out, nat.ptr(stats), nat.stream(dev),
        ),
        "kgx_negative_edges",
    )
    return out, stats


@dataclass
class EdgeBatch:
    """A batch of positive edges with their negatives (NegativeSampler.sample).

    a_idx     int32 [P]         the positives' destinations (global ids)
    b_idx     int32 [P, 1 + Q]  column 0 the true source, columns 1.. the Q corrupted sources
    labels    fp32  [P, 1 + Q]  1 in column 0, 0 elsewhere
    edge_ids  int32 [P]         the positives' input edge ids (the sampler's keys)
    stats     int32 [2] on the device: negatives that used up max_tries, edge ids out of range
    extras    per-batch cache (ops.edge_dot keeps the backward's pair graph here)
    """

    a_idx: torch.Tensor
    b_idx: torch.Tensor
    labels: torch.Tensor
    edge_ids: torch.Tensor
    stats: torch.Tensor
    extras: dict = field(default_factory=dict)

    @property
    def num_negatives(self) -> int:
        return int(self.b_idx.shape[1]) - 1

    def fallbacks(self) -> int:
        """Negatives whose every try was rejected (they hold the last candidate).
        Reads the device counters: the batch's only synchronise.  IndexError
        for an edge id outside the sampler's edge list."""
        fell, bad = (int(v) for v in self.stats.tolist())
        if bad:
            raise IndexError(f"EdgeBatch: {bad} edge id(s) outside the sampler's edge list")
        return fell

    def relabel(self):
        """(node_ids, a_local, b_local): the batch's distinct node ids,
        ascending (the seeds to hand to NeighborSampler), and a_idx / b_idx as
        positions in node_ids -- the indices into the encoder's seed rows.  A
        composed torch.unique: it runs once per batch, beside the encoder's
        own sampling."""
        P = int(self.a_idx.numel())
        ids, inv = torch.unique(torch.cat([self.a_idx, self.b_idx.reshape(-1)]), sorted=True, return_inverse=True)
        inv = inv.to(torch.int32)
        return ids, inv[:P].contiguous(), inv[P:].reshape(self.b_idx.shape).contiguous()


class NegativeSampler:
    """Positive edges with Q uniformly drawn corrupted sources each, on the device.

    A negative of the positive (s -> d) is a pair (s' -> d): s' uniform over
    the nodes, redrawn (at most max_tries times) while it is d itself
    (no_self) or a source of one of d's input edges (reject_edges).  The
    draw is keyed on (seed, epoch, the positive's input edge id, q) only
    (kgx_negative_edges; the epoch enters as in epoch_seed), so a positive
    draws the same negatives in every batch, at every position, on every
    device.  The CSR by destination is built once, through the layers' graph
    cache; its rows are sorted ascending once, here, with one composed
    torch.sort of row * num_nodes + col keys -- per graph, not per batch."""

    def __init__(self, edge_index, num_nodes: int, num_negatives: int, seed: int = 0, reject_edges: bool = True,
                 no_self: bool = True, max_tries: int = 8) -> None:
        self.num_nodes = int(num_nodes)
        self.num_negatives = int(num_negatives)
        if self.num_nodes < 1 or self.num_negatives < 1:
            raise ValueError("NegativeSampler needs num_nodes >= 1 and num_negatives >= 1")
        if not 1 <= int(max_tries) <= 64:
            raise ValueError(f"max_tries must lie in 1..64, got {max_tries}")
        self.seed = int(seed)
        self.reject_edges, self.no_self, self.max_tries = bool(reject_edges), bool(no_self), int(max_tries)
        self._edge_index = edge_index  # the graph cache is keyed on the caller's object
        ei = edge_index_tensor(edge_index, None, allow_transpose=True)
        self.src, self.dst = ei[0].contiguous(), ei[1].contiguous()
        g = self.graph = graph_for(edge_index, ei, self.num_nodes, self.num_nodes)
        if g.kept:
            from .graph import row_of_slot

            keys = row_of_slot(g).long() * self.num_nodes + g.col.long()
            self.col_sorted = (torch.sort(keys).values % self.num_nodes).to(torch.int32)
        else:
            self.col_sorted = torch.zeros(1, dtype=torch.int32, device=g.device)

    @property
    def device(self) -> torch.device:
        return self.graph.device

    def sample(self, edge_ids, epoch: int = 0) -> EdgeBatch:
        """The positives `edge_ids` (input edge ids) with their negatives.  No
        synchronise: an id outside the edge list gets a_idx = -1 and all-(-1)
        b_idx (edge_dot scores them NaN) and is reported by fallbacks()."""
        dev = self.device
        ids = _seed_tensor(edge_ids, dev)
        P, Q, E = int(ids.numel()), self.num_negatives, int(self.src.numel())
        b_idx = torch.empty((P, 1 + Q), dtype=torch.int32, device=dev)
        if E:
            ok = (ids >= 0) & (ids < E)
            safe = ids.clamp(0, E - 1).long()
            a_idx = torch.where(ok, self.dst[safe], -1)
            b_idx[:, 0] = torch.where(ok, self.src[safe], -1)
        else:
            a_idx = torch.full((P,), -1, dtype=torch.int32, device=dev)
            b_idx[:, 0] = -1
        _, stats = negative_edges(self.graph.rowptr, self.col_sorted, self.num_nodes, self.num_nodes, a_idx, ids, Q,
                                  epoch_seed(self.seed, epoch), max_tries=self.max_tries, no_self=self.no_self,
                                  reject_edges=self.reject_edges, out=b_idx[:, 1:])
        labels = torch.zeros((P, 1 + Q), dtype=torch.float32, device=dev)
        labels[:, 0] = 1.0
        return EdgeBatch(a_idx=a_idx, b_idx=b_idx, labels=labels, edge_ids=ids, stats=stats)
