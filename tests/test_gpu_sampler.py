"""The GPU neighbour sampler against its numpy restatement (GPU).

kgx_sample_neighbors / kgx_relabel_frontier / NeighborSampler produce integers
that are a pure function of their arguments, so every check here is exact
equality against tests/sampling_ref.py (itself checked on the CPU by
tests/test_sampler_host.py); the two layer checks at the end run existing
layers on the sampled subgraph.
"""

import numpy as np
import pytest
import torch

import keras_geometric_amd as kgx
import sampling_ref as SR
from keras_geometric_amd import graph as G
from keras_geometric_amd import sampling, synthetic

pytestmark = pytest.mark.gpu
T = torch.from_numpy


def _np(t):
    return t.detach().cpu().numpy()


def _csr(ei: np.ndarray, n: int, dev):
    e = T(ei.astype(np.int32)).to(dev)
    return G.build_csr(e[0].contiguous(), e[1].contiguous(), n, n)


def _one_hop(dev, g, csr_ref, seeds, k, seed, hop=0):
    rowptr, src, eid = sampling.sample_neighbors(g, T(np.asarray(seeds, np.int32)).to(dev), k, seed, hop)
    r_rowptr, r_src, r_eid = SR.sample_hop(csr_ref, seeds, k, seed, hop)
    assert np.array_equal(_np(rowptr), r_rowptr)
    assert np.array_equal(_np(src), r_src)
    assert np.array_equal(_np(eid), r_eid)
    return _np(rowptr), _np(src), _np(eid)


# ---------------------------------------------------------------------------
# one hop
# ---------------------------------------------------------------------------
BOUNDARY_N = 40
# row -> in-degree: 0, 1, 2 (k = 1: half width 1, superset 4), k and k + 1 for k in {1, 3, 10},
# 8 and 9 (a power of two and one above it)
BOUNDARY_DEG = {0: 0, 1: 1, 2: 2, 3: 3, 4: 4, 5: 8, 6: 9, 7: 10, 8: 11, 9: 5, 10: 6}


def _boundary_graph():
    rng = np.random.default_rng(7)
    src, dst = [], []
    for r, d in BOUNDARY_DEG.items():
        s = rng.permutation(np.arange(11, BOUNDARY_N))[:d]  # distinct sources, none of them a listed row
        if r == 9:
            s[2] = 9  # a self loop
        if r == 10:
            s[4] = s[1]  # a duplicated edge
        src += s.tolist()
        dst += [r] * d
    order = rng.permutation(len(src))  # input order is not CSR order: eid != slot
    return np.stack([np.array(src)[order], np.array(dst)[order]]).astype(np.int32)


@pytest.mark.parametrize("k", [1, 3, 10, -1])
def test_one_hop_boundaries(dev, k):
    ei = _boundary_graph()
    g = _csr(ei, BOUNDARY_N, dev)
    csr_ref = SR.build_csr(ei, BOUNDARY_N)
    assert np.array_equal(_np(g.rowptr), csr_ref[0]) and np.array_equal(_np(g.col), csr_ref[1])
    assert np.array_equal(_np(g.eid), csr_ref[2])
    seeds = np.random.default_rng(k + 5).permutation(BOUNDARY_N)  # every row, in no particular order
    rowptr, src, eid = _one_hop(dev, g, csr_ref, seeds, k, seed=99)
    r_rowptr, col, ceid = csr_ref
    for i, r in enumerate(seeds):
        b, d = r_rowptr[r], r_rowptr[r + 1] - r_rowptr[r]
        s, e = src[rowptr[i]: rowptr[i + 1]], eid[rowptr[i]: rowptr[i + 1]]
        assert len(e) == (d if k < 0 else min(d, k))
        assert len(set(e.tolist())) == len(e), "a CSR slot drawn twice"  # eid names the slot
        assert (ei[1][e] == r).all() and (ei[0][e] == s).all(), "not a slot of this row"
        if k < 0 or d <= k:  # taken whole, in CSR order
            assert np.array_equal(s, col[b: b + d]) and np.array_equal(e, ceid[b: b + d])
    # the duplicated edge has two slots, each drawn at most once; both are drawn when the row is taken whole
    if k < 0 or k >= 6:
        i = int(np.where(seeds == 10)[0][0])
        s = src[rowptr[i]: rowptr[i + 1]]
        assert len(s) - len(set(s.tolist())) == 1


def test_one_hub_row(dev):
    """One row of degree 70 001 (> 2^16: half width 9) among 100 ordinary rows."""
    n, hub_deg = 101, 70_001
    rng = np.random.default_rng(3)
    src = np.concatenate([rng.integers(0, n, hub_deg), rng.integers(0, n, 400)])
    dst = np.concatenate([np.full(hub_deg, 17), rng.integers(0, n, 400)])
    order = rng.permutation(len(src))
    ei = np.stack([src[order], dst[order]]).astype(np.int32)
    g = _csr(ei, n, dev)
    csr_ref = SR.build_csr(ei, n)
    assert csr_ref[0][18] - csr_ref[0][17] >= hub_deg
    rowptr, src_s, eid_s = _one_hop(dev, g, csr_ref, np.arange(n), 10, seed=1234)
    hub = eid_s[rowptr[17]: rowptr[18]]
    assert len(set(hub.tolist())) == 10 and (ei[1][hub] == 17).all()


# ---------------------------------------------------------------------------
# R-MAT: the whole sampler
# ---------------------------------------------------------------------------
RN, RE = 2000, 20000


@pytest.fixture(scope="module")
def rmat(dev):
    ei_d = synthetic.rmat_edge_index(RN, RE, seed=5, device=dev)
    ei = _np(ei_d)
    csr_ref = SR.build_csr(ei, RN)
    deg = np.diff(csr_ref[0])
    rng = np.random.default_rng(11)
    zero = np.where(deg == 0)[0]
    assert len(zero) >= 8 and (deg > 5).sum() >= 50
    rest = rng.permutation(np.setdiff1d(np.arange(RN), zero[:8]))[: 257 - 8]
    seeds = rng.permutation(np.concatenate([zero[:8], rest])).astype(np.int32)  # 257: not a multiple of 64
    return {"ei_d": ei_d, "ei": ei, "csr": csr_ref, "deg": deg, "seeds": seeds}


def _assert_subgraph(sub, ref):
    assert np.array_equal(_np(sub.node_ids), ref["node_ids"])
    assert np.array_equal(_np(sub.edge_index), ref["edge_index"])
    assert np.array_equal(_np(sub.edge_ids), ref["edge_ids"])
    assert sub.n_seeds == ref["n_seeds"] and list(sub.hop_node_counts) == list(ref["hop_node_counts"])
    assert sub.node_ids.dtype == sub.edge_index.dtype == sub.edge_ids.dtype == torch.int32


@pytest.mark.parametrize("fanouts", [[5, 3], [-1]])
@pytest.mark.parametrize("n_seeds", [257, 1])
def test_rmat_subgraph_equals_restatement(dev, rmat, fanouts, n_seeds):
    seeds = rmat["seeds"][:n_seeds]
    if n_seeds == 1:  # one seed whose row is sampled, not taken whole
        seeds = rmat["seeds"][rmat["deg"][rmat["seeds"]] > 5][:1]
    sampler = kgx.NeighborSampler(rmat["ei_d"], RN, fanouts, seed=21)
    sub = sampler.sample(T(seeds).to(dev), epoch=2)
    ref = SR.sample_subgraph(rmat["csr"], seeds, fanouts, seed=21, epoch=2)
    _assert_subgraph(sub, ref)
    assert (sampler._map == -1).all()
    # seeds first, every id once, local ids in range, edges are input edges
    ids = _np(sub.node_ids)
    assert np.array_equal(ids[:n_seeds], seeds) and len(set(ids.tolist())) == len(ids)
    loc, e = _np(sub.edge_index), _np(sub.edge_ids)
    assert np.array_equal(ids[loc[0]], rmat["ei"][0][e]) and np.array_equal(ids[loc[1]], rmat["ei"][1][e])
    # a second call gives identical tensors
    again = sampler.sample(T(seeds).to(dev), epoch=2)
    assert torch.equal(again.node_ids, sub.node_ids) and torch.equal(again.edge_index, sub.edge_index)
    assert torch.equal(again.edge_ids, sub.edge_ids)


def _hop0_rows(sub):
    """{seed id: (its hop-0 sources, edge ids)} of a sampled subgraph."""
    ids, loc, e = _np(sub.node_ids), _np(sub.edge_index), _np(sub.edge_ids)
    out = {}
    for j in np.where(loc[1] < sub.n_seeds)[0]:
        out.setdefault(int(ids[loc[1][j]]), []).append((int(ids[loc[0][j]]), int(e[j])))
    return out


def test_sample_is_independent_of_the_batch_and_changes_with_the_epoch(dev, rmat):
    seeds = rmat["seeds"]
    sampler = kgx.NeighborSampler(rmat["ei_d"], RN, [5], seed=21)
    a = _hop0_rows(sampler.sample(T(seeds[:100].copy()).to(dev)))
    b = _hop0_rows(sampler.sample(T(seeds[60:257][::-1].copy()).to(dev)))  # another batch, other positions
    shared = [int(s) for s in seeds[60:100] if rmat["deg"][s] > 0]
    assert len(shared) >= 20
    for s in shared:
        assert a[s] == b[s], f"node {s} drew different neighbours in two batches"
    c = _hop0_rows(sampler.sample(T(seeds[:100].copy()).to(dev), epoch=1))
    big = [int(s) for s in seeds[:100] if rmat["deg"][s] > 5]
    assert big and any(a[s] != c[s] for s in big), "the epoch does not change the sample"
    for s in (int(s) for s in seeds[:100] if 0 < rmat["deg"][s] <= 5):
        assert a[s] == c[s]  # rows taken whole do not depend on the keys


# ---------------------------------------------------------------------------
# relabel
# ---------------------------------------------------------------------------
def test_relabel_local_ids_and_map_protocol(dev):
    i32 = dict(dtype=torch.int32, device=dev)
    node_map = torch.full((64,), -1, **i32)
    nodes = torch.tensor([5, 9, 2], **i32)
    rowptr = torch.tensor([0, 2, 3, 5], **i32)
    src = torch.tensor([9, 30, 30, 2, 7], **i32)  # 9 and 2 are seeds; 30 is sampled from two seeds
    new, s_l, d_l = sampling.relabel_frontier(nodes, nodes, rowptr, src, node_map)
    assert new.tolist() == [7, 30]  # each once, ascending
    assert s_l.tolist() == [1, 4, 4, 2, 3]  # a source that is another seed gets that seed's index
    assert d_l.tolist() == [0, 0, 1, 2, 2]
    assert (node_map == -1).all()
    r_new, r_s, r_d = SR.relabel([5, 9, 2], [5, 9, 2], _np(rowptr), _np(src))
    assert np.array_equal(_np(new), r_new) and np.array_equal(_np(s_l), r_s) and np.array_equal(_np(d_l), r_d)
    # a later hop: the frontier is the tail of the node list
    nodes2 = torch.tensor([5, 9, 2, 7, 30], **i32)
    frontier2 = nodes2[3:].contiguous()
    rowptr2 = torch.tensor([0, 0, 3], **i32)  # node 7 has no in-edges
    src2 = torch.tensor([63, 5, 0], **i32)
    new2, s2, d2 = sampling.relabel_frontier(nodes2, frontier2, rowptr2, src2, node_map)
    assert new2.tolist() == [0, 63] and s2.tolist() == [6, 0, 5] and d2.tolist() == [4, 4, 4]
    assert (node_map == -1).all()
    # duplicate ids in the node list: reported, and the map is clean again
    with pytest.raises(ValueError, match="duplicate"):
        sampling.relabel_frontier(torch.tensor([5, 9, 5], **i32), nodes, rowptr, src, node_map)
    assert (node_map == -1).all()
    # an id past the map: reported, never used as an index
    with pytest.raises(IndexError):
        sampling.relabel_frontier(nodes, nodes, rowptr, torch.tensor([9, 64, 30, 2, 7], **i32), node_map)
    assert (node_map == -1).all()


def test_sampler_rejects_bad_seeds_and_keeps_its_map_clean(dev, rmat):
    sampler = kgx.NeighborSampler(rmat["ei_d"], RN, [5, 3], seed=1)
    good = rmat["seeds"][:16]
    with pytest.raises(ValueError, match="duplicate"):
        sampler.sample(np.concatenate([good, good[3:4]]))
    assert (sampler._map == -1).all()
    for bad in (RN, -1):
        with pytest.raises(IndexError):
            sampler.sample(np.concatenate([good, [bad]]).astype(np.int32))
        assert (sampler._map == -1).all()
    ref = SR.sample_subgraph(rmat["csr"], good, [5, 3], seed=1)
    _assert_subgraph(sampler.sample(good), ref)  # still usable
    empty = sampler.sample(np.zeros(0, np.int32))
    assert empty.node_ids.numel() == 0 and tuple(empty.edge_index.shape) == (2, 0) and empty.hop_node_counts == [0]


# ---------------------------------------------------------------------------
# the layers on a sampled subgraph
# ---------------------------------------------------------------------------
def test_full_fanout_matches_the_full_graph_at_the_seeds(dev, rmat):
    """fanouts = [-1]: every seed keeps all its in-edges in CSR order, so an
    exact sum over the subgraph is the full graph's sum at the seed rows, bit
    for bit; SAGEConv(mean) within the project's fp32 bar (1e-5 scaled)."""
    seeds = T(rmat["seeds"]).to(dev)
    sub = kgx.NeighborSampler(rmat["ei_d"], RN, [-1], seed=0).sample(seeds)
    x = T(np.random.default_rng(2).standard_normal((RN, 36)).astype(np.float32)).to(dev)
    xs = sub.gather(x)
    assert torch.equal(xs, x[sub.node_ids.long()])
    mp = kgx.MessagePassing(aggregator="sum", exact=True)
    full = mp([x, rmat["ei_d"]])[seeds.long()]
    part = mp([xs, sub.edge_index])[: sub.n_seeds]
    assert torch.equal(part, full), "exact sum over the sampled subgraph is not bit-identical"
    torch.manual_seed(0)
    sage = kgx.SAGEConv(20, aggregator="mean")
    ref = sage([x, rmat["ei_d"]])[seeds.long()]
    got = sage([xs, sub.edge_index])[: sub.n_seeds]
    err = ((got - ref).abs() / ref.abs().clamp_min(1.0)).max().item()
    print(f"SAGEConv(mean) subgraph vs full graph at the seeds: max scaled err {err:.3e}")
    assert err <= 1e-5


def test_training_step_on_a_sampled_subgraph(dev, rmat):
    """SAGEConv forward + backward on a [5, 3] subgraph: finite gradients of the
    right shapes, equal to those from the restatement's subgraph."""
    seeds = rmat["seeds"]
    sub = kgx.NeighborSampler(rmat["ei_d"], RN, [5, 3], seed=4).sample(T(seeds).to(dev), epoch=1)
    ref = SR.sample_subgraph(rmat["csr"], seeds, [5, 3], seed=4, epoch=1)
    x = T(np.random.default_rng(9).standard_normal((RN, 36)).astype(np.float32)).to(dev)
    gout = T(np.random.default_rng(10).standard_normal((len(seeds), 20)).astype(np.float32)).to(dev)
    torch.manual_seed(0)
    layer = kgx.SAGEConv(20, aggregator="mean")

    def step(node_ids, edge_index):
        for w in layer.weights:
            w.grad = None
        xs = x[node_ids.long()].clone().requires_grad_(True)
        y = layer([xs, edge_index])[: len(seeds)]
        y.backward(gout)
        return y.detach(), xs.grad, [w.grad.clone() for w in layer.weights]

    y, gx, gw = step(sub.node_ids, sub.edge_index)
    yr, gxr, gwr = step(T(ref["node_ids"]).to(dev), T(ref["edge_index"]).to(dev))
    assert gx.shape == (sub.node_ids.numel(), 36) and torch.isfinite(gx).all() and gx.abs().sum() > 0
    assert [tuple(g.shape) for g in gw] == [tuple(w.shape) for w in layer.weights]
    assert all(torch.isfinite(g).all() and g.abs().sum() > 0 for g in gw)
    assert torch.equal(y, yr) and torch.equal(gx, gxr)
    for a, b in zip(gw, gwr):
        assert torch.equal(a, b)
