"""Sampled blocks on the device (GPU): kgx_block_csr, NeighborSampler.sample_blocks
and SAGEConv on a Block.

kgx_block_csr's outputs are integers and a pure function of its inputs, so
they are compared for equality with two oracles: tests/blocks_ref.py (checked
on the CPU by tests/test_blocks_host.py) and the arrays the existing graph
build makes of the same edges, graph.transpose(graph.build_csr(...)).  The
layer checks run one model over the blocks and over the merged subgraph.
"""

import ctypes

import numpy as np
import pytest
import torch

import blocks_ref as BR
import keras_geometric_amd as kgx
import sampling_ref as SR
from keras_geometric_amd import _native as nat
from keras_geometric_amd import graph as G
from keras_geometric_amd import ops as kops
from keras_geometric_amd import sampling, synthetic

pytestmark = pytest.mark.gpu
T = torch.from_numpy
RN, RE = 2000, 20000
FANOUTS = [[5, 3], [4, 3, 2], [-1, 2], [3]]
SENTINEL = -7


def _np(t):
    return t.detach().cpu().numpy()


def _scaled(a, b):
    return ((a - b).abs() / b.abs().clamp_min(1.0)).max().item() if b.numel() else 0.0


@pytest.fixture(scope="module")
def rmat(dev):
    """The fixture shape of test_gpu_sampler.py: R-MAT 2000 / 20000, 257 seeds, 8 of them without in-edges."""
    ei_d = synthetic.rmat_edge_index(RN, RE, seed=5, device=dev)
    ei = _np(ei_d)
    csr_ref = SR.build_csr(ei, RN)
    deg = np.diff(csr_ref[0])
    rng = np.random.default_rng(11)
    zero = np.where(deg == 0)[0]
    assert len(zero) >= 8 and (deg > 5).sum() >= 50
    rest = rng.permutation(np.setdiff1d(np.arange(RN), zero[:8]))[: 257 - 8]
    seeds = rng.permutation(np.concatenate([zero[:8], rest])).astype(np.int32)  # 257: not a multiple of 64
    return {"ei_d": ei_d, "ei": ei, "csr": csr_ref, "deg": deg, "seeds": seeds, "zero": zero.astype(np.int32)}


# ---------------------------------------------------------------------------
# kgx_block_csr at op level
# ---------------------------------------------------------------------------
class _Buffers:
    """Caller-side arrays of one kgx_block_csr call, pre-filled with a sentinel."""

    def __init__(self, dev, E, n_src, n_dst):
        full = lambda n: torch.full((max(n, 1),), SENTINEL, dtype=torch.int32, device=dev)  # noqa: E731
        self.E, self.n_src, self.n_dst = E, n_src, n_dst
        self.rowptr, self.deg = full(n_dst + 1), full(n_dst)
        self.t_rowptr, self.t_deg, self.t_col, self.t_eid = full(n_src + 1), full(n_src), full(E), full(E)
        nbytes = ctypes.c_size_t(0)
        assert nat.lib().kgx_block_workspace_bytes(E, n_src, ctypes.byref(nbytes)) == 0
        self.ws = torch.empty(max(nbytes.value, 1), dtype=torch.uint8, device=dev)

    def call(self, src, dst):
        info = (ctypes.c_int64 * 4)()
        rc = nat.lib().kgx_block_csr(nat.ptr(src), nat.ptr(dst), self.E, self.n_src, self.n_dst, nat.ptr(self.rowptr),
                                     nat.ptr(self.deg), nat.ptr(self.t_rowptr), nat.ptr(self.t_deg),
                                     nat.ptr(self.t_col), nat.ptr(self.t_eid), nat.ptr(self.ws), self.ws.numel(), info,
                                     nat.stream(src.device))
        return rc, list(info)

    def arrays(self):
        return [_np(self.rowptr[: self.n_dst + 1]), _np(self.deg[: self.n_dst]), _np(self.t_rowptr[: self.n_src + 1]),
                _np(self.t_deg[: self.n_src]), _np(self.t_col[: self.E]), _np(self.t_eid[: self.E])]

    def untouched(self):
        return all((t == SENTINEL).all() for t in (self.rowptr, self.deg, self.t_rowptr, self.t_deg, self.t_col,
                                                   self.t_eid))


def _check_block_csr(dev, src, dst, n_src, n_dst):
    """All six arrays of kgx_block_csr(src, dst) against both oracles; returns info."""
    src, dst = np.asarray(src, np.int32), np.asarray(dst, np.int32)
    E = len(src)
    s_d, d_d = T(src).to(dev), T(dst).to(dev)
    buf = _Buffers(dev, E, n_src, n_dst)
    rc, info = buf.call(s_d, d_d)
    assert rc == 0, nat.lib().kgx_last_error()
    got = buf.arrays()
    names = ["rowptr", "deg", "t_rowptr", "t_deg", "t_col", "t_eid"]
    ref = [*BR.forward_csr(dst, n_dst), *BR.transposed_csr(src, dst, n_src)]
    for name, a, b in zip(names, got, ref):
        assert a.dtype == np.int32 and np.array_equal(a, b), f"{name} differs from blocks_ref"
    g = G.build_csr(s_d, d_d, n_src, n_dst)
    t = G.transpose(g)
    assert np.array_equal(_np(g.col), src) and np.array_equal(_np(g.eid), np.arange(E))  # the edge list is the CSR
    built = [g.rowptr, g.deg, t.rowptr, t.deg, t.col, t.eid]
    for name, a, b in zip(names, got, built):
        assert np.array_equal(a, _np(b)), f"{name} differs from graph.transpose(graph.build_csr(...))"
    assert info == [int(ref[1].max()) if n_dst else 0, int(ref[3].max()) if n_src else 0, 0, 0]
    # the wrapper the sampler uses returns the same arrays
    (rowptr, deg), tt, maxes = sampling.block_csr(s_d, d_d, n_src, n_dst)
    for a, b in zip(got, [rowptr, deg, *tt]):
        assert np.array_equal(a, _np(b))
    assert list(maxes) == info[:2]
    (none_a, none_b), tt2, _ = sampling.block_csr(s_d, d_d, n_src, n_dst, forward=False)
    assert none_a is None and none_b is None and all(torch.equal(a, b) for a, b in zip(tt, tt2))
    return info


@pytest.mark.parametrize("fanouts", FANOUTS)
def test_block_csr_on_sampled_blocks(dev, rmat, fanouts):
    sub = SR.sample_subgraph(rmat["csr"], rmat["seeds"], fanouts, seed=21, epoch=2)
    src, dst = sub["edge_index"]
    bounds = BR.block_bounds(sub, len(fanouts))
    assert bounds[0][2] == len(src) > 0 and bounds[0][0] != bounds[0][1]  # n_src != n_dst
    for n_src, n_dst, e in bounds:
        _check_block_csr(dev, src[:e], dst[:e], n_src, n_dst)
    assert (np.bincount(dst, minlength=bounds[0][1]) == 0).sum() >= 8  # rows of degree 0 were covered


def test_block_csr_small_shapes(dev):
    z = np.zeros(0, np.int32)
    assert _check_block_csr(dev, z, z, 5, 3) == [0, 0, 0, 0]        # E = 0
    assert _check_block_csr(dev, z, z, 0, 0) == [0, 0, 0, 0]        # nothing at all
    src = np.array([6, 2, 2, 0, 5, 2, 6], np.int32)                  # n_dst = 1; sources 1, 3, 4 have no edge
    assert _check_block_csr(dev, src, np.zeros(7, np.int32), 7, 1) == [7, 3, 0, 0]
    rng = np.random.default_rng(1)                                    # more than one workgroup of edges and rows
    dst = np.sort(rng.integers(0, 300, 3001)).astype(np.int32)
    assert _check_block_csr(dev, rng.integers(0, 1025, 3001).astype(np.int32), dst, 1025, 300)[2:] == [0, 0]


def test_block_csr_errors_write_nothing_and_leave_the_buffers_usable(dev):
    rng = np.random.default_rng(2)
    E, n_src, n_dst = 700, 90, 40
    src = rng.integers(0, n_src, E).astype(np.int32)
    dst = np.sort(rng.integers(0, n_dst, E)).astype(np.int32)
    buf = _Buffers(dev, E, n_src, n_dst)
    unsorted = dst.copy()
    unsorted[[100, 500]] = unsorted[[500, 100]]
    assert unsorted[100] > unsorted[101]
    rc, info = buf.call(T(src).to(dev), T(unsorted).to(dev))
    assert rc == nat.KGX_ERR_ARG and info[2] >= 1 and info[3] == 0 and b"sorted" in nat.lib().kgx_last_error()
    assert buf.untouched()
    for bad_src, bad_dst in ((n_src, None), (-1, None), (None, n_dst)):
        s, d = src.copy(), dst.copy()
        if bad_src is not None:
            s[333] = bad_src
        if bad_dst is not None:
            d[-1] = bad_dst  # still sorted
        rc, info = buf.call(T(s).to(dev), T(d).to(dev))
        assert rc == nat.KGX_ERR_INDEX and info[2:] == [0, 1], (rc, info)
        assert buf.untouched()
    with pytest.raises(ValueError, match="sorted"):
        sampling.block_csr(T(src).to(dev), T(unsorted).to(dev), n_src, n_dst)
    with pytest.raises(IndexError):
        sampling.block_csr(T(src).to(dev), T(dst).to(dev), int(src.max()), n_dst)  # the largest id is one too large
    rc, info = buf.call(T(src).to(dev), T(dst).to(dev))  # a good call on the same buffers
    assert rc == 0 and info[2:] == [0, 0]
    ref = [*BR.forward_csr(dst, n_dst), *BR.transposed_csr(src, dst, n_src)]
    for a, b in zip(buf.arrays(), ref):
        assert np.array_equal(a, b)


# ---------------------------------------------------------------------------
# sample_blocks
# ---------------------------------------------------------------------------
def _block_tensors(blocks):
    out = [blocks.node_ids]
    for b in blocks:
        t = b.graph.extras["T"]
        out += [b.edge_index, b.edge_ids, b.graph.rowptr, b.graph.col, b.graph.eid, b.graph.deg,
                t.rowptr, t.col, t.eid, t.deg, t.extras["fwd_slot"]]
    return out


def _assert_blocks(sampler, blocks, sub, ref, n_layers):
    assert torch.equal(blocks.node_ids, sub.node_ids) and blocks.n_seeds == sub.n_seeds
    assert list(blocks.hop_node_counts) == list(sub.hop_node_counts) == list(ref["hop_node_counts"])
    assert len(blocks) == n_layers == len(list(blocks))
    bounds = BR.block_bounds(ref, n_layers)
    for layer, (blk, (n_src, n_dst, e)) in enumerate(zip(blocks, bounds)):
        assert (blk.n_src, blk.n_dst, blk.edge_index.shape[1]) == (n_src, n_dst, e)
        assert torch.equal(blk.edge_index, sub.edge_index[:, :e]) and torch.equal(blk.edge_ids, sub.edge_ids[:e])
        assert blk.edge_index.dtype == blk.edge_ids.dtype == torch.int32
        if layer + 1 < n_layers:
            assert blk.n_dst == blocks[layer + 1].n_src
        g, t = blk.graph, blk.graph.extras["T"]
        assert (g.n_src, g.n_dst, g.kept, g.n_input_edges, g.flags, g.w) == (n_src, n_dst, e, e, 0, None)
        assert (t.n_src, t.n_dst, t.kept) == (n_dst, n_src, e)
        src, dst = ref["edge_index"][0][:e], ref["edge_index"][1][:e]
        want = [*BR.forward_csr(dst, n_dst), *BR.transposed_csr(src, dst, n_src)]
        for a, b in zip([g.rowptr, g.deg, t.rowptr, t.deg, t.col, t.eid], want):
            assert a.dtype == torch.int32 and np.array_equal(_np(a), b)
        assert np.array_equal(_np(g.col), src) and np.array_equal(_np(g.eid), np.arange(e))
        assert torch.equal(t.extras["fwd_slot"], t.eid.long())
        assert g.max_degree == (int(want[1].max()) if n_dst else 0)
        assert t.max_degree == (int(want[3].max()) if n_src else 0)
        # prefix views of one shared set of arrays
        g0 = blocks[0].graph
        assert g.rowptr.data_ptr() == g0.rowptr.data_ptr() and g.col.data_ptr() == g0.col.data_ptr()
        assert g.deg.data_ptr() == g0.deg.data_ptr() and blk.edge_index.data_ptr() == blocks[0].edge_index.data_ptr()
    assert blocks[-1].n_dst == blocks.n_seeds
    assert (sampler._map == -1).all()


@pytest.mark.parametrize("fanouts", FANOUTS)
def test_sample_blocks_is_the_sample_cut_into_blocks(dev, rmat, fanouts):
    seeds = T(rmat["seeds"]).to(dev)
    sampler = kgx.NeighborSampler(rmat["ei_d"], RN, fanouts, seed=21)
    sub = sampler.sample(seeds, epoch=2)
    blocks = sampler.sample_blocks(seeds, epoch=2)
    assert isinstance(blocks, kgx.SampledBlocks) and isinstance(blocks[0], kgx.Block)
    ref = SR.sample_subgraph(rmat["csr"], rmat["seeds"], fanouts, seed=21, epoch=2)
    _assert_blocks(sampler, blocks, sub, ref, len(fanouts))
    again = sampler.sample_blocks(seeds, epoch=2)
    for a, b in zip(_block_tensors(blocks), _block_tensors(again)):
        assert torch.equal(a, b)
    x = T(np.random.default_rng(2).standard_normal((RN, 12)).astype(np.float32)).to(dev)
    assert torch.equal(blocks.gather(x), x[sub.node_ids.long()])


def test_sample_blocks_small_batches(dev, rmat):
    sampler = kgx.NeighborSampler(rmat["ei_d"], RN, [5, 3], seed=21)
    one = rmat["seeds"][rmat["deg"][rmat["seeds"]] > 5][:1]
    for seeds in (one, rmat["zero"][:8], np.zeros(0, np.int32)):
        sub = sampler.sample(seeds, epoch=2)
        blocks = sampler.sample_blocks(seeds, epoch=2)
        ref = SR.sample_subgraph(rmat["csr"], seeds, [5, 3], seed=21, epoch=2)
        _assert_blocks(sampler, blocks, sub, ref, 2)
    # zero-degree seeds: hop 1 never ran and there are still two blocks, both without edges
    blocks = sampler.sample_blocks(rmat["zero"][:8])
    assert [(b.n_src, b.n_dst, b.edge_index.shape[1]) for b in blocks] == [(8, 8, 0), (8, 8, 0)]
    torch.manual_seed(0)
    layer = kgx.SAGEConv(6, aggregator="mean")
    h = T(np.random.default_rng(3).standard_normal((8, 10)).astype(np.float32)).to(dev)
    out = layer([h, blocks[0]])
    assert torch.equal(out, layer([h, blocks[0].edge_index]))  # no edges: the self term alone


# ---------------------------------------------------------------------------
# aggregation over a block: bit identity with the merged subgraph
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def batch(dev, rmat):
    """One [5, 3] sample as a merged subgraph and as blocks, and features for it."""
    seeds = T(rmat["seeds"]).to(dev)
    sampler = kgx.NeighborSampler(rmat["ei_d"], RN, [5, 3], seed=4)
    sub = sampler.sample(seeds, epoch=1)
    blocks = sampler.sample_blocks(seeds, epoch=1)
    rng = np.random.default_rng(9)
    x = {f: T(rng.standard_normal((sub.node_ids.numel(), f)).astype(np.float32)).to(dev) for f in (36, 128)}
    gout = {f: T(rng.standard_normal((len(seeds), f)).astype(np.float32)).to(dev) for f in (12,)}
    return {"sub": sub, "blocks": blocks, "x": x, "gout": gout, "n_sub": int(sub.node_ids.numel())}


def test_exact_sum_over_a_block_is_bit_identical_to_the_merged_graph(dev, batch):
    """Same CSR order, one chain per row: forward and gradient agree bit for bit
    (a merged transposed row only appends the zero gradients of later hops' edges)."""
    sub, n_sub = batch["sub"], batch["n_sub"]
    gm = G.build_csr(sub.edge_index[0].contiguous(), sub.edge_index[1].contiguous(), n_sub, n_sub)
    x = batch["x"][36]
    for blk in batch["blocks"]:
        gout = T(np.random.default_rng(blk.n_dst).standard_normal((blk.n_dst, 36)).astype(np.float32)).to(dev)
        xb = x[: blk.n_src].clone().requires_grad_(True)
        yb = kops.aggregate(blk.graph, xb, "sum", exact=True)
        yb.backward(gout)
        xm = x.clone().requires_grad_(True)
        ym = kops.aggregate(gm, xm, "sum", exact=True)[: blk.n_dst]
        ym.backward(gout)
        assert yb.shape == (blk.n_dst, 36) and torch.equal(yb.detach(), ym.detach())
        assert torch.equal(xb.grad, xm.grad[: blk.n_src]) and xb.grad.abs().sum() > 0
        assert not xm.grad[blk.n_src:].any()


def test_star_block_backward_takes_the_split_path(dev):
    """One source feeding 600 sampled destinations: its transposed row is longer
    than the smallest hub chunk (256), so the backward schedule splits it."""
    n_leaf, hub = 600, 600
    leaves = np.arange(n_leaf)
    src = np.concatenate([np.full(n_leaf, hub), 601 + leaves % 5])
    ei = np.stack([src, np.concatenate([leaves, leaves])]).astype(np.int32)
    sampler = kgx.NeighborSampler(T(ei).to(dev), 606, [2], seed=0)
    blocks = sampler.sample_blocks(leaves.astype(np.int32))
    (blk,) = blocks
    assert (blk.n_src, blk.n_dst, blk.edge_index.shape[1]) == (606, 600, 1200)
    s, d = _np(blk.edge_index)
    info = _check_block_csr(dev, s, d, blk.n_src, blk.n_dst)
    assert info[:2] == [2, 600]
    t = blk.graph.extras["T"]
    assert t.split_len == 256 and t.n_split >= 1 and t.max_degree == 600
    # small integers: every partial sum is exact in fp32, so the chunked reduction must give
    # the float64 result exactly, in whatever order the chunks are folded
    rng = np.random.default_rng(6)
    x = T(rng.integers(-8, 9, (606, 36)).astype(np.float32)).to(dev).requires_grad_(True)
    gout = T(rng.integers(-8, 9, (600, 36)).astype(np.float32)).to(dev)
    y = kops.aggregate(blk.graph, x, "sum")  # scheduled, not exact: the split row reduces in chunks
    y.backward(gout)
    s, d = T(s).long(), T(d).long()
    y_ref = torch.zeros((600, 36), dtype=torch.float64).index_add_(0, d, x.detach().cpu().double()[s])
    g_ref = torch.zeros((606, 36), dtype=torch.float64).index_add_(0, s, gout.cpu().double()[d])
    assert torch.equal(y.detach().cpu().double(), y_ref)
    assert torch.equal(x.grad.cpu().double(), g_ref) and g_ref[hub].abs().max() > 8


# ---------------------------------------------------------------------------
# SAGEConv over blocks against SAGEConv over the merged subgraph
# ---------------------------------------------------------------------------
def _two_layers(f_hidden, f_out, **kw):
    torch.manual_seed(0)
    return [kgx.SAGEConv(f_hidden, **kw), kgx.SAGEConv(f_out, **kw)]


def _run(layers, x, batch, over_blocks, gout=None, training=None):
    for layer in layers:
        for w in layer.weights:
            w.grad = None
    xs = x.clone().requires_grad_(gout is not None)
    h = xs
    kw = {} if training is None else {"training": training}
    if over_blocks:
        for layer, blk in zip(layers, batch["blocks"]):
            h = layer([h, blk], **kw)
    else:
        for layer in layers:
            h = layer([h, batch["sub"].edge_index], **kw)
        h = h[: batch["sub"].n_seeds]
    if gout is None:
        return h.detach(), None, None
    h.backward(gout)
    return h.detach(), xs.grad, [w.grad.clone() for layer in layers for w in layer.weights]


@pytest.mark.parametrize("kw", [
    dict(aggregator="mean"), dict(aggregator="max"), dict(aggregator="pooling"),
    dict(aggregator="mean", root_weight=False), dict(aggregator="mean", normalize=True, activation=None),
], ids=["mean", "max", "pooling", "no-root", "normalize"])
def test_two_layer_sage_over_blocks_matches_the_merged_subgraph(batch, kw):
    """F 36 -> 20 -> 12, same weights: outputs at the seeds, x-gradient rows and
    weight gradients within the project's fp32 bar (1e-5 scaled).

    normalize runs without the relu: relu zeroes some whole rows of 12 outputs,
    and the gradient of the L2 normalisation at an all-zero row is 0 * inf = NaN.
    The merged leg meets such rows among the 410 non-seed rows its second layer
    computes (measured: NaN x-gradient rows in the merged leg, the case's own
    reference), the blocks never compute them."""
    layers = _two_layers(20, 12, **kw)
    x, gout = batch["x"][36], batch["gout"][12]
    y_m, gx_m, gw_m = _run(layers, x, batch, False, gout)
    y_b, gx_b, gw_b = _run(layers, x, batch, True, gout)
    assert y_b.shape == y_m.shape == (batch["sub"].n_seeds, 12) and gx_b.shape == gx_m.shape == x.shape
    errs = {"out": _scaled(y_b, y_m), "dx": _scaled(gx_b, gx_m),
            "dw": max(_scaled(a, b) for a, b in zip(gw_b, gw_m))}
    print(f"SAGEConv {kw} blocks vs merged (max scaled err): {errs}")
    assert len(gw_b) == len(gw_m) and all(a.shape == b.shape for a, b in zip(gw_b, gw_m))
    assert y_m.abs().sum() > 0 and gx_m.abs().sum() > 0 and all(g.abs().sum() > 0 for g in gw_m)
    assert torch.isfinite(gx_b).all() and all(torch.isfinite(g).all() for g in gw_b)
    assert all(e <= 1e-5 for e in errs.values()), errs  # a NaN fails this


def test_training_step_with_message_dropout_over_blocks(batch):
    layers = _two_layers(20, 12, aggregator="mean", dropout_rate=0.3)
    x, gout = batch["x"][36], batch["gout"][12]
    y, gx, gw = _run(layers, x, batch, True, gout, training=True)
    assert y.shape == (batch["sub"].n_seeds, 12) and torch.isfinite(y).all()
    assert gx.shape == x.shape and torch.isfinite(gx).all() and gx.abs().sum() > 0
    weights = [w for layer in layers for w in layer.weights]
    assert [tuple(g.shape) for g in gw] == [tuple(w.shape) for w in weights]
    assert all(torch.isfinite(g).all() and g.abs().sum() > 0 for g in gw)
    y_eval, _, _ = _run(layers, x, batch, True)
    assert not torch.equal(y, y_eval), "training=True dropped nothing"


def test_fused_inference_path_over_blocks(batch, monkeypatch):
    """KGX_FUSED_SAGE=1, F 128 -> 64 -> 12, no gradients: both layers take the
    fused aggregate-transform launch on the block's graph."""
    monkeypatch.setenv("KGX_FUSED_SAGE", "1")
    layers = _two_layers(64, 12, aggregator="mean")
    x = batch["x"][128]
    calls = []
    real = kops.aggregate_transform
    monkeypatch.setattr(kops, "aggregate_transform", lambda g, *a, **k: (calls.append(g), real(g, *a, **k))[1])
    with torch.no_grad():
        y_b, _, _ = _run(layers, x, batch, True)
        assert len(calls) == 2 and all(g is blk.graph for g, blk in zip(calls, batch["blocks"])), \
            "the fused path did not run on the blocks' graphs"
        y_m, _, _ = _run(layers, x, batch, False)
    monkeypatch.setenv("KGX_FUSED_SAGE", "0")
    with torch.no_grad():
        y_two_step, _, _ = _run(layers, x, batch, True)
    e_m, e_t = _scaled(y_b, y_m), _scaled(y_b, y_two_step)
    print(f"fused SAGEConv over blocks: vs merged {e_m:.3e}, vs the two-step path {e_t:.3e}")
    assert y_b.shape == (batch["sub"].n_seeds, 12) and e_m <= 1e-5 and e_t <= 1e-5


def test_block_input_with_a_wrong_row_count_raises(batch):
    layer = kgx.SAGEConv(8, aggregator="mean")
    blk = batch["blocks"][1]
    x = batch["x"][36]
    assert blk.n_src != blk.n_dst
    for rows in (blk.n_dst, blk.n_src + 1):
        with pytest.raises(ValueError, match="n_src"):
            layer([x[:rows], blk])
    assert layer([x[: blk.n_src], blk]).shape == (blk.n_dst, 8)
