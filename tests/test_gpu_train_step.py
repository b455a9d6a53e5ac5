"""The fused training step ("Training step") against float64 on every
row class: the forward that keeps P = PRE(A x) (kgx::spmm_gemm_save, the
agg_out stores of spmm_gemm.hip / spmm_gemm256.hip), the dx pass that reruns
the fused kernel on graph.transpose(g), and dW / db through kgx_gemm_tn.

One graph (train_ref.class_graph, seed 0, 12288 nodes) puts hub rows split
into chunks, main rows, degree 3..7 short rows and the degree <= 2 records
into the schedule of the graph and of its transpose, and is not symmetric.
The reference is tests/train_ref.py: float64 autograd straight from the CSR
arrays.  Every tolerance is 1e-5 * max(1, the same computation on |terms|)
per element (fused_ref.check, tests/test_gpu_gemm_tn.py); selections (max /
min) and one-order sums (rows of degree <= 2) are compared bitwise with an
fp32 restatement.  Failures name the row and its kernel; a dx failure names
the kernel in the transposed schedule.

Before every checked launch the caching allocator's free blocks are filled
with NaN (train_ref.poison): the outputs are torch.empty, and a row no kernel
stores would otherwise show the previous identical call's right answer.

Each step test also guards its path (the tests this module joins had silently
left the fused path): kgx_gemm_tn runs once, and for a sum / mean without the
GIN pre-scale the dx pass is one fused launch over graph.transpose(g),
unsliced.  With the pre-scale, or a max, dx is the unfused
dOut W^T -> aggregation backward by design (ops._AggregateTransformFn).
"""

from types import SimpleNamespace

import numpy as np
import pytest
import torch

import fused_ref
import train_ref
from keras_geometric_amd import _native as nat
from keras_geometric_amd import graph as G
from keras_geometric_amd import ops as kops
from keras_geometric_amd import tiny
from keras_geometric_amd.layers import GCNConv, GINConv

pytestmark = pytest.mark.gpu
T = torch.from_numpy
N = train_ref.CLASS_N
GIN = 1.25  # exact in fp32
KERNELS = {"split", "main", "short", "tiny"}


class World:
    """The module's graph in its build variants, inputs and float64 references,
    each made once."""

    def __init__(self, dev):
        self.dev = dev
        src, dst = train_ref.class_graph(0)
        self.src, self.dst = T(src).to(dev), T(dst).to(dev)
        self._graphs, self._inputs, self._fwd, self._steps = {}, {}, {}, {}

    def graph(self, weighted: bool, split_len=None, F: int = 128):
        """weighted: self loops + GCN norm; else bare edges (degree-0 rows, no weights)."""
        F = 256 if F == 256 else 128  # the chunk-length hint of the build: the 256-wide kernels' or the default
        key = (weighted, split_len, F)
        if key not in self._graphs:
            self._graphs[key] = G.build_csr(self.src, self.dst, N, N, self_loops=weighted, gcn_norm=weighted,
                                            split_len=split_len, n_features=F)
        return self._graphs[key]

    def inputs(self, F: int, Fo: int):
        """x [N, F], W [F, Fo], b [Fo], dOut [N, Fo]: continuous draws (no max / min ties but duplicate edges')."""
        if (F, Fo) not in self._inputs:
            rng = np.random.default_rng(1000 * F + Fo)
            x = rng.standard_normal((N, F)).astype(np.float32)
            W = (rng.standard_normal((F, Fo)) / np.sqrt(F)).astype(np.float32)
            b = rng.standard_normal(Fo).astype(np.float32)
            dOut = rng.standard_normal((N, Fo)).astype(np.float32)
            self._inputs[(F, Fo)] = tuple(T(t).to(self.dev) for t in (x, W, b, dOut))
        return self._inputs[(F, Fo)]

    def forward_ref(self, weighted, F, Fo, red, gin):
        """fused_ref.reference with its aggregate: (y, scale, a, aa).  The CSR arrays
        do not depend on the chunk length, so one reference serves every schedule."""
        key = (weighted, F, Fo, red, gin)
        if key not in self._fwd:
            x, W, b, _ = self.inputs(F, Fo)
            self._fwd[key] = fused_ref.reference(self.graph(weighted, None, F), x, W, red, weighted, b, pre_gin=gin,
                                                 gin_scale=GIN if gin else 1.0, with_agg=True)
        return self._fwd[key]

    def step_ref(self, weighted, F, Fo, red, gin, bias=True):
        key = (weighted, F, Fo, red, gin, bias)
        if key not in self._steps:
            x, W, b, dOut = self.inputs(F, Fo)
            self._steps[key] = train_ref.grads(self.graph(weighted, None, F), x, W, b if bias else None, dOut, red,
                                               weighted, gin, GIN if gin else 1.0)
        return self._steps[key]


@pytest.fixture(scope="module")
def world(dev):
    return World(dev)


def _tn_workspace_floats(F, Fo):
    import ctypes

    nbytes = ctypes.c_size_t(0)
    nat.check(nat.lib().kgx_gemm_tn_workspace_bytes(N, F, Fo, ctypes.byref(nbytes)), "kgx_gemm_tn_workspace_bytes")
    return max(nbytes.value, 4) // 4 + 1


def _poison(g, F, Fo, t=None, side=False):
    """NaN into every cached block that could become out, agg / dx, the hub
    partials (of g and of the transposed graph t), dW, db or kgx_gemm_tn's
    workspace -- in the caller's stream's pool, where every launch of the
    default step allocates, and with side=True also in the side stream's,
    where KGX_TN_OVERLAP=1 allocates dW, db and the workspace (the allocator
    pools per stream; each pool costs a device allocation per shape, so only
    the overlap test pays for the second)."""
    shapes = [(N, Fo), (N, F), (max(g.n_slots, 1), 256 if F == 256 else 128), (F, Fo), (Fo,),
              (_tn_workspace_floats(F, Fo),)]
    if t is not None:
        shapes.append((max(t.n_slots, 1), 256 if Fo == 256 else 128))
    train_ref.poison(g.device, *shapes, streams=(None, kops._side_stream(g.device)) if side else (None,))


def _report(what, **errs):
    print("[train_step] " + what + " " + " ".join(f"{k}={v:.3g}" for k, v in errs.items()))


# ---------------------------------------------------------------------------
# coverage of the schedule classes: asserted, not assumed
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("weighted", [True, False])
@pytest.mark.parametrize("F", [128, 256])
def test_class_graph_reaches_every_kernel(world, weighted, F):
    g = world.graph(weighted, None, F)
    assert g.kept == 73142 + (N if weighted else 0)
    rows = torch.arange(N, device=world.dev)
    for name, gg in (("graph", g), ("transpose", G.transpose(g))):
        own = fused_ref.owners(gg, rows)
        for k in KERNELS:
            assert own.count(k) >= 1, f"{name}: no row on the {k} kernel"
        assert own.count("none") == 0
        assert own.count("split") == 2 and gg.n_split == 2 and gg.split_len == 256
        pack, tw, start, n2 = tiny.tiny_pack(gg)
        assert pack is not None and gg.n_items - start >= tiny._MIN_ROWS
        assert (tw is not None) == weighted  # the transposed records carry the weights assigned after its build
        deg = tiny.records(pack, tw, gg.n_items - start, n2)[0][:, 1]
        # (with self loops the rows of degree 2 are short rows and the tail holds degrees 2 and 1)
        assert set(deg.unique().tolist()) == ({1, 2} if weighted else {0, 1, 2})
    # many split rows for the forward launches with chunks of 16
    g16 = world.graph(weighted, 16, F)
    assert g16.n_split >= 1000 and torch.equal(g16.rowptr, g.rowptr) and torch.equal(g16.col, g.col)
    assert weighted is False or torch.equal(g16.w, g.w)
    assert KERNELS <= set(fused_ref.owners(g16, rows))


# ---------------------------------------------------------------------------
# a / d: the saved aggregate
# ---------------------------------------------------------------------------
def _saving_launch(g, x, W, b, red, weighted, gin, exact):
    """kgx::spmm_gemm_save as _AggregateTransformFn.forward calls it."""
    items, _, split, _, n_slots = g.work(exact)
    w = g.w if weighted else None
    _poison(g, x.shape[1], W.shape[1])
    return torch.ops.kgx.spmm_gemm_save(
        x, g.rowptr, g.rows, items, split, g.col, w, n_slots, kops._reduce_id(red), W, b, bool(gin),
        float(GIN if gin else 1.0), g.n_long if items is not None else -1, *kops._tiny_of(g, items))


def _check_saved(world, g, F, Fo, red, weighted, gin, exact, label):
    x, W, b, _ = world.inputs(F, Fo)
    y64, scale, a, aa = world.forward_ref(weighted, F, Fo, red, gin)
    y, P = _saving_launch(g, x, W, b, red, weighted, gin, exact)
    e_p = train_ref.check_rows(P, g, a, aa, f"{label}: saved P")
    e_y = fused_ref.check(y, g, (y64, scale), f"{label}: y of the saving launch")
    _report(label, P=e_p, y=e_y)
    # selections and one-order sums: the fp32 restatement's bits
    p32, exact_rows = train_ref.aggregate32(g, x, red, weighted, gin, GIN)
    if red in ("max", "min"):
        assert bool(exact_rows.all())
    elif red == "sum":
        assert int(exact_rows.sum()) >= tiny._MIN_ROWS
    bad = torch.nonzero(exact_rows & (P != p32).any(1)).flatten()
    assert bad.numel() == 0, (f"{label}: P differs from the fp32 restatement on {bad.numel()} rows, first "
                              f"{bad[:8].tolist()} on {fused_ref.owners(g, bad[:8])}")
    deg = g.rowptr[1:] - g.rowptr[:-1]
    empty = deg == 0
    if not weighted:
        assert int(empty.sum()) == 686
        want = (torch.tensor(GIN, device=x.device) * x[empty]) if gin else torch.zeros_like(x[empty])
        assert torch.equal(P[empty], want), f"{label}: P of the degree-0 rows"
        if not gin:
            assert torch.equal(y[empty], b.expand(int(empty.sum()), -1)), f"{label}: y of the degree-0 rows != bias"
    # the same launch without the agg_out stores: one stream, unsliced -> the same bits
    _poison(g, F, Fo)
    y0 = kops._aggregate_transform_raw(g, x, W, kops._reduce_id(red), weighted, b, gin, GIN if gin else 1.0, exact,
                                       allow_slice=False)
    bad = torch.nonzero((y != y0).any(1)).flatten()
    assert bad.numel() == 0, (f"{label}: y with and without the saved aggregate differ on {bad.numel()} rows, first "
                              f"{bad[:8].tolist()} on {fused_ref.owners(g, bad[:8])}")
    return y, P


_SAVE_CASES = [(red, weighted, gin, Fo, sched)
               for red in ("sum", "mean", "max", "min") for weighted in (True, False) for gin in (False, True)
               for Fo in (128, 64) for sched in ("default", "split16")]
_SAVE_CASES += [(red, weighted, False, 128, "rows") for red in ("sum", "max") for weighted in (True, False)]


@pytest.mark.parametrize("red,weighted,gin,Fo,sched", _SAVE_CASES)
def test_saved_aggregate_128(world, red, weighted, gin, Fo, sched):
    """P and y of the saving launch at F_in 128 on every row.  Sum rows of degree
    <= 2 are held to bit equality (0 + m0 + m1 in __fadd_rn has one order, the
    kernels' pre-scale is __fmul_rn then __fadd_rn), max / min rows all."""
    g = world.graph(weighted, 16 if sched == "split16" else None)
    _check_saved(world, g, 128, Fo, red, weighted, gin, sched == "rows",
                 f"save128 {red} weighted={weighted} gin={gin} F_out={Fo} {sched}")


@pytest.mark.parametrize("red,weighted,gin", [("sum", True, False), ("sum", False, True), ("max", False, True)])
def test_saved_aggregate_256(world, red, weighted, gin):
    """The 256-wide kernels: the same checks, and agg bit-equal to the unfused
    aggregation (kops.aggregate), whose per-row order they keep."""
    g = world.graph(weighted, None, 256)
    assert kops.fused_transform_supported(256, 256)
    y, P = _check_saved(world, g, 256, 256, red, weighted, gin, False, f"save256 {red} weighted={weighted} gin={gin}")
    x = world.inputs(256, 256)[0]
    with torch.no_grad():
        want = kops.aggregate(g, x, red, weighted=weighted, epilogue=nat.EPI_GIN if gin else nat.EPI_NONE,
                              xroot=x if gin else None, gin_scale=GIN if gin else 1.0)
    bad = torch.nonzero((P != want).any(1)).flatten()
    assert bad.numel() == 0, f"agg != kops.aggregate on rows {bad[:8].tolist()} ({fused_ref.owners(g, bad[:8])})"


# ---------------------------------------------------------------------------
# the whole step through the public op
# ---------------------------------------------------------------------------
class _Spy:
    """Records the calls that tell the paths apart: the public ops a layer
    dispatches to (kops.aggregate_transform / kops.aggregate, with their graph
    and keywords), the saving forward launch (kgx::spmm_gemm_save), and the
    backward's two module globals, looked up by name at call time
    (kops.gemm_tn, with the stream it was issued on, and
    kops._aggregate_transform_raw)."""

    def __init__(self, mp):
        self.tn, self.raw, self.at, self.agg, self.save = [], [], [], [], []
        real_tn, real_raw = kops.gemm_tn, kops._aggregate_transform_raw
        real_at, real_agg, real_save = kops.aggregate_transform, kops.aggregate, torch.ops.kgx.spmm_gemm_save

        def tn(P, D, with_db=False):
            self.tn.append((P, D, torch.cuda.current_stream(P.device)))
            return real_tn(P, D, with_db)

        def raw(g, *a, **kw):
            self.raw.append((g, kw.get("allow_slice", True)))
            return real_raw(g, *a, **kw)

        def at(g, *a, **kw):
            self.at.append((g, kw))
            return real_at(g, *a, **kw)

        def agg(g, *a, **kw):
            self.agg.append((g, kw))
            return real_agg(g, *a, **kw)

        def save(*a, **kw):
            self.save.append(a[0].shape)
            return real_save(*a, **kw)

        mp.setattr(kops, "gemm_tn", tn)
        mp.setattr(kops, "_aggregate_transform_raw", raw)
        mp.setattr(kops, "aggregate_transform", at)
        mp.setattr(kops, "aggregate", agg)
        mp.setattr(torch.ops.kgx, "spmm_gemm_save", save)


def _step(world, monkeypatch, g, F, Fo, red, weighted, gin, need=(True, True, True), bias=True, after=None,
          side=False):
    """One forward + backward of kops.aggregate_transform, poisoned and spied on."""
    x, W, b, dOut = world.inputs(F, Fo)
    with monkeypatch.context() as mp:
        spy = _Spy(mp)
        xg = x.clone().requires_grad_(need[0])
        Wg = W.clone().requires_grad_(need[1])
        bg = b.clone().requires_grad_(need[2]) if bias else None
        t = G.transpose(g)
        _poison(g, F, Fo, t, side)
        y = kops.aggregate_transform(g, xg, Wg, red, weighted=weighted, bias=bg, pre_gin=gin,
                                     gin_scale=GIN if gin else 1.0)
        _poison(g, F, Fo, t, side)
        y.backward(dOut)
        r = SimpleNamespace(y=y.detach(), dx=xg.grad, dW=Wg.grad, db=bg.grad if bias else None, spy=spy,
                            P=spy.tn[0][0] if spy.tn else None, early=after(xg, Wg, bg) if after else None)
    return r


def _guard(r, g, red, gin, F, Fo):
    """The step took the path it claims: one kgx_gemm_tn, and for sum / mean
    without the pre-scale one fused launch over the transposed graph."""
    assert len(r.spy.tn) == 1, f"kgx_gemm_tn ran {len(r.spy.tn)} times"
    assert len(r.spy.save) == 1, f"{len(r.spy.save)} saving forward launches (kgx::spmm_gemm_save)"
    if red in ("sum", "mean") and not gin:
        assert kops.fused_transform_supported(Fo, F), "the dx pass is not fused at this shape"
        assert len(r.spy.raw) == 1, f"{len(r.spy.raw)} fused launches in the backward"
        assert r.spy.raw[0][0] is G.transpose(g), "the dx pass did not run on graph.transpose(g)"
        assert r.spy.raw[0][1] is False, "the dx pass was allowed the sliced schedule"
    else:  # dOut W^T -> aggregation backward (the pre-scale's / max's path by design)
        assert len(r.spy.raw) == 0


def _check_step(world, r, g, F, Fo, red, weighted, gin, label, fused_dx=True, bias=True):
    x, W, b, dOut = world.inputs(F, Fo)
    ref, mag = world.step_ref(weighted, F, Fo, red, gin, bias)
    errs = {"y": fused_ref.check(r.y, g, (ref.y, mag.y), f"{label}: y")}
    if r.P is not None:
        errs["P"] = train_ref.check_rows(r.P, g, ref.P, mag.P, f"{label}: P kept for dW")
    if r.dx is not None:
        # the rows of dx are sources: their kernels are the transposed schedule's (fused dx pass only)
        own = G.transpose(g) if fused_dx else SimpleNamespace(items=None, n_dst=N)
        errs["dx"] = train_ref.check_rows(r.dx, own, ref.dx, mag.dx,
                                          f"{label}: dx ({'transposed schedule' if fused_dx else 'unfused backward'})")
    if r.dW is not None:
        # kgx_gemm_tn's own bound, on the P the kernel kept; then the whole chain: 1e-5 for P + 1e-5 for the product
        P64, D64 = r.P.double(), dOut.double()
        errs["dW|P"] = train_ref.check_dense(r.dW, P64.t() @ D64, P64.abs().t() @ D64.abs(), f"{label}: dW vs P^T dOut")
        errs["dW"] = train_ref.check_dense(r.dW, ref.dW, mag.dW, f"{label}: dW", tol=2e-5)
    if r.db is not None:
        errs["db"] = train_ref.check_dense(r.db, ref.db, mag.db, f"{label}: db")
    _report(label, **errs)


@pytest.mark.parametrize("red,weighted,gin", [("sum", True, False), ("sum", False, False), ("mean", False, False),
                                              ("mean", True, False), ("max", False, True)])
def test_step_128(world, monkeypatch, red, weighted, gin):
    """128 -> 128 with x, W and bias requiring grad: y, P, dx, dW, db.  Sum / mean
    take dx through the fused kernel on the transposed graph; max with the GIN
    pre-scale is GIN's training path (fused forward keeping P, unfused
    kgx_spmm_max_backward)."""
    assert kops.fused_transform_supported(128, 128)
    g = world.graph(weighted)
    r = _step(world, monkeypatch, g, 128, 128, red, weighted, gin)
    _guard(r, g, red, gin, 128, 128)
    _check_step(world, r, g, 128, 128, red, weighted, gin, f"step128 {red} weighted={weighted} gin={gin}",
                fused_dx=not gin)


@pytest.mark.parametrize("weighted,gin", [(True, False), (False, True)])
def test_step_256(world, monkeypatch, weighted, gin):
    """256 -> 256 on the class graph: dx per row against its own |terms| bound."""
    assert kops.fused_transform_supported(256, 256)
    g = world.graph(weighted, None, 256)
    r = _step(world, monkeypatch, g, 256, 256, "sum", weighted, gin)
    _guard(r, g, "sum", gin, 256, 256)
    _check_step(world, r, g, 256, 256, "sum", weighted, gin, f"step256 sum weighted={weighted} gin={gin}",
                fused_dx=not gin)


@pytest.mark.parametrize("F,Fo", [(100, 100), (128, 20)])
@pytest.mark.parametrize("red", ["sum", "max"])
@pytest.mark.parametrize("weighted", [True, False])
def test_step_masked_shapes(world, monkeypatch, F, Fo, red, weighted):
    """The NARROW instantiations through the public op: agg_out is stored under
    the f_ok lane mask (F_in 100) and the product is cut at F_out (20); P is the
    tensor the backward hands to kgx_gemm_tn."""
    g = world.graph(weighted)
    r = _step(world, monkeypatch, g, F, Fo, red, weighted, False)
    assert len(r.spy.tn) == 1 and r.P.shape == (N, F)
    assert not kops.fused_transform_supported(Fo, F) and len(r.spy.raw) == 0  # dx: the unfused backward
    label = f"masked {F}->{Fo} {red} weighted={weighted}"
    _check_step(world, r, g, F, Fo, red, weighted, False, label, fused_dx=False)
    x = world.inputs(F, Fo)[0]
    p32, exact_rows = train_ref.aggregate32(g, x, red, weighted)
    bad = torch.nonzero(exact_rows & (r.P != p32).any(1)).flatten()
    assert bad.numel() == 0, f"{label}: P != fp32 restatement on rows {bad[:8].tolist()} ({fused_ref.owners(g, bad[:8])})"


# ---------------------------------------------------------------------------
# f: partial gradients, g: ordering and determinism
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def full_step(world):
    """The full 128 -> 128 weighted-sum step's results, for the bitwise comparisons."""
    mp = pytest.MonkeyPatch()
    try:
        return _step(world, mp, world.graph(True), 128, 128, "sum", True, False)
    finally:
        mp.undo()


def test_partial_gradients(world, monkeypatch, full_step):
    g = world.graph(True)
    # x only: the forward keeps no P and runs the plain launch; dW is not computed
    r = _step(world, monkeypatch, g, 128, 128, "sum", True, False, need=(True, False, False))
    assert len(r.spy.tn) == 0 and len(r.spy.save) == 0 and r.dW is None and r.db is None
    # forward (no saved aggregate), then the dx pass
    assert len(r.spy.raw) == 2 and r.spy.raw[0][0] is g and r.spy.raw[1][0] is G.transpose(g)
    t = G.transpose(g)
    train_ref.assert_same(r.y, full_step.y, g, "x only: y vs the full step's")
    train_ref.assert_same(r.dx, full_step.dx, t, "x only: dx vs the full step's (transposed schedule)")
    # W and bias only: the dx pass is skipped
    r = _step(world, monkeypatch, g, 128, 128, "sum", True, False, need=(False, True, True))
    assert len(r.spy.raw) == 0 and r.dx is None and len(r.spy.tn) == 1
    train_ref.assert_same(r.dW, full_step.dW, None, "W and bias only: dW vs the full step's")
    train_ref.assert_same(r.db, full_step.db, None, "W and bias only: db vs the full step's")
    train_ref.assert_same(r.y, full_step.y, g, "W and bias only: y vs the full step's")
    # no bias: the same P, dx and dW; y against the reference without it
    r = _step(world, monkeypatch, g, 128, 128, "sum", True, False, bias=False)
    _guard(r, g, "sum", False, 128, 128)
    train_ref.assert_same(r.dx, full_step.dx, t, "bias=None: dx vs the full step's (transposed schedule)")
    train_ref.assert_same(r.dW, full_step.dW, None, "bias=None: dW vs the full step's")
    train_ref.assert_same(r.P, full_step.P, g, "bias=None: P vs the full step's")
    _check_step(world, r, g, 128, 128, "sum", True, False, "step128 sum weighted bias=None", bias=False)


def test_tn_overlap_same_bits(world, monkeypatch, full_step):
    """KGX_TN_OVERLAP=1 (dW / db on the side stream beside the dx pass): the same
    bits, and each result is complete when the caller's stream reads it right
    after backward()."""
    def early(xg, Wg, bg):
        return xg.grad.sum(0), Wg.grad.sum(0), bg.grad.sum()

    monkeypatch.setenv("KGX_TN_OVERLAP", "1")
    g = world.graph(True)
    t = G.transpose(g)
    caller = torch.cuda.current_stream(world.dev)
    assert full_step.spy.tn[0][2] == caller, "the default step ran kgx_gemm_tn off the caller's stream"
    r = _step(world, monkeypatch, g, 128, 128, "sum", True, False, after=early, side=True)
    _guard(r, g, "sum", False, 128, 128)
    side = r.spy.tn[0][2]
    assert side != caller and side == kops._side_stream(world.dev), "KGX_TN_OVERLAP=1 left kgx_gemm_tn on the caller's stream"
    torch.cuda.synchronize()
    train_ref.assert_same(r.dx, full_step.dx, t, "KGX_TN_OVERLAP=1: dx vs the default (transposed schedule)")
    train_ref.assert_same(r.dW, full_step.dW, None, "KGX_TN_OVERLAP=1: dW vs the default")
    train_ref.assert_same(r.db, full_step.db, None, "KGX_TN_OVERLAP=1: db vs the default")
    late = (r.dx.sum(0), r.dW.sum(0), r.db.sum())
    for name, a, b in zip(("dx", "dW", "db"), r.early, late):
        train_ref.assert_same(a, b, None, f"KGX_TN_OVERLAP=1: {name} reduced right after backward() vs later "
                                          f"(read before it was complete)")


@pytest.mark.parametrize("F", [128, 256])
def test_step_deterministic(world, monkeypatch, full_step, F):
    """No atomics, partials summed in order: three repeats of the whole step give the same bits."""
    g = world.graph(True, None, F)
    first = full_step if F == 128 else _step(world, monkeypatch, g, F, F, "sum", True, False)
    for i in range(2):
        r = _step(world, monkeypatch, g, F, F, "sum", True, False)
        for name, own in (("y", g), ("dx", G.transpose(g)), ("dW", None), ("db", None)):
            train_ref.assert_same(getattr(r, name), getattr(first, name), own, f"{name} of repeat {i + 2} vs the first")


# ---------------------------------------------------------------------------
# h: layers
# ---------------------------------------------------------------------------
def _layer_graph(ei, **kw):
    """The graph the layer's own lookup gives for this edge_index (layers._edges.graph_for:
    built on the first call, served from the cache after); the tests then assert that the
    layer's launches ran on this very object."""
    from keras_geometric_amd.layers._edges import edge_index_tensor, graph_for

    return graph_for(ei, edge_index_tensor(ei, ei.device, allow_transpose=False), N, N, **kw)


def _layer_ops(spy, g, fused: bool, **want):
    """The public ops the layer dispatched to, on graph g: the fused
    aggregate_transform (with the saving launch: the weights require grad) or
    the unfused aggregation, never both."""
    n_at, n_agg, n_save = (1, 0, 1) if fused else (0, 1, 0)
    assert (len(spy.at), len(spy.agg), len(spy.save)) == (n_at, n_agg, n_save), \
        (f"the layer is {'' if fused else 'not '}expected on the fused path: {len(spy.at)} aggregate_transform, "
         f"{len(spy.agg)} aggregate, {len(spy.save)} kgx::spmm_gemm_save calls")
    called_g, kw = (spy.at if fused else spy.agg)[0]
    assert called_g is g, "the layer ran on another graph than its cached one"
    for k, v in want.items():
        assert kw.get(k) == v, f"{k}={kw.get(k)!r}, expected {v!r}"


@pytest.mark.parametrize("F", [128, 256])
def test_gcn_layer_step(world, monkeypatch, F):
    """GCNConv(F) on F features: the layer's own graph build, cache and dispatch."""
    assert kops.fused_transform_supported(F, F)
    x, W, b, dOut = world.inputs(F, F)
    ei = torch.stack([world.src, world.dst]).long()
    torch.manual_seed(0)
    layer = GCNConv(F)
    with torch.no_grad():
        layer([x, ei])
    layer.set_weights([W.cpu().numpy(), b.cpu().numpy()])
    g = _layer_graph(ei, self_loops=True, gcn_norm=True, n_features=F)
    assert g.n_dst == N and g.kept == 73142 + N and g.w is not None
    t = G.transpose(g)
    with monkeypatch.context() as mp:
        spy = _Spy(mp)
        xg = x.clone().requires_grad_(True)
        _poison(g, F, F, t)
        y = layer([xg, ei])
        _poison(g, F, F, t)
        y.backward(dOut)
    r = SimpleNamespace(y=y.detach(), dx=xg.grad, dW=layer.kernel.grad, db=layer.bias.grad, spy=spy, P=spy.tn[0][0])
    _layer_ops(spy, g, True, weighted=True)
    _guard(r, g, "sum", False, F, F)
    _check_step(world, r, g, F, F, "sum", True, False, f"GCNConv({F})")


def _gin_reference(g, x, ws, dOut, aggr, eps, mask, train_eps):
    """float64 autograd of relu(((1+eps) x + AGG x) W1 + b1) W2 + b2 on the
    kernel's own ReLU branches (mask: the step at 0 is not differentiable, and
    a pre-activation within rounding of it may fall on either side), and the
    same on |terms|.  Returns (ref, mag): dicts y, P, dx, grads [per weight]."""
    out = []
    for absolute in (False, True):
        f = (lambda v: v.double().abs()) if absolute else (lambda v: v.double())
        x64 = f(x).requires_grad_(True)
        w64 = [f(w).requires_grad_(True) for w in ws]
        if train_eps:
            e64, W1, b1, W2, b2 = w64
            scale = 1 + e64
        else:
            W1, b1, W2, b2 = w64
            scale = float(np.float32(1 + eps))
        red = "sum" if absolute else aggr
        z, P = train_ref.forward64(g, x64, W1, b1, red, False, True, scale, None if absolute else x)
        yy = (z * mask.double()) @ W2 + b2
        yy.backward(f(dOut))
        out.append(dict(y=yy.detach(), P=P.detach(), dx=x64.grad, grads=[w.grad for w in w64]))
    return out


@pytest.mark.parametrize("aggr", ["sum", "max"])
@pytest.mark.parametrize("train_eps", [False, True])
def test_gin_layer_step(world, monkeypatch, aggr, train_eps):
    """GINConv(128, mlp_hidden=[128]) on 128 features: relu=True with grad, where
    the fused launch keeps P and ReLU runs outside the kernel.  A trainable eps
    keeps (1 + eps) in the autograd graph, so that form is the unfused
    aggregation + Dense by design.  The path guard tells the two apart by the
    op the layer dispatches to (both run kgx_gemm_tn twice: kgx_dense's
    backward calls it too): train_eps=False must make one
    kops.aggregate_transform call (pre_gin, relu) with one kgx::spmm_gemm_save
    launch and no kops.aggregate; train_eps=True the reverse."""
    F = 128
    assert kops.fused_transform_supported(F, F)
    x, _, _, dOut = world.inputs(F, F)
    ei = torch.stack([world.src, world.dst]).long()
    torch.manual_seed(0)
    layer = GINConv(output_dim=F, mlp_hidden=[F], aggregator=aggr, eps_init=0.25, train_eps=train_eps)
    with torch.no_grad():
        layer([x, ei])
        rng = np.random.default_rng(77)
        for w in layer.weights:  # non-trivial biases; eps stays 0.25
            if w.dim() == 1 and w.numel() == F:
                w.copy_(T(rng.standard_normal(F).astype(np.float32)))
    g = _layer_graph(ei, n_features=F)
    assert g.n_dst == N and g.kept == 73142 and g.w is None
    ws = [w.detach().clone() for w in layer.weights]
    W1, b1 = ws[-4], ws[-3]
    with torch.no_grad():  # the kernel's own pre-activations: the ReLU branches of the reference
        if train_eps:
            z = kops.dense((1 + ws[0]) * x + kops.aggregate(g, x, aggr), W1, b1)
        else:
            z = kops.aggregate_transform(g, x, W1, aggr, bias=b1, pre_gin=True, gin_scale=layer._scale())
    mask = z > 0
    with monkeypatch.context() as mp:
        spy = _Spy(mp)
        xg = x.clone().requires_grad_(True)
        _poison(g, F, F)
        y = layer([xg, ei])
        _poison(g, F, F)
        y.backward(dOut)
    if train_eps:
        _layer_ops(spy, g, False)
    else:
        _layer_ops(spy, g, True, pre_gin=True, relu=True, gin_scale=layer._scale())
    # kgx_gemm_tn: the second Dense's dW first, then the first transform's, whose P is (1+eps) x + AGG x;
    # dx is the unfused aggregation backward either way (the pre-scale's path)
    assert len(spy.tn) == 2 and len(spy.raw) == 0
    P = spy.tn[-1][0]
    ref, mag = _gin_reference(g, x, ws, dOut, aggr, 0.25, mask, train_eps)
    label = f"GINConv {aggr} train_eps={train_eps}"
    errs = {"y": fused_ref.check(y.detach(), g, (ref["y"], mag["y"]), f"{label}: y"),
            "P": train_ref.check_rows(P, g, ref["P"], mag["P"], f"{label}: P"),
            "dx": train_ref.check_rows(xg.grad, SimpleNamespace(items=None, n_dst=N), ref["dx"], mag["dx"],
                                       f"{label}: dx")}
    for w, name, gr, gm in zip(layer.weights, ("eps", "W1", "b1", "W2", "b2")[0 if train_eps else 1:], ref["grads"],
                               mag["grads"]):
        errs[name] = train_ref.check_dense(w.grad, gr, gm, f"{label}: d{name}", tol=2e-5 if name[0] == "W" else 1e-5)
    _report(label, **errs)


# ---------------------------------------------------------------------------
# i: non-finite inputs
# ---------------------------------------------------------------------------
def test_step_nonfinite(world, monkeypatch):
    """One inf and one NaN in x, each on a source that feeds a hub row, a short
    row and a record row (the two sources of out-degree > 256): the NaN / inf
    pattern of y, P and dW is float64's, position by position, and the finite
    entries stay within the tolerance.  Sum, unweighted."""
    F = 128
    g = world.graph(False)
    x0, W, b, dOut = world.inputs(F, F)
    out_deg = torch.bincount(g.col.long(), minlength=N)
    hubs = torch.nonzero(out_deg > 256).flatten().tolist()
    assert len(hubs) == 2
    rows_of = G.row_of_slot(g).long()
    for s in hubs:
        fed = set(fused_ref.owners(g, rows_of[g.col.long() == s].unique()))
        assert {"split", "short", "tiny"} <= fed, f"source {s} feeds only {fed}"
    x = x0.clone()
    x[hubs[0], 3] = float("inf")
    x[hubs[1], 7] = float("nan")
    ref, mag = train_ref.grads(g, x, W, b, dOut, "sum", False)
    with monkeypatch.context() as mp:
        spy = _Spy(mp)
        xg, Wg, bg = x.clone().requires_grad_(True), W.clone().requires_grad_(True), b.clone().requires_grad_(True)
        t = G.transpose(g)
        _poison(g, F, F, t)
        y = kops.aggregate_transform(g, xg, Wg, "sum", bias=bg)
        _poison(g, F, F, t)
        y.backward(dOut)
    assert len(spy.tn) == 1 and len(spy.save) == 1

    def same_pattern(name, got, want, what):
        bad = torch.nonzero((got != want).reshape(got.shape[0], -1).any(1)).flatten()
        own = f" on {fused_ref.owners(g, bad[:8])} kernels" if name != "dW" else ""
        assert bad.numel() == 0, f"{name}: {what} pattern differs from float64's on {bad.numel()} rows, first {bad[:8].tolist()}{own}"

    errs = {}
    for name, got, r64, m64 in (("y", y.detach(), ref.y, mag.y), ("P", spy.tn[0][0], ref.P, mag.P),
                                ("dW", Wg.grad, ref.dW, mag.dW)):
        assert not bool(torch.isfinite(r64).all()), f"{name}: the reference has no non-finite entry"
        same_pattern(name, torch.isnan(got), torch.isnan(r64), "NaN")
        inf = torch.isinf(r64)
        same_pattern(name, torch.isinf(got), inf, "inf")
        same_pattern(name, torch.where(inf, torch.sign(got).double(), 0.0), torch.where(inf, torch.sign(r64), 0.0),
                     "inf sign")
        fin = torch.isfinite(r64)  # the finite entries (the others count as met: compared above)
        got_f, ref_f = torch.where(fin, got, 0.0), torch.where(fin, r64, 0.0)
        mag_f = torch.where(fin, m64, 1.0)
        if name == "dW":
            errs[name] = train_ref.check_dense(got_f, ref_f, mag_f, "nonfinite: finite entries of dW", tol=2e-5)
        else:
            errs[name] = train_ref.check_rows(got_f, g, ref_f, mag_f, f"nonfinite: finite entries of {name}")
    # dx and db do not read x: finite, and the transposed pass's as ever
    errs["dx"] = train_ref.check_rows(xg.grad, t, ref.dx, mag.dx, "nonfinite: dx")
    errs["db"] = train_ref.check_dense(bg.grad, ref.db, mag.db, "nonfinite: db")
    _report("nonfinite sum unweighted", **errs)
