"""The sliced schedule of the fused aggregate -> transform (kgx_slice_build,
kgx_fused_args.slice): the builder's integer invariants, the sliced launch against
the float64 restatement (tests/fused_ref.py) and against the unsliced launch
(rows below T bit-identical), its flags, non-finite inputs, and independence
of the grid the main kernel is launched with.

One hand-built graph (T = 16, C = 8, split_len = 32) holds every case: rows of
degree T-1, T, T+1; a degree-300 row whose sources share one class; one spread
over all classes; a row with more than split_len edges in one class; a row
that repeats one source; rows of degree 0, 1, 2 and 3..7 so every tail kernel
runs; with and without self loops."""

import dataclasses

import pytest
import torch

from keras_geometric_amd import _native as nat
from keras_geometric_amd import graph as G
from keras_geometric_amd import ops as kops
from keras_geometric_amd import slice as S

pytestmark = pytest.mark.gpu

T, C, SPLIT = 16, 8, 32
N = 8192
ONE_CLASS, SPREAD, FAT_CLASS, REPEAT = 0, 1, 2, 3  # the special rows
INF_SRC, NAN_SRC = 4001, 4002


def _edges():
    gen = torch.Generator().manual_seed(11)
    cls = torch.tensor([S.slice_class(c, C) for c in range(N)])
    by_cls = [torch.nonzero(cls == c).flatten() for c in range(C)]
    src, dst = [], []

    def add(row, sources):
        src.append(torch.as_tensor(sources, dtype=torch.int64))
        dst.append(torch.full((len(sources),), row, dtype=torch.int64))

    def rnd(k):
        return torch.randint(0, N, (k,), generator=gen)

    add(ONE_CLASS, by_cls[3][torch.randperm(by_cls[3].numel(), generator=gen)[:300]])  # seven empty groups
    spread = rnd(300)
    spread[5], spread[250] = INF_SRC, NAN_SRC
    add(SPREAD, spread)
    fat = torch.cat([by_cls[5][:100], rnd(200)])  # cut inside a class
    fat[100] = INF_SRC  # (an infinite source without a NaN beside it)
    add(FAT_CLASS, fat[torch.randperm(300, generator=gen)])
    add(REPEAT, torch.full((40,), 7))
    row = 4
    for d in (T - 2, T - 1, T, T + 1):  # with self loops: T-1 .. T+2
        add(row, rnd(d))
        row += 1
    for d in list(range(18, 32)) + [32, 33, 47, 64, 65, 100]:  # sliced rows below and above the hub split
        add(row, rnd(d))
        row += 1
    for d in range(8, T - 2):  # unsliced main-kernel rows
        for _ in range(12):
            add(row, rnd(d))
            row += 1
    for d in range(3, 8):  # short rows
        for _ in range(40):
            add(row, rnd(d))
            row += 1
    for d in (2, 1):  # tiny rows; the rest have no input edge
        for _ in range(2400):
            add(row, rnd(d))
            row += 1
    assert row < N - 500
    return torch.cat(src).to(torch.int32), torch.cat(dst).to(torch.int32)


@pytest.fixture(scope="module", params=[True, False], ids=["loops", "noloops"])
def case(request, dev):
    """(graph, sliced schedule, x, W, b, float64 reference of the weighted or plain sum): built once."""
    import fused_ref

    loops = request.param
    src, dst = _edges()
    g = G.build_csr(src.to(dev), dst.to(dev), N, N, self_loops=loops, gcn_norm=loops, split_len=SPLIT)
    assert g.n_split > 0 and g.n_long > 0 and kops._tiny_of(g, g.items)[0] is not None
    sl = S.build(g, T, C, SPLIT)
    gen = torch.Generator(device=dev).manual_seed(3)
    x = torch.randn(N, 128, device=dev, generator=gen)
    W = torch.randn(128, 128, device=dev, generator=gen) * 0.1
    b = torch.randn(128, device=dev, generator=gen)
    ref = fused_ref.reference(g, x, W, "sum", loops, b)
    return g, sl, x, W, b, ref, loops


def _launch(g, sl, x, W, b, weighted, flags=0, gin_scale=1.0, agg=False, out=None):
    items, _, split, _, n_slots = g.work(False)
    n = g.n_dst
    out = torch.empty((n, W.shape[1]), dtype=torch.float32, device=x.device) if out is None else out
    aggt = torch.empty((n, 128), dtype=torch.float32, device=x.device) if agg else None
    if sl is not None and not weighted:
        sl = dataclasses.replace(sl, w=None)
    kops._fused_launch(out, aggt, x, None, g.rowptr, g.rows, items, split, g.col, g.w if weighted else None, n_slots,
                       nat.SUM, W, b, flags, gin_scale, False, g.n_long, *kops._tiny_of(g, items), x.device, sl)
    return (out, aggt) if agg else out


def _below(g):
    deg = (g.rowptr[1:] - g.rowptr[:-1]).long()
    return deg < S.effective_threshold(T, g.split_len)


def test_builder_invariants(case):
    g, sl, *_, loops = case
    rowptr, col = g.rowptr.cpu().tolist(), g.col.cpu().tolist()
    wbits = g.w.view(torch.int32).cpu().tolist() if g.w is not None else [0] * len(col)
    cs = sl.col.cpu().tolist()
    ws = sl.w.view(torch.int32).cpu().tolist() if sl.w is not None else [0] * len(cs)
    items, lists, fix = sl.items.cpu().tolist(), sl.lists.cpu().tolist(), sl.fix.cpu().tolist()
    deg = [rowptr[r + 1] - rowptr[r] for r in range(g.n_dst)]
    sliced_rows = [r for r in range(g.n_dst) if deg[r] >= T]
    assert sorted(f[0] for f in fix) == sorted(sliced_rows) and len(fix) == sl.n_rows
    for r in (4, 5, 6, 7):  # degrees T-1 .. T+2 or T-2 .. T+1: sliced exactly from T
        assert (r in {f[0] for f in fix}) == (deg[r] >= T)
    chunks = {}  # row -> [(slot, class, edges)]
    rest, slots = [], []
    assert sum(L[1] for L in lists) == len(items)
    for c, (first, n, n_chunk, _) in enumerate(lists):
        assert first == sum(L[1] for L in lists[:c])  # back to back
        for i, (row, beg, end, slot) in enumerate(items[first: first + n]):
            if i < n_chunk:
                assert slot >= 0 and 0 < end - beg <= SPLIT
                ed = list(zip(cs[beg:end], ws[beg:end]))
                assert {S.slice_class(s, C) for s, _ in ed} == {c}  # one class, its list's
                chunks.setdefault(row, []).append((slot, c, ed))
                slots.append(slot)
            else:
                assert slot == -1
                rest.append((row, beg, end, slot))
    assert sorted(slots) == list(range(sl.n_slots))  # dense and unique
    for row, first, n, d in fix:
        got = sorted(chunks[row])
        assert [s for s, _, _ in got] == list(range(first, first + n)) and d == deg[row]  # consecutive per row
        assert [c for _, c, _ in got] == sorted(c for _, c, _ in got)  # class order, then chunk order
        csr = list(zip(col[rowptr[row]: rowptr[row + 1]], wbits[rowptr[row]: rowptr[row + 1]]))
        for c in range(C):  # CSR order kept inside a class (hence inside a chunk); the multisets agree
            mine = [e for _, cc, ed in got if cc == c for e in ed]
            assert mine == [e for e in csr if S.slice_class(e[0], C) == c]
        assert sum(len(ed) for _, _, ed in got) == d
    one = sorted(chunks[ONE_CLASS])
    # seven empty groups (six with the self loop, whose source is the row itself)
    assert {c for _, c, _ in one} == ({3, S.slice_class(ONE_CLASS, C)} if loops else {3})
    assert sum(1 for _, c, _ in one if c == 3) == (300 + SPLIT - 1) // SPLIT
    assert sum(1 for _, c, _ in chunks[FAT_CLASS] if c == 5) >= 4  # cut inside a class
    # every other long item sits in exactly one list
    others = [tuple(v) for v in g.items[sl.n_items_s: sl.n_long].cpu().tolist()]
    assert sorted(rest) == sorted(others) and len(set(rest)) == len(rest)
    assert all(deg[v[0]] < T for v in others)
    # the CSR is untouched and a second build gives the same arrays
    again = S.build(g, T, C, SPLIT)
    for a, b_ in ((sl.col, again.col), (sl.w, again.w), (sl.items, again.items), (sl.lists, again.lists),
                  (sl.fix, again.fix)):
        assert (a is None and b_ is None) or torch.equal(a, b_)
    assert g.col.cpu().tolist() == col


def test_values_and_rows_below_threshold(case):
    import fused_ref

    g, sl, x, W, b, ref, loops = case
    below = _below(g)
    assert 0 < int((~below).sum()) == sl.n_rows
    for weighted in ([True, False] if loops else [False]):  # (the graph without self loops carries no weights)
        r = ref if weighted == loops else fused_ref.reference(g, x, W, "sum", weighted, b)
        y0 = _launch(g, None, x, W, b, weighted)
        y1 = _launch(g, sl, x, W, b, weighted)
        fused_ref.check(y0, g, r, f"unsliced weighted={weighted}")
        fused_ref.check(y1, g, r, f"sliced weighted={weighted}")
        assert torch.equal(y1[below], y0[below])  # bit-identical
        assert torch.equal(_launch(g, sl, x, W, b, weighted), y1)  # two identical launches


def test_flags_on_sliced_rows(case):
    import fused_ref

    g, sl, x, W, b, _, loops = case
    below = _below(g)
    # agg_out + GIN pre-scale: the kept aggregate, then the transform of it
    y0, a0 = _launch(g, None, x, W, b, loops, flags=nat.FUSED_PRE_GIN, gin_scale=1.25, agg=True)
    y1, a1 = _launch(g, sl, x, W, b, loops, flags=nat.FUSED_PRE_GIN, gin_scale=1.25, agg=True)
    r = fused_ref.reference(g, x, W, "sum", loops, b, pre_gin=True, gin_scale=1.25)
    fused_ref.check(y1, g, r, "sliced pre_gin")
    assert torch.equal(y1[below], y0[below]) and torch.equal(a1[below], a0[below])
    eye = torch.eye(128, device=x.device)
    ra = fused_ref.reference(g, x, eye, "sum", loops, None, pre_gin=True, gin_scale=1.25)
    fused_ref.check(a1, g, ra, "sliced agg_out")
    # relu and accumulate
    r = fused_ref.reference(g, x, W, "sum", loops, b)
    base = torch.randn(g.n_dst, 128, device=x.device, generator=torch.Generator(device=x.device).manual_seed(8))
    acc = _launch(g, sl, x, W, b, loops, flags=nat.FUSED_ACCUMULATE | nat.FUSED_RELU, out=base.clone())
    want = torch.relu(r[0] + base.double())
    err = (acc.double() - want).abs() / (r[1] + base.double().abs()).clamp_min(1.0)
    assert float(err.max()) <= 1e-5
    acc0 = _launch(g, None, x, W, b, loops, flags=nat.FUSED_ACCUMULATE | nat.FUSED_RELU, out=base.clone())
    assert torch.equal(acc[below], acc0[below])


def test_non_finite_sources(case):
    g, sl, x, W, b, _, loops = case
    xb = x.clone()
    xb[INF_SRC, 17] = float("inf")
    xb[NAN_SRC, 90] = float("nan")
    y0 = _launch(g, None, xb, W, b, loops)
    y1 = _launch(g, sl, xb, W, b, loops)
    assert torch.isnan(y0[SPREAD]).any() and torch.isinf(y0[FAT_CLASS]).any()  # the sliced rows saw them
    assert torch.equal(torch.isnan(y1), torch.isnan(y0))
    assert torch.equal(torch.isinf(y1), torch.isinf(y0))
    assert torch.equal(torch.signbit(y1[torch.isinf(y1)]), torch.signbit(y0[torch.isinf(y0)]))


def test_ops_build_lazily_and_switch(case, monkeypatch):
    """aggregate_transform under KGX_FUSED_SLICE=1: nothing on the first forward,
    the schedule on the second, beside g.items / g.split; KGX_FUSED_SLICE=0 is
    the plain launch; CU-masked streams change nothing."""
    import fused_ref

    g, sl, x, W, b, ref, loops = case
    g.extras.pop("fused_slice", None)
    g.extras.pop("fused_slice_uses", None)
    items, split = g.items, g.split
    monkeypatch.setenv("KGX_FUSED_SLICE", "0")
    y0 = kops.aggregate_transform(g, x, W, "sum", weighted=loops, bias=b)
    assert "fused_slice_uses" not in g.extras
    monkeypatch.setenv("KGX_FUSED_SLICE", "1")
    monkeypatch.setenv("KGX_FUSED_SLICE_T", str(T))
    monkeypatch.setenv("KGX_FUSED_SLICE_C", str(C))
    y_first = kops.aggregate_transform(g, x, W, "sum", weighted=loops, bias=b)
    assert "fused_slice" not in g.extras and torch.equal(y_first, y0)
    y1 = kops.aggregate_transform(g, x, W, "sum", weighted=loops, bias=b)
    built = g.extras["fused_slice"][1]
    assert built is not None and built.n_rows == sl.n_rows and torch.equal(built.items, sl.items)
    assert g.items is items and g.split is split
    fused_ref.check(y1, g, ref, "ops sliced")
    assert torch.equal(y1, _launch(g, sl, x, W, b, loops))
    monkeypatch.setenv("KGX_FUSED_FORK", "3")
    assert torch.equal(kops.aggregate_transform(g, x, W, "sum", weighted=loops, bias=b), y1)
    # ... nor does running half of the short rows on the head's CUs (same kernel, same rows)
    monkeypatch.setenv("KGX_FUSED_SLICE_HEAD", "0.5")
    assert torch.equal(kops.aggregate_transform(g, x, W, "sum", weighted=loops, bias=b), y1)
    built = g.extras["fused_slice"][1]
    assert g.n_long < built.head_short_end < kops._tiny_of(g, g.items)[2]


def test_placement_independent(dev, monkeypatch):
    """Enough long items that the main kernel's grid is its resident cap: the
    same launch under KGX_FUSED_SHARE_GPU (a smaller cap, another multiple of
    C, so other blocks own the items) gives the same bits."""
    import fused_ref

    n = 32768
    gen = torch.Generator().manual_seed(5)
    deg = torch.cat([torch.tensor([400, 300, 200, 90, 60, 40, 33, 20, 17, 16]), torch.full((20000,), 9),
                     torch.randint(0, 8, (n - 20010,), generator=gen)])
    dst = torch.repeat_interleave(torch.arange(n), deg).to(torch.int32)
    src = torch.randint(0, n, (int(deg.sum()),), generator=gen).to(torch.int32)
    g = G.build_csr(src.to(dev), dst.to(dev), n, n, self_loops=True, gcn_norm=True, split_len=SPLIT)
    sl = S.build(g, T, C, SPLIT)
    assert sl.tiles * C > 1024  # more tiles than any resident grid: the cap sets the grid
    dgen = torch.Generator(device=dev).manual_seed(6)
    x = torch.randn(n, 128, device=dev, generator=dgen)
    W = torch.randn(128, 128, device=dev, generator=dgen) * 0.1
    y = _launch(g, sl, x, W, None, True)
    fused_ref.check(y, g, fused_ref.reference(g, x, W, "sum", True, None), "sliced, full grid")
    monkeypatch.setenv("KGX_SHARE_DEN", "3")
    assert torch.equal(_launch(g, sl, x, W, None, True, flags=nat.FUSED_SHARE_GPU), y)
    monkeypatch.setenv("KGX_SHARE_DEN", "2")
    assert torch.equal(_launch(g, sl, x, W, None, True, flags=nat.FUSED_SHARE_GPU), y)
