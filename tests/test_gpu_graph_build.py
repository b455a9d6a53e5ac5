"""csrc/graph_build.hip against its host restatement (tests/graph_build_ref.py),
array for array: the CSR build and the schedule on every named case, and
kgx_schedule_build, kgx_schedule_suffixes, kgx_tiny_pack, kgx_gcn_edge_norm,
kgx_gcn_dinv(_table) and kgx_select_dst_range through the ABI; graph.transpose,
graph.restrict_rows and graph.split_by_part on other than square graphs; the
argument errors of the two builders.  Everything is integer-exact or bit-exact:
there are no tolerances here.

`stride` (8.5M CSR slots, 2.1M rows) is the one case large enough to send every
grid-stride loop of the file round a second time; it is built once per module.
"""

import ctypes

import numpy as np
import pytest
import torch

import graph_build_ref as ref
from keras_geometric_amd import _native as nat
from keras_geometric_amd import graph as G

pytestmark = pytest.mark.gpu


def dt(a, dev):
    return torch.tensor(np.asarray(a)).to(dev)


def host(t):
    return t.cpu().numpy()


def eq(a, b, what=""):
    np.testing.assert_array_equal(np.asarray(a), np.asarray(b), err_msg=what)


def bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float32)).view(np.int32)


def build(b, dev, **over):
    kw = dict(b["kw"], split_len=b["split_len"])
    kw.update(over)
    return G.build_csr(dt(b["src"], dev), dt(b["dst"], dev), b["n_src"], b["n_dst"], **kw)


def check_schedule(g, rowptr, split_len, tag=""):
    rows, items, split, n_slots = ref.schedule(rowptr, split_len)
    assert g.split_len == split_len
    eq(host(g.rows), rows, tag + "rows")
    if g.n_dst == 0:
        assert g.n_items == 0 and g.work(False) == (None, 0, None, 0, 0)
        return
    assert (g.n_items, g.n_split, g.n_slots) == (items.shape[0], split.shape[0], n_slots), tag
    eq(host(g.items), items, tag + "items")
    eq(host(g.split), split, tag + "split")
    assert g.n_long == ref.suffixes(items, 7, 7)[0], tag + "n_long"
    work = g.work(False)
    assert work[0] is g.items and work[2] is g.split and (work[1], work[3], work[4]) == (g.n_items, g.n_split, g.n_slots)


def check_graph(g, b):
    assert (g.n_src, g.n_dst, g.n_input_edges) == (b["n_src"], b["n_dst"], b["src"].shape[0])
    assert (g.kept, g.max_degree) == (b["kept"], b["max_degree"])
    eq(host(g.rowptr), b["rowptr"], "rowptr")
    eq(host(g.col), b["col"], "col")
    eq(host(g.eid), b["eid"], "eid")
    eq(host(g.deg), b["deg"], "deg")
    check_schedule(g, b["rowptr"], b["split_len"])


@pytest.fixture(scope="module")
def stride(dev):
    b = ref.built("stride")
    g = build(b, dev)
    yield b, g
    del b, g
    torch.cuda.empty_cache()


# ---------------------------------------------------------------------------
# graph.build_csr on every case
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", ref.SMALL_CASES)
def test_build_csr_equals_restatement(dev, name):
    b = ref.built(name)
    check_graph(build(b, dev), b)


def test_build_csr_stride(stride):
    b, g = stride
    check_graph(g, b)
    table = G._dinv_values(0, b["max_degree"] + 1).numpy()  # the reference's own dinv per degree
    eq(bits(host(g.dinv)), bits(table[b["deg"]]), "dinv")


@pytest.mark.parametrize("name", ["wrap", "ladder64"])
def test_build_is_deterministic(dev, name):
    b = ref.built(name)
    g1, g2 = build(b, dev), build(b, dev)
    for f in ("rowptr", "col", "eid", "deg", "rows", "items", "split"):
        assert torch.equal(getattr(g1, f), getattr(g2, f)), f
    assert (g1.kept, g1.max_degree, g1.n_items, g1.n_split, g1.n_slots, g1.n_long) == \
        (g2.kept, g2.max_degree, g2.n_items, g2.n_split, g2.n_slots, g2.n_long)


# ---------------------------------------------------------------------------
# kgx_schedule_build through the ABI
# ---------------------------------------------------------------------------
def abi_schedule(rowptr_t, split_len, cap_items, ws_short=0):
    dev = rowptr_t.device
    n = rowptr_t.numel() - 1
    L = nat.lib()
    rows = torch.full((max(n, 1),), -7, dtype=torch.int32, device=dev)
    items = torch.full((max(cap_items, 1), 4), -7, dtype=torch.int32, device=dev)
    split = torch.full((max(n, 1), 4), -7, dtype=torch.int32, device=dev)
    nbytes = ctypes.c_size_t(0)
    assert L.kgx_schedule_workspace_bytes(n, ctypes.byref(nbytes)) == nat.KGX_OK
    ws = torch.empty(max(nbytes.value, 1), dtype=torch.uint8, device=dev)
    info = (ctypes.c_int64 * 4)(-1, -1, -1, -1)
    rc = L.kgx_schedule_build(nat.ptr(rowptr_t), n, split_len, nat.ptr(rows), nat.ptr(items), cap_items,
                              nat.ptr(split), nat.ptr(ws), nbytes.value - ws_short, info, nat.stream(dev))
    return rc, rows, items, split, [int(v) for v in info]


@pytest.mark.parametrize("name", ref.LADDERS)
def test_schedule_build_abi(dev, name):
    b = ref.built(name)
    rowptr_t = dt(b["rowptr"], dev)
    n = b["n_dst"]
    for L in (-1, 0, 1, 2, 16, 64, 2**20):
        rows, items, split, n_slots = ref.schedule(b["rowptr"], L)
        n_items = items.shape[0]
        rc, drows, ditems, dsplit, info = abi_schedule(rowptr_t, L, n_items)  # exactly n_items: enough
        assert rc == nat.KGX_OK, (L, nat.lib().kgx_last_error())
        assert info == [n_items, split.shape[0], n_slots, 0], L
        eq(host(drows)[:n], rows, f"rows L={L}")
        eq(host(ditems)[:n_items], items, f"items L={L}")
        eq(host(dsplit)[: split.shape[0]], split, f"split L={L}")
        assert abi_schedule(rowptr_t, L, n_items - 1)[0] == nat.KGX_ERR_ARG, L  # one item short
    for L in (3, 48, 2**20 + 1):
        assert abi_schedule(rowptr_t, L, 4 * b["kept"] + n)[0] == nat.KGX_ERR_ARG, L


# ---------------------------------------------------------------------------
# kgx_schedule_suffixes and kgx_tiny_pack through the ABI
# ---------------------------------------------------------------------------
def abi_suffixes(items_t, short_max, tiny_max):
    ws = torch.empty(16, dtype=torch.uint8, device=items_t.device)
    out = (ctypes.c_int64 * 2)(-1, -1)
    n = int(items_t.shape[0])
    rc = nat.lib().kgx_schedule_suffixes(nat.ptr(items_t), n, short_max, tiny_max, nat.ptr(ws), out,
                                         nat.stream(items_t.device))
    assert rc == nat.KGX_OK
    return int(out[0]), int(out[1])


def abi_tiny(items_t, start, n, col_t, w_t, n_col):
    dev = items_t.device
    pack = torch.full((max(n, 1), 4), -7, dtype=torch.int32, device=dev)
    tw = torch.full((max(n, 1), 2), float("nan"), dtype=torch.float32, device=dev) if w_t is not None else None
    ws = torch.empty(16, dtype=torch.uint8, device=dev)
    out = (ctypes.c_int64 * 2)(-1, -1)
    rc = nat.lib().kgx_tiny_pack(nat.ptr(items_t), start, n, nat.ptr(col_t), nat.ptr(w_t), n_col, nat.ptr(pack),
                                 nat.ptr(tw), nat.ptr(ws), out, nat.stream(dev))
    assert rc == nat.KGX_OK, nat.lib().kgx_last_error()
    return host(pack)[:n], (host(tw)[:n] if tw is not None else None), (int(out[0]), int(out[1]))


def check_tiny(items, col, w, n_col, dev, starts=None, tag=""):
    """Device records of items [start, n_items) == the restatement's, for every start."""
    items_t, col_t = dt(items, dev), dt(col, dev)
    w_t = dt(w, dev) if w is not None else None
    n_items = items.shape[0]
    for bound in ((7, 2), (2, 7), (0, 64)):
        assert abi_suffixes(items_t, *bound) == ref.suffixes(items, *bound), (tag, bound)
    if starts is None:
        starts = sorted({0, ref.suffixes(items, 2, 2)[1], max(n_items - 1, 0), n_items})
    for start in starts:
        n = n_items - start
        pack, tw, out = abi_tiny(items_t, start, n, col_t, w_t, n_col)
        rpack, rtw, rout = ref.tiny_records(items, start, n, col, w, n_col)
        eq(pack, rpack, f"{tag} pack start={start}")
        assert out == rout, (tag, start, out, rout)
        if w is not None:
            eq(bits(tw), bits(rtw), f"{tag} tw start={start}")
    return out


@pytest.mark.parametrize("weighted", [True, False])
@pytest.mark.parametrize("name", ref.LADDERS + ["bipartite_tall"])
def test_suffixes_and_tiny_pack_abi(dev, name, weighted):
    b = ref.built(name)
    items, col, kept = b["items"], b["col"], b["kept"]
    rng = np.random.default_rng(5)
    w = rng.standard_normal(kept).astype(np.float32) if weighted else None
    check_tiny(items, col, w, kept, dev, tag="schedule")
    # a restricted list that is no longer degree-descending: the degree-2 records are not a prefix
    keep = rng.random(b["n_dst"]) < 0.6
    it = ref.restrict(items, b["split"], keep)[0][::-1].copy()
    full = ref.tiny_records(it, 0, it.shape[0], col, w, kept)[2]
    assert full[0] > 0 and full[1] != full[0]
    check_tiny(it, col, w, kept, dev, tag="reversed")
    # an all-zero-degree tail
    zero = items[items[:, 2] == items[:, 1]]
    if zero.shape[0]:
        assert check_tiny(zero, col, w, kept, dev, starts=[0], tag="zero-degree") == (0, 0)
    # the clamp: n_col ends at the end of one of the longest tail items, so that item is the last one
    # in range and every later begin (zero-degree rows included) is clamped to n_col - 1
    ln = items[:, 2] - items[:, 1]
    tail = items[(ln <= 2) & (items[:, 3] < 0)]
    ln = tail[:, 2] - tail[:, 1]
    assert ln.max() >= 1
    n_col = int(tail[ln == ln.max(), 2].min())
    assert (tail[:, 2] == n_col).any() and (tail[:, 1] >= n_col).any()
    check_tiny(tail, col[:n_col].copy(), w[:n_col].copy() if weighted else None, n_col, dev, starts=[0], tag="clamp")


@pytest.mark.parametrize("weighted", [True, False])
def test_suffixes_and_tiny_pack_stride(stride, weighted):
    b, g = stride
    items = b["items"]
    w = host(g.w) if weighted else None
    dev = g.device
    assert abi_suffixes(g.items, 7, 2) == ref.suffixes(items, 7, 2)
    start = ref.suffixes(items, 2, 2)[1]
    n = items.shape[0] - start
    assert n > 2048 * 256
    pack, tw, out = abi_tiny(g.items, start, n, g.col, g.w if weighted else None, b["kept"])
    rpack, rtw, rout = ref.tiny_records(items, start, n, b["col"], w, b["kept"])
    eq(pack, rpack)
    assert out == rout and out[0] == out[1]  # degree-descending: the degree-2 records are a prefix
    if weighted:
        eq(bits(tw), bits(rtw))


# ---------------------------------------------------------------------------
# kgx_gcn_edge_norm, kgx_gcn_dinv, kgx_gcn_dinv_table
# ---------------------------------------------------------------------------
def abi_edge_norm(rowptr_t, col_t, dd_t, ds_t, kept):
    w = torch.full((max(kept, 1),), float("nan"), dtype=torch.float32, device=rowptr_t.device)
    rc = nat.lib().kgx_gcn_edge_norm(nat.ptr(rowptr_t), nat.ptr(col_t), rowptr_t.numel() - 1, nat.ptr(dd_t),
                                     nat.ptr(ds_t), nat.ptr(w), nat.stream(rowptr_t.device))
    assert rc == nat.KGX_OK
    return host(w)[:kept]


def check_norm_three_ways(g, b):
    """w of the op == w of the fused build (csr_col_kernel<true>) == the restatement, bit for bit."""
    dinv = host(g.dinv)
    want = bits(ref.edge_norm(b["rowptr"], b["col"], dinv, dinv))
    eq(bits(host(g.w)), want, "fused build")
    eq(bits(abi_edge_norm(g.rowptr, g.col, g.dinv, g.dinv, g.kept)), want, "kgx_gcn_edge_norm")


@pytest.mark.parametrize("name", [k for k in ref.LADDERS if k.endswith("_loops")])
def test_edge_norm_ladder(dev, name):
    b = ref.built(name)
    g = build(b, dev, gcn_norm=True)
    assert {64, 65} <= set(b["deg"].tolist())  # the hand-over between the 8-lane and the wave kernel
    check_graph(g, b)
    check_norm_three_ways(g, b)


def test_edge_norm_stride(stride):
    b, g = stride
    check_norm_three_ways(g, b)


def test_edge_norm_two_tables(dev):
    """The shard use: rows and sources index different dinv tables."""
    b = ref.built("bipartite_wide")
    rng = np.random.default_rng(6)
    dd = (rng.random(b["n_dst"]) + 0.01).astype(np.float32)
    ds = (rng.random(b["n_src"]) + 0.01).astype(np.float32)
    assert b["max_degree"] > 64 and b["deg"].min() <= 64
    got = abi_edge_norm(dt(b["rowptr"], dev), dt(b["col"], dev), dt(dd, dev), dt(ds, dev), b["kept"])
    eq(bits(got), bits(ref.edge_norm(b["rowptr"], b["col"], dd, ds)))


def test_gcn_dinv_equals_correctly_rounded_table(dev):
    """kgx_gcn_dinv == kgx_gcn_dinv_table over a correctly-rounded table of
    (float(k) + 1e-12f)^-0.5, k <= 2^24 (float64 1/sqrt rounded once to float32),
    at the listed degrees; degrees past 2^24 read the last entry."""
    deg = np.array([0, 1, 2, 3, 64, 65, 4095, 4096, 4097, 2**24, 2**24 + 1, 2**31 - 1], np.int64).astype(np.int32)
    x = np.arange(2**24 + 1, dtype=np.float32) + np.float32(1e-12)
    table = (1.0 / np.sqrt(x.astype(np.float64))).astype(np.float32)
    deg_t, table_t = dt(deg, dev), dt(table, dev)
    a = torch.full((deg.shape[0],), float("nan"), dtype=torch.float32, device=dev)
    c = torch.full((deg.shape[0],), float("nan"), dtype=torch.float32, device=dev)
    L = nat.lib()
    assert L.kgx_gcn_dinv(nat.ptr(deg_t), deg.shape[0], nat.ptr(a), nat.stream(dev)) == nat.KGX_OK
    assert L.kgx_gcn_dinv_table(nat.ptr(deg_t), deg.shape[0], nat.ptr(table_t), table.shape[0], nat.ptr(c),
                                nat.stream(dev)) == nat.KGX_OK
    want = table[np.minimum(deg.astype(np.int64), 2**24)]
    eq(bits(host(c)), bits(want), "kgx_gcn_dinv_table")
    eq(bits(host(a)), bits(want), "kgx_gcn_dinv")
    del table_t
    torch.cuda.empty_cache()


# ---------------------------------------------------------------------------
# kgx_select_dst_range
# ---------------------------------------------------------------------------
def abi_select(src_t, dst_t, n, lo, hi, ws_short=0):
    dev = src_t.device
    L = nat.lib()
    nbytes = ctypes.c_size_t(0)
    assert L.kgx_select_workspace_bytes(n, ctypes.byref(nbytes)) == nat.KGX_OK
    ws = torch.empty(max(nbytes.value, 1), dtype=torch.uint8, device=dev)
    so = torch.full((max(n, 1),), -7, dtype=torch.int32, device=dev)
    do = torch.full((max(n, 1),), -7, dtype=torch.int32, device=dev)
    n_out = ctypes.c_int64(-1)
    rc = L.kgx_select_dst_range(nat.ptr(src_t), nat.ptr(dst_t), n, lo, hi, nat.ptr(so), nat.ptr(do), nat.ptr(ws),
                                nbytes.value - ws_short, ctypes.byref(n_out), nat.stream(dev))
    return rc, so, do, int(n_out.value)


@pytest.mark.parametrize("n", [0, 1, 255, 256, 257, 8192 * 256 + 5])
def test_select_dst_range(dev, n):
    rng = np.random.default_rng(7 + n % 1000)
    n_nodes = 1000
    src = rng.integers(0, 2**31 - 1, n).astype(np.int32)  # distinct enough to show the order
    dst = rng.integers(-3, n_nodes, n).astype(np.int32)
    if n:
        dst[-1] = 500  # the last edge is selected by the full and the middle range
    src_t, dst_t = dt(src, dev), dt(dst, dev)
    for lo, hi in ((400, 400), (-3, n_nodes), (250, 750), (750, 250), (0, 1)):
        rc, so, do, n_out = abi_select(src_t, dst_t, n, lo, hi)
        assert rc == nat.KGX_OK
        rs, rd = ref.select_dst_range(src, dst, lo, hi)
        assert n_out == rs.shape[0], (lo, hi)
        eq(host(so)[:n_out], rs, f"src [{lo}, {hi})")
        eq(host(do)[:n_out], rd, f"dst [{lo}, {hi})")
        if n:
            assert bool((so[n_out:] == -7).all()) and bool((do[n_out:] == -7).all())  # nothing past the count
    if n:
        assert abi_select(src_t, dst_t, n, 0, n_nodes, ws_short=1)[0] == nat.KGX_ERR_ARG


# ---------------------------------------------------------------------------
# graph.transpose
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["bipartite_wide", "bipartite_tall", "wrap", "segment"])
def test_transpose(dev, name):
    b = ref.built(name)
    g = build(b, dev)
    rng = np.random.default_rng(8)
    E, n_src, n_dst = b["src"].shape[0], b["n_src"], b["n_dst"]
    w_of_edge = rng.standard_normal(E + n_dst).astype(np.float32)  # a weight per input edge id
    g.w = dt(w_of_edge[b["eid"]], dev)
    t = G.transpose(g)
    # the kept edges in input-edge order, from the inputs alone
    s, d = b["src"].astype(np.int64), b["dst"].astype(np.int64)
    if b["kw"].get("segment_only"):
        keep = (d >= 0) & (d < n_dst)
    else:
        keep, s = d >= 0, np.where(s < 0, s + n_src, s)
    ids = np.arange(E)[keep]
    s, d = s[keep], d[keep]
    if b["kw"].get("self_loops"):
        loops = np.arange(n_dst)
        s, d, ids = np.concatenate([s, loops]), np.concatenate([d, loops]), np.concatenate([ids, E + loops])
    # row j of T: the out-edges of source j in input-edge order
    rowptr, col, pos, deg, kept, max_degree = ref.csr(d, s, n_dst, n_src)
    assert (t.n_src, t.n_dst, t.kept, t.max_degree) == (n_dst, n_src, kept, max_degree) and kept == g.kept
    eq(host(t.rowptr), rowptr, "rowptr")
    eq(host(t.col), col, "col = destination row")
    eq(host(t.eid), ids[pos], "eid = input edge id")  # dropped edges are absent
    eq(host(t.deg), deg, "deg")
    eq(bits(host(t.w)), bits(w_of_edge[ids[pos]]), "w")
    check_schedule(t, rowptr, ref.default_split_len(kept), "T ")
    # fwd_slot: the forward CSR slot of every transposed slot
    slot = host(t.extras["fwd_slot"])
    eq(np.sort(slot), np.arange(kept), "fwd_slot is a permutation")
    eq(b["eid"][slot], ids[pos], "fwd_slot eid")
    eq(b["col"][slot], np.repeat(np.arange(n_src), deg), "fwd_slot source")
    eq(np.repeat(np.arange(n_dst), b["deg"])[slot], col, "fwd_slot row")
    assert G.transpose(g) is t


# ---------------------------------------------------------------------------
# graph.restrict_rows, graph.split_by_part
# ---------------------------------------------------------------------------
def test_restrict_rows(dev):
    b = ref.built("ladder16")
    g = build(b, dev)
    n = b["n_dst"]
    deg = b["deg"]
    rng = np.random.default_rng(9)
    masks = {"all": np.ones(n, bool), "none": np.zeros(n, bool), "split rows": deg >= 16, "zero-degree": deg == 0,
             "half": rng.random(n) < 0.5}
    assert masks["split rows"].any() and masks["zero-degree"].any()
    for tag, m in masks.items():
        sub = G.restrict_rows(g, dt(m, dev))
        items, split, n_long = ref.restrict(b["items"], b["split"], m)
        assert (sub.n_items, sub.n_split, sub.n_long) == (items.shape[0], split.shape[0], n_long), tag
        assert sub.n_slots == g.n_slots == b["n_slots"] and sub.split_len == 16, tag  # slots keep their numbers
        eq(host(sub.items), items, tag + " items")
        eq(host(sub.split), split, tag + " split")
        for f in ("rowptr", "col", "eid", "deg", "rows"):
            assert getattr(sub, f) is getattr(g, f), (tag, f)  # the CSR is shared
        assert (sub.kept, sub.n_dst, sub.n_src) == (g.kept, g.n_dst, g.n_src)
    check_graph(g, b)  # the parent is left as it was


def test_default_split_len_restated():
    for e in (0, 1, 5000, 16384 * 1023, 16384 * 1024, 16384 * 4096 + 1, 10**8, 2**31 - 2):
        for f in (1, 32, 128, 256):
            assert ref.default_split_len(e, f) == G.default_split_len(e, f), (e, f)


@pytest.mark.parametrize("accumulate_from", [1, 3])
@pytest.mark.parametrize("name", ["ladder16", "bipartite_wide"])
def test_split_by_part(dev, name, accumulate_from):
    b = ref.built(name)
    g = build(b, dev)
    rng = np.random.default_rng(10)
    w = rng.standard_normal(b["kept"]).astype(np.float32)
    g.w = dt(w, dev)
    cut = b["n_src"] // 3
    part_of = np.where(b["col"] < cut, 0, 2)  # part 1 is empty
    sources = [(0, cut), (cut, 0), (cut, b["n_src"] - cut)]
    got = G.split_by_part(g, dt(part_of, dev), sources, accumulate_from=accumulate_from)
    want = ref.parts(b["rowptr"], b["col"], b["eid"], w, part_of, sources, accumulate_from=accumulate_from)
    assert len(got) == 3 and want[1]["kept"] == 0 and want[0]["kept"] > 0 and want[2]["kept"] > 0
    for k, (p, r) in enumerate(zip(got, want)):
        tag = f"part {k} "
        assert (p.n_src, p.n_dst, p.kept, p.n_input_edges, p.max_degree) == \
            (r["n_src"], b["n_dst"], r["kept"], r["kept"], r["max_degree"]), tag
        for f in ("rowptr", "col", "eid", "deg", "rows", "items", "split"):
            eq(host(getattr(p, f)), r[f], tag + f)
        eq(bits(host(p.w)), bits(r["w"]), tag + "w")
        assert (p.n_items, p.n_split, p.n_slots, p.split_len, p.n_long) == \
            (r["n_items"], r["n_split"], r["n_slots"], r["split_len"], r["n_long"]), tag
        assert ("accumulate_only" in p.extras) == (k >= accumulate_from and b["n_dst"] > 0), tag
        if k >= accumulate_from:
            assert bool((p.items[:, 2] > p.items[:, 1]).all()), tag  # no row it adds nothing to
    assert got[1].n_items == (0 if accumulate_from == 1 else b["n_dst"])


# ---------------------------------------------------------------------------
# argument errors: the return code only
# ---------------------------------------------------------------------------
def abi_csr(dev, src, dst, n_src, n_dst, flags, ws_short=0):
    L = nat.lib()
    E = len(src)
    src_t, dst_t = dt(np.asarray(src, np.int32), dev), dt(np.asarray(dst, np.int32), dev)
    cap = E + (n_dst if flags & nat.CSR_SELF_LOOPS else 0)
    i32 = dict(dtype=torch.int32, device=dev)
    f32 = dict(dtype=torch.float32, device=dev)
    rowptr, deg = torch.empty(n_dst + 1, **i32), torch.empty(max(n_dst, 1), **i32)
    col, eid = torch.empty(max(cap, 1), **i32), torch.empty(max(cap, 1), **i32)
    dinv, w = torch.empty(max(n_dst, 1), **f32), torch.empty(max(cap, 1), **f32)
    table = G.gcn_dinv_table(dev)
    nbytes = ctypes.c_size_t(0)
    assert L.kgx_csr_workspace_bytes(E, n_dst, flags, ctypes.byref(nbytes)) == nat.KGX_OK
    ws = torch.empty(max(nbytes.value, 1), dtype=torch.uint8, device=dev)
    info = (ctypes.c_int64 * 4)(-1, -1, -1, -1)
    rc = L.kgx_csr_build2(nat.ptr(src_t), nat.ptr(dst_t), E, n_src, n_dst, flags, nat.ptr(rowptr), nat.ptr(col),
                          nat.ptr(eid), nat.ptr(deg), nat.ptr(dinv), nat.ptr(w), nat.ptr(table), table.numel(),
                          nat.ptr(ws), nbytes.value - ws_short, info, nat.stream(dev))
    return rc, [int(v) for v in info]


def test_csr_build_argument_errors(dev):
    s, d = [0, 1, 2, 3], [1, 2, 3, 0]
    NORM, SEG, LOOPS = nat.CSR_GCN_NORM, nat.CSR_SEGMENT_ONLY, nat.CSR_SELF_LOOPS
    assert abi_csr(dev, s, d, 4, 4, NORM)[0] == nat.KGX_OK
    assert abi_csr(dev, s, d, 4, 4, NORM | LOOPS)[0] == nat.KGX_OK
    assert abi_csr(dev, s, d, 4, 4, SEG)[0] == nat.KGX_OK
    # dinv has n_dst entries and is read with the source id
    assert abi_csr(dev, s, d, 9, 4, NORM)[0] == nat.KGX_ERR_ARG
    assert abi_csr(dev, s, d, 4, 9, NORM)[0] == nat.KGX_ERR_ARG
    # SEGMENT_ONLY neither checks nor wraps the sources
    assert abi_csr(dev, s, d, 4, 4, NORM | SEG)[0] == nat.KGX_ERR_ARG
    assert abi_csr(dev, s, d, 4, 4, NORM | SEG | LOOPS)[0] == nat.KGX_ERR_ARG
    assert abi_csr(dev, s, d, 9, 4, LOOPS)[0] == nat.KGX_ERR_ARG
    assert abi_csr(dev, s, d, 4, 9, LOOPS)[0] == nat.KGX_ERR_ARG
    assert abi_csr(dev, s, d, 4, 4, 0, ws_short=1)[0] == nat.KGX_ERR_ARG
    assert abi_csr(dev, s, d, 4, 4, 0)[0] == nat.KGX_OK
    rowptr_t = dt(np.array([0, 1, 3, 3, 4], np.int32), dev)
    assert abi_schedule(rowptr_t, 2, 8, ws_short=1)[0] == nat.KGX_ERR_ARG
    assert abi_schedule(rowptr_t, 2, 8)[0] == nat.KGX_OK
    # default mode: ids outside [-n, n) are counted, one per bad edge
    rc, info = abi_csr(dev, [0, 4, -5, 1, 2, 9], [1, 2, 3, 4, -5, -9], 4, 4, 0)
    assert rc == nat.KGX_ERR_INDEX and info[2] == 5
    rc, info = abi_csr(dev, [0, -4, 3], [-4, 3, -1], 4, 4, 0)
    assert rc == nat.KGX_OK and info[0] == 1 and info[2] == 0


def test_build_csr_refuses_gcn_norm_misuse(dev):
    s, d = dt(np.array([0, 1, 2], np.int32), dev), dt(np.array([1, 2, 0], np.int32), dev)
    with pytest.raises(ValueError, match="n_src == n_dst"):
        G.build_csr(s, d, 7, 3, gcn_norm=True)
    with pytest.raises(ValueError, match="n_src == n_dst"):
        G.build_csr(s, d, 3, 7, gcn_norm=True)
    with pytest.raises(ValueError, match="segment_only"):
        G.build_csr(s, d, 3, 3, gcn_norm=True, segment_only=True)
    with pytest.raises(ValueError):
        G.build_csr(s, d, 7, 3, self_loops=True)
