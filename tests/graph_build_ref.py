"""numpy restatement of csrc/graph_build.hip's graph preparation: what
kgx_csr_build2, kgx_schedule_build, kgx_schedule_suffixes, kgx_tiny_pack,
kgx_gcn_edge_norm and kgx_select_dst_range must produce, and what
graph.restrict_rows / graph.split_by_part must return, as plain array code
(no torch, no library), plus the named graphs the tests build (CASES).

Everything here is integer-exact; edge_norm is one float32 multiply, which
numpy rounds correctly as __fmul_rn does, so it is bit-exact too.

The vectorised restatements are held to per-edge / per-row Python loops
written without sorting in tests/test_graph_build_ref_host.py.
"""

import numpy as np

from oracle.reference import csr_by_destination

INT32_MIN, INT32_MAX = -(2**31), 2**31 - 1
DEG_KEY_MAX = 2**24 - 1  # degrees at or above it tie in the schedule order (degree_key)
SHORT_ROW_MAX = 7        # KGX_SHORT_ROW_MAX


# ---------------------------------------------------------------------------
# CSR
# ---------------------------------------------------------------------------
def csr(src, dst, n_src, n_dst, *, self_loops=False, segment_only=False):
    """(rowptr, col, eid, deg, kept, max_degree) of kgx_csr_build2.

    Default mode is oracle.reference.csr_by_destination (negative src wrap,
    negative dst are dropped, anything outside [-n, n) raises IndexError).
    segment_only: an edge is kept iff 0 <= dst < n_dst, src is taken as is
    (neither checked nor wrapped) and nothing raises."""
    if not segment_only:
        rowptr, col, eid, deg = csr_by_destination(src, dst, n_src, n_dst, self_loops)
    else:
        src = np.asarray(src, dtype=np.int64)
        dst = np.asarray(dst, dtype=np.int64)
        E = src.shape[0]
        eid = np.arange(E, dtype=np.int64)
        if self_loops:
            loops = np.arange(n_dst, dtype=np.int64)
            src, dst, eid = np.concatenate([src, loops]), np.concatenate([dst, loops]), np.concatenate([eid, E + loops])
        keep = (dst >= 0) & (dst < n_dst)
        src, dst, eid = src[keep], dst[keep], eid[keep]
        order = np.argsort(dst, kind="stable")
        deg = np.bincount(dst, minlength=n_dst)[:n_dst].astype(np.int32)
        rowptr = np.zeros(n_dst + 1, dtype=np.int32)
        np.cumsum(deg, out=rowptr[1:])
        col, eid = src[order].astype(np.int32), eid[order].astype(np.int32)
    kept = int(rowptr[-1])
    return rowptr, col, eid, deg, kept, (int(deg.max()) if n_dst else 0)


# ---------------------------------------------------------------------------
# schedule
# ---------------------------------------------------------------------------
def schedule(rowptr, split_len):
    """(rows, items [n_items, 4], split [n_split, 4], n_slots) of kgx_schedule_build.

    rows: stable argsort of descending min(deg, 2^24 - 1).  Walking rows in
    that order, a row of degree d is split iff split_len > 0 and d >=
    split_len: it emits ceil(d / L) items {row, b, e, slot} with b = beg + c*L,
    e = min(end, b + L) and consecutive slots, and one split record {row,
    first_slot, n_chunks, d}; every other row emits {row, beg, end, -1}."""
    rowptr = np.asarray(rowptr, dtype=np.int64)
    n = rowptr.shape[0] - 1
    L = int(split_len)
    deg = np.diff(rowptr)
    rows = np.argsort(-np.minimum(deg, DEG_KEY_MAX), kind="stable")
    d, beg, end = deg[rows], rowptr[rows], rowptr[rows + 1]
    sp = (d >= L) if L > 0 else np.zeros(n, bool)
    nc = np.where(sp, -(-d // max(L, 1)), 1)
    off = np.cumsum(nc) - nc
    ns = np.where(sp, nc, 0)
    s_off = np.cumsum(ns) - ns
    n_items = int(nc.sum())
    pos = np.repeat(np.arange(n), nc)  # schedule position of every item
    c = np.arange(n_items) - off[pos]  # its chunk number
    b = beg[pos] + c * L
    e = np.where(sp[pos], np.minimum(end[pos], b + L), end[pos])
    slot = np.where(sp[pos], s_off[pos] + c, -1)
    items = np.stack([rows[pos], b, e, slot], 1).astype(np.int32).reshape(n_items, 4)
    split = np.stack([rows[sp], s_off[sp], nc[sp], d[sp]], 1).astype(np.int32).reshape(-1, 4)
    return rows.astype(np.int32), items, split, int(ns.sum())


def suffixes(items, short_max, tiny_max):
    """kgx_schedule_suffixes: for each bound, 1 + the last item that is split
    (slot >= 0) or longer than the bound; 0 if there is none."""
    items = np.asarray(items).reshape(-1, 4)
    ln = items[:, 2].astype(np.int64) - items[:, 1]
    out = []
    for bound in (short_max, tiny_max):
        hit = np.nonzero((items[:, 3] >= 0) | (ln > bound))[0]
        out.append(int(hit[-1]) + 1 if hit.size else 0)
    return tuple(out)


def tiny_records(items, start, n, col, w, n_col):
    """kgx_tiny_pack on items [start, start + n): (pack [n, 4] = {row, deg, col0,
    col1}, tw [n, 2] = {w0, w1} or None, (records of degree 2, 1 + the last of
    them)).  col1 = col0 for degree 1, both 0 for degree 0, weights 0 where
    absent; both edge indices are clamped to n_col - 1."""
    t = np.asarray(items).reshape(-1, 4)[start:start + n].astype(np.int64)
    deg = t[:, 2] - t[:, 1]
    last = n_col - 1
    i0 = np.minimum(t[:, 1], last)
    i1 = np.minimum(t[:, 1] + (deg > 1), last)
    col = np.asarray(col)
    c0 = np.where(deg > 0, col[i0], 0)
    c1 = np.where(deg > 0, col[i1], 0)
    pack = np.stack([t[:, 0], deg, c0, c1], 1).astype(np.int32).reshape(n, 4)
    tw = None
    if w is not None:
        w = np.asarray(w, np.float32)
        tw = np.stack([np.where(deg > 0, w[i0], np.float32(0)), np.where(deg > 1, w[i1], np.float32(0))],
                      1).astype(np.float32).reshape(n, 2)
    two = np.nonzero(deg == 2)[0]
    return pack, tw, (int(two.size), int(two[-1]) + 1 if two.size else 0)


# ---------------------------------------------------------------------------
# GCN edge norm, range selection
# ---------------------------------------------------------------------------
def edge_norm(rowptr, col, dinv_dst, dinv_src):
    """kgx_gcn_edge_norm: w[e] = dinv_dst[row(e)] * dinv_src[col[e]] in float32."""
    rowptr = np.asarray(rowptr, np.int64)
    row = np.repeat(np.arange(rowptr.shape[0] - 1), np.diff(rowptr))
    return np.asarray(dinv_dst, np.float32)[row] * np.asarray(dinv_src, np.float32)[np.asarray(col, np.int64)]


def select_dst_range(src, dst, lo, hi):
    """kgx_select_dst_range: the edges with lo <= dst < hi, input order kept."""
    src, dst = np.asarray(src), np.asarray(dst)
    m = (dst.astype(np.int64) >= lo) & (dst.astype(np.int64) < hi)
    return src[m], dst[m]


# ---------------------------------------------------------------------------
# graph.restrict_rows, graph.split_by_part
# ---------------------------------------------------------------------------
def restrict(items, split, row_mask):
    """(items, split, n_long) of graph.restrict_rows: both lists filtered in
    order by row_mask[row]; slots keep their numbers (n_slots is the parent's);
    n_long = the short-row suffix start of the filtered list."""
    items, split = np.asarray(items).reshape(-1, 4), np.asarray(split).reshape(-1, 4)
    row_mask = np.asarray(row_mask, bool)
    it = items[row_mask[items[:, 0]]]
    return it, split[row_mask[split[:, 0]]], suffixes(it, SHORT_ROW_MAX, SHORT_ROW_MAX)[0]


def default_split_len(n_edges, n_features=128):
    """graph.default_split_len restated (the chunk length split_by_part gives each part)."""
    lanes = max(1, (max(n_features, 1) + 3) // 4)
    G = min(64, 1 << (lanes - 1).bit_length())
    share = max(1, n_edges // (2048 * 256 // G))
    return int(min(8192, max(256, 1 << (max(share // 4, 1).bit_length() - 1))))


def parts(rowptr, col, eid, w, part_of, sources, accumulate_from=1):
    """graph.split_by_part: per part k a dict of rowptr / col / eid / w / deg /
    kept / max_degree (the row's edges with part_of == k in CSR order, col
    re-based to sources[k][0]) and its schedule from schedule() at
    default_split_len(kept): rows / items / split / n_items / n_split / n_slots
    / split_len / n_long.  Parts k >= accumulate_from are accumulate-only: the
    items of their zero-degree rows (the end of the list) are cut off."""
    rowptr = np.asarray(rowptr, np.int64)
    n_dst = rowptr.shape[0] - 1
    row = np.repeat(np.arange(n_dst), np.diff(rowptr))
    part_of = np.asarray(part_of)
    out = []
    for k, (base, n_src) in enumerate(sources):
        m = part_of == k
        deg = np.bincount(row[m], minlength=n_dst)[:n_dst].astype(np.int32)
        rp = np.zeros(n_dst + 1, np.int32)
        np.cumsum(deg, out=rp[1:])
        kept = int(m.sum())
        L = default_split_len(kept)
        rows, items, split, n_slots = schedule(rp, L)
        n_long = suffixes(items, SHORT_ROW_MAX, SHORT_ROW_MAX)[0]
        if k >= accumulate_from and items.shape[0]:
            items = items[: items.shape[0] - int((deg == 0).sum())]
            n_long = min(n_long, items.shape[0])
        out.append(dict(
            n_src=n_src, rowptr=rp, col=(np.asarray(col)[m] - base).astype(np.int32), eid=np.asarray(eid)[m],
            w=None if w is None else np.asarray(w)[m], deg=deg, kept=kept, max_degree=int(deg.max()) if n_dst else 0,
            rows=rows, items=items, split=split, n_items=int(items.shape[0]), n_split=int(split.shape[0]),
            n_slots=n_slots, split_len=L, n_long=n_long,
        ))
    return out


# ---------------------------------------------------------------------------
# the named graphs: name -> () -> (src, dst, n_src, n_dst, build_csr kwargs, split_len)
# ---------------------------------------------------------------------------
def _i32(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.int64).astype(np.int32))


def _edges_for_degrees(rng, deg, n_src):
    """A shuffled edge list giving row r exactly deg[r] in-edges from random sources."""
    dst = np.repeat(np.arange(len(deg)), deg)
    src = rng.integers(0, n_src, dst.shape[0])
    p = rng.permutation(dst.shape[0])
    return src[p], dst[p]


def ladder_degrees(L):
    """The degrees a ladder(L) graph holds, two rows each."""
    return sorted({0, 1, 2, 3, 7, 8, 9, 63, 64, 65, 66, L - 1, L, L + 1, 2 * L - 1, 2 * L, 2 * L + 1, 3 * L + 5})


def _ladder(L, loops):
    """Two rows at every degree of ladder_degrees(L), at shuffled row ids (the
    schedule order is not the row order), random sources, shuffled edge order.
    With self-loops the input edges are one fewer per row, so the built graph
    holds the same degrees (degree 0 cannot exist then: those rows have 1)."""
    def make():
        rng = np.random.default_rng(1000 + L + (500 if loops else 0))
        final = np.repeat(ladder_degrees(L), 2)
        n = final.shape[0]
        deg = np.zeros(n, np.int64)
        deg[rng.permutation(n)] = np.maximum(final - 1, 0) if loops else final
        src, dst = _edges_for_degrees(rng, deg, n)
        return _i32(src), _i32(dst), n, n, dict(self_loops=loops), L
    return make


def _keybits(n_dst):
    def make():
        rng = np.random.default_rng(2000 + n_dst)
        E = 3 * n_dst + 1
        n_src = 77
        src = rng.integers(0, n_src, E)
        dst = rng.integers(0, n_dst, E)
        dst[rng.random(E) < 0.125] = -1  # dropped: their sort key is n_dst itself
        dst[0], dst[1] = -1, n_dst - 1
        return _i32(src), _i32(dst), n_src, n_dst, {}, 16
    return make


def _coltail(kept, dropped):
    def make():
        rng = np.random.default_rng(3000 + kept + dropped)
        n = 300
        src = rng.integers(0, n, kept + dropped)
        dst = rng.integers(0, n, kept + dropped)
        dst[rng.permutation(kept + dropped)[:dropped]] = -1
        return _i32(src), _i32(dst), n, n, {}, 64
    return make


def _bipartite(n_src, n_dst, E, seed):
    def make():
        rng = np.random.default_rng(seed)
        src = rng.integers(0, n_src, E)
        dst = rng.integers(0, n_dst, E)
        src[E // 2:E // 2 + 40], dst[E // 2:E // 2 + 40] = src[:40], dst[:40]  # exact duplicates
        return _i32(src), _i32(dst), n_src, n_dst, {}, 16
    return make


def _wrap():
    rng = np.random.default_rng(4000)
    n, E = 200, 1500
    src = rng.integers(-n, n, E)
    dst = rng.integers(-n, n, E)
    src[:4], dst[:4] = [-n, -1, -n, -1], [5, 6, -n, -1]  # both ends of both negative ranges
    loops = rng.integers(0, n, 30)
    src[10:40], dst[10:40] = loops, loops                # self loops already in the input
    src[40:50], dst[40:50] = loops[:10] - n, loops[:10]  # ... and written with a wrapping source
    src[100:160], dst[100:160] = src[200:260], dst[200:260]  # exact duplicates
    return _i32(src), _i32(dst), n, n, dict(self_loops=True), 8


SEGMENT_OUT_OF_RANGE = ("-1", "n_dst", "n_dst+7", "INT32_MIN", "INT32_MAX")


def segment_out_of_range_values(n_dst):
    return [-1, n_dst, n_dst + 7, INT32_MIN, INT32_MAX]


def SEGMENT_RAW_SOURCES(n_src):
    return [-1, -n_src, n_src, n_src + 9, INT32_MIN, INT32_MAX]


def _segment(n_dst, mode):
    def make():
        rng = np.random.default_rng(5000 + n_dst + len(mode))
        n_src, E = 100, 500
        src = rng.integers(0, n_src, E)
        bad = np.array(segment_out_of_range_values(n_dst))
        dst = bad[rng.integers(0, bad.shape[0], E)]
        if mode in ("mixed", "rawsrc"):
            ok = rng.random(E) < 0.7
            dst = np.where(ok, rng.integers(0, n_dst, E), dst)
            dst[:5] = bad
        if mode == "rawsrc":  # sources are taken as they are, whatever they hold
            src[10:16] = SEGMENT_RAW_SOURCES(n_src)
            dst[10:16] = rng.integers(0, n_dst, 6)
        return _i32(src), _i32(dst), n_src, n_dst, dict(segment_only=True), 16
    return make


def _empty(n_dst, loops):
    def make():
        z = np.zeros(0, np.int32)
        return z, z.copy(), n_dst, n_dst, dict(self_loops=loops), 16
    return make


ONEHUB_DEGREE = 5000


def _onehub(L):
    def make():
        rng = np.random.default_rng(6000)
        n_src, n_dst = 300, 7
        return (_i32(rng.integers(0, n_src, ONEHUB_DEGREE)), _i32(np.full(ONEHUB_DEGREE, 3)), n_src, n_dst, {}, L)
    return make


# The one large case: the sizes come from the grid caps of graph_build.hip (blocks of 256 threads).
STRIDE_N = 8192 * 256 + 321
STRIDE_E = 6_400_000
STRIDE_HUB = 200


def _stride():
    rng = np.random.default_rng(7000)
    n, E = STRIDE_N, STRIDE_E
    # every fifth row takes input edges, so four fifths have the self loop alone
    dst = rng.integers(0, n // 5, E) * 5
    src = rng.integers(0, n, E)
    at = rng.permutation(E)[:STRIDE_HUB]
    dst[at] = n - 1  # a long row in the second trip of the row-strided loops
    return _i32(src), _i32(dst), n, n, dict(self_loops=True, gcn_norm=True), 64


CASES = {}
for _L in (2, 16, 64):
    CASES[f"ladder{_L}"] = _ladder(_L, False)
    CASES[f"ladder{_L}_loops"] = _ladder(_L, True)
KEYBITS_N = (1, 2, 3, 255, 256, 257, 1023, 1024, 1025, 65535, 65536, 65537)
for _n in KEYBITS_N:
    CASES[f"keybits{_n}"] = _keybits(_n)
COLTAIL_KEPT = (1, 1023, 1024, 1025, 2047, 2049)
COLTAIL_DROPPED = 37
for _k in COLTAIL_KEPT:
    CASES[f"coltail{_k}"] = _coltail(_k, 0)
    CASES[f"coltail{_k}_dropped"] = _coltail(_k, COLTAIL_DROPPED)
CASES["bipartite_wide"] = _bipartite(2000, 50, 3000, 11)
CASES["bipartite_tall"] = _bipartite(50, 2000, 400, 12)
CASES["wrap"] = _wrap
CASES["segment"] = _segment(40, "mixed")
CASES["segment_rawsrc"] = _segment(40, "rawsrc")
CASES["segment_all_dropped"] = _segment(40, "dropped")
CASES["segment_n0"] = _segment(0, "dropped")
for _n in (0, 1, 300):
    CASES[f"empty{_n}"] = _empty(_n, False)
    CASES[f"empty{_n}_loops"] = _empty(_n, True)
ONEHUB_SPLIT = (0, 1, 64, 4096, 8192)
for _L in ONEHUB_SPLIT:
    CASES[f"onehub_split{_L}"] = _onehub(_L)
CASES["stride"] = _stride

SMALL_CASES = [k for k in CASES if k != "stride"]
LADDERS = [k for k in CASES if k.startswith("ladder")]

_BUILT = {}


def built(name):
    """The case's inputs with its expected CSR and schedule, computed once per
    process and shared (read-only) by the tests: a namespace-like dict with src,
    dst, n_src, n_dst, kw, split_len, rowptr, col, eid, deg, kept, max_degree,
    rows, items, split, n_slots."""
    b = _BUILT.get(name)
    if b is None:
        src, dst, n_src, n_dst, kw, split_len = CASES[name]()
        flags = {k: v for k, v in kw.items() if k != "gcn_norm"}
        rowptr, col, eid, deg, kept, max_degree = csr(src, dst, n_src, n_dst, **flags)
        rows, items, split, n_slots = schedule(rowptr, split_len)
        b = dict(name=name, src=src, dst=dst, n_src=n_src, n_dst=n_dst, kw=kw, split_len=split_len, rowptr=rowptr,
                 col=col, eid=eid, deg=deg, kept=kept, max_degree=max_degree, rows=rows, items=items, split=split,
                 n_slots=n_slots)
        for v in b.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        if name != "stride":  # the large one is dropped by the fixture that owns it
            _BUILT[name] = b
    return b
