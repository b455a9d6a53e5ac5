"""tests/graph_build_ref.py checked on the host: the vectorised restatement of
the CSR build, the schedule, the tails, the edge norm, the range selection and
the restricted / split graphs against per-edge and per-row Python loops written
without sorting; the schedule's invariants on every case; and every named case
really being what its name says, so that none of them goes vacuous."""

import numpy as np
import pytest

import graph_build_ref as ref

BRUTE_MAX_EDGES = 5000


def _brute_cases():
    out = []
    for name in ref.SMALL_CASES:
        n = name[len("keybits"):] if name.startswith("keybits") else ""
        if n.isdigit() and 3 * int(n) + 1 > BRUTE_MAX_EDGES:
            continue
        out.append(name)
    return out


# ---------------------------------------------------------------------------
# brute force: Python loops, no sort
# ---------------------------------------------------------------------------
def brute_csr(src, dst, n_src, n_dst, self_loops=False, segment_only=False):
    E = len(src)
    rows = [[] for _ in range(n_dst)]
    for e in range(E):
        s, d = int(src[e]), int(dst[e])
        if segment_only:
            if 0 <= d < n_dst:
                rows[d].append((s, e))
            continue
        assert -n_src <= s < n_src and -n_dst <= d < n_dst
        if s < 0:
            s += n_src
        if d >= 0:
            rows[d].append((s, e))
    if self_loops:
        for i in range(n_dst):
            rows[i].append((i, E + i))
    rowptr, col, eid = [0], [], []
    for r in rows:
        col += [s for s, _ in r]
        eid += [e for _, e in r]
        rowptr.append(len(col))
    deg = [len(r) for r in rows]
    return rowptr, col, eid, deg, len(col), max(deg, default=0)


def brute_schedule(rowptr, L):
    n = len(rowptr) - 1
    deg = [int(rowptr[r + 1] - rowptr[r]) for r in range(n)]
    by_key = {}
    for r in range(n):  # ascending row id inside every degree class
        by_key.setdefault(min(deg[r], ref.DEG_KEY_MAX), []).append(r)
    rows = []
    for k in range(max(by_key, default=-1), -1, -1):
        rows += by_key.get(k, [])
    items, split, slot = [], [], 0
    for r in rows:
        beg, end = int(rowptr[r]), int(rowptr[r + 1])
        if L > 0 and deg[r] >= L:
            first = slot
            b = beg
            while b < end:
                items.append([r, b, min(end, b + L), slot])
                slot += 1
                b += L
            split.append([r, first, slot - first, deg[r]])
        else:
            items.append([r, beg, end, -1])
    return rows, items, split, slot


def _eq(a, b, what=""):
    np.testing.assert_array_equal(np.asarray(a), np.asarray(b), err_msg=what)


@pytest.mark.parametrize("name", _brute_cases())
def test_restatement_equals_brute_force(name):
    b = ref.built(name)
    flags = {k: v for k, v in b["kw"].items() if k != "gcn_norm"}
    rowptr, col, eid, deg, kept, mx = brute_csr(b["src"], b["dst"], b["n_src"], b["n_dst"], **flags)
    _eq(b["rowptr"], rowptr, "rowptr")
    _eq(b["col"], np.asarray(col, np.int64), "col")
    _eq(b["eid"], np.asarray(eid, np.int64), "eid")
    _eq(b["deg"], np.asarray(deg, np.int64), "deg")
    assert (b["kept"], b["max_degree"]) == (kept, mx)
    for L in sorted({b["split_len"], 0, 1, 4}):
        rows, items, split, n_slots = ref.schedule(b["rowptr"], L)
        brows, bitems, bsplit, bslots = brute_schedule(b["rowptr"], L)
        _eq(rows, np.asarray(brows, np.int64), f"rows L={L}")
        _eq(items, np.asarray(bitems, np.int64).reshape(-1, 4), f"items L={L}")
        _eq(split, np.asarray(bsplit, np.int64).reshape(-1, 4), f"split L={L}")
        assert n_slots == bslots


def test_default_mode_raises_like_take():
    with pytest.raises(IndexError):
        ref.csr([0, 1, 15], [1, 2, 3], 10, 10)
    with pytest.raises(IndexError):
        ref.csr([0, 1], [1, -11], 10, 10)
    ref.csr([0, 15], [1, -11], 10, 10, segment_only=True)  # no IndexError


def test_degree_key_saturates():
    """Degrees at or above 2^24 - 1 tie: such rows keep their row order."""
    deg = np.array([3, 2**24 + 5, 2**24 - 1, 2**24 - 2, 2**24], np.int64)
    rowptr = np.concatenate([[0], np.cumsum(deg)])
    rows, items, split, n_slots = ref.schedule(rowptr, 2**23)
    _eq(rows, [1, 2, 4, 3, 0])
    assert split.shape[0] == 4 and n_slots == 3 + 2 + 2 + 2
    _eq(split[:, 0], [1, 2, 4, 3])
    _eq(split[:, 2], [3, 2, 2, 2])


@pytest.mark.parametrize("name", ["ladder2", "ladder16_loops", "onehub_split64", "bipartite_tall", "empty300"])
def test_tails_equal_brute_force(name):
    b = ref.built(name)
    items, col = b["items"], b["col"]
    rng = np.random.default_rng(1)
    w = rng.standard_normal(max(b["kept"], 1)).astype(np.float32)
    for bound in (0, 2, 7, 64):
        last = 0
        for i, (r, s, e, slot) in enumerate(items.tolist()):
            if slot >= 0 or e - s > bound:
                last = i + 1
        assert ref.suffixes(items, bound, bound) == (last, last)
    shuffled = items[rng.permutation(items.shape[0])]  # not degree-descending any more
    n_col = max(b["kept"], 1)
    colx = col if b["kept"] else np.zeros(1, np.int32)
    for its in (items, shuffled):
        for start in sorted({0, ref.suffixes(its, 2, 2)[1], max(its.shape[0] - 1, 0), its.shape[0]}):
            n = its.shape[0] - start
            pack, tw, (cnt, last2) = ref.tiny_records(its, start, n, colx, w, n_col)
            bc = bl = 0
            for i, (r, s, e, slot) in enumerate(its[start:].tolist()):
                d = e - s
                i0, i1 = min(s, n_col - 1), min(s + (1 if d > 1 else 0), n_col - 1)
                assert pack[i].tolist() == [r, d, int(colx[i0]) if d > 0 else 0, int(colx[i1]) if d > 0 else 0]
                assert tw[i].tolist() == [float(w[i0]) if d > 0 else 0.0, float(w[i1]) if d > 1 else 0.0]
                if d == 2:
                    bc, bl = bc + 1, i + 1
            assert (cnt, last2) == (bc, bl)
            assert ref.tiny_records(its, start, n, colx, None, n_col)[1] is None


def test_edge_norm_and_select_equal_brute_force():
    b = ref.built("bipartite_wide")
    rng = np.random.default_rng(2)
    dd = rng.random(b["n_dst"]).astype(np.float32) + np.float32(0.01)
    ds = rng.random(b["n_src"]).astype(np.float32) + np.float32(0.01)
    w = ref.edge_norm(b["rowptr"], b["col"], dd, ds)
    assert w.dtype == np.float32
    for r in range(b["n_dst"]):
        for e in range(b["rowptr"][r], b["rowptr"][r + 1]):
            assert w[e] == np.float32(dd[r]) * np.float32(ds[b["col"][e]])
    for lo, hi in ((0, 0), (0, b["n_dst"]), (10, 30), (30, 10), (-5, 7)):
        s, d = ref.select_dst_range(b["src"], b["dst"], lo, hi)
        want = [(int(x), int(y)) for x, y in zip(b["src"], b["dst"]) if lo <= y < hi]
        assert list(zip(s.tolist(), d.tolist())) == want


@pytest.mark.parametrize("name", ["ladder16", "bipartite_wide"])
def test_restrict_and_parts_equal_brute_force(name):
    b = ref.built(name)
    rng = np.random.default_rng(3)
    mask = rng.random(b["n_dst"]) < 0.5
    it, sp, n_long = ref.restrict(b["items"], b["split"], mask)
    assert it.tolist() == [v for v in b["items"].tolist() if mask[v[0]]]
    assert sp.tolist() == [v for v in b["split"].tolist() if mask[v[0]]]
    assert n_long == ref.suffixes(it, 7, 7)[0]
    part_of = rng.integers(0, 2, b["kept"]) * 2  # parts 0 and 2; part 1 stays empty
    bases = [(0, b["n_src"]), (3, b["n_src"] - 3), (0, b["n_src"])]
    w = rng.standard_normal(b["kept"]).astype(np.float32)
    for acc in (1, 3):
        got = ref.parts(b["rowptr"], b["col"], b["eid"], w, part_of, bases, accumulate_from=acc)
        for k, p in enumerate(got):
            rows = [[] for _ in range(b["n_dst"])]
            for r in range(b["n_dst"]):
                for e in range(b["rowptr"][r], b["rowptr"][r + 1]):
                    if part_of[e] == k:
                        rows[r].append(e)
            flat = [e for r in rows for e in r]
            _eq(p["col"], b["col"][flat] - bases[k][0])
            _eq(p["eid"], b["eid"][flat])
            _eq(p["w"], w[flat])
            _eq(p["deg"], [len(r) for r in rows])
            _eq(p["rowptr"], np.concatenate([[0], np.cumsum([len(r) for r in rows])]))
            assert p["split_len"] == 256 and p["kept"] == len(flat)
            brows, bitems, bsplit, bslots = brute_schedule(p["rowptr"], 256)
            if k >= acc:
                bitems = [v for v in bitems if v[2] > v[1]]
            _eq(p["rows"], np.asarray(brows, np.int64))
            _eq(p["items"], np.asarray(bitems, np.int64).reshape(-1, 4))
            _eq(p["split"], np.asarray(bsplit, np.int64).reshape(-1, 4))
            assert p["n_items"] == len(bitems) and p["n_slots"] == bslots
            assert p["n_long"] == ref.suffixes(p["items"], 7, 7)[0]


def test_default_split_len_restated():
    """Pinned values of graph.default_split_len (the package cannot be imported
    without torch; tests/test_gpu_graph_build.py holds the two equal)."""
    assert [ref.default_split_len(e) for e in (0, 5000, 16384 * 1024, 16384 * 4096, 10**9)] == \
        [256, 256, 256, 1024, 8192]


# ---------------------------------------------------------------------------
# schedule invariants, every case
# ---------------------------------------------------------------------------
def check_schedule_invariants(rowptr, kept, L, rows, items, split, n_slots):
    rowptr = np.asarray(rowptr, np.int64)
    n = rowptr.shape[0] - 1
    deg = np.diff(rowptr)
    _eq(np.sort(rows), np.arange(n), "rows is a permutation")
    it = items.astype(np.int64)
    r, b, e, s = it[:, 0], it[:, 1], it[:, 2], it[:, 3]
    assert np.all((rowptr[r] <= b) & (b <= e) & (e <= rowptr[r + 1])), "an item leaves its row"
    # items cover [0, kept) exactly once
    nz = e > b
    order = np.argsort(b[nz], kind="stable")
    bb, ee = b[nz][order], e[nz][order]
    if kept:
        assert bb[0] == 0 and ee[-1] == kept and np.all(ee[:-1] == bb[1:]), "items do not tile [0, kept)"
    else:
        assert bb.size == 0
    # slots are exactly 0 .. n_slots-1, each used once, in item order
    at = np.nonzero(s >= 0)[0]
    _eq(s[at], np.arange(n_slots), "slots")
    # every split record's chunks are that row's items, in order
    sp = split.astype(np.int64)
    is_split = (deg >= L) if L > 0 else np.zeros(n, bool)
    assert sp.shape[0] == int(is_split.sum()), "n_split != count(deg >= L)"
    if sp.shape[0]:
        _eq(np.sort(sp[:, 0]), np.nonzero(is_split)[0], "split rows")
        _eq(sp[:, 3], deg[sp[:, 0]], "split degree")
        _eq(sp[:, 2], -(-sp[:, 3] // L), "n_chunks")
        _eq(sp[:, 1], np.cumsum(sp[:, 2]) - sp[:, 2], "first_slot")
        rec = np.repeat(np.arange(sp.shape[0]), sp[:, 2])
        c = np.arange(rec.shape[0]) - sp[rec, 1]
        _eq(at, at[0] + np.arange(at.shape[0]), "split items are consecutive")
        _eq(r[at], sp[rec, 0], "chunk row")
        _eq(b[at], rowptr[sp[rec, 0]] + c * L, "chunk begin")
        _eq(e[at], np.minimum(rowptr[sp[rec, 0] + 1], b[at] + L), "chunk end")
    # one item per unsplit row
    un = s < 0
    _eq(np.sort(r[un]), np.nonzero(~is_split)[0], "unsplit rows")
    assert np.all((b[un] == rowptr[r[un]]) & (e[un] == rowptr[r[un] + 1]))


@pytest.fixture(scope="module")
def stride():
    return ref.built("stride")


def _case(name, stride):
    return stride if name == "stride" else ref.built(name)


@pytest.mark.parametrize("name", list(ref.CASES))
def test_schedule_invariants(name, request):
    b = _case(name, request.getfixturevalue("stride") if name == "stride" else None)
    check_schedule_invariants(b["rowptr"], b["kept"], b["split_len"], b["rows"], b["items"], b["split"], b["n_slots"])
    d = b["deg"].astype(np.int64)[b["rows"]]
    assert np.all(np.diff(d) <= 0)
    assert np.all(np.diff(b["rows"])[np.diff(d) == 0] > 0)


# ---------------------------------------------------------------------------
# every case is what its name says
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", ref.LADDERS)
def test_ladder_holds_its_degrees(name):
    b = ref.built(name)
    L = b["split_len"]
    loops = bool(b["kw"].get("self_loops"))
    count = np.bincount(b["deg"])
    for d in ref.ladder_degrees(L):
        if d == 0 and loops:
            continue
        assert count[d] == (4 if loops and d == 1 else 2), (d, count[d])
    for d in (0, 1, 2, 3, 7, 8, 9, 63, 64, 65, 66, L - 1, L, L + 1, 2 * L - 1, 2 * L, 2 * L + 1, 3 * L + 5):
        assert d in ref.ladder_degrees(L)
    assert not np.all(np.diff(b["rows"]) > 0)  # schedule order is not row order
    assert not np.all(np.diff(b["dst"]) >= 0)  # input order is not CSR order
    assert 0 < b["split"].shape[0] < b["n_dst"]


@pytest.mark.parametrize("n_dst", ref.KEYBITS_N)
def test_keybits_has_kept_and_dropped(n_dst):
    b = ref.built(f"keybits{n_dst}")
    E = b["src"].shape[0]
    assert b["n_dst"] == n_dst and E == 3 * n_dst + 1
    assert b["kept"] > 0 and E - b["kept"] > 0
    assert b["deg"][n_dst - 1] > 0  # the highest row key is in play, next to the dropped bucket's


@pytest.mark.parametrize("kept", ref.COLTAIL_KEPT)
def test_coltail_has_its_kept(kept):
    a, d = ref.built(f"coltail{kept}"), ref.built(f"coltail{kept}_dropped")
    assert a["kept"] == kept == a["src"].shape[0] and a["n_dst"] == 300 and not a["kw"]
    assert d["kept"] == kept and d["src"].shape[0] == kept + ref.COLTAIL_DROPPED == kept + 37
    at = np.nonzero(d["dst"] < 0)[0]
    assert at.shape[0] == 37 and (kept == 1 or at.max() - at.min() > 37)  # mixed in, not appended


def test_bipartite_cases():
    w, t = ref.built("bipartite_wide"), ref.built("bipartite_tall")
    assert (w["n_src"], w["n_dst"], t["n_src"], t["n_dst"]) == (2000, 50, 50, 2000)
    for b in (w, t):
        pairs = b["src"].astype(np.int64) * 10**6 + b["dst"]
        assert np.unique(pairs).shape[0] < pairs.shape[0]  # duplicates
        assert b["col"].max() < b["n_src"]
    assert (t["deg"] == 0).mean() > 0.5
    assert w["split"].shape[0] > 0


def test_wrap_case():
    b = ref.built("wrap")
    n, E = b["n_dst"], b["src"].shape[0]
    s, d = b["src"], b["dst"]
    assert b["kw"] == dict(self_loops=True) and b["n_src"] == n
    assert s.min() == -n and (s == -1).any() and d.min() == -n and (d == -1).any()
    assert set(np.unique(s[s < 0])) >= {-n, -1} and np.unique(s[s < 0]).shape[0] > n // 2
    assert b["kept"] == int((d >= 0).sum()) + n
    sw = np.where(s < 0, s + n, s)
    assert ((sw == d) & (d >= 0)).sum() >= 30 and ((s < 0) & (sw == d)).any()  # input self loops
    pairs = s.astype(np.int64) * 10**6 + d
    assert np.unique(pairs).shape[0] < E
    _eq(np.sort(b["eid"][b["eid"] >= E]), E + np.arange(n))  # loop ids E + i
    _eq(b["eid"][b["rowptr"][1:] - 1], E + np.arange(n))  # each last in its row


def test_segment_cases():
    b = ref.built("segment")
    assert b["kw"] == dict(segment_only=True)
    for v in ref.segment_out_of_range_values(b["n_dst"]):
        assert (b["dst"] == v).any(), v
    assert 0 < b["kept"] < 500 and b["src"].min() >= 0 and b["src"].max() < b["n_src"]
    raw = ref.built("segment_rawsrc")
    for v in ref.SEGMENT_RAW_SOURCES(raw["n_src"]):  # kept with the source exactly as given
        assert (raw["col"] == v).any(), v
    for name, n_dst in (("segment_all_dropped", 40), ("segment_n0", 0)):
        z = ref.built(name)
        assert z["n_dst"] == n_dst and z["src"].shape[0] == 500 and z["kept"] == 0
        assert z["rowptr"].tolist() == [0] * (n_dst + 1)


def test_empty_and_onehub_cases():
    for n in (0, 1, 300):
        a, l = ref.built(f"empty{n}"), ref.built(f"empty{n}_loops")
        assert a["src"].shape[0] == l["src"].shape[0] == 0 and a["n_dst"] == l["n_dst"] == n
        assert a["kept"] == 0 and l["kept"] == n
    for L in ref.ONEHUB_SPLIT:
        b = ref.built(f"onehub_split{L}")
        assert b["max_degree"] == 5000 == b["kept"] and (b["deg"] > 0).sum() == 1 and b["split_len"] == L
    n_chunks = {L: int((ref.built(f"onehub_split{L}")["items"][:, 3] >= 0).sum()) for L in ref.ONEHUB_SPLIT}
    assert n_chunks == {0: 0, 1: 5000, 64: 79, 4096: 2, 8192: 0}
    assert ref.built("onehub_split64")["items"][78].tolist()[1:] == [78 * 64, 5000, 78]  # the short last chunk


def test_stride_meets_its_inequalities(stride):
    b = stride
    n, E = b["n_dst"], b["src"].shape[0]
    block = 256
    assert (n, E) == (8192 * 256 + 321, 6_400_000) and b["kw"] == dict(self_loops=True, gcn_norm=True)
    assert b["kept"] == E + n > kept_per_trip(block)  # csr_col: 4 slots per thread, 8192 blocks
    assert n + 1 > 8192 * block  # csr_rowptr, sched_*, the long-row norm kernel
    assert n > 1024 * block  # csr_deg and the suffix kernel
    start = ref.suffixes(b["items"], 2, 2)[1]
    assert b["items"].shape[0] - start >= 2048 * block + 1  # tiny_pack
    assert np.bincount(b["dst"], minlength=n)[:n].astype(bool).mean() <= 0.25  # >= 3/4 take no input edge
    assert b["deg"][n - 1] == 201 and n - 1 >= 8192 * block  # the far hub: loop trips 2 do work
    assert b["split"].shape[0] >= 1 and b["split"][0].tolist() == [n - 1, 0, 4, 201]


def kept_per_trip(block):
    return 4 * 8192 * block
