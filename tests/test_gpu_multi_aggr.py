"""kgx_multi_aggr at op level (GPU): one gather, several reducers.

Boundary graph (tests/multi_aggr_ref.py): 80 rows, split_len 16, row degrees
0, 1, 2, around the kernel's gathers in flight U (6, or 4 for F > 256), 15 / 16 /
17, 33 (three chunks, the last of one edge) and 100, duplicate edges, a self
loop and a source nobody reads.  F in 1, 3, 4, 100, 128, 260: every vector
width, G from 1 to 64, one and two column tiles.

EXACT mode: every block equals the single-reducer EXACT kernel bit for bit
(std included: the operation sequence is the same), also on a table with
+-inf, NaN, +-0, an all-equal row and a three-way max tie.  Scheduled mode:
sum / mean / max / min equal the scheduled single-reducer kernels bit for bit;
std equals EXACT std on unsplit rows and the float64 restatement within 1e-5
scaled on split rows (the chunked M2 merge re-associates; a numpy simulation of
it stays below 3e-6 for these inputs).  Backward: composed from existing
kernels, against float64 autograd and against the concatenated single-reducer
ops, within 1e-5 scaled, NaN positions included.
"""

import functools

import numpy as np
import pytest
import torch

import multi_aggr_ref as MR

pytestmark = pytest.mark.gpu

FS = [1, 3, 4, 100, 128, 260]
TOL = 1e-5


@functools.lru_cache(maxsize=None)
def _boundary(F):
    from keras_geometric_amd import build_csr

    dev = torch.device("cuda", 0)
    src, dst, degs = MR.boundary_graph()
    n = len(degs)
    g = build_csr(torch.as_tensor(src, device=dev), torch.as_tensor(dst, device=dev), n, n,
                  split_len=MR.SPLIT_LEN, n_features=F)
    assert g.n_split >= 3, "the split path would be skipped"
    assert g.split_len == MR.SPLIT_LEN and g.kept == len(src)
    return g, src, dst, degs


@functools.lru_cache(maxsize=None)
def _finite(F):
    from keras_geometric_amd import build_csr

    dev = torch.device("cuda", 0)
    src, dst = MR.finite_graph()
    n = 60
    g = build_csr(torch.as_tensor(src, device=dev), torch.as_tensor(dst, device=dev), n, n,
                  split_len=MR.SPLIT_LEN, n_features=F)
    assert g.n_split >= 3 and int(g.deg.min()) >= 2
    return g, src, dst


def _singles(g, x, exact, by_edge=False):
    from keras_geometric_amd import ops

    return {n: ops.aggregate(g, x, n, exact=exact, by_edge=by_edge) for n in MR.ALL_FIVE}


def _assert_blocks_equal(out, names, singles, F):
    assert out.shape == (singles[names[0]].shape[0], len(names) * F)
    for k, name in enumerate(names):
        torch.testing.assert_close(out[:, k * F:(k + 1) * F], singles[name], rtol=0, atol=0, equal_nan=True,
                                   msg=lambda m, name=name: f"block {name} of {names}: {m}")


@pytest.mark.parametrize("special", [False, True], ids=["normal", "special"])
@pytest.mark.parametrize("F", FS)
def test_exact_blocks_equal_single_reducers(dev, F, special):
    from keras_geometric_amd import ops

    g, src, dst, degs = _boundary(F)
    n = len(degs)
    x = (MR.special_features(n, F, src, dst) if special else MR.features(n, F)).to(dev)
    singles = _singles(g, x, exact=True)
    for names in MR.REDUCER_LISTS:
        out = ops.multi_aggregate(g, x, names, exact=True)
        _assert_blocks_equal(out, names, singles, F)
    # empty rows give 0 in every block
    assert not out[torch.as_tensor(degs == 0, device=dev)].any()


@pytest.mark.parametrize("F", FS)
def test_scheduled_blocks(dev, F):
    from keras_geometric_amd import ops

    g, src, dst, degs = _boundary(F)
    n = len(degs)
    x = MR.features(n, F).to(dev)
    sched = _singles(g, x, exact=False)
    exact_std = ops.aggregate(g, x, "std", exact=True)
    f64_std = MR.aggregate_f64("std", x.cpu()[torch.as_tensor(src).long()], torch.as_tensor(dst), n)
    split_rows = torch.as_tensor(degs >= MR.SPLIT_LEN)
    assert int(split_rows.sum()) == g.n_split
    for names in MR.REDUCER_LISTS:
        out = ops.multi_aggregate(g, x, names)
        for k, name in enumerate(names):
            blk = out[:, k * F:(k + 1) * F]
            if name != "std":
                torch.testing.assert_close(blk, sched[name], rtol=0, atol=0, msg=f"block {name} of {names}")
                continue
            torch.testing.assert_close(blk[~split_rows.to(dev)], exact_std[~split_rows.to(dev)], rtol=0, atol=0)
            err = MR.scaled_err(blk.cpu()[split_rows], f64_std[split_rows])
            print(f"F={F} {names}: scheduled std on split rows, scaled err {err:.3e}")
            assert err <= TOL


@pytest.mark.parametrize("F", FS)
def test_by_edge_matches_the_aggregators(dev, F):
    from keras_geometric_amd import ops
    from keras_geometric_amd.layers import AggregatorFactory

    g, src, dst, degs = _boundary(F)
    n = len(degs)
    msg = MR.features(len(src), F, seed=4).to(dev)  # one row per INPUT edge
    tgt = torch.as_tensor(dst, device=dev)
    f64_std = MR.aggregate_f64("std", msg.cpu(), torch.as_tensor(dst), n)
    for exact in (True, False):
        singles = {name: AggregatorFactory.create(name).aggregate(msg, tgt, n, graph=g, exact=exact)
                   for name in MR.ALL_FIVE}
        out = ops.multi_aggregate(g, msg, MR.ALL_FIVE, by_edge=True, exact=exact)
        multi = AggregatorFactory.create_multi(MR.ALL_FIVE).aggregate(msg, tgt, n, graph=g, exact=exact)
        assert torch.equal(out, multi)
        for k, name in enumerate(MR.ALL_FIVE):
            blk = out[:, k * F:(k + 1) * F]
            if exact or name != "std":
                torch.testing.assert_close(blk, singles[name], rtol=0, atol=0, equal_nan=True, msg=name)
            else:
                assert MR.scaled_err(blk.cpu(), f64_std) <= TOL


@pytest.mark.parametrize("F", [4, 260])
def test_scheduled_run_to_run_bit_identical(dev, F):
    from keras_geometric_amd import ops

    g, src, dst, degs = _boundary(F)
    x = MR.features(len(degs), F).to(dev)
    a = ops.multi_aggregate(g, x, MR.ALL_FIVE)
    b = ops.multi_aggregate(g, x, MR.ALL_FIVE)
    assert torch.equal(a, b)


def test_no_edges_and_no_rows(dev):
    from keras_geometric_amd import build_csr, ops

    e = torch.empty(0, dtype=torch.int32, device=dev)
    g = build_csr(e, e, 5, 5)
    out = ops.multi_aggregate(g, MR.features(5, 4).to(dev), MR.PNA_FOUR)
    assert out.shape == (5, 16) and not out.any()
    g0 = build_csr(e, e, 5, 0)
    assert ops.multi_aggregate(g0, MR.features(5, 4).to(dev), ["max", "std"]).shape == (0, 8)


def test_realistic_degree_mix(dev, golden):
    """tests/golden/rmat_small.npz with the default split_len."""
    from keras_geometric_amd import build_csr, ops

    z = golden("rmat_small")
    x = torch.from_numpy(z["x"]).to(dev)
    ei = torch.from_numpy(z["edge_index"]).to(torch.int32)
    n, F = x.shape
    g = build_csr(ei[0].to(dev).contiguous(), ei[1].to(dev).contiguous(), n, n, n_features=F)
    singles = _singles(g, x, exact=True)
    for names in (MR.ALL_FIVE, MR.PNA_FOUR):
        _assert_blocks_equal(ops.multi_aggregate(g, x, names, exact=True), names, singles, F)
    out = ops.multi_aggregate(g, x, MR.PNA_FOUR)
    f64_std = MR.aggregate_f64("std", x.cpu()[ei[0].long()], ei[1], n)
    err = MR.scaled_err(out[:, 3 * F:].cpu(), f64_std)
    print(f"rmat_small scheduled std scaled err {err:.3e}")
    assert err <= TOL


def _grads(fn, x, cot):
    x = x.detach().clone().requires_grad_(True)
    (fn(x) * cot).sum().backward()
    return x.grad


def _composed(g, names, by_edge, exact=False):
    from keras_geometric_amd import ops

    return lambda t: torch.cat([ops.aggregate(g, t, n, by_edge=by_edge, exact=exact) for n in names], dim=1)


@pytest.mark.parametrize("names", [MR.ALL_FIVE, MR.PNA_FOUR, ["max", "std"], ["min", "sum"], ["mean"]],
                         ids=lambda n: "+".join(n))
@pytest.mark.parametrize("F", [3, 100, 260])
def test_backward_finite_graph(dev, F, names):
    from keras_geometric_amd import ops

    g, src, dst = _finite(F)
    n = 60
    x = MR.features(n, F, seed=2).to(dev)
    cot = torch.randn((n, len(names) * F), generator=torch.Generator().manual_seed(7)).to(dev)
    got = _grads(lambda t: ops.multi_aggregate(g, t, names), x, cot)
    comp = _grads(_composed(g, names, False), x, cot)
    x64 = x.cpu().double().requires_grad_(True)
    out64 = MR.multi_aggregate_f64(names, x64.index_select(0, torch.as_tensor(src).long()), torch.as_tensor(dst), n)
    (out64 * cot.cpu().double()).sum().backward()
    e64, ecomp = MR.scaled_err(got.cpu(), x64.grad), MR.scaled_err(got, comp)
    print(f"F={F} {names}: grad_x scaled err vs float64 {e64:.3e}, vs composed {ecomp:.3e}")
    assert torch.isfinite(got).all()
    assert e64 <= TOL and ecomp <= TOL


@pytest.mark.parametrize("exact", [False, True], ids=["scheduled", "exact"])
@pytest.mark.parametrize("F", [4, 128])
def test_backward_boundary_graph(dev, F, exact):
    """Rows of one message (and the duplicate-edge row's zero variance) make the std
    gradient NaN / inf as the reference's autograd does: same positions, same finite values."""
    from keras_geometric_amd import ops

    g, src, dst, degs = _boundary(F)
    n = len(degs)
    x = MR.features(n, F, seed=2).to(dev)
    for names in (MR.ALL_FIVE, ["max", "std"], ["mean", "max", "min"]):
        cot = torch.randn((n, len(names) * F), generator=torch.Generator().manual_seed(8)).to(dev)
        got = _grads(lambda t: ops.multi_aggregate(g, t, names, exact=exact), x, cot)
        comp = _grads(_composed(g, names, False, exact), x, cot)
        assert torch.equal(torch.isnan(got), torch.isnan(comp)), names
        fin = torch.isfinite(comp)
        assert torch.equal(torch.isfinite(got), fin), names
        assert MR.scaled_err(got[fin], comp[fin]) <= TOL, names
        if "std" in names:
            assert torch.isnan(got).any()
        assert not got[n - 1].any()  # the source nobody reads


@pytest.mark.parametrize("F", [3, 128])
def test_backward_by_edge(dev, F):
    from keras_geometric_amd import ops

    g, src, dst = _finite(F)
    n, E = 60, len(src)
    msg = MR.features(E, F, seed=5).to(dev)
    names = MR.ALL_FIVE
    cot = torch.randn((n, len(names) * F), generator=torch.Generator().manual_seed(9)).to(dev)
    got = _grads(lambda t: ops.multi_aggregate(g, t, names, by_edge=True), msg, cot)
    comp = _grads(_composed(g, names, True), msg, cot)
    m64 = msg.cpu().double().requires_grad_(True)
    (MR.multi_aggregate_f64(names, m64, torch.as_tensor(dst), n) * cot.cpu().double()).sum().backward()
    e64, ecomp = MR.scaled_err(got.cpu(), m64.grad), MR.scaled_err(got, comp)
    print(f"F={F} by_edge: grad scaled err vs float64 {e64:.3e}, vs composed {ecomp:.3e}")
    assert e64 <= TOL and ecomp <= TOL
    # boundary graph: NaN positions as the composed form
    gb, srcb, dstb, degs = _boundary(F)
    msgb = MR.features(len(srcb), F, seed=6).to(dev)
    cotb = torch.randn((len(degs), len(names) * F), generator=torch.Generator().manual_seed(10)).to(dev)
    gotb = _grads(lambda t: ops.multi_aggregate(gb, t, names, by_edge=True), msgb, cotb)
    compb = _grads(_composed(gb, names, True), msgb, cotb)
    assert torch.equal(torch.isnan(gotb), torch.isnan(compb))
    fin = torch.isfinite(compb)
    assert MR.scaled_err(gotb[fin], compb[fin]) <= TOL
