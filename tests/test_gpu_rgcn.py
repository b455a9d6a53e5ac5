"""ops.rgcn_aggregate (kgx_rgcn_run, composed backward) and RGCNConv against the float64 restatement of
tests/rgcn_ref.py on its typed fixture graph at piece_len = 64: two tiles of 64 pieces (one ragged), a hub
node of 10 pieces with a cut inside a pair and one on a pair boundary, a node of 2 pieces, edge-less
nodes, an empty relation, a relation only one node uses, duplicate triples, shuffled input order.

Bound (the project's own): |got - ref| <= 1e-5 * max(1, A), A = the sum of the magnitudes of the
contributions to the element.  Layer test: 1e-5 * max(1, max |ref|) per tensor.

Largest err / bound seen (MI355X, all cases of this module):
  out 0.017   d x 0.014   d W 0.030   d W_root 0.024 (composed leg; 0.015 fused)   d b 0.005
The layer test's largest err / bound is 0.024 (root).
"""

from __future__ import annotations

import ctypes

import numpy as np
import pytest
import torch

import rgcn_ref as R
from keras_geometric_amd import _native as nat
from keras_geometric_amd import graph as G
from keras_geometric_amd import ops as kops

gpu = pytest.mark.gpu
_RG: dict = {}


def test_fixture_has_the_properties():
    src, dst, typ = R.make_graph()
    L, n = R.PIECE_LEN, np.bincount(dst * R.R + typ, minlength=R.N_DST * R.R).reshape(R.N_DST, R.R)
    deg = n.sum(1)
    assert src.size <= 3000 and R.N_SRC > R.N_DST and all(deg[i] == 0 for i in R.EMPTY_NODES)
    assert n[:, R.EMPTY_REL].sum() == 0 and np.flatnonzero(n[:, R.LONE_REL]).tolist() == [R.LONE]
    pieces = np.maximum(1, -(-deg // L))
    assert pieces.sum() > 64 and pieces.sum() % 64 != 0 and pieces.sum() <= 128  # one full tile, one ragged
    assert np.flatnonzero(pieces > 1).tolist() == [R.HUB, R.SECOND] and pieces[R.HUB] > 8 and pieces[R.SECOND] == 2
    ends = np.cumsum(n[R.HUB])  # the hub's pair boundaries; its cuts are the multiples of L below its degree
    cuts = np.arange(L, deg[R.HUB], L)
    assert (n[R.HUB] > 0).sum() >= 3 and np.isin(cuts, ends).any() and (~np.isin(cuts, ends)).any()
    trip = np.stack([src, dst, typ], 1)
    assert len(np.unique(trip, axis=0)) < len(trip)  # duplicates
    order = np.argsort(dst * R.R + typ, kind="stable")
    assert not np.array_equal(order, np.arange(order.size))  # eid is not the identity


def _edges(Rn=R.R, keep=None):
    src, dst, typ = R.make_graph()
    keep = np.ones(src.size, bool) if keep is None else keep
    return src[keep], dst[keep], typ[keep] % Rn


def _rg(dev, Rn=R.R, piece_len=R.PIECE_LEN, keep=None):
    key = (Rn, piece_len, keep is None)
    if key not in _RG:
        t = [torch.from_numpy(a).to(torch.int32).to(dev) for a in _edges(Rn, keep)]
        _RG[key] = G.build_relation_csr(*t, R.N_SRC, R.N_DST, Rn, piece_len=piece_len)
    return _RG[key]


def _run(dev, rg, i, aggr="mean", root=True, bias=True, fused=None):
    t = {k: i[k].to(dev).requires_grad_(True) for k in ("x", "W") + (("root",) if root else ()) + (("b",) if bias else ())}
    out = kops.rgcn_aggregate(rg, t["x"], t["W"], t.get("root"), t.get("b"), aggr=aggr, fused=fused)
    out.backward(i["gout"].to(dev))
    return {"out": out.detach(), **{"d_" + k: v.grad for k, v in t.items()}}


def _check(label, got, ref):
    r = {k: R.ratio(v, ref[k], ref["A_" + k.split("_")[-1]]) for k, v in got.items()}
    msg = f"{label}: err / bound " + ", ".join(f"{k} {v:.3f}" for k, v in r.items())
    print(msg)
    assert all(v <= 1.0 for v in r.values()), msg


def _ref(i, aggr, root, bias, Rn=R.R, keep=None):
    return R.rgcn64(i["x"], i["W"], i["root"] if root else None, i["b"] if bias else None, *_edges(Rn, keep), R.N_DST,
                    aggr == "mean", i["gout"])


@gpu
@pytest.mark.parametrize("rb", [True, False])
@pytest.mark.parametrize("aggr", ["mean", "sum"])
@pytest.mark.parametrize("F_in,F_out", [(4, 4), (20, 36), (128, 128), (64, 256)])
def test_forward_backward_against_float64(dev, F_in, F_out, aggr, rb):
    i = R.make_inputs(F_in, F_out)
    _check(f"F {F_in}->{F_out} {aggr} root/bias {rb}", _run(dev, _rg(dev), i, aggr, rb, rb), _ref(i, aggr, rb, rb))


@gpu
def test_fused_against_composed_and_edgeless_rows(dev):
    i, rg = R.make_inputs(128, 128), _rg(dev)
    _check("composed 128->128", _run(dev, rg, i, fused=False), _ref(i, "mean", True, True))
    t = [torch.from_numpy(a).to(torch.int32).to(dev) for a in _edges()]
    none = G.build_relation_csr(t[0], torch.full_like(t[1], -1), t[2], R.N_SRC, R.N_DST, R.R)  # every edge dropped
    rows = list(R.EMPTY_NODES)
    with torch.no_grad():
        x, W, root, b = (i[k].to(dev) for k in ("x", "W", "root", "b"))
        alone = kops.rgcn_aggregate(none, x, W, root, b)  # b + xroot W_root from the fused kernel
        assert torch.equal(kops.rgcn_aggregate(rg, x, W, root, b)[rows], alone[rows])
        _check("edge-free graph", {"out": alone}, {"out": (i["x"][: R.N_DST].double() @ i["root"].double() + i["b"].double()),
                                                    "A_out": i["x"][: R.N_DST].abs().double() @ i["root"].abs().double()})
        assert not bool(kops.rgcn_aggregate(rg, x, W)[rows].any())


@gpu
def test_bit_identity_and_column_slice_views(dev):
    i, rg, pad = R.make_inputs(128, 128), _rg(dev), 4
    x, W, root, b = (i[k].to(dev) for k in ("x", "W", "root", "b"))
    first = kops.rgcn_aggregate(rg, x, W, root, b)
    assert torch.equal(first, kops.rgcn_aggregate(rg, x, W, root, b))
    xw = torch.cat([torch.full((R.N_SRC, pad), 7.0), i["x"], torch.full((R.N_SRC, pad), -7.0)], 1).to(dev)
    ow = torch.full((R.N_DST, 128 + 2 * pad), 5.0, device=dev)
    kops.rgcn_into(ow[:, pad:pad + 128], rg, xw[:, pad:pad + 128], W, root, b)
    assert torch.equal(ow[:, pad:pad + 128], first)
    assert bool((ow[:, :pad] == 5.0).all()) and bool((ow[:, pad + 128:] == 5.0).all())


@gpu
@pytest.mark.parametrize("Rn,piece_len,F_in", [(1, R.PIECE_LEN, 20), (3, None, 20), (R.R, R.PIECE_LEN, 6)])
def test_other_relation_counts_and_fallback(dev, Rn, piece_len, F_in):
    src, dst, typ = R.make_graph()
    keep = ~np.isin(dst, (R.HUB, R.SECOND)) if piece_len is None else None  # default piece_len: no node is split
    rg = _rg(dev, Rn, piece_len, keep)
    assert (rg.n_split_pieces == 0) == (piece_len is None) and kops.rgcn_supported(F_in, 36) == (F_in != 6)
    i = R.make_inputs(F_in, 36, Rn)
    _check(f"R {Rn} F_in {F_in}", _run(dev, rg, i), _ref(i, "mean", True, True, Rn, keep))


@gpu
def test_argument_errors(dev):
    t = [torch.from_numpy(a).to(torch.int32).to(dev) for a in R.make_graph()]
    with pytest.raises(ValueError, match="edge type"):
        G.build_relation_csr(*t, R.N_SRC, R.N_DST, 3)
    with pytest.raises(ValueError, match="int32"):
        G.build_relation_csr(*t, 2**30, 2**30, 2)
    with pytest.raises(ValueError, match="n_src"):
        G.build_relation_csr(*t, R.N_DST - 1, R.N_DST, R.R)
    i = R.make_inputs(20, 36)
    with pytest.raises(ValueError, match="aggr"):
        kops.rgcn_aggregate(_rg(dev), i["x"].to(dev), i["W"].to(dev), aggr="max")
    lib, p = nat.lib(), 16

    def run(**kw):
        f = dict(struct_size=ctypes.sizeof(nat.RgcnArgs), rowptr=p, col=p, pieces=p, n_pieces=1, n_split_pieces=0,
                 n_rows=1, R=2, x=p, ld_x=128, F_in=128, W=p, F_out=128, out=p, ld_out=128, workspace=p,
                 workspace_bytes=1 << 30)
        f.update(kw)
        return lib.kgx_rgcn_run(ctypes.byref(nat.RgcnArgs(**f)), None)

    assert run(struct_size=8) == nat.KGX_ERR_ARG and b"struct_size" in lib.kgx_last_error()
    assert run(workspace_bytes=64) == nat.KGX_ERR_ARG and b"workspace" in lib.kgx_last_error()
    assert run(F_in=132, ld_x=132) == nat.KGX_ERR_UNSUPPORTED and b"F_in" in lib.kgx_last_error()


@gpu
@pytest.mark.parametrize("num_bases", [None, 2])
def test_rgcnconv_layer(dev, num_bases):
    import keras_geometric_amd as kgx

    n, F, E, Rn = 30, 20, 203, 5
    gen = torch.Generator().manual_seed(5)
    x, ei = torch.randn(n, F, generator=gen), torch.randint(0, n, (2, E), generator=gen)
    et = torch.randint(0, Rn, (E,), generator=gen)
    layer = kgx.RGCNConv(8, Rn, num_bases=num_bases)
    xd = x.to(dev).requires_grad_(True)
    out = layer([xd, ei.to(dev)], edge_type=et.to(dev)) if num_bases else layer([xd, ei.t().to(dev), et.to(dev)])
    gout = torch.randn(n, 8, generator=gen)
    out.backward(gout.to(dev))
    w64 = {k: v.detach().double().cpu().requires_grad_(True) for k, v in layer.named_parameters()}
    assert sorted(w64) == sorted((["bases", "comp"] if num_bases else ["kernel"]) + ["root", "bias"])
    x64 = x.double().requires_grad_(True)
    W = torch.einsum("rb,bfo->rfo", w64["comp"], w64["bases"]) if num_bases else w64["kernel"]
    key = ei[1] * Rn + et
    cnt = torch.zeros(n * Rn, dtype=torch.float64).index_add_(0, key, torch.ones(E, dtype=torch.float64))
    H = torch.zeros(n * Rn, F, dtype=torch.float64).index_add(0, key, x64[ei[0]]) / cnt.clamp_min(1).unsqueeze(1)
    y = H.view(n, Rn * F) @ W.reshape(Rn * F, 8) + x64 @ w64["root"] + w64["bias"]
    y.backward(gout.double())
    pairs = [("out", out.detach(), y.detach()), ("d_x", xd.grad, x64.grad)]
    pairs += [(k, v.grad, w64[k].grad) for k, v in layer.named_parameters()]
    for k, got, ref in pairs:
        err, bound = float((got.double().cpu() - ref).abs().max()), 1e-5 * max(1.0, float(ref.abs().max()))
        print(f"RGCNConv num_bases={num_bases} {k}: err / bound {err / bound:.3f}")
        assert err <= bound, k
    clone = kgx.RGCNConv.from_config(layer.get_config())
    assert clone.get_config() == layer.get_config() and clone.num_bases == num_bases
