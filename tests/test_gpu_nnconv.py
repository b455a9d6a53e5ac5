"""ops.nnconv_aggregate (kgx_nnconv_run; backward: the same kernel over the transposed graph for d x, composed
legs for the rest) and NNConv against the float64 restatement of tests/nnconv_ref.py, which follows the
literal per-edge definition, on the fixture graph of tests/rgcn_ref.py at piece_len = 64: two tiles of 64
pieces (one ragged), a hub node of 10 pieces, a node of 2 pieces, edge-less nodes, duplicate edges,
shuffled input order (tests/test_nnconv_host.py asserts these).  F_in = 80 is the width class (64, 96] whose
lane groups have lanes past the LDS tile's columns.

Bound (the project's own): |got - ref| <= 1e-5 * max(1, A), A = the sum of the magnitudes of the
contributions to the element.  Layer test: 1e-5 * max(1, max |ref|) per tensor.

Largest err / bound seen (MI355X, all cases of this module):
  out 0.024 (edge-free graph; 0.012 elsewhere)   d x 0.012   d coef 0.018   d W 0.011   d W_bias 0.018
  d W_root 0.018   d b 0.004
Fused against composed directly: 0.005 of twice the bound (d x).
The layer test's largest err / bound is 0.035 (kernel, mean).
"""

from __future__ import annotations

import ctypes
import functools

import numpy as np
import pytest
import torch

import nnconv_ref as NR
import rgcn_ref as R
from keras_geometric_amd import _native as nat
from keras_geometric_amd import graph as G
from keras_geometric_amd import ops as kops

gpu = pytest.mark.gpu
_G: dict = {}
L = R.PIECE_LEN


def _edges(keep=None):
    src, dst, _ = R.make_graph()
    keep = np.ones(src.size, bool) if keep is None else keep
    return src[keep], dst[keep]


def _graph(dev, keep=None):
    if (keep is None) not in _G:
        s, d = (torch.from_numpy(a).to(torch.int32).to(dev) for a in _edges(keep))
        _G[keep is None] = G.build_csr(s, d, R.N_SRC, R.N_DST)
    return _G[keep is None]


def _run(dev, g, i, aggr="sum", rb=True, fused=None, keep=None, piece_len=L):
    names = ("x", "coef", "W") + (("B", "root", "b") if rb else ())
    t = {k: (i[k][keep] if k == "coef" and keep is not None else i[k]).to(dev).requires_grad_(True) for k in names}
    out = kops.nnconv_aggregate(g, t["x"], t["coef"], t["W"], t.get("B"), t.get("root"), t.get("b"), aggr=aggr, fused=fused,
                                piece_len=piece_len)
    out.backward(i["gout"].to(dev))
    return {"out": out.detach(), **{"d_" + k: v.grad for k, v in t.items()}}


@functools.lru_cache(maxsize=None)
def _ref(F_in, F_out, D, aggr, rb):
    i = NR.make_inputs(F_in, F_out, D)
    return NR.nnconv64(i["x"], i["coef"], i["W"], *((i["B"], i["root"], i["b"]) if rb else (None, None, None)), *_edges(),
                       R.N_DST, aggr == "mean", i["gout"])


def _check(label, got, ref):
    r = {k: R.ratio(v, ref[k], ref["A_" + k.split("_")[-1]]) for k, v in got.items()}
    msg = f"{label}: err / bound " + ", ".join(f"{k} {v:.3f}" for k, v in r.items())
    print(msg)
    assert all(v <= 1.0 for v in r.values()), msg


@gpu
@pytest.mark.parametrize("rb", [True, False])
@pytest.mark.parametrize("aggr", ["mean", "sum"])
@pytest.mark.parametrize("F_in,F_out,D", [(4, 4, 1), (20, 36, 5), (80, 36, 5), (128, 128, 32), (64, 256, 16)])
def test_forward_backward_against_float64(dev, F_in, F_out, D, aggr, rb):
    g = _graph(dev)
    pieces, n_split = G.csr_pieces(g, piece_len=L)
    assert n_split == 12 and pieces.shape[0] == 85  # the hub's 10 pieces and the 2-piece node come first
    got = _run(dev, g, NR.make_inputs(F_in, F_out, D), aggr, rb)
    _check(f"F {F_in}->{F_out} D {D} {aggr} root/bias/weight_bias {rb}", got, _ref(F_in, F_out, D, aggr, rb))


@gpu
def test_fused_against_composed_and_edgeless_rows(dev):
    i, g, ref = NR.make_inputs(128, 128, 32), _graph(dev), _ref(128, 128, 32, "mean", True)
    composed, fused = _run(dev, g, i, "mean", fused=False), _run(dev, g, i, "mean", fused=True)
    _check("composed 128->128 D 32", composed, ref)
    # directly: each is within 1e-5 * max(1, A) of the reference, so they differ by at most twice that
    _check("fused - composed, over twice the bound", {k: (fused[k] - composed[k]) / 2 for k in fused},
           {k: (torch.zeros_like(v) if k[:2] != "A_" else v) for k, v in ref.items()})
    s, d = (torch.from_numpy(a).to(torch.int32).to(dev) for a in _edges())
    none = G.build_csr(s, torch.full_like(d, -1), R.N_SRC, R.N_DST)  # every edge dropped
    rows = list(R.EMPTY_NODES)
    with torch.no_grad():
        x, c, W, B, root, b = (i[k].to(dev) for k in ("x", "coef", "W", "B", "root", "b"))
        alone = kops.nnconv_aggregate(none, x, c, W, B, root, b, piece_len=L)  # b + x W_root from the fused kernel
        assert torch.equal(kops.nnconv_aggregate(g, x, c, W, B, root, b, piece_len=L)[rows], alone[rows])
        xr = i["x"][: R.N_DST].double()
        _check("edge-free graph", {"out": alone}, {"out": xr @ i["root"].double() + i["b"].double(),
                                                    "A_out": xr.abs() @ i["root"].abs().double()})
        assert not bool(kops.nnconv_aggregate(g, x, c, W, B, piece_len=L)[rows].any())


@gpu
def test_bit_identity_and_column_slice_views(dev):
    i, g, pad = NR.make_inputs(128, 128, 32), _graph(dev), 4
    x, c, W, B, root, b = (i[k].to(dev) for k in ("x", "coef", "W", "B", "root", "b"))
    first = kops.nnconv_aggregate(g, x, c, W, B, root, b, piece_len=L)
    assert torch.equal(first, kops.nnconv_aggregate(g, x, c, W, B, root, b, piece_len=L))
    xw = torch.cat([torch.full((R.N_SRC, pad), 7.0), i["x"], torch.full((R.N_SRC, pad), -7.0)], 1).to(dev)
    ow = torch.full((R.N_DST, 128 + 2 * pad), 5.0, device=dev)
    kops.nnconv_into(ow[:, pad:pad + 128], g, xw[:, pad:pad + 128], c, W, B, root, b, piece_len=L)
    assert torch.equal(ow[:, pad:pad + 128], first)
    assert bool((ow[:, :pad] == 5.0).all()) and bool((ow[:, pad + 128:] == 5.0).all())


@gpu
@pytest.mark.parametrize("F_in,D", [(20, 5), (6, 5), (20, 33)])
def test_uncut_pieces_and_fallback(dev, F_in, D):
    keep = ~np.isin(R.make_graph()[1], (R.HUB, R.SECOND))  # default piece_len: no node is cut
    g = _graph(dev, keep)
    assert G.csr_pieces(g)[1] == 0 and G.csr_pieces(g, piece_len=None)[1] == 0
    assert G.csr_pieces(_graph(dev), piece_len=None)[1] == 0 and G.csr_pieces(_graph(dev), piece_len=None)[0].shape[0] == R.N_DST
    assert kops.nnconv_supported(F_in, 36, D) == (F_in == 20 and D == 5)
    i = dict(NR.make_inputs(F_in, 36, D))
    got = _run(dev, g, i, "mean", keep=keep, piece_len=G.NNCONV_PIECE_LEN)
    i["coef"] = i["coef"][keep]
    ref = NR.nnconv64(i["x"], i["coef"], i["W"], i["B"], i["root"], i["b"], *_edges(keep), R.N_DST, True, i["gout"])
    _check(f"uncut F_in {F_in} D {D}", got, ref)
    if F_in == 20 and D == 5:  # the whole graph as one piece per node: the fix-up is never launched
        x, c, W = (NR.make_inputs(20, 36, 5)[k].to(dev) for k in ("x", "coef", "W"))
        out = torch.empty(R.N_DST, 36, device=dev)
        kops.nnconv_into(out, _graph(dev), x, c, W, piece_len=None)
        _check("piece_len=None", {"out": out}, _ref(20, 36, 5, "sum", False))


@gpu
def test_argument_errors(dev):
    i, g = NR.make_inputs(20, 36, 5), _graph(dev)
    x, c, W = (i[k].to(dev) for k in ("x", "coef", "W"))
    with pytest.raises(ValueError, match="aggr"):
        kops.nnconv_aggregate(g, x, c, W, aggr="max")
    with pytest.raises(ValueError, match="coef"):
        kops.nnconv_aggregate(g, x, c[:-1], W)
    with pytest.raises(ValueError, match="weight"):
        kops.nnconv_aggregate(g, x, c, W[:, :-4])
    lib, p = nat.lib(), 16

    def run(**kw):
        f = dict(struct_size=ctypes.sizeof(nat.NnconvArgs), rowptr=p, col=p, pieces=p, n_pieces=1, n_split_pieces=0,
                 n_rows=1, n_src=1, x=p, ld_x=128, F_in=128, coef=p, ld_coef=8, n_e=1, D=8, W=p, F_out=128, out=p,
                 ld_out=128, workspace=p, workspace_bytes=1 << 30)
        f.update(kw)
        return lib.kgx_nnconv_run(ctypes.byref(nat.NnconvArgs(**f)), None)

    assert run(struct_size=8) == nat.KGX_ERR_ARG and b"struct_size" in lib.kgx_last_error()
    assert run(workspace_bytes=64) == nat.KGX_ERR_ARG and b"workspace" in lib.kgx_last_error()
    assert run(F_in=132, ld_x=132) == nat.KGX_ERR_UNSUPPORTED and b"F_in" in lib.kgx_last_error()
    assert run(D=33, ld_coef=36) == nat.KGX_ERR_UNSUPPORTED and b"D = 33" in lib.kgx_last_error()


@gpu
@pytest.mark.parametrize("aggr", ["sum", "mean"])
@pytest.mark.parametrize("edge_hidden", [None, (7,)])
def test_nnconv_layer(dev, edge_hidden, aggr):
    import keras_geometric_amd as kgx

    n, F, E, De = 30, 20, 203, 5
    gen = torch.Generator().manual_seed(5)
    x, ei = torch.randn(n, F, generator=gen), torch.randint(0, n, (2, E), generator=gen)
    ea, gout = torch.randn(E, De, generator=gen), torch.randn(n, 8, generator=gen)
    layer = kgx.NNConv(8, edge_hidden=edge_hidden, aggregator=aggr, bias_initializer="glorot_uniform")
    xd, ead = x.to(dev).requires_grad_(True), ea.to(dev).requires_grad_(True)
    out = layer([xd, ei.to(dev), ead]) if aggr == "sum" else layer([xd, ei.to(dev)], edge_attr=ead)
    out.backward(gout.to(dev))
    w = {k: v.detach().double().cpu().requires_grad_(True) for k, v in layer.named_parameters()}
    hidden = ["edge_net.0.kernel", "edge_net.0.bias"] if edge_hidden else []
    assert sorted(w) == sorted(["kernel", "kernel_bias", "root", "bias"] + hidden)
    assert tuple(w["kernel"].shape) == (7 if edge_hidden else De, F, 8)
    x64, ea64 = x.double().requires_grad_(True), ea.double().requires_grad_(True)
    c = torch.relu(ea64 @ w["edge_net.0.kernel"] + w["edge_net.0.bias"]) if edge_hidden else ea64
    theta = torch.einsum("ed,dfo->efo", c, w["kernel"]) + w["kernel_bias"]  # [E, F_in, F_out], the literal form
    msg = torch.einsum("ef,efo->eo", x64[ei[0]], theta)
    agg = torch.zeros(n, 8, dtype=torch.float64).index_add(0, ei[1], msg)
    if aggr == "mean":
        agg = agg / torch.bincount(ei[1], minlength=n).clamp_min(1).double().unsqueeze(1)
    (agg + x64 @ w["root"] + w["bias"]).backward(gout.double())
    y = (agg + x64 @ w["root"] + w["bias"]).detach()
    pairs = [("out", out.detach(), y), ("d_x", xd.grad, x64.grad), ("d_edge_attr", ead.grad, ea64.grad)]
    pairs += [(k, v.grad, w[k].grad) for k, v in layer.named_parameters()]
    for k, got, ref in pairs:
        err, bound = float((got.double().cpu() - ref).abs().max()), 1e-5 * max(1.0, float(ref.abs().max()))
        print(f"NNConv edge_hidden={edge_hidden} {aggr} {k}: err / bound {err / bound:.3f}")
        assert err <= bound, k
    clone = kgx.NNConv.from_config(layer.get_config())
    assert clone.get_config() == layer.get_config() and kgx.ECConv is kgx.NNConv
    with pytest.raises(ValueError, match="one row per edge"):
        layer([xd, ei.to(dev), ead[:-1]])
