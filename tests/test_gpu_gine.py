"""kgx_gine_run / kgx_gine_backward_run (ops.gine_aggregate) and GINEConv against the float64
restatement of tests/gine_ref.py, on its two graphs (hub rows of more than kFixB = 8 spans, empty rows,
rows inside and across span boundaries) and its two input families.

grid: every z = x + eps is exact in fp32 in any order, some exactly 0, so the relu branch equals the
reference's with no mask; all quantities are checked.  normal: N(0, 1), `out` only (continuous in z).

Bounds (the project's own): |got - ref| <= 1e-5 * max(1, A), A = the sum of the magnitudes of the
per-edge contributions to the element.  Layer test: 1e-5 * max(1, max |ref|) per tensor (no per-element
A is formed through the MLP).

Largest err / bound seen (MI355X, all cases of this module):
  out 0.042   d x 0.055   d W_e 0.009   d b_e 0.037   d a 0.000 (a copy of dz)
The layer test's largest err / bound is 0.022 (lin_edge.bias, edge_dim=40).
"""

from __future__ import annotations

import ctypes

import pytest
import torch

import gine_ref as R
from keras_geometric_amd import _native as nat
from keras_geometric_amd import graph as G
from keras_geometric_amd import ops as kops

pytestmark = pytest.mark.gpu
FS, DS = (4, 20, 128, 512), (1, 7, 32, 0)  # D = 0: the plain variant
_GRAPHS: dict = {}


def _graph(dev, name, src=None, dst=None):
    key = name if src is None else None
    if key not in _GRAPHS:
        s, d, n_src, n_dst = R.make_graph(name)
        s, d = (s, d) if src is None else (src, dst)
        g = G.build_csr(s.to(torch.int32).to(dev), d.to(torch.int32).to(dev), n_src, n_dst)
        if key is None:
            return g
        _GRAPHS[key] = g
    return _GRAPHS[key]


def _run(dev, g, i, order="input", pad=0, xroot=None, scale=0.0):
    """Forward + backward on the device.  csr: the table in slot order, its gradient un-permuted; pad:
    x and a are the middle column blocks of wider tensors."""
    proj = i["W"] is not None
    a = i["a"][g.eid.long().cpu()] if order == "csr" else i["a"]

    def wide(t, grad):
        if not pad:
            w = t.to(dev).requires_grad_(grad)
            return w, w
        w = torch.cat([torch.full((t.shape[0], pad), 7.0), t, torch.full((t.shape[0], pad), -7.0)], 1).to(dev)
        w.requires_grad_(grad)
        return w, w[:, pad:pad + t.shape[1]]

    xw, xv = wide(i["x"], True)
    aw, av = wide(a, not proj)
    W, b = (i["W"].to(dev).requires_grad_(True), i["b"].to(dev).requires_grad_(True)) if proj else (None, None)
    out = kops.gine_aggregate(g, xv, av, weight=W, bias=b, edge_order=order,
                              xroot=None if xroot is None else xroot.to(dev), gin_scale=scale)
    out.backward(i["gout"].to(dev))
    got = {"out": out.detach(), "d_x": xw.grad[:, pad:pad + i["x"].shape[1]]}
    if pad:
        assert not bool(xw.grad[:, :pad].any()) and not bool(xw.grad[:, -pad:].any())
    if proj:
        got.update(d_W=W.grad, d_b=b.grad)
    else:
        d_a = aw.grad[:, pad:pad + a.shape[1]]
        if pad:
            assert not bool(aw.grad[:, :pad].any()) and not bool(aw.grad[:, -pad:].any()), "pad columns written"
        if order == "csr":
            d_a = torch.empty_like(d_a).index_copy_(0, g.eid.long(), d_a)
        got["d_a"] = d_a
    return got


def _check(label, got, ref, keys=None):
    r = {k: R.ratio(v, ref[k], ref["A_" + k[2:] if k != "out" else "A_out"]) for k, v in got.items()
         if keys is None or k in keys}
    msg = f"{label}: err / bound " + ", ".join(f"{k} {v:.3f}" for k, v in r.items())
    print(msg)
    assert all(v <= 1.0 for v in r.values()), msg


def _ref(name, i, **kw):
    src, dst, _, n_dst = R.make_graph(name)
    return R.gine64(i["x"], i["a"], i["W"], i["b"], src, dst, n_dst, i["gout"], **kw)


@pytest.mark.parametrize("name", ["a", "b"])
def test_graphs_have_the_properties(dev, name):
    src, dst, n_src, n_dst = R.make_graph(name)
    g = _graph(dev, name)
    assert n_src != n_dst and g.kept == src.numel() <= 2000 and g.kept % 64 != 0
    for gr, hub, empty in ((g, R.HUB_DST, (0, R.MID_EMPTY, n_dst - 1)), (G.transpose(g), R.HUB_SRC, (n_src - 1,))):
        rp = gr.rowptr.cpu().long()
        b, e = rp[:-1], rp[1:]
        assert all(int(e[r] - b[r]) == 0 for r in empty)
        spans = (e - 1) // 64 - b // 64 + 1
        assert int(spans[hub]) > 8  # more partials than the fix-up loads per step
        live = e > b
        assert bool((live & (spans == 1)).any()) and bool((live & (spans == 2)).any())
    assert not torch.equal(g.eid.cpu(), torch.arange(g.kept, dtype=torch.int32))


@pytest.mark.parametrize("order", ["input", "csr"])
@pytest.mark.parametrize("D", DS)
@pytest.mark.parametrize("F", FS)
@pytest.mark.parametrize("name", ["a", "b"])
def test_grid_all_quantities(dev, name, F, D, order):
    i = R.make_inputs("grid", name, F, D)
    ref = _ref(name, i)
    z = ref["z"]
    assert bool((z == 0).any()) and bool((z > 0).any()) and bool((z < 0).any())
    assert bool((z.float().double() == z).all()) and float(z.abs().max()) < 128  # exact in fp32
    _check(f"grid {name} F{F} D{D} {order}", _run(dev, _graph(dev, name), i, order), ref)


@pytest.mark.parametrize("D", DS)
@pytest.mark.parametrize("F", FS)
def test_normal_out(dev, F, D):
    i = R.make_inputs("normal", "b", F, D)
    _check(f"normal F{F} D{D}", _run(dev, _graph(dev, "b"), i), _ref("b", i), keys=("out",))


@pytest.mark.parametrize("D", [7, 0])
def test_bit_identity_orders_and_strides(dev, D):
    """run to run, csr against input order, and column-slice views: the same bits"""
    g, i = _graph(dev, "b"), R.make_inputs("grid", "b", 128, D)
    first = _run(dev, g, i)
    for other in (_run(dev, g, i), _run(dev, g, i, order="csr"), _run(dev, g, i, pad=4)):
        for k in first:
            assert torch.equal(first[k], other[k]), k
    if D == 0:  # grad_a written into the middle block of a wider buffer: ld_ga != F, the pads keep their 5.0
        t, F, pad = G.transpose(g), 128, 4
        x, a, gout = (i[k].to(dev) for k in ("x", "a", "gout"))
        buf = torch.full((a.shape[0], F + 2 * pad), 5.0, device=dev)
        g_x, _, _ = kops.gine_backward_into(buf[:, pad:pad + F], gout, x, a, None, None, t.rowptr, t.col,
                                            G.row_of_slot(t), t.eid)
        assert torch.equal(buf[:, pad:pad + F], first["d_a"]) and torch.equal(g_x, first["d_x"])
        assert bool((buf[:, :pad] == 5.0).all()) and bool((buf[:, pad + F:] == 5.0).all())


@pytest.mark.parametrize("F,D", [(20, 7), (128, 32)])
def test_projected_equals_plain_fed_the_projection(dev, F, D):
    for family, keys in (("normal", ("out",)), ("grid", ("out", "d_x"))):  # grid: eps exact, the same relu branch
        i = R.make_inputs(family, "a", F, D)
        eps = (i["a"].double() @ i["W"].double() + i["b"].double()).float()
        got = _run(dev, _graph(dev, "a"), dict(i, a=eps, W=None, b=None))
        _check(f"plain fed eps {family} F{F} D{D}", got, _ref("a", i), keys=keys)


@pytest.mark.parametrize("D", [7, 0])
def test_dropped_input_edges_have_zero_gradient(dev, D):
    src, dst, n_src, n_dst = R.make_graph("a")
    bad = torch.tensor([3, 64, 700, src.numel() - 1])
    dst = dst.clone()
    dst[bad] = -1  # the build drops these input edges
    g = _graph(dev, "a", src, dst)
    keep = torch.ones(src.numel(), dtype=torch.bool)
    keep[bad] = False
    assert g.kept == int(keep.sum()) and g.n_input_edges == src.numel()
    i = R.make_inputs("grid", "a", 20, D)
    ref = R.gine64(i["x"], i["a"][keep], i["W"], i["b"], src[keep], dst[keep], n_dst, i["gout"])
    got = _run(dev, g, i)
    if not D:
        assert not bool(got["d_a"][bad].any()), "a dropped edge's grad_a row is not 0"
        got["d_a"] = got["d_a"][keep]
    _check(f"dropped edges D{D}", got, ref)


def test_epilogue_on_empty_rows_and_fallback(dev):
    src, dst, n_src, n_dst = R.make_graph("a")
    none = _graph(dev, "a", src, torch.full_like(dst, -1))  # every input edge dropped: the epilogue alone
    i = R.make_inputs("grid", "a", 20, 7)
    xroot = torch.randn(n_dst, 20, generator=torch.Generator().manual_seed(1))
    assert none.kept == 0 and none.n_input_edges == src.numel()
    assert torch.equal(_run(dev, none, i, xroot=xroot, scale=0.5)["out"].cpu(), 0.5 * xroot)
    g = _graph(dev, "a")
    for F in (20, 6):  # 6: not a multiple of 4, the composed form
        i = R.make_inputs("grid", "a", F, 7)
        xroot = torch.randn(g.n_dst, F, generator=torch.Generator().manual_seed(F))
        got = _run(dev, g, i, xroot=xroot, scale=1.25)
        _check(f"epilogue F{F}", got, _ref("a", i, xroot=xroot, scale=1.25))
        for r in (0, R.MID_EMPTY, g.n_dst - 1):
            assert torch.equal(got["out"][r].cpu(), 1.25 * xroot[r])


def test_python_argument_errors(dev):
    i = R.make_inputs("grid", "a", 20, 7)
    x, a, W = (i[k].to(dev) for k in ("x", "a", "W"))
    src, dst, n_src, _ = R.make_graph("a")
    loops = G.build_csr(src.to(torch.int32).to(dev) % 29, dst.clamp_min(0).to(torch.int32).to(dev), 29, 29,
                        self_loops=True)
    with pytest.raises(ValueError, match="self-loop"):
        kops.gine_aggregate(loops, x[:29], a, weight=W)
    with pytest.raises(NotImplementedError, match="edge"):
        kops.gine_aggregate(_graph(dev, "a"), x, a.clone().requires_grad_(True), weight=W)
    with pytest.raises(ValueError, match="edge_order"):
        kops.gine_aggregate(_graph(dev, "a"), x, a, weight=W, edge_order="coo")


def test_argument_errors_of_the_c_entry_points():
    lib, p = nat.lib(), 16

    def fwd(**kw):
        f = dict(struct_size=ctypes.sizeof(nat.GineArgs), rowptr=p, col=p, row_of_slot=p, eid=p, n_rows=1, n_slots=1,
                 x=p, ld_x=128, F=128, edge=p, ld_edge=16, n_e=1, D=16, W=p, ld_w=128, out=p, ld_out=128, workspace=p,
                 workspace_bytes=1 << 20)
        f.update(kw)
        return lib.kgx_gine_run(ctypes.byref(nat.GineArgs(**f)), None)

    def bwd(**kw):
        f = dict(struct_size=ctypes.sizeof(nat.GineBackwardArgs), t_rowptr=p, t_col=p, t_row_of_slot=p, t_eid=p,
                 n_rows=1, n_slots=1, x=p, ld_x=128, F=128, edge=p, ld_edge=16, n_e=1, D=16, W=p, ld_w=128, gout=p,
                 ld_gout=128, grad_x=p, ld_gx=128, grad_W=p, workspace=p, workspace_bytes=1 << 20)
        f.update(kw)
        return lib.kgx_gine_backward_run(ctypes.byref(nat.GineBackwardArgs(**f)), None)

    for call in (fwd, bwd):
        assert call(struct_size=8) == nat.KGX_ERR_ARG and b"struct_size" in lib.kgx_last_error()
        assert call(ld_edge=15) == nat.KGX_ERR_ARG and b"leading dimension" in lib.kgx_last_error()
        assert call(ld_x=2**31) == nat.KGX_ERR_ARG and b"2^31" in lib.kgx_last_error()
        assert call(n_e=-1) == nat.KGX_ERR_ARG and call(n_e=2**31) == nat.KGX_ERR_ARG
        assert b"edge table" in lib.kgx_last_error()
        assert call(workspace_bytes=8) == nat.KGX_ERR_ARG and b"workspace" in lib.kgx_last_error()
        for kw in (dict(F=6, ld_x=8), dict(F=516, ld_x=516, ld_w=516), dict(D=33, ld_edge=40)):
            assert call(**kw) == nat.KGX_ERR_UNSUPPORTED
    assert fwd(ld_out=100) == nat.KGX_ERR_ARG
    assert bwd(grad_x=None) == nat.KGX_ERR_ARG and b"grad_x" in lib.kgx_last_error()
    assert bwd(grad_W=None) == nat.KGX_ERR_ARG and b"grad_W" in lib.kgx_last_error()
    assert bwd(D=0, W=None, ld_edge=128) == nat.KGX_ERR_ARG and b"grad_edge" in lib.kgx_last_error()


@pytest.mark.parametrize("edge_dim,train_eps", [(None, False), (8, False), (40, False), (8, True)])
def test_gineconv_layer(dev, edge_dim, train_eps):
    import keras_geometric_amd as kgx

    n, F, E = 30, 20, 203
    gen = torch.Generator().manual_seed(5)
    x = torch.randn(n, F, generator=gen)
    ei = torch.randint(0, n, (2, E), generator=gen)
    ea = torch.randn(E, edge_dim or F, generator=gen)
    layer = kgx.GINEConv(8, mlp_hidden=[16], eps_init=0.25, edge_dim=edge_dim, train_eps=train_eps)
    xd = x.to(dev).requires_grad_(True)
    # trainable eps: edge_attr as a keyword, and eps stays in autograd
    out = layer([xd, ei.to(dev)], edge_attr=ea.to(dev)) if train_eps else layer([xd, ei.to(dev), ea.to(dev)])
    gout = torch.randn(n, 8, generator=gen)
    out.backward(gout.to(dev))
    names = [k for k, _ in layer.named_parameters()]
    assert (edge_dim is not None) == any("lin_edge" in k for k in names)
    w64 = {k: v.detach().double().cpu().requires_grad_(True) for k, v in layer.named_parameters()}
    x64 = x.double().requires_grad_(True)
    e = ea.double()
    if edge_dim is not None:
        e = e @ w64[next(k for k in names if "lin_edge" in k and "kernel" in k)] + \
            w64[next(k for k in names if "lin_edge" in k and "bias" in k)]
    eps = [k for k in names if k.split(".")[-1] == "eps"]
    scale = 1 + w64[eps[0]] if train_eps else 1.25
    h = scale * x64 + torch.zeros(n, F, dtype=torch.float64).index_add(0, ei[1], torch.relu(x64[ei[0]] + e))
    assert train_eps == bool(eps)
    mlp = [k for k in names if "lin_edge" not in k and k not in eps]
    y = torch.relu(h @ w64[mlp[0]] + w64[mlp[1]]) @ w64[mlp[2]] + w64[mlp[3]]
    y.backward(gout.double())
    pairs = [("out", out.detach(), y.detach()), ("d_x", xd.grad, x64.grad)]
    pairs += [(k, v.grad, w64[k].grad) for k, v in layer.named_parameters()]
    for k, got, ref in pairs:
        err, bound = float((got.double().cpu() - ref).abs().max()), 1e-5 * max(1.0, float(ref.abs().max()))
        print(f"GINEConv edge_dim={edge_dim} train_eps={train_eps} {k}: err / bound {err / bound:.3f}")
        assert err <= bound, k
