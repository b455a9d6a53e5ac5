"""ops.gated_aggregate's composed form and ResGatedGraphConv on the CPU against the float64 restatements of
tests/gated_ref.py (the bounds of tests/test_gpu_gated.py), the op's argument errors and the config round-trip."""

from __future__ import annotations

import pytest
import torch

import gated_ref as DR
import gatv2_edge_ref as ER
import gatv2_ref as GR
import keras_geometric_amd as kgx
from keras_geometric_amd import _native as nat
from keras_geometric_amd import ops as kops

F = 12


def _small():
    src, dst, n_src, n_dst = GR.make_graph("small")
    return DR.cpu_csr(src, dst, n_src, n_dst), DR.inputs("small", F)


@pytest.mark.parametrize("with_edge", [False, True], ids=["plain", "edge"])
def test_composed_form_against_float64(with_edge):
    g, x = _small()
    t = {n: x[n].clone().requires_grad_(True) for n in ("k", "q", "v", "root", "bias")}
    e = x["e"].clone().requires_grad_(True) if with_edge else None
    out = kops.gated_aggregate(g, t["k"], t["q"], t["v"], edge=e, root=t["root"], bias=t["bias"], fused=False)
    out.backward(x["gout"])
    got = {"out": out.detach(), "d_k": t["k"].grad, "d_q": t["q"].grad, "d_v": t["v"].grad,
           "d_e": e.grad if with_edge else None}
    r = DR.ratios(got, DR.reference("small", F, with_edge))
    print(", ".join(f"{k} {v:.3f}" for k, v in r.items()))
    assert all(v <= 1.0 for v in r.values()), r
    assert torch.equal(out[0].detach(), x["root"][0] + x["bias"])  # the destination without in-edges
    assert torch.equal(t["root"].grad, x["gout"]) and torch.allclose(t["bias"].grad, x["gout"].sum(0))


@pytest.mark.parametrize("root_weight", [True, False], ids=["root", "noroot"])
@pytest.mark.parametrize("edge_dim", [None, DR.LAYER_D], ids=["plain", "edge_dim"])
def test_layer_on_the_host_against_float64(edge_dim, root_weight):
    r = ER.layer_ratios(DR.run_layer(torch.device("cpu"), edge_dim, root_weight), DR.layer_ref(edge_dim, root_weight))
    print(", ".join(f"{k} {v:.3f}" for k, v in r.items()))
    assert all(v <= 1.0 for v in r.values()), r


def test_argument_errors():
    g, x = _small()
    k, q, v, e = x["k"], x["q"], x["v"], x["e"]
    bad = [dict(k=k[:-1]), dict(q=q[:, :-4]), dict(v=v[:-1]), dict(root=q), dict(bias=x["bias"][:-1]),
           dict(edge=e[:-1]), dict(edge=e, edge_order="slot"), dict(edge=e[:, :4])]
    for kw in bad:
        args = {"k": k, "q": q, "v": v, **kw}
        with pytest.raises(ValueError, match="gated: "):
            kops.gated_aggregate(g, args.pop("k"), args.pop("q"), args.pop("v"), fused=False, **args)
    g.flags = nat.CSR_SELF_LOOPS  # added self-loop slots carry no edge feature
    with pytest.raises(ValueError, match="self-loop"):
        kops.gated_aggregate(g, k, q, v, edge=e, fused=False)
    assert [kops.gated_supported(f) for f in (4, 6, 100, 512, 516, 0)] == [True, False, True, True, False, False]


def test_layer_contract():
    layer = kgx.ResGatedGraphConv(24, edge_dim=5, root_weight=False, use_bias=False, kernel_initializer="he_uniform")
    cfg = layer.get_config()
    assert kgx.ResGatedGraphConv.from_config(cfg).get_config() == cfg and "aggregator" not in cfg
    assert (cfg["output_dim"], cfg["edge_dim"], cfg["root_weight"], cfg["use_bias"]) == (24, 5, False, False)
    kgx.ResGatedGraphConv(8, act="sigmoid")
    with pytest.raises(ValueError, match="sigmoid"):
        kgx.ResGatedGraphConv(8, act="relu")
    with pytest.raises(ValueError, match="edge_dim"):
        kgx.ResGatedGraphConv(8, edge_dim=0)
