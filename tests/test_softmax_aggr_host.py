"""ops.softmax_aggregate's composed form and a host-built GENConv on the CPU against the float64 restatements
of tests/softmax_aggr_ref.py (the bounds of tests/test_gpu_softmax_aggr.py), and kgx_softmax_aggr's argument
errors, which return before any device call."""

from __future__ import annotations

import ctypes

import pytest
import torch

import gated_ref as DR
import gatv2_edge_ref as ER
import gatv2_ref as GR
import keras_geometric_amd as kgx
import softmax_aggr_ref as SR
from keras_geometric_amd import _native as nat
from keras_geometric_amd import ops as kops

F = 12
P = 16  # a non-null, 16-byte aligned address that is never dereferenced


def _small():
    src, dst, n_src, n_dst = GR.make_graph("small")
    return DR.cpu_csr(src, dst, n_src, n_dst), SR.inputs("small", F)


@pytest.mark.parametrize("form", SR.FORMS)
def test_composed_form_against_float64(form):
    g, v = _small()
    got = SR.run_op(kops, g, v, form, fused=False)
    r = SR.ratios(got, SR.reference("small", F, form))  # an absent operand has no gradient to compare
    print(", ".join(f"{k} {x:.3f}" for k, x in r.items()))
    assert all(x <= 1.0 for x in r.values()), r
    assert not bool(got["out"][0].any())  # the destination without in-edges


@pytest.mark.parametrize("f_in,edge_dim", [(24, None), (24, SR.LAYER_D), (20, SR.LAYER_D), (20, 24)])
def test_layer_on_the_host_against_float64(f_in, edge_dim):
    r = ER.layer_ratios(SR.run_layer(torch.device("cpu"), f_in, 24, edge_dim), SR.layer_ref(f_in, 24, edge_dim))
    print(", ".join(f"{k} {x:.3f}" for k, x in r.items()))
    assert all(x <= 1.0 for x in r.values()), r


def test_op_and_layer_argument_errors():
    g, v = _small()
    x, e = v["x"], v["e"]
    for kw in (dict(x=None), dict(x=x[:-1]), dict(edge=e[:-1]), dict(edge=e[:, :4]), dict(edge=e, edge_order="slot"),
               dict(message="relu"), dict(temp=torch.ones(F + 4)), dict(temp=torch.ones(1, F))):
        args = {"x": x, **kw}
        with pytest.raises(ValueError, match="softmax_aggregate: "):
            kops.softmax_aggregate(g, args.pop("x"), args.pop("temp", 1.0), fused=False, **args)
    g.flags = nat.CSR_SELF_LOOPS  # added self-loop slots carry no edge feature
    with pytest.raises(ValueError, match="self-loop"):
        kops.softmax_aggregate(g, x, edge=e, fused=False)
    assert [kops.softmax_aggr_supported(f) for f in (4, 6, 100, 512, 516, 0)] == [True, False, True, True, False, False]
    for kw in (dict(aggr="powermean"), dict(msg_norm=True), dict(semi_grad=True), dict(learn_p=True), dict(p=2.0),
               dict(norm="instance")):
        with pytest.raises(ValueError, match=next(iter(kw))):
            kgx.GENConv(8, 8, **kw)
    assert kgx.layers.AggregatorFactory.create_softmax(0.5).t == 0.5
    assert kgx.layers.AggregatorFactory.get_available_aggregators() == ["mean", "max", "sum", "min", "std"]
    assert kgx.MessagePassing(aggregator=kgx.layers.SoftmaxAggregator()).get_config()["aggregator"] == "softmax"


def _call(**kw):
    a = dict(rowptr=P, rows=P, n_rows=4, col=P, x=P, ld_x=8, temp=P, F=8, out=P, ld_out=8)
    a.update(kw)
    size = a.pop("struct_size", ctypes.sizeof(nat.SoftmaxAggrArgs))
    return nat.lib().kgx_softmax_aggr(ctypes.byref(nat.SoftmaxAggrArgs(struct_size=size, **a)), None)


@pytest.mark.parametrize("kw,rc,text", [
    (dict(struct_size=8), nat.KGX_ERR_ARG, b"struct_size"),
    (dict(x=None), nat.KGX_ERR_ARG, b"both absent"),
    (dict(F=6, ld_x=8), nat.KGX_ERR_UNSUPPORTED, b"multiple of 4"),
    (dict(F=516, ld_x=516, ld_out=516), nat.KGX_ERR_UNSUPPORTED, b"multiple of 4"),
    (dict(ld_x=4), nat.KGX_ERR_ARG, b"leading dimension of x"),
    (dict(x=None, edge=P, n_e=9, ld_e=4), nat.KGX_ERR_ARG, b"leading dimension of edge"),
    (dict(ld_out=4), nat.KGX_ERR_ARG, b"leading dimension of out"),
], ids=["struct_size", "no_message", "F6", "F516", "ld_x", "ld_e", "ld_out"])
def test_abi_argument_errors(kw, rc, text):
    assert _call(**kw) == rc
    assert text in nat.lib().kgx_last_error()
    assert _call(n_rows=0) == nat.KGX_OK  # nothing to do is not an error, and nothing is launched
