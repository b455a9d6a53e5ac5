"""ops.gat_aggregate's composed form (fused=False) on the CPU against the float64
restatement of tests/gat_ref.py on `small` (bipartite, an empty destination,
a short edge table in input order): the bounds of tests/test_gpu_gat.py."""

from __future__ import annotations

import pytest
import torch

import gat_ref as AR
import gatv2_ref as GR
from keras_geometric_amd import graph as G
from keras_geometric_amd import ops as kops


def _cpu_csr(src, dst, n_src, n_dst):
    """The CSR a stable build gives, as a host CSRGraph (no schedule: the composed form needs none)."""
    order = torch.sort(dst, stable=True).indices
    deg = torch.bincount(dst, minlength=n_dst).to(torch.int32)
    rowptr = torch.zeros(n_dst + 1, dtype=torch.int32)
    rowptr[1:] = torch.cumsum(deg, 0)
    return G.CSRGraph(n_src=n_src, n_dst=n_dst, n_input_edges=src.numel(), kept=src.numel(),
                      max_degree=int(deg.max()), flags=0, rowptr=rowptr, col=src[order].to(torch.int32),
                      eid=order.to(torch.int32), deg=deg)


@pytest.mark.parametrize("n_cut", [None, 0, 137], ids=["no_edge", "full_table", "short_table"])
@pytest.mark.parametrize("heads,channels", [(8, 16), (3, 12)], ids=["8x16", "3x12"])
def test_composed_form_against_float64(heads, channels, n_cut):
    src, dst, n_src, n_dst = GR.make_graph("small")
    x = AR.inputs("small", heads, channels)
    edge = None if n_cut is None else x["a_edge"][: src.numel() - n_cut]
    ref = AR.gat_grads64(x["h_src"], x["a_src"], x["a_dst"], edge, x["bias"], src, dst, n_dst, heads, channels,
                         GR.SLOPE, x["gout"])
    leaves = {k: x[k].clone().requires_grad_(True) for k in ("h_src", "a_src", "a_dst", "bias")}
    e = None if edge is None else edge.clone().requires_grad_(True)
    out = kops.gat_aggregate(_cpu_csr(src, dst, n_src, n_dst), leaves["h_src"], leaves["a_src"], leaves["a_dst"],
                             heads, channels, GR.SLOPE, bias=leaves["bias"], edge=e, fused=False)
    out.backward(x["gout"])
    got = {"out": out.detach(), "d_src": leaves["h_src"].grad, "d_asrc": leaves["a_src"].grad,
           "d_adst": leaves["a_dst"].grad, "d_edge": None if e is None else e.grad}
    r = AR.ratios(got, ref)
    print(", ".join(f"{k} {v:.3f}" for k, v in r.items()))
    assert all(v <= 1.0 for v in r.values()), r
    assert torch.equal(out[0].detach(), x["bias"])  # the destination without in-edges
    assert torch.allclose(leaves["bias"].grad, x["gout"].sum(0))
