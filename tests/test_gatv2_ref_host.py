"""The GATv2 op-level reference (tests/gatv2_ref.py) checked on the CPU, before
any kernel is judged by it (tests/test_gpu_gatv2_op.py).

* The restatement equals oracle.reference.gatv2_forward, output and
  gradients, to 1e-12 in float64 on a square graph with self loops
  (h_src = h_dst = x @ kernel).  The oracle's segment_sum / segment_max follow
  Keras' torch backend and round their data through float32 whatever the
  input dtype, which alone puts a float64 evaluation 1e-8 away from any true
  float64 one; for this comparison the two segment ops keep the input dtype
  (same code otherwise), so the 1e-12 is about the formulas.  Unpatched and in
  float32, where that cast is the identity, the two must agree to a few ulp.
* The per-edge gradients of gatv2_grads64 sum to plain autograd's (1e-12).
* Fixture validity: for every (graph, shape) pair the GPU module uses, the
  float32 evaluation of the restatement is within HALF the GPU test's bounds
  of the float64 one: out within 0.5 * 1e-5 max(1, |ref|), d h_src / d h_dst /
  d att within 0.5 * 1e-5 max(1, A).  Measured maxima over all pairs (this
  file, `pytest -s`): out 0.27, d h_src 0.26, d h_dst 0.17, d att 0.02.
* The shape list reaches every channels-per-lane K of both rules of
  csrc/kgx_attn_layout.h, mirrored in gatv2_ref.fwd_layout / bwd_layout
  (tests/test_attn_layout_host.py holds the mirrors equal to the C++).
"""

from __future__ import annotations

import numpy as np
import pytest
import torch

import gatv2_ref as GR
from oracle import keras_torch as K
from oracle import reference as R


def _segment(op):
    def f(data, segment_ids, num_segments):
        data = K.convert(data)
        ids = K.convert(segment_ids).long()
        ids = ids.reshape((-1,) + (1,) * (data.dim() - 1)).expand_as(data)
        shape = (num_segments,) + tuple(data.shape[1:])
        if op == "sum":
            return torch.zeros(shape, dtype=data.dtype).scatter_add(0, ids, data)
        return torch.full(shape, -float("inf"), dtype=data.dtype).scatter_reduce(0, ids, data, "amax")

    return f


def _square(dtype):
    N, E, FI, H, C = 40, 300, 12, 4, 6
    rng = np.random.default_rng(3)
    ei = torch.from_numpy(rng.integers(0, N, (2, E)).astype(np.int32))
    g = torch.Generator().manual_seed(4)
    x = torch.randn(N, FI, generator=g).to(dtype)
    kern = (0.3 * torch.randn(FI, H * C, generator=g)).to(dtype)
    att = (0.3 * torch.randn(H, C, generator=g)).to(dtype)
    bias = torch.randn(H * C, generator=g).to(dtype)
    gout = torch.randn(N, H * C, generator=g).to(dtype)
    return N, H, C, ei, x, kern, att, bias, gout


def _both(dtype):
    N, H, C, ei, x, kern, att, bias, gout = _square(dtype)
    res = []
    for which in ("oracle", "restatement"):
        xr, kr, ar, br = (t.clone().requires_grad_(True) for t in (x, kern, att, bias))
        if which == "oracle":
            y = R.gatv2_forward(xr, ei, kr, ar, br, heads=H, concat=True, negative_slope=GR.SLOPE)
        else:
            eil = R.add_self_loops(ei, N)
            h = xr @ kr
            y = GR.gatv2_ref(h, h, ar, br, eil[0], eil[1], N, H, C, GR.SLOPE)
        y.backward(gout)
        res.append({"y": y.detach(), "dx": xr.grad, "dkernel": kr.grad, "datt": ar.grad, "dbias": br.grad})
    return res


def _gap(a, b) -> float:
    return float(((a - b).abs() / b.abs().clamp_min(1.0)).max())


def test_restatement_equals_oracle_fp64(monkeypatch):
    monkeypatch.setattr(K, "segment_sum", _segment("sum"))
    monkeypatch.setattr(K, "segment_max", _segment("max"))
    oracle, mine = _both(torch.float64)
    for k in oracle:
        assert mine[k].dtype == torch.float64
        assert _gap(mine[k], oracle[k]) <= 1e-12, k


def test_restatement_equals_unpatched_oracle_fp32():
    """The oracle as it stands, in float32, where its cast is the identity:
    the same operations on the same floats, only the order inside the sums may
    differ, so the suite's fp32 tolerance 1e-5 max(1, |ref|) holds with room."""
    oracle, mine = _both(torch.float32)
    for k in oracle:
        assert _gap(mine[k].double(), oracle[k].double()) <= 1e-5, k


@pytest.mark.parametrize("masked", [False, True])
def test_per_edge_gradients_sum_to_the_full_ones(masked):
    H, C = 3, 12
    src, dst, _, n_dst = GR.make_graph("small")
    x = GR.make_inputs("small", H, C)
    mask = None
    if masked:
        g = torch.Generator().manual_seed(9)
        mask = (torch.rand(src.numel(), H, generator=g) >= 0.25).double() / 0.75
    args = (x["h_src"], x["h_dst"], x["att"], x["bias"], src, dst, n_dst, H, C, GR.SLOPE, x["gout"])
    full = GR.gatv2_grads(torch.float64, *args, mask=mask)
    per = GR.gatv2_grads64(*args, mask=mask)
    for k in ("out", "d_src", "d_dst", "d_att", "d_bias"):
        assert _gap(per[k], full[k]) <= 1e-12, k
    for k, a in (("d_src", "A_src"), ("d_dst", "A_dst"), ("d_att", "A_att")):
        assert bool((per[a] >= per[k].abs() - 1e-12).all()), a  # triangle inequality


def test_graphs_are_what_the_gpu_cases_need():
    for name, (n_src, n_dst, n_rand, n_in, n_out, _) in GR.GRAPHS.items():
        src, dst, ns, nd = GR.make_graph(name)
        assert (ns, nd) == (n_src, n_dst) and ns != nd
        assert src.numel() == n_rand + n_in + n_out
        indeg = torch.bincount(dst, minlength=nd)
        outdeg = torch.bincount(src, minlength=ns)
        assert int(indeg[0]) == 0 and int(outdeg[ns - 1]) == 0
        assert int(indeg[GR.HUB_DST]) == n_in and int(outdeg[GR.HUB_SRC]) == n_out
        assert torch.unique(src * nd + dst).numel() < src.numel()  # multi-edges
        assert int((indeg < GR.SPLIT_LEN).sum()) > 1 and int((indeg >= GR.SPLIT_LEN).sum()) > 1
        assert int(outdeg.max()) >= 256  # graph.transpose schedules with default_split_len = 256
    # deep: 63 chunks of 16 (> 16, not a multiple of 8); 10 chunks of 256 (> 8, last one partial)
    _, _, _, n_in, n_out, _ = GR.GRAPHS["deep"]
    assert -(-n_in // GR.SPLIT_LEN) == 63 and n_in % GR.SPLIT_LEN
    assert -(-n_out // 256) == 10 and n_out % 256
    for pos in GR.DOMINANT_POS.values():
        src, dst, _, _ = GR.dominant_graph(pos)
        row = torch.nonzero(dst == GR.HUB_DST).flatten()
        hits = torch.nonzero(src[row] == GR.DOMINANT_SRC).flatten()
        assert hits.tolist() == [pos % row.numel()]


def _pairs():
    return ([("small", h, c) for h, c in GR.SHAPES] + [("deep", h, c) for h, c in GR.DEEP_SHAPES]
            + [("deep",) + GR.DROPOUT_SHAPE])


_WORST = {}


@pytest.mark.parametrize("name,heads,channels", _pairs())
def test_fp32_reference_sits_within_half_the_bound(name, heads, channels):
    src, dst, _, n_dst = GR.make_graph(name)
    x = GR.make_inputs(name, heads, channels)
    ref = GR.reference(name, heads, channels)
    got = GR.gatv2_grads(torch.float32, x["h_src"], x["h_dst"], x["att"], x["bias"], src, dst, n_dst, heads,
                         channels, GR.SLOPE, x["gout"])
    r = GR.ratios(got, ref)
    for k, v in r.items():
        _WORST[k] = max(_WORST.get(k, 0.0), v)
    print(f"fp32 / fp64 restatement {name} {heads}x{channels}: "
          + ", ".join(f"{k} {v:.3f}" for k, v in r.items())
          + " | worst so far: " + ", ".join(f"{k} {v:.3f}" for k, v in _WORST.items()))
    assert all(v <= 0.5 for v in r.values()), r


def test_shape_list_reaches_every_lane_layout():
    fwd = {hc: GR.fwd_layout(*hc) for hc in GR.SHAPES}
    bwd = {hc: GR.bwd_layout(*hc) for hc in GR.SHAPES}
    for hc, (kf, kb) in GR.LAYOUTS.items():
        assert (fwd[hc][0], bwd[hc][0]) == (kf, kb), hc
    assert {k for k, _ in fwd.values()} == {1, 2, 4, 8, 16}
    assert {k for k, _ in bwd.values()} == {1, 2, 4, 8, 16}
    assert {32, 64} <= {lh for _, lh in bwd.values()}
    # the layouts the table's remarks name
    assert bwd[(4, 256)] == (16, 16) and bwd[(2, 64)] == (2, 32) and bwd[(1, 64)] == (1, 64)
    assert fwd[(3, 12)] == (4, 4) and fwd[(16, 4)] == (4, 1) and fwd[(2, 6)] == (2, 4)
    assert bwd[(5, 24)] == (4, 8)
    # unsupported shapes stay unsupported
    assert GR.fwd_layout(8, 256) is None and GR.bwd_layout(8, 256) is None
    for hc in GR.DEEP_SHAPES + [GR.DROPOUT_SHAPE] + GR.DOMINANT_SHAPES:
        assert GR.fwd_layout(*hc) and GR.bwd_layout(*hc)


@pytest.mark.parametrize("heads,channels", GR.DOMINANT_SHAPES)
@pytest.mark.parametrize("pos", list(GR.DOMINANT_POS))
def test_dominant_edge_fixture(pos, heads, channels):
    """Case e's premise, in float64: the dominant edge's score is > 200 above
    every other score of the row in every head, so every other weight is an
    exact 0 in fp32 expf (which underflows below -104) and 100 / (1 + 1e-10)
    rounds to the float 100."""
    src, dst, _, n_dst = GR.dominant_graph(GR.DOMINANT_POS[pos])
    x = GR.dominant_inputs(heads, channels)
    H, C = heads, channels
    row = torch.nonzero(dst == GR.HUB_DST).flatten()
    z = x["h_dst"].double().reshape(-1, H, C)[dst[row]] + x["h_src"].double().reshape(-1, H, C)[src[row]]
    s = (torch.where(z > 0, z, GR.SLOPE * z) * x["att"].double()).sum(-1)
    dom = src[row] == GR.DOMINANT_SRC
    assert int(dom.sum()) == 1
    assert float((s[dom] - s[~dom].max(0).values).min()) > 200.0
    assert np.float32(np.float64(100.0) / (1.0 + 1e-10)) == np.float32(100.0)
    out = GR.gatv2_ref(x["h_src"], x["h_dst"], x["att"], None, src, dst, n_dst, H, C, GR.SLOPE)
    assert torch.equal(out[GR.HUB_DST], x["h_src"][GR.DOMINANT_SRC])
