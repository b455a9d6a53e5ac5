"""Restatements for the fused multi-aggregation and PNAConv tests (CPU only).

* blocks_reference: every block through oracle.reference.aggregate (the
  reference's own arithmetic, fp32), concatenated in the caller's order.
* multi_aggregate_f64 / pna_forward_f64: float64 torch restatements, written
  with differentiable torch ops so that autograd gives the gradients the
  reference's autograd would (scatter amax shares ties evenly; the count <= 1
  guard of std sends 0 into sqrt'(0), hence NaN, as the reference does).
* boundary_graph / finite_graph: the small graphs of the GPU tests.
* scaled_err: |a - b| / max(|b|, 1), the project's error measure (bar 1e-5).
"""

from __future__ import annotations

import numpy as np
import torch

from oracle import reference as R

PNA_FOUR = ["mean", "max", "min", "std"]
ALL_FIVE = ["sum", "mean", "max", "min", "std"]
# every list the op tests run: enum order, the PNA four, a permutation, every singleton, a pair with std but no mean
REDUCER_LISTS = [ALL_FIVE, PNA_FOUR, ["std", "min", "sum", "max", "mean"], ["sum"], ["mean"], ["max"], ["min"],
                 ["std"], ["max", "std"]]
# degrees of the boundary graph's first rows: 0, 1, 2; U-1, U, U+1, 2U+1 for the kernel's U = 6 (F <= 256
# at four floats per lane) and U = 4 (wider rows); 15, 16, 17 around split_len = 16; 33 = three chunks, the
# last of one edge; 100
BOUNDARY_DEGREES = [0, 1, 2, 3, 4, 5, 6, 7, 9, 13, 15, 16, 17, 33, 100]
SPLIT_LEN = 16


def scaled_err(a: torch.Tensor, b: torch.Tensor) -> float:
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    if a.numel() == 0:
        return 0.0
    return float(((a - b).abs() / b.abs().clamp_min(1.0)).max())


def blocks_reference(names, messages: torch.Tensor, target_idx: torch.Tensor, dim_size: int) -> torch.Tensor:
    return torch.cat([R.aggregate(n, messages, target_idx, dim_size) for n in names], dim=1)


def _segment_amax(m: torch.Tensor, idx: torch.Tensor, n: int) -> torch.Tensor:
    init = torch.full((n, m.shape[1]), -float("inf"), dtype=m.dtype)
    return init.scatter_reduce(0, idx.view(-1, 1).expand_as(m), m, "amax", include_self=True)


def aggregate_f64(name: str, messages: torch.Tensor, target_idx: torch.Tensor, dim_size: int) -> torch.Tensor:
    """One aggregator in float64, differentiable in messages (aggregators.py:48-232)."""
    m = messages.double()
    idx = target_idx.long()
    zeros = torch.zeros((dim_size, m.shape[1]), dtype=torch.float64)
    count = torch.zeros(dim_size, dtype=torch.float64).index_add(0, idx, torch.ones(len(idx), dtype=torch.float64))
    safe = count.clamp_min(1e-8).unsqueeze(1)
    if name == "sum":
        return zeros.index_add(0, idx, m)
    if name == "mean":
        return zeros.index_add(0, idx, m) / safe
    if name == "max":
        a = _segment_amax(m, idx, dim_size)
        return torch.where(torch.isinf(a), torch.zeros_like(a), a)
    if name == "min":
        a = -_segment_amax(-m, idx, dim_size)
        return torch.where(torch.isinf(a), torch.zeros_like(a), a)
    if name == "std":
        mean = zeros.index_add(0, idx, m) / safe
        ssd = zeros.index_add(0, idx, torch.square(m - mean.index_select(0, idx)))
        std = torch.sqrt(torch.clamp_min(ssd / safe, 0.0))
        return torch.where(count.unsqueeze(1) <= 1, torch.zeros_like(std), std)
    raise ValueError(name)


def multi_aggregate_f64(names, messages, target_idx, dim_size: int) -> torch.Tensor:
    return torch.cat([aggregate_f64(n, messages, target_idx, dim_size) for n in names], dim=1)


def average_log_degree_f64(dst: np.ndarray, n: int) -> float:
    deg = np.bincount(np.asarray(dst, dtype=np.int64), minlength=n).astype(np.float64)
    return float(np.log(deg + 1.0).mean())


def pna_forward_f64(x, edge_index, w_root, w_aggr, bias, aggregators, scalers, delta: float, activation=None,
                    parts: bool = False):
    """PNAConv in float64: act(x W_root + concat_s(s_s * A) W_aggr + b), scaler-major z.
    parts=True: (out, z, pre-activation), the pre-activation keeping its .grad."""
    x = x.double()
    n = x.shape[0]
    out = torch.zeros((n, w_aggr.shape[1]), dtype=torch.float64)
    z = torch.zeros((n, w_aggr.shape[0]), dtype=torch.float64)
    if w_root is not None:
        out = out + x @ w_root.double()
    src, dst = edge_index[0].long(), edge_index[1].long()
    if len(src):
        A = multi_aggregate_f64(aggregators, x.index_select(0, src), dst, n)
        deg = torch.bincount(dst, minlength=n).double()
        log_d = torch.log(deg.clamp_min(1.0) + 1.0).unsqueeze(1)
        scale = {"identity": torch.ones_like(log_d), "amplification": log_d / delta, "attenuation": delta / log_d}
        z = torch.cat([scale[s] * A for s in scalers], dim=1)
        out = out + z @ w_aggr.double()
    if bias is not None:
        out = out + bias.double()
    if parts:
        out.retain_grad()
        return (out if activation is None else activation(out)), z, out
    return out if activation is None else activation(out)


def boundary_graph(seed: int = 3, n: int = 80):
    """(src, dst) int32 over n nodes: rows 0.. have BOUNDARY_DEGREES, the rest 0 or
    3..12 edges; row 2 reads one source twice and the degree-100 row draws with
    replacement (duplicate edges), row 4 reads itself (self loop), and source n-1
    is read by nobody.  Apart from row 2 no row has only two distinct messages
    (rows of up to 40 edges read distinct sources): there std = |a - b| / 2 comes
    arbitrarily close to 0 and the gradient's 1 / std factor amplifies the fp32
    rounding of x * T(A) - T(A * mean), about eps * |mean| / std, in any
    formulation past a fixed bar (a row (a, a, b) with std 0.0014 at one feature
    gave 2e-5 per rounding); row 2 is the exactly-zero case, NaN in every form."""
    rng = np.random.default_rng(seed)
    fill = n - len(BOUNDARY_DEGREES)
    degs = list(BOUNDARY_DEGREES) + [0 if z else int(d) for z, d in
                                     zip(rng.random(fill) < 0.1, rng.integers(3, 13, fill))]
    src, dst = [], []
    for row, d in enumerate(degs):
        # source n-1 never drawn
        s = rng.permutation(n - 1)[:d] if d <= 40 else rng.integers(0, n - 1, d)
        if row == 2:
            s[:] = s[0]
        if row == 4:
            s[1] = row
        src.append(s)
        dst.append(np.full(d, row))
    src, dst = np.concatenate(src), np.concatenate(dst)
    perm = rng.permutation(len(src))  # input order is not CSR order
    return src[perm].astype(np.int32), dst[perm].astype(np.int32), np.asarray(degs)


def finite_graph(seed: int = 9, n: int = 60):
    """Every row has 6..40 DISTINCT sources.  With continuous values that means no
    ties and no zero variance, and sample deviations of at least six N(0,1) draws
    stay far enough from 0 for the std gradient's 1 / std factor to be well
    conditioned in fp32 (relative error about eps * |mean| / std)."""
    rng = np.random.default_rng(seed)
    src, dst = [], []
    for row in range(n):
        d = int(rng.integers(6, 41))
        src.append(rng.permutation(n)[:d])
        dst.append(np.full(d, row))
    src, dst = np.concatenate(src), np.concatenate(dst)
    perm = rng.permutation(len(src))
    return src[perm].astype(np.int32), dst[perm].astype(np.int32)


def features(n: int, F: int, seed: int = 0) -> torch.Tensor:
    """N(0,1) + 3 in fp32."""
    g = torch.Generator().manual_seed(seed)
    return torch.randn((n, F), generator=g, dtype=torch.float32) + 3.0


def special_features(n: int, F: int, src: np.ndarray, dst: np.ndarray, seed: int = 1) -> torch.Tensor:
    """features() with +-inf, NaN and +-0 entries, an all-equal row (every source
    of the degree-5 row holds 2.5) and a row whose max ties at three edges (three
    distinct sources of the degree-13 row hold 9.0, above everything finite)."""
    x = features(n, F, seed)
    rng = np.random.default_rng(seed)
    specials = [float("inf"), -float("inf"), float("nan"), 0.0, -0.0]
    for i, v in enumerate(specials * 3):
        x[int(rng.integers(0, n - 1)), int(rng.integers(0, F))] = v
    row_eq, row_tie = BOUNDARY_DEGREES.index(5), BOUNDARY_DEGREES.index(13)
    eq_src = np.unique(src[dst == row_eq])
    x[torch.as_tensor(eq_src).long()] = 2.5
    tie_src = np.setdiff1d(np.unique(src[dst == row_tie]), eq_src)[:3]
    assert len(tie_src) == 3
    x[torch.as_tensor(tie_src).long()] = 9.0
    return x
