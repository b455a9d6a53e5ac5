"""float64 restatement of the GINE aggregation (kgx_gine_run / kgx_gine_backward_run), its two seeded
test graphs and its two input families (tests/test_gpu_gine.py)."""

import functools

import numpy as np
import torch

HUB_DST, HUB_SRC, MID_EMPTY = 5, 7, 13
GRAPHS = {"a": (37, 29, 300, 580, 590, 11), "b": (50, 41, 700, 600, 650, 12)}  # n_src, n_dst, random, hub in, hub out


@functools.lru_cache(maxsize=None)
def make_graph(name):
    """(src, dst, n_src, n_dst) int64 COO: destinations 0, MID_EMPTY and the last one empty, the last source
    without out-edge, one hub destination and one hub source of more than 8 spans of 64 slots each."""
    n_src, n_dst, n_rand, n_in, n_out, seed = GRAPHS[name]
    rng = np.random.default_rng(seed)
    sp = np.array([j for j in range(n_src - 1) if j != HUB_SRC])
    dp = np.array([i for i in range(1, n_dst - 1) if i not in (HUB_DST, MID_EMPTY)])
    src = np.concatenate([rng.choice(sp, n_rand), rng.choice(sp, n_in), np.full(n_out, HUB_SRC)])
    dst = np.concatenate([rng.choice(dp, n_rand), np.full(n_in, HUB_DST), rng.choice(dp, n_out)])
    perm = rng.permutation(src.size)
    return torch.from_numpy(src[perm]).long(), torch.from_numpy(dst[perm]).long(), n_src, n_dst


def gine64(x, a, W, b, src, dst, n_dst, gout, xroot=None, scale=0.0):
    """out, the gradients and, per element, A = the sum of the magnitudes of its per-edge contributions."""
    x, a, gout = x.double(), a.double(), gout.double()
    eps = a if W is None else a @ W.double() + (0 if b is None else b.double())
    z = x[src] + eps
    m, dz = torch.relu(z), gout[dst] * (z > 0)
    add = lambda idx, v, n: torch.zeros(n, v.shape[1], dtype=torch.float64).index_add_(0, idx, v)  # noqa: E731
    r = {"z": z, "out": add(dst, m, n_dst), "A_out": add(dst, m.abs(), n_dst),
         "d_x": add(src, dz, x.shape[0]), "A_x": add(src, dz.abs(), x.shape[0])}
    if xroot is not None:
        r["out"] += scale * xroot.double()
        r["A_out"] += (scale * xroot.double()).abs()
    if W is None:
        r.update(d_a=dz, A_a=dz.abs())
    else:
        r.update(d_W=a.T @ dz, A_W=a.abs().T @ dz.abs(), d_b=dz.sum(0), A_b=dz.abs().sum(0))
    return r


def ratio(got, ref, A):
    """max of |got - ref| / (1e-5 * max(1, A))"""
    return float(((got.double().cpu() - ref).abs() / (1e-5 * A.clamp_min(1.0))).max())


@functools.lru_cache(maxsize=None)
def make_inputs(family, name, F, D):
    """D = 0: the plain variant (a is [E, F]).  grid: every z exact in fp32 (multiples of 2^-16 below 2^7),
    some of them forced to exactly 0; normal: N(0, 1) everywhere."""
    src, dst, n_src, n_dst = make_graph(name)
    E, g = src.numel(), torch.Generator().manual_seed(100 * F + D + (1 if name == "b" else 0))
    grid = lambda shape, lo, step: torch.randint(-lo, lo + 1, shape, generator=g).float() * step  # noqa: E731
    if family == "grid":
        x, b = grid((n_src, F), 4 << 16, 2.0**-16), grid((F,), 4 << 16, 2.0**-16)
        a = grid((E, D), 64, 2.0**-5) if D else grid((E, F), 4 << 16, 2.0**-16)
        W = grid((D, F), 2048, 2.0**-11) if D else None
        eps = (a.double() @ W.double() + b.double()) if D else a.double()
        first = {int(s): e for e, s in reversed(list(enumerate(src.tolist())))}  # a source's first edge
        for k, (s, e) in enumerate(list(first.items())[:16]):
            if abs(float(eps[e, k % F])) <= 4:
                x[s, k % F] = -eps[e, k % F].float()
    else:
        x, b = torch.randn(n_src, F, generator=g), torch.randn(F, generator=g)
        a = torch.randn(E, D if D else F, generator=g)
        W = torch.randn(D, F, generator=g) if D else None
    return {"x": x, "a": a, "W": W, "b": b if D else None, "gout": torch.randn(n_dst, F, generator=g)}
