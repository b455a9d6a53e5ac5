"""float64 restatement of R-GCN's layer map (ops.rgcn_aggregate / kgx_rgcn_run) with plain index_add, and
the seeded typed fixture graph of tests/test_gpu_rgcn.py.  No project code."""

import functools

import numpy as np
import torch

N_SRC, N_DST, R, PIECE_LEN = 90, 75, 5, 64
EMPTY_NODES = (0, 37, N_DST - 1)
HUB, HUB_COUNTS = 5, (128, 200, 250)  # 578 slots, 10 pieces: the cut at 64 is inside pair (5, 0), the one at 128 ends it
SECOND, SECOND_COUNTS = 20, (40, 50)  # 90 slots: exactly 2 pieces
LONE, LONE_REL, EMPTY_REL = 10, 3, 4  # relation 3 is used by node 10 alone, relation 4 by nobody


@functools.lru_cache(maxsize=None)
def make_graph():
    """(src, dst, type) int64 numpy arrays in shuffled input order, duplicates included."""
    rng = np.random.default_rng(7)
    plain = np.array([i for i in range(N_DST) if i not in EMPTY_NODES + (HUB, SECOND)])
    dst, typ = [rng.choice(plain, 600)], [rng.integers(0, 3, 600)]
    for node, counts in ((HUB, HUB_COUNTS), (SECOND, SECOND_COUNTS)):
        for r, c in enumerate(counts):
            dst.append(np.full(c, node))
            typ.append(np.full(c, r))
    dst.append(np.full(6, LONE))
    typ.append(np.full(6, LONE_REL))
    dst, typ = np.concatenate(dst), np.concatenate(typ)
    src = rng.integers(0, N_SRC, dst.size)
    dup = rng.choice(600, 12, replace=False)  # the same (src, dst, type) twice, among the plain nodes
    src, dst, typ = (np.concatenate([a, a[dup]]) for a in (src, dst, typ))
    perm = rng.permutation(dst.size)
    return src[perm], dst[perm], typ[perm]


def rgcn64(x, W, root, b, src, dst, typ, n_dst, mean, gout):
    """out, the gradients and, per element, A = the sum of the magnitudes of its contributions."""
    x, W, gout = x.double(), W.double(), gout.double()
    Rn, F_in, F_out = W.shape
    src, key = torch.as_tensor(src).long(), torch.as_tensor(dst).long() * Rn + torch.as_tensor(typ).long()
    add = lambda idx, v, n: torch.zeros(n, v.shape[1], dtype=torch.float64).index_add_(0, idx, v)  # noqa: E731
    cnt = torch.zeros(n_dst * Rn, dtype=torch.float64).index_add_(0, key, torch.ones(key.numel(), dtype=torch.float64))
    norm = (1.0 / cnt.clamp_min(1.0) if mean else torch.ones_like(cnt)).unsqueeze(1)
    H, Ha = (add(key, v[src], n_dst * Rn) * norm for v in (x, x.abs()))
    H, Ha = H.view(n_dst, Rn * F_in), Ha.view(n_dst, Rn * F_in)
    Wc = W.reshape(Rn * F_in, F_out)
    Z, Za = ((g @ w.T).view(n_dst * Rn, F_in) * norm for g, w in ((gout, Wc), (gout.abs(), Wc.abs())))
    r = {"out": H @ Wc, "A_out": Ha @ Wc.abs(), "d_W": (H.T @ gout).view_as(W), "A_W": (Ha.T @ gout.abs()).view_as(W),
         "d_x": add(src, Z[key], x.shape[0]), "A_x": add(src, Za[key], x.shape[0])}
    if root is not None:
        xr, root = x[:n_dst], root.double()
        r["out"] += xr @ root
        r["A_out"] += xr.abs() @ root.abs()
        r["d_x"][:n_dst] += gout @ root.T
        r["A_x"][:n_dst] += gout.abs() @ root.abs().T
        r.update(d_root=xr.T @ gout, A_root=xr.abs().T @ gout.abs())
    if b is not None:
        r["out"] += b.double()
        r["A_out"] += b.double().abs()
        r.update(d_b=gout.sum(0), A_b=gout.abs().sum(0))
    return r


def ratio(got, ref, A):
    """max of |got - ref| / (1e-5 * max(1, A))"""
    return float(((got.double().cpu() - ref).abs() / (1e-5 * A.clamp_min(1.0))).max())


@functools.lru_cache(maxsize=None)
def make_inputs(F_in, F_out, Rn=R):
    g = torch.Generator().manual_seed(1000 * F_in + F_out + Rn)
    return {"x": torch.randn(N_SRC, F_in, generator=g), "W": torch.randn(Rn, F_in, F_out, generator=g),
            "root": torch.randn(F_in, F_out, generator=g), "b": torch.randn(F_out, generator=g),
            "gout": torch.randn(N_DST, F_out, generator=g)}
