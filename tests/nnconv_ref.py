"""float64 restatement of the edge-conditioned convolution (ops.nnconv_aggregate / kgx_nnconv_run) from its
LITERAL definition: per edge Theta_e = B + sum_d c_e[d] W_d, m_e = x_j Theta_e, then an index_add.  The
graph is tests/rgcn_ref.py's fixture with the edge types ignored.  No project code."""

import functools

import torch

from rgcn_ref import N_DST, N_SRC, make_graph, ratio  # noqa: F401  (ratio: the shared err / bound)


def nnconv64(x, coef, W, B, root, b, src, dst, n_dst, mean, gout):
    """out, the six gradients and, per element, A = the sum of the magnitudes of its contributions."""
    x, coef, W, gout = x.double(), coef.double(), W.double(), gout.double()
    src, dst = torch.as_tensor(src).long(), torch.as_tensor(dst).long()
    cnt = torch.zeros(n_dst, dtype=torch.float64).index_add_(0, dst, torch.ones(dst.numel(), dtype=torch.float64))
    norm = (1.0 / cnt.clamp_min(1.0) if mean else torch.ones_like(cnt))[dst]  # per edge
    add = lambda idx, v, n: torch.zeros(n, *v.shape[1:], dtype=torch.float64).index_add_(0, idx, v)  # noqa: E731
    theta, theta_a = torch.einsum("ed,dfo->efo", coef, W), torch.einsum("ed,dfo->efo", coef.abs(), W.abs())
    if B is not None:
        theta, theta_a = theta + B.double(), theta_a + B.double().abs()
    xs, gd = x[src] * norm[:, None], gout[dst] * norm[:, None]  # the edge's source row and output gradient, normed
    r = {"out": add(dst, torch.einsum("ef,efo->eo", xs, theta), n_dst),
         "A_out": add(dst, torch.einsum("ef,efo->eo", xs.abs(), theta_a), n_dst),
         "d_x": add(src, torch.einsum("eo,efo->ef", gd, theta), x.shape[0]),
         "A_x": add(src, torch.einsum("eo,efo->ef", gd.abs(), theta_a), x.shape[0])}
    outer, outer_a = torch.einsum("ef,eo->efo", x[src], gd), torch.einsum("ef,eo->efo", x[src].abs(), gd.abs())
    r.update(d_coef=torch.einsum("efo,dfo->ed", outer, W), A_coef=torch.einsum("efo,dfo->ed", outer_a, W.abs()),
             d_W=torch.einsum("ed,efo->dfo", coef, outer), A_W=torch.einsum("ed,efo->dfo", coef.abs(), outer_a))
    if B is not None:
        r.update(d_B=outer.sum(0), A_B=outer_a.sum(0))
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


@functools.lru_cache(maxsize=None)
def make_inputs(F_in, F_out, D):
    g = torch.Generator().manual_seed(1000 * F_in + F_out + 7 * D)
    E = make_graph()[0].size
    return {"x": torch.randn(N_SRC, F_in, generator=g), "coef": torch.randn(E, D, generator=g),
            "W": torch.randn(D, F_in, F_out, generator=g), "B": torch.randn(F_in, F_out, generator=g),
            "root": torch.randn(F_in, F_out, generator=g), "b": torch.randn(F_out, generator=g),
            "gout": torch.randn(N_DST, F_out, generator=g)}
