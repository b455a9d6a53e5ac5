"""float64 restatement of kgx_edge_dot and of its backward identity.

    out[p, k] = sum_f xa[a_idx[p], f] * xb[b_idx[p, k], f]

edge_dot() also returns mag[p, k] = sum_f |xa| |xb|, the scale of the fp32
error bound the GPU tests hold: an fp32 dot of F terms in any summation order
errs by at most gamma_F * mag with gamma_F = F u / (1 - F u), u = 2^-24; the
tests use F * 2^-23 * mag, twice that to first order.
"""

import numpy as np
import torch


def edge_dot(xa, xb, a_idx, b_idx):
    """(scores float64 [P, K], mag float64 [P, K]); an index outside its table gives NaN."""
    xa, xb = np.asarray(xa, np.float64), np.asarray(xb, np.float64)
    a_idx, b_idx = np.asarray(a_idx, np.int64), np.asarray(b_idx, np.int64)
    b2 = b_idx.reshape(a_idx.shape[0], -1)
    bad = ((a_idx < 0) | (a_idx >= xa.shape[0]))[:, None] | (b2 < 0) | (b2 >= xb.shape[0])
    ra = xa[np.clip(a_idx, 0, xa.shape[0] - 1)][:, None, :]
    rb = xb[np.clip(b2, 0, xb.shape[0] - 1)]
    with np.errstate(invalid="ignore", over="ignore"):
        s = (ra * rb).sum(-1)
        mag = (np.abs(ra) * np.abs(rb)).sum(-1)
    s[bad] = np.nan
    return s, mag


def bound(F, mag):
    return F * 2.0**-23 * mag


def composed(xa, xb, a_idx, b_idx):
    """The composed torch form users write today (any dtype / device), [P, K]."""
    b2 = b_idx.reshape(a_idx.shape[0], -1).long()
    return (xa[a_idx.long()].unsqueeze(1) * xb[b2]).sum(-1)


def backward_identity(xa, xb, a_idx, b_idx, D):
    """(d xa, d xb) by the identity the library's backward uses, restated with
    index_add over the pair graph (src = b_idx.flatten(), dst = a_idx repeated K
    times, weight = D.flatten()):
        d xa[i] = sum_{pairs with a = i} D * xb[b],  d xb[j] = sum_{pairs with b = j} D * xa[a]."""
    K = b_idx.reshape(a_idx.shape[0], -1).shape[1]
    src = b_idx.reshape(-1).long()
    dst = a_idx.long().repeat_interleave(K)
    w = D.reshape(-1, 1)
    g_xa = torch.zeros_like(xa).index_add(0, dst, w * xb[src])
    g_xb = torch.zeros_like(xb).index_add(0, src, w * xa[dst])
    return g_xa, g_xb
