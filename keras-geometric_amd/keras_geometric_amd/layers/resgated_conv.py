"""ResGatedGraphConv: the residual gated graph convolution (Bresson & Laurent; PyG's
ResGatedGraphConv; keras-geometric has no such layer), also the local layer of
GatedGCN / GraphGPS stacks.

h'_i = lin_skip(x_i) + bias + sum_{j->i} sigmoid(lin_key(x_i) + lin_query(x_j) + lin_edge(e_ij)) * lin_value(x_j)

kgx forward: ONE dense pass over the concatenated kernel [W_key | W_query | W_value |
W_skip] gives the table [k | q | v | skip], whose column views ONE fused kernel
(ops.gated_aggregate, kgx_gated) reads in place: it forms every gate per channel,
sums per destination and adds skip and bias in its store.  q and v are adjacent
columns, so one source's two gathered rows share DRAM pages.  No [E, F] gate or
message tensor is written, and the backward recomputes the gates instead of
keeping them.  edge_attr is projected by kgx_dense ([E, F], no bias).  Sum
aggregation only; no self loops are added; square graphs only.

A layer whose weights were built on the host (layer._build_device = cpu) keeps CPU
tensors on the host and runs the op's composed torch form.
"""

from __future__ import annotations

from typing import Any

import torch

from .. import graph as G
from .. import ops as kops
from ._edges import edge_index_tensor, graph_for
from .base import Dense, to_device_tensor
from .message_passing import MessagePassing


def _host_csr(ei: torch.Tensor, n: int) -> G.CSRGraph:
    """The CSR a stable build gives, on the host and without a schedule (the composed form needs none)."""
    src, dst = ei[0].long(), ei[1].long()
    order = torch.sort(dst, stable=True).indices
    deg = torch.bincount(dst, minlength=n).to(torch.int32)
    rowptr = torch.zeros(n + 1, dtype=torch.int32)
    rowptr[1:] = torch.cumsum(deg, 0)
    return G.CSRGraph(n_src=n, n_dst=n, n_input_edges=src.numel(), kept=src.numel(), max_degree=int(deg.max()),
                      flags=0, rowptr=rowptr, col=src[order].to(torch.int32), eid=order.to(torch.int32), deg=deg)


class ResGatedGraphConv(MessagePassing):
    def __init__(
        self,
        output_dim: int,
        edge_dim: int | None = None,
        root_weight: bool = True,
        use_bias: bool = True,
        kernel_initializer: str = "glorot_uniform",
        bias_initializer: str = "zeros",
        **kwargs: Any,
    ) -> None:
        act = kwargs.pop("act", "sigmoid")
        if act != "sigmoid":
            raise ValueError(f"ResGatedGraphConv: the gate is a sigmoid (the fused kernel has no other), got act={act!r}")
        kwargs.pop("aggregator", None)
        super().__init__(aggregator="sum", **kwargs)
        if edge_dim is not None and int(edge_dim) < 1:
            raise ValueError(f"ResGatedGraphConv: edge_dim must be a positive int or None, got {edge_dim!r}")
        self.output_dim = int(output_dim)
        self.edge_dim = None if edge_dim is None else int(edge_dim)
        self.root_weight = bool(root_weight)
        self.use_bias = bool(use_bias)
        self.kernel_initializer = kernel_initializer
        self.bias_initializer = bias_initializer
        self.bias = None
        self.lin_key: Dense | None = None
        self.lin_query: Dense | None = None
        self.lin_value: Dense | None = None
        self.lin_skip: Dense | None = None
        self.lin_edge: Dense | None = None

    def _dense(self, name: str, in_dim: int, use_bias: bool) -> Dense:
        d = Dense(self.output_dim, use_bias=use_bias, kernel_initializer=self.kernel_initializer,
                  bias_initializer=self.bias_initializer, name=name)
        d._build_device = getattr(self, "_build_device", None)
        d.build((None, in_dim))
        return d

    def build(self, input_shape: Any) -> None:
        node_shape = input_shape[0] if isinstance(input_shape, (list, tuple)) and len(input_shape) >= 1 \
            and isinstance(input_shape[0], (list, tuple)) else input_shape
        if node_shape is None or len(node_shape) < 2 or node_shape[1] is None:
            raise ValueError(f"Expected node features shape (N, F), got {node_shape}")
        in_dim = int(node_shape[1])
        if self.use_bias:
            self.bias = self.add_weight((self.output_dim,), self.bias_initializer, name="final_bias")
        self.lin_key = self._dense("lin_key", in_dim, True)
        self.lin_query = self._dense("lin_query", in_dim, True)
        self.lin_value = self._dense("lin_value", in_dim, True)
        if self.root_weight:
            self.lin_skip = self._dense("lin_skip", in_dim, False)
        if self.edge_dim is not None:
            self.lin_edge = self._dense("lin_edge", self.edge_dim, False)
        self.built = True

    def _node_table(self, x):
        """(k, q, v, skip) of x as column views of one dense pass over [W_key | W_query | W_value | W_skip]."""
        F = self.output_dim
        lins = [self.lin_key, self.lin_query, self.lin_value]
        kernels, biases = [d.kernel for d in lins], [d.bias for d in lins]
        if self.root_weight:
            kernels.append(self.lin_skip.kernel)
            biases.append(biases[0].new_zeros(F))
        t = kops.dense(x, torch.cat(kernels, dim=1), torch.cat(biases))
        return t[:, :F], t[:, F:2 * F], t[:, 2 * F:3 * F], (t[:, 3 * F:] if self.root_weight else None)

    def call(self, inputs, edge_attr=None, training=None):
        if not isinstance(inputs, (list, tuple)) or len(inputs) < 2:
            raise ValueError("Inputs must be a list or tuple containing [x, edge_index] or [x, edge_index, edge_attr]")
        if len(inputs) > 2 and inputs[2] is not None:
            if edge_attr is not None:
                raise ValueError("ResGatedGraphConv: edge_attr given both as inputs[2] and as a keyword")
            edge_attr = inputs[2]
        if (edge_attr is None) != (self.edge_dim is None):
            raise ValueError(f"ResGatedGraphConv(edge_dim={self.edge_dim}): edge_attr "
                             + ("is needed (keyword or inputs[2])" if edge_attr is None else "needs edge_dim"))
        host = isinstance(inputs[0], torch.Tensor) and not inputs[0].is_cuda and not self.lin_key.kernel.is_cuda
        x = inputs[0].to(torch.float32) if host else to_device_tensor(inputs[0], torch.float32)
        N, F = x.shape[0], self.output_dim
        if N == 0:
            return torch.zeros((0, F), dtype=x.dtype, device=x.device)
        ei = torch.as_tensor(inputs[1]) if host else edge_index_tensor(inputs[1], x.device, allow_transpose=False)
        E = ei.shape[1]
        ea = None
        if edge_attr is not None:
            ea = edge_attr.to(torch.float32) if host else to_device_tensor(edge_attr, torch.float32, x.device)
            if ea.dim() != 2 or tuple(ea.shape) != (E, self.edge_dim):
                raise ValueError(f"ResGatedGraphConv: edge_attr must be [{E}, {self.edge_dim}] (one row per edge), "
                                 f"got {tuple(ea.shape)}")
        bias = self.bias if self.use_bias else None
        if E == 0:  # no message: the skip connection and the bias
            out = self.lin_skip(x) if self.root_weight else torch.zeros((N, F), dtype=x.dtype, device=x.device)
            return out if bias is None else out + bias
        g = _host_csr(ei, N) if host else graph_for(inputs[1], ei, N, N, n_features=F)
        k, q, v, skip = self._node_table(x)
        edge = None if ea is None else kops.dense(ea, self.lin_edge.kernel)
        return kops.gated_aggregate(g, k, q, v, edge=edge, edge_order="input", root=skip, bias=bias, exact=self.exact)

    def compute_output_shape(self, input_shape):
        x_shape = input_shape[0] if isinstance(input_shape, (list, tuple)) else input_shape
        return (x_shape[0], self.output_dim)

    def get_config(self) -> dict[str, Any]:
        config = super().get_config()
        config.pop("aggregator", None)
        config.update(
            {
                "output_dim": self.output_dim,
                "edge_dim": self.edge_dim,
                "root_weight": self.root_weight,
                "use_bias": self.use_bias,
                "kernel_initializer": self.kernel_initializer,
                "bias_initializer": self.bias_initializer,
            }
        )
        return config
