"""GATConv (no reference counterpart; semantics are PyG's GATConv on this
project's shared-weight convention: one linear_transform without bias serves
both sides, bipartite inputs come as [x_i, x_j]).

h = x @ W, a_src[j,h] = <h[j,h,:], att_src[h,:]>, a_dst[i,h] = <h[i,h,:], att_dst[h,:]>,
score leaky_relu(a_dst[i] + a_src[j] (+ a_edge)), softmax by target, alpha-weighted
sum of h_j, + bias: ONE fused kgx kernel per layer (ops.gat_aggregate, kgx_gat).

The node scalars cost no pass of their own: the folded columns W att_src and
W att_dst ([F_in, heads] each) are appended to W, padded to a multiple of 4
columns, so one dense pass yields the table [h | a_src | a_dst], whose column
views the kernel reads in place; autograd carries the fold.

edge_dim: a_edge[e,h] = <lin_edge(edge_attr_e)[h,:], att_edge[h,:]> enters the
score; the message stays h_j.  The projected [E, heads * output_dim] rows never
exist: V[d,h] = sum_c W_e[d, h C + c] att_edge[h,c] is folded first and
a_edge = edge_attr_full @ V is [E (+ n), heads].  edge_attr, add_self_loops and
fill_value are GATv2Conv's (the fill is computed in edge_dim space; input self
loops stay ordinary edges, the documented deviation from PyG).
"""

from __future__ import annotations

from typing import Any

import torch

from .. import ops as kops
from ._edges import check_fill_value, edge_index_tensor, graph_for, loop_attr
from .base import Dense, to_device_tensor
from .message_passing import MessagePassing


class GATConv(MessagePassing):
    def __init__(
        self,
        output_dim: int,
        heads: int = 1,
        concat: bool = True,
        negative_slope: float = 0.2,
        dropout: float = 0.0,
        use_bias: bool = True,
        kernel_initializer: str = "glorot_uniform",
        bias_initializer: str = "zeros",
        att_initializer: str = "glorot_uniform",
        add_self_loops: bool = True,
        edge_dim: int | None = None,
        fill_value: float | str | torch.Tensor = "mean",
        **kwargs,
    ) -> None:
        super().__init__(aggregator="sum", **kwargs)
        self.edge_dim = None if edge_dim is None else int(edge_dim)
        if self.edge_dim is not None and self.edge_dim <= 0:
            raise ValueError(f"GATConv: edge_dim must be positive, got {edge_dim}")
        self.fill_value = check_fill_value("GATConv", fill_value, self.edge_dim)
        self.output_dim = output_dim
        self.heads = heads
        self.concat = concat
        self.negative_slope = negative_slope
        self.dropout_rate = dropout
        self.use_bias = use_bias
        self.kernel_initializer = kernel_initializer
        self.bias_initializer = bias_initializer
        self.att_initializer = att_initializer
        self.add_self_loops_flag = add_self_loops
        self.features_per_head = output_dim
        self.linear_transform: Dense | None = None
        self.att_src = None
        self.att_dst = None
        self.bias = None
        self.lin_edge: Dense | None = None
        self.att_edge = None

    def build(self, input_shape) -> None:
        shape = input_shape[0] if isinstance(input_shape, list) and len(input_shape) >= 1 else input_shape
        shape = tuple(shape) if shape is not None else None
        if shape is None or len(shape) != 2:
            raise ValueError(f"Expected features input shape like (N, F), but got {shape}")
        if shape[1] is None:
            raise ValueError("Input feature dimension cannot be None.")
        H, C = self.heads, self.features_per_head
        self.linear_transform = Dense(H * C, use_bias=False, kernel_initializer=self.kernel_initializer,
                                      name="linear_transform")
        self.linear_transform._build_device = getattr(self, "_build_device", None)
        self.linear_transform.build((None, shape[1]))
        self.att_src = self.add_weight((1, H, C), self.att_initializer, name="att_src")
        self.att_dst = self.add_weight((1, H, C), self.att_initializer, name="att_dst")
        if self.use_bias:
            self.bias = self.add_weight((H * C if self.concat else C,), self.bias_initializer, name="final_bias")
        if self.edge_dim is not None:  # last: the weights of a layer without edge_dim keep their order
            self.lin_edge = Dense(H * C, use_bias=False, kernel_initializer=self.kernel_initializer, name="lin_edge")
            self.lin_edge._build_device = getattr(self, "_build_device", None)
            self.lin_edge.build((None, self.edge_dim))
            self.att_edge = self.add_weight((1, H, C), self.att_initializer, name="att_edge")
        self.built = True

    def _out_dim(self) -> int:
        return self.heads * self.features_per_head if self.concat else self.features_per_head

    def _edge_rows(self, edge_attr, n_edges: int, device):
        """edge_attr as fp32 [n_edges, edge_dim] on `device`; None for a layer without edge_dim (which ignores it)."""
        if self.edge_dim is None:
            return None
        if edge_attr is None:
            raise ValueError(f"GATConv(edge_dim={self.edge_dim}) needs edge_attr [E, {self.edge_dim}]")
        ea = to_device_tensor(edge_attr, torch.float32, device)
        if ea.dim() != 2 or tuple(ea.shape) != (n_edges, self.edge_dim):
            raise ValueError(f"GATConv: edge_attr must be [{n_edges}, {self.edge_dim}] (one row per edge), "
                             f"got {tuple(ea.shape)}")
        return ea

    def _inputs(self, x, edge_index, edge_attr):
        if isinstance(x, (list, tuple)):
            x_i = to_device_tensor(x[0], torch.float32)
            x_j = to_device_tensor(x[1], torch.float32, x_i.device)
        else:
            x_i = x_j = to_device_tensor(x, torch.float32)
        ei = edge_index_tensor(edge_index, x_i.device, allow_transpose=False)
        return x_i, x_j, ei, self._edge_rows(edge_attr, ei.shape[1], x_i.device)

    def call(self, inputs, edge_attr=None, training=None):
        if not (isinstance(inputs, (list, tuple)) and len(inputs) >= 2):
            raise ValueError(f"Expected inputs to be [x, edge_index], got {inputs}")
        if self.edge_dim is not None and len(inputs) > 2 and inputs[2] is not None:
            if edge_attr is not None:
                raise ValueError("GATConv: edge_attr given both as inputs[2] and as a keyword")
            edge_attr = inputs[2]
        x_i, x_j, ei, ea = self._inputs(inputs[0], inputs[1], edge_attr)
        return self._gat_propagate(x_i, x_j, ei, inputs[1], training=training, edge_attr=ea)

    def propagate(self, x, edge_index, edge_attr=None, size=None, **kwargs):
        x_i, x_j, ei, ea = self._inputs(x, edge_index, edge_attr)
        return self._gat_propagate(x_i, x_j, ei, edge_index, self_loops=False, edge_attr=ea)

    def _fold(self, kernel, att):
        """[F, heads]: sum_c kernel[:, h C + c] att[h, c], the scalar a linear map and an attention vector give."""
        H, C = self.heads, self.features_per_head
        return (kernel.view(kernel.shape[0], H, C) * att.view(1, H, C)).sum(-1)

    def _node_table(self, x, with_src: bool, with_dst: bool):
        """(h, a_src, a_dst) of x as column views of one dense pass over [W | W att_src | W att_dst | 0]."""
        H, hc = self.heads, self.heads * self.features_per_head
        W = self.linear_transform.kernel
        cols = [W] + [self._fold(W, a) for a, on in ((self.att_src, with_src), (self.att_dst, with_dst)) if on]
        width = hc + H * (len(cols) - 1)
        if width % 4:
            cols.append(W.new_zeros((W.shape[0], 4 - width % 4)))
        t = kops.dense(x, torch.cat(cols, dim=1))
        a_src = t[:, hc:hc + H] if with_src else None
        lo = hc + (H if with_src else 0)
        return t[:, :hc], a_src, (t[:, lo:lo + H] if with_dst else None)

    def _gat_propagate(self, x_i, x_j, ei, edge_index_obj, self_loops: bool | None = None, training=None,
                       edge_attr=None):
        n, n_src = x_i.shape[0], x_j.shape[0]
        loops = self.add_self_loops_flag if self_loops is None else self_loops
        if loops and x_i is not x_j:
            raise ValueError("GATConv: add_self_loops requires a non-bipartite graph")
        if n == 0 or ei.shape[1] + (n if loops else 0) == 0:  # as GATv2Conv: zeros, no bias
            return torch.zeros((n, self._out_dim()), dtype=x_i.dtype, device=x_i.device)
        H, C = self.heads, self.features_per_head
        if x_j is x_i:
            h_src, a_src, a_dst = self._node_table(x_j, True, True)
        else:  # the destination side needs its scalars only: x_i @ (W att_dst), [n, F] x [F, heads]
            h_src, a_src, _ = self._node_table(x_j, True, False)
            a_dst = x_i @ self._fold(self.linear_transform.kernel, self.att_dst)
        g = graph_for(edge_index_obj, ei, n_src, n, self_loops=loops, n_features=H * C)
        use_b = self.use_bias and self.bias is not None
        drop = bool(training) and self.dropout_rate > 0
        a_edge = None
        if edge_attr is not None:  # input order; with loops, rows E + i are the loop of node i
            if loops:
                edge_attr = torch.cat([edge_attr, loop_attr(g, edge_attr, self.fill_value, self.exact)], dim=0)
            a_edge = edge_attr @ self._fold(self.lin_edge.kernel, self.att_edge)
        out = kops.gat_aggregate(g, h_src, a_src, a_dst, H, C, self.negative_slope,
                                 bias=self.bias if (use_b and self.concat) else None, exact=self.exact,
                                 dropout=self.dropout_rate if drop else 0.0,
                                 seed=int(torch.randint(0, 2**62, (1,)).item()) if drop else 0,
                                 edge=a_edge, edge_order="input")
        if not self.concat:
            out = out.view(n, H, C).mean(dim=1)
            if use_b:
                out = out + self.bias
        return out

    def message(self, x_i, x_j, edge_attr=None, edge_index=None, size=None, **kwargs):
        return x_j

    def get_config(self) -> dict[str, Any]:
        config = super().get_config()
        config.update(
            {
                "output_dim": self.output_dim,
                "heads": self.heads,
                "concat": self.concat,
                "negative_slope": self.negative_slope,
                "dropout": self.dropout_rate,
                "use_bias": self.use_bias,
                "kernel_initializer": self.kernel_initializer,
                "bias_initializer": self.bias_initializer,
                "att_initializer": self.att_initializer,
                "add_self_loops": self.add_self_loops_flag,
            }
        )
        if self.edge_dim is not None:
            fill = self.fill_value
            config.update({"edge_dim": self.edge_dim,
                           "fill_value": fill.tolist() if isinstance(fill, torch.Tensor) else fill})
        return config

    @classmethod
    def from_config(cls, config: dict[str, Any]) -> "GATConv":
        config = dict(config)
        config.pop("aggregator", None)
        if isinstance(config.get("fill_value"), (list, tuple)):
            config["fill_value"] = torch.tensor(config["fill_value"], dtype=torch.float32)
        return cls(**config)
