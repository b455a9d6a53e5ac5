"""GATv2Conv (mirror of src/keras_geometric/layers/gatv2_conv.py).

h = x @ W (one shared Dense, no bias; gatv2_conv.py:95-101, 224-239), then ONE
fused kgx kernel per layer: per-edge score a . leaky_relu(h_i + h_j), segment
softmax by target, alpha-weighted sum of h_j, + bias (concat) — instead of the
reference's 4 gathers, 3 segment ops and E x H x C intermediates
(gatv2_conv.py:241-352).

edge_dim (no reference counterpart; semantics are PyG's GATv2Conv with
edge_dim, on the reference's shared-weight layer): eps_e = lin_edge(edge_attr_e)
(no bias) joins the score, s_e = att . leaky_relu(h_i + h_j + eps_e); the message
stays h_j.  edge_attr [E, edge_dim] is a keyword or inputs[2], one row per edge
of edge_index in its order.  With add_self_loops the added loop of node i gets
fill_value: "mean" / "add" of edge_attr over the input edges into i (0 for a
node without one), a float, or an [edge_dim] tensor; it is computed in edge_dim
space and gradients flow through it to edge_attr.  The projected rows [E (+ n),
heads * output_dim] exist (and their gradient); the kernel (kgx_gatv2_edge)
gathers them by edge id, and no E x H score or weight tensor is built.
Deviation from PyG: PyG removes the input's self loops before adding its own;
the graph build here keeps them as ordinary edges, so they keep their own
edge_attr rows and count in the fill.  Without edge_dim a passed edge_attr is
ignored, as in the reference.
"""

from __future__ import annotations

from typing import Any

import torch

from .. import ops as kops
from ._edges import edge_index_tensor, graph_for
from .base import Dense, to_device_tensor
from .message_passing import MessagePassing


class GATv2Conv(MessagePassing):
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
            raise ValueError(f"GATv2Conv: edge_dim must be positive, got {edge_dim}")
        if isinstance(fill_value, str):
            if fill_value in ("max", "min", "mul"):
                raise NotImplementedError(f"GATv2Conv: fill_value {fill_value!r} is not implemented; use 'mean', "
                                          "'add', a float or an [edge_dim] tensor")
            if fill_value not in ("mean", "add"):
                raise ValueError(f"GATv2Conv: unknown fill_value {fill_value!r}")
        elif isinstance(fill_value, torch.Tensor):
            if self.edge_dim is not None and tuple(fill_value.shape) != (self.edge_dim,):
                raise ValueError(f"GATv2Conv: a tensor fill_value must be [{self.edge_dim}], got "
                                 f"{tuple(fill_value.shape)}")
        else:
            fill_value = float(fill_value)
        self.fill_value = fill_value
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
        self.att = None
        self.bias = None
        self.lin_edge: Dense | None = None

    def build(self, input_shape) -> None:
        shape = input_shape[0] if isinstance(input_shape, list) and len(input_shape) >= 1 else input_shape
        shape = tuple(shape) if shape is not None else None
        if shape is None or len(shape) != 2:
            raise ValueError(f"Expected features input shape like (N, F), but got {shape}")
        if shape[1] is None:
            raise ValueError("Input feature dimension cannot be None.")
        self.linear_transform = Dense(self.heads * self.features_per_head, use_bias=False,
                                      kernel_initializer=self.kernel_initializer, name="linear_transform")
        self.linear_transform._build_device = getattr(self, "_build_device", None)
        self.linear_transform.build((None, shape[1]))
        self.att = self.add_weight((1, self.heads, self.features_per_head), self.att_initializer, name="att")
        if self.use_bias:
            n = self.heads * self.features_per_head if self.concat else self.features_per_head
            self.bias = self.add_weight((n,), self.bias_initializer, name="final_bias")
        if self.edge_dim is not None:  # last: the weights of a layer without edge_dim keep their order
            self.lin_edge = Dense(self.heads * self.features_per_head, use_bias=False,
                                  kernel_initializer=self.kernel_initializer, name="lin_edge")
            self.lin_edge._build_device = getattr(self, "_build_device", None)
            self.lin_edge.build((None, self.edge_dim))
        self.built = True

    def _out_dim(self) -> int:
        return self.heads * self.features_per_head if self.concat else self.features_per_head

    def _edge_rows(self, edge_attr, n_edges: int, device):
        """edge_attr as fp32 [n_edges, edge_dim] on `device`; None for a layer without edge_dim
        (which ignores edge_attr, as the reference does)."""
        if self.edge_dim is None:
            return None
        if edge_attr is None:
            raise ValueError(f"GATv2Conv(edge_dim={self.edge_dim}) needs edge_attr [E, {self.edge_dim}]")
        ea = to_device_tensor(edge_attr, torch.float32, device)
        if ea.dim() != 2 or tuple(ea.shape) != (n_edges, self.edge_dim):
            raise ValueError(f"GATv2Conv: edge_attr must be [{n_edges}, {self.edge_dim}] (one row per edge), "
                             f"got {tuple(ea.shape)}")
        return ea

    def call(self, inputs, edge_attr=None, training=None):
        if isinstance(inputs, (list, tuple)) and len(inputs) >= 2:
            x, edge_index = inputs[0], inputs[1]
        else:
            raise ValueError(f"Expected inputs to be [x, edge_index], got {inputs}")
        if self.edge_dim is not None and len(inputs) > 2 and inputs[2] is not None:
            if edge_attr is not None:
                raise ValueError("GATv2Conv: edge_attr given both as inputs[2] and as a keyword")
            edge_attr = inputs[2]
        if isinstance(x, (list, tuple)):
            x_i = to_device_tensor(x[0], torch.float32)
            x_j = to_device_tensor(x[1], torch.float32, x_i.device)
        else:
            x_i = x_j = to_device_tensor(x, torch.float32)
        ei = edge_index_tensor(edge_index, x_i.device, allow_transpose=False)
        ea = self._edge_rows(edge_attr, ei.shape[1], x_i.device)
        return self._gatv2_propagate(x_i, x_j, ei, edge_index, training=training, edge_attr=ea)

    def propagate(self, x, edge_index, edge_attr=None, size=None, **kwargs):
        if isinstance(x, (list, tuple)):
            x_i = to_device_tensor(x[0], torch.float32)
            x_j = to_device_tensor(x[1], torch.float32, x_i.device)
        else:
            x_i = x_j = to_device_tensor(x, torch.float32)
        ei = edge_index_tensor(edge_index, x_i.device, allow_transpose=False)
        ea = self._edge_rows(edge_attr, ei.shape[1], x_i.device)
        return self._gatv2_propagate(x_i, x_j, ei, edge_index, self_loops=False, edge_attr=ea)

    def _loop_attr(self, g, edge_attr):
        """[n, edge_dim]: the edge_attr row of the self loop the graph added to every node (fill_value)."""
        n = g.n_dst
        fill = self.fill_value
        if isinstance(fill, str):
            # by-edge sum over the loop graph itself (no second CSR): its loop slots read the zero rows E + i
            table = torch.cat([edge_attr, edge_attr.new_zeros((n, self.edge_dim))], dim=0)
            tot = kops.aggregate(g, table, "sum", by_edge=True, exact=self.exact)
            if fill == "add":
                return tot
            return tot / (g.deg.to(tot.dtype) - 1.0).clamp_min(1.0)[:, None]  # the loop-free in-degree
        if isinstance(fill, torch.Tensor):
            return fill.to(edge_attr).reshape(1, self.edge_dim).expand(n, -1)
        return edge_attr.new_full((n, self.edge_dim), fill)

    def _gatv2_propagate(self, x_i, x_j, ei, edge_index_obj, self_loops: bool | None = None, training=None,
                         edge_attr=None):
        n, n_src = x_i.shape[0], x_j.shape[0]
        loops = self.add_self_loops_flag if self_loops is None else self_loops
        if loops and x_i is not x_j:
            raise ValueError("GATv2Conv: add_self_loops requires a non-bipartite graph")
        if n == 0:
            return torch.zeros((0, self._out_dim()), dtype=x_i.dtype, device=x_i.device)
        e = ei.shape[1] + (n if loops else 0)
        if e == 0:  # gatv2_conv.py:204-210 (no bias)
            return torch.zeros((n, self._out_dim()), dtype=x_i.dtype, device=x_i.device)
        H, C = self.heads, self.features_per_head
        h_dst = self.linear_transform(x_i).contiguous()
        h_src = h_dst if x_j is x_i else self.linear_transform(x_j).contiguous()
        g = graph_for(edge_index_obj, ei, n_src, n, self_loops=loops, n_features=H * C)
        use_b = self.use_bias and self.bias is not None
        drop = bool(training) and self.dropout_rate > 0  # attention dropout, gatv2_conv.py:252-253
        eps = None
        if edge_attr is not None:  # projected in input order; with loops, rows E + i are the loop of node i
            if loops:
                edge_attr = torch.cat([edge_attr, self._loop_attr(g, edge_attr)], dim=0)
            eps = self.lin_edge(edge_attr)
        out = kops.gatv2_aggregate(g, h_src, h_dst, self.att, H, C, self.negative_slope,
                                   bias=self.bias if (use_b and self.concat) else None, exact=self.exact,
                                   dropout=self.dropout_rate if drop else 0.0,
                                   seed=int(torch.randint(0, 2**62, (1,)).item()) if drop else 0,
                                   edge=eps, edge_order="input")
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
        if self.edge_dim is not None:  # a layer without edge_dim keeps its config
            fill = self.fill_value
            config.update({"edge_dim": self.edge_dim,
                           "fill_value": fill.tolist() if isinstance(fill, torch.Tensor) else fill})
        return config

    @classmethod
    def from_config(cls, config: dict[str, Any]) -> "GATv2Conv":
        config = dict(config)
        config.pop("aggregator", None)
        if isinstance(config.get("fill_value"), (list, tuple)):
            config["fill_value"] = torch.tensor(config["fill_value"], dtype=torch.float32)
        return cls(**config)
