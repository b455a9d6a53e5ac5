"""TransformerConv: dot-product (query / key / value) attention over edges.

No reference counterpart (like PNAConv and DotProductDecoder); semantics are
PyG's `TransformerConv`, with edge features when `edge_dim` is set:

    q_i = lin_query(x_i),  k_j = lin_key(x_j),  v_j = lin_value(x_j)
    eps_e = lin_edge(edge_attr_e)                    edge_dim (no bias), else 0
    alpha_e = softmax_i(<q_i, k_j + eps_e>_h / sqrt(C))   per destination i and head h
    out_i = sum_e dropout(alpha_e) (v_j + eps_e)     heads concatenated or averaged
    r_i = lin_skip(x_i)                              root_weight
    out_i = beta_i r_i + (1 - beta_i) out_i,  beta_i = sigmoid(lin_beta([out_i, r_i, out_i - r_i]))   beta
    out_i = out_i + r_i                              root_weight without beta

The scores, the segment softmax and the weighted sum are ONE fused kgx kernel
(kgx_dot_attention, kgx_dot_attention_edge with edge features): no E x H
score or weight tensor exists, forward or backward.  The projected edge rows
eps [E, heads * output_dim] (and their gradient) do exist; they are made in
input-edge order and the kernel gathers them by edge id.  key and value come from one kgx_dense launch with [W_k | W_v] when
2 * heads * output_dim <= KGX_DENSE_MAX_N; the kernel reads the two column
halves in place.  No self loops are added (PyG adds none).

inputs[0] may be a pair (x_i, x_j) of a bipartite graph, and inputs[1] a
sampled Block (x then holds the block's n_src source rows, the output its
first n_dst rows), as SAGEConv accepts it.  edge_attr [E, edge_dim] is a keyword
or inputs[2], one row per edge of edge_index in its order; with a Block, one
row per block edge: edge_attr_full[blk.edge_ids].
"""

from __future__ import annotations

from typing import Any

import torch

from .. import _native as nat
from .. import ops as kops
from ..graph import Block
from ._edges import edge_index_tensor, graph_for
from .base import Dense, _first_device, shape_of, to_device_tensor
from .message_passing import MessagePassing


class TransformerConv(MessagePassing):
    def __init__(
        self,
        output_dim: int,
        heads: int = 1,
        concat: bool = True,
        beta: bool = False,
        dropout: float = 0.0,
        root_weight: bool = True,
        edge_dim: int | None = None,
        use_bias: bool = True,
        kernel_initializer: str = "glorot_uniform",
        bias_initializer: str = "zeros",
        **kwargs,
    ) -> None:
        super().__init__(aggregator="sum", **kwargs)
        if not 0.0 <= float(dropout) < 1.0:
            raise ValueError(f"TransformerConv: dropout must be in [0, 1), got {dropout}")
        self.output_dim = int(output_dim)
        self.heads = int(heads)
        self.concat = bool(concat)
        self.beta = bool(beta)
        self.dropout_rate = float(dropout)
        self.root_weight = bool(root_weight)
        self.edge_dim = None if edge_dim is None else int(edge_dim)
        if self.edge_dim is not None and self.edge_dim <= 0:
            raise ValueError(f"TransformerConv: edge_dim must be positive, got {edge_dim}")
        self.use_bias = bool(use_bias)
        self.kernel_initializer = kernel_initializer
        self.bias_initializer = bias_initializer
        self.lin_query: Dense | None = None
        self.lin_key: Dense | None = None
        self.lin_value: Dense | None = None
        self.lin_skip: Dense | None = None
        self.lin_beta: Dense | None = None
        self.lin_edge: Dense | None = None

    def _out_dim(self) -> int:
        return self.heads * self.output_dim if self.concat else self.output_dim

    def _dense(self, units: int, in_dim: int, name: str, use_bias: bool) -> Dense:
        d = Dense(units, use_bias=use_bias, kernel_initializer=self.kernel_initializer,
                  bias_initializer=self.bias_initializer, name=name)
        d._build_device = getattr(self, "_build_device", None)
        d.build((None, in_dim))
        return d

    def build(self, input_shape) -> None:
        shape = input_shape[0] if isinstance(input_shape, (list, tuple)) and len(input_shape) >= 1 else input_shape
        if isinstance(shape, (list, tuple)) and len(shape) == 2 and isinstance(shape[0], (list, tuple)):
            dst_shape, src_shape = tuple(shape[0]), tuple(shape[1])  # a pair (x_i, x_j)
        else:
            dst_shape = src_shape = tuple(shape) if shape is not None else None
        for s in (dst_shape, src_shape):
            if s is None or len(s) != 2 or s[1] is None:
                raise ValueError(f"Expected features input shape like (N, F), but got {s}")
        hc = self.heads * self.output_dim
        self.lin_query = self._dense(hc, dst_shape[1], "lin_query", self.use_bias)
        self.lin_key = self._dense(hc, src_shape[1], "lin_key", self.use_bias)
        self.lin_value = self._dense(hc, src_shape[1], "lin_value", self.use_bias)
        if self.root_weight:
            self.lin_skip = self._dense(self._out_dim(), dst_shape[1], "lin_skip", self.use_bias)
            if self.beta:
                self.lin_beta = self._dense(1, 3 * self._out_dim(), "lin_beta", False)
        if self.edge_dim is not None:  # last: the weights of a layer without edge_dim keep their order
            self.lin_edge = self._dense(hc, self.edge_dim, "lin_edge", False)
        self.built = True

    def forward(self, inputs, *args, **kwargs):
        if not self.built:  # Layer.forward, with the shapes of a pair (x_i, x_j) taken per tensor
            x = inputs[0] if isinstance(inputs, (list, tuple)) and inputs else inputs
            pair = isinstance(x, (list, tuple)) and len(x) == 2 and all(hasattr(t, "shape") for t in x)
            self._build_device = _first_device(inputs)
            self.build([(shape_of(x[0]), shape_of(x[1])) if pair else shape_of(x)])
            self.built = True
        return self.call(inputs, *args, **kwargs)

    def compute_output_shape(self, input_shape) -> tuple:
        node_shape = input_shape[0] if isinstance(input_shape, (list, tuple)) and input_shape else None
        if node_shape and isinstance(node_shape[0], (list, tuple)):
            node_shape = node_shape[0]
        return (node_shape[0] if node_shape else None, self._out_dim())

    def _edge_rows(self, edge_attr, n_edges: int, device):
        """edge_attr as fp32 [n_edges, edge_dim] on `device`; None for a layer without edge_dim."""
        if self.edge_dim is None:
            if edge_attr is not None:
                raise NotImplementedError("TransformerConv: edge features (edge_attr) need a layer built with "
                                          "edge_dim")
            return None
        if edge_attr is None:
            raise ValueError(f"TransformerConv(edge_dim={self.edge_dim}) needs edge_attr [E, {self.edge_dim}]")
        ea = to_device_tensor(edge_attr, torch.float32, device)
        if ea.dim() != 2 or tuple(ea.shape) != (n_edges, self.edge_dim):
            raise ValueError(f"TransformerConv: edge_attr must be [{n_edges}, {self.edge_dim}] (one row per edge), "
                             f"got {tuple(ea.shape)}")
        return ea

    def call(self, inputs, edge_attr=None, training=None):
        if not isinstance(inputs, (list, tuple)) or len(inputs) < 2:
            raise ValueError(f"Expected inputs to be [x, edge_index], got {inputs}")
        if len(inputs) > 2 and inputs[2] is not None:
            if edge_attr is not None:
                raise ValueError("TransformerConv: edge_attr given both as inputs[2] and as a keyword")
            edge_attr = inputs[2]
        x, edge_index = inputs[0], inputs[1]
        if isinstance(x, (list, tuple)):
            x_i = to_device_tensor(x[0], torch.float32)
            x_j = to_device_tensor(x[1], torch.float32, x_i.device)
        else:
            x_i = x_j = to_device_tensor(x, torch.float32)
        if isinstance(edge_index, Block):
            blk = edge_index
            if x_j.dim() != 2 or x_j.shape[0] != blk.n_src:
                raise ValueError(f"TransformerConv on a Block expects node features of {blk.n_src} rows (the "
                                 f"block's n_src), got shape {tuple(x_j.shape)}")
            if x_i is x_j:
                x_i = x_j[: blk.n_dst]
            elif x_i.shape[0] != blk.n_dst:
                raise ValueError(f"TransformerConv on a Block expects {blk.n_dst} destination rows, got "
                                 f"{x_i.shape[0]}")
            ea = self._edge_rows(edge_attr, blk.edge_index.shape[1], x_i.device)
            return self._attend(x_i, x_j, blk.graph if blk.edge_index.shape[1] else None, training, ea)
        ei = edge_index_tensor(edge_index, x_i.device, allow_transpose=False)
        ea = self._edge_rows(edge_attr, ei.shape[1], x_i.device)
        g = None
        if ei.shape[1] > 0 and x_i.shape[0] > 0:
            g = graph_for(edge_index, ei, x_j.shape[0], x_i.shape[0], n_features=self.heads * self.output_dim)
        return self._attend(x_i, x_j, g, training, ea)

    def _key_value(self, x_j):
        """(k, v): the two column halves of one kgx_dense with [W_k | W_v] when
        it fits the kernel's N, else two transforms."""
        hc = self.heads * self.output_dim
        Wk, Wv = self.lin_key.kernel, self.lin_value.kernel
        if 2 * hc <= nat.DENSE_MAX_N and x_j.is_cuda and kops.dense_supported(x_j, Wk):
            W = torch.cat([Wk, Wv], dim=1)
            b = torch.cat([self.lin_key.bias, self.lin_value.bias]) if self.use_bias else None
            kv = kops.dense(x_j, W, b)
            return kv[:, :hc], kv[:, hc:]
        return self.lin_key(x_j), self.lin_value(x_j)

    def _attend(self, x_i, x_j, g, training, edge_attr=None):
        n, H, C = x_i.shape[0], self.heads, self.output_dim
        if n == 0:
            return torch.zeros((0, self._out_dim()), dtype=x_i.dtype, device=x_i.device)
        if g is None:  # no edges: every destination aggregates nothing
            out = torch.zeros((n, H * C), dtype=x_i.dtype, device=x_i.device)
        else:
            q = self.lin_query(x_i)
            k, v = self._key_value(x_j)
            drop = bool(training) and self.dropout_rate > 0
            eps = None if edge_attr is None else self.lin_edge(edge_attr)
            out = kops.dot_attention(g, q, k, v, H, C, exact=self.exact,
                                     dropout=self.dropout_rate if drop else 0.0,
                                     seed=int(torch.randint(0, 2**62, (1,)).item()) if drop else 0,
                                     edge=eps, edge_order="input")
        if not self.concat:
            out = out.view(n, H, C).mean(dim=1)
        if self.root_weight:
            r = self.lin_skip(x_i)
            if self.lin_beta is not None:
                b = torch.sigmoid(self.lin_beta(torch.cat([out, r, out - r], dim=-1)))
                out = b * r + (1.0 - b) * out
            else:
                out = out + r
        return out

    def propagate(self, x, edge_index, edge_attr=None, size=None, **kwargs):
        return self.call([x, edge_index], edge_attr=edge_attr)

    def message(self, x_i, x_j, edge_attr=None, edge_index=None, size=None, **kwargs):
        return x_j

    def get_config(self) -> dict[str, Any]:
        config = super().get_config()
        config.pop("aggregator", None)
        config.update(
            {
                "output_dim": self.output_dim,
                "heads": self.heads,
                "concat": self.concat,
                "beta": self.beta,
                "dropout": self.dropout_rate,
                "root_weight": self.root_weight,
                "edge_dim": self.edge_dim,
                "use_bias": self.use_bias,
                "kernel_initializer": self.kernel_initializer,
                "bias_initializer": self.bias_initializer,
            }
        )
        return config

    @classmethod
    def from_config(cls, config: dict[str, Any]) -> "TransformerConv":
        config = dict(config)
        config.pop("aggregator", None)
        return cls(**config)
