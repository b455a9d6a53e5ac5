"""EdgeConv and DynamicEdgeConv of Wang et al.'s DGCNN (PyG's EdgeConv / DynamicEdgeConv;
keras-geometric has no such layers).

h'_i = aggr_{j->i} MLP([x_i || x_j - x_i]),   MLP = `hidden` Dense + activation layers, then
                                                    Dense(output_dim) + activation

The first Dense, kernel [W_a; W_b] of [2 F, H] and bias b, is always folded into node tables,

[u | v] = x [W_a - W_b | W_b] + [b | 0]        (one kgx_dense pass),

so the pre-activation of edge j -> i is u_i + v_j and no [E, 2 F] concatenation is formed.

Commuted path -- no hidden layer, a non-decreasing activation (the package's own relu, leaky_relu, elu,
linear, sigmoid or tanh, given by name or as that function; any other callable counts as unknown) and
aggregator "max" or "min": the reduction commutes with the activation,
h'_i = act(u_i + max_j v_j), which is ONE max aggregation of v (kgx_spmm) and an elementwise epilogue.
No per-edge tensor exists, forward or backward.

Composed path -- hidden layers, "sum" or "mean", or another activation: u[dst] + v[src] is gathered,
the remaining Dense layers run through kgx_dense on [E, .] rows and ops.aggregate(by_edge=True)
reduces them.  This path WRITES [E, F] TENSORS (one per layer of the MLP).

A node without neighbours gets 0 on both paths.  EdgeConv is called as layer([x, edge_index]) (or with
a CSRGraph from knn_csr in place of edge_index); DynamicEdgeConv as layer([x, batch]) or layer(x): it
builds the k-NN graph of its own input with knn_csr (kgx_knn; loop=False) and runs EdgeConv on it.
The graph build is not differentiated: gradients reach x through the EdgeConv leg only, as in PyG.
"""

from __future__ import annotations

from typing import Any

import torch

from .. import ops as kops
from ..graph import CSRGraph, row_of_slot
from ._edges import edge_index_tensor, graph_for
from .base import _ACTIVATIONS, Dense, Layer, get_activation, serialize_activation, to_device_tensor

_MONOTONE = ("relu", "leaky_relu", "elu", "linear", "sigmoid", "tanh")


class EdgeConv(Layer):
    def __init__(
        self,
        output_dim: int,
        hidden: int | list[int] | tuple[int, ...] | None = None,
        activation: Any = "relu",
        aggregator: str = "max",
        use_bias: bool = True,
        kernel_initializer: str = "glorot_uniform",
        bias_initializer: str = "zeros",
        **kwargs: Any,
    ) -> None:
        super().__init__(**kwargs)
        if aggregator not in ("max", "min", "sum", "mean"):
            raise ValueError(f"EdgeConv: aggregator must be 'max', 'min', 'sum' or 'mean', got {aggregator!r}")
        widths = [] if hidden is None else ([hidden] if isinstance(hidden, int) else [int(h) for h in hidden])
        if any(h < 1 for h in widths) or int(output_dim) < 1:
            raise ValueError(f"EdgeConv: output_dim and hidden widths must be positive, got {output_dim!r}, {hidden!r}")
        self.output_dim = int(output_dim)
        self.hidden = widths
        self.activation = get_activation(activation)
        self.aggregator = aggregator
        self.use_bias = use_bias
        self.kernel_initializer = kernel_initializer
        self.bias_initializer = bias_initializer
        self.kernel = self.bias = None  # the first Dense, [2 F, H] and [H]
        self.mlp = torch.nn.ModuleList()  # the Dense layers after it
        # By identity with the package's own functions: a user callable takes the composed path whatever its name.
        self.commuted = (not widths and aggregator in ("max", "min")
                         and (self.activation is None or any(self.activation is _ACTIVATIONS[n] for n in _MONOTONE)))

    def build(self, input_shape: Any) -> None:
        node_shape = input_shape[0] if isinstance(input_shape[0], (list, tuple)) else input_shape
        if node_shape is None or len(node_shape) < 2 or node_shape[1] is None:
            raise ValueError(f"Expected node features shape (N, F), got {node_shape}")
        F = int(node_shape[1])
        widths = self.hidden + [self.output_dim]
        self.kernel = self.add_weight((2 * F, widths[0]), self.kernel_initializer, name="kernel")
        if self.use_bias:
            self.bias = self.add_weight((widths[0],), self.bias_initializer, name="bias")
        for i, h in enumerate(widths[1:]):
            layer = Dense(h, activation=self.activation, use_bias=self.use_bias,
                          kernel_initializer=self.kernel_initializer, bias_initializer=self.bias_initializer,
                          name=f"mlp_{i + 1}")
            layer._build_device = getattr(self, "_build_device", None)
            layer.build((None, widths[i]))
            self.mlp.append(layer)
        self.built = True

    def _act(self, t: torch.Tensor) -> torch.Tensor:
        return t if self.activation is None else self.activation(t)

    def _node_tables(self, x: torch.Tensor):
        F, H = x.shape[1], self.kernel.shape[1]
        wa, wb = self.kernel[:F], self.kernel[F:]
        w = torch.cat([wa - wb, wb], dim=1)
        b = torch.cat([self.bias, torch.zeros_like(self.bias)]) if self.bias is not None else None
        uv = kops.dense(x, w, b)
        return uv[:, :H], uv[:, H:].contiguous()

    def _on_graph(self, x: torch.Tensor, g: CSRGraph, src: torch.Tensor, dst: torch.Tensor) -> torch.Tensor:
        """src / dst: the edges in the order of g.eid (read by the composed path only)."""
        if g.kept == 0:
            return x.new_zeros((x.shape[0], self.output_dim))
        u, v = self._node_tables(x)
        if self.commuted:
            m = kops.aggregate(g, v, self.aggregator)
            return torch.where((g.deg > 0)[:, None], self._act(u + m), 0.0)
        h = self._act(u[dst.long()] + v[src.long()])  # [E, H]
        for layer in self.mlp:
            h = layer(h)
        return kops.aggregate(g, h, self.aggregator, by_edge=True)

    def call(self, inputs, training=None):
        if not isinstance(inputs, (list, tuple)) or len(inputs) != 2:
            raise ValueError("Inputs must be a list or tuple containing [x, edge_index]")
        x = to_device_tensor(inputs[0], torch.float32)
        N, F = x.shape
        if 2 * F != self.kernel.shape[0]:
            raise ValueError(f"EdgeConv: x has {F} columns, the layer was built for {self.kernel.shape[0] // 2}")
        if isinstance(inputs[1], CSRGraph):
            g = inputs[1]
            if g.n_src != N or g.n_dst != N:
                raise ValueError(f"EdgeConv: the graph is {g.n_dst} x {g.n_src}, x has {N} rows")
            if g.kept and not self.commuted:
                inv = torch.empty_like(g.eid, dtype=torch.long)
                inv[g.eid.long()] = torch.arange(g.kept, device=g.device)  # slot of every edge
                return self._on_graph(x, g, g.col[inv], row_of_slot(g)[inv])
            return self._on_graph(x, g, g.col, g.col)
        ei = edge_index_tensor(inputs[1], x.device, allow_transpose=True)
        if N == 0 or ei.shape[1] == 0:
            return x.new_zeros((N, self.output_dim))
        g = graph_for(inputs[1], ei, N, N, n_features=self.kernel.shape[1])
        return self._on_graph(x, g, ei[0], ei[1])

    def compute_output_shape(self, input_shape):
        x_shape = input_shape[0] if isinstance(input_shape[0], (list, tuple)) else input_shape
        return (x_shape[0], self.output_dim)

    def get_config(self) -> dict[str, Any]:
        config = super().get_config()
        config.update(
            {
                "output_dim": self.output_dim,
                "hidden": list(self.hidden) if self.hidden else None,
                "activation": serialize_activation(self.activation),
                "aggregator": self.aggregator,
                "use_bias": self.use_bias,
                "kernel_initializer": self.kernel_initializer,
                "bias_initializer": self.bias_initializer,
            }
        )
        return config


class DynamicEdgeConv(EdgeConv):
    def __init__(self, output_dim: int, k: int, hidden=None, **kwargs: Any) -> None:
        super().__init__(output_dim, hidden=hidden, **kwargs)
        if int(k) < 1:
            raise ValueError(f"DynamicEdgeConv: k must be >= 1, got {k!r}")
        self.k = int(k)

    def call(self, inputs, training=None):
        from ..knn import knn_csr  # deferred: knn imports the samplers, which import the layers' graph cache

        x, batch = (inputs[0], inputs[1]) if isinstance(inputs, (list, tuple)) else (inputs, None)
        x = to_device_tensor(x, torch.float32)
        if batch is not None and not isinstance(batch, torch.Tensor):
            batch = to_device_tensor(batch, torch.int64, x.device)
        if x.shape[0] == 0:
            return x.new_zeros((0, self.output_dim))
        g = knn_csr(x.detach(), self.k, batch, loop=False, n_features=self.kernel.shape[1])
        return super().call([x, g], training=training)

    def get_config(self) -> dict[str, Any]:
        config = super().get_config()
        config["k"] = self.k
        return config
