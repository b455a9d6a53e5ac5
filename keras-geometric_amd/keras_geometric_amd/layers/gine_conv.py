"""GINEConv: GIN with edge features (PyG's GINEConv; keras-geometric has no such layer).

h'_i = MLP((1 + eps) * x_i + sum_{j->i} relu(x_j + e_ij)),   e_ij = lin_edge(edge_attr_ij)

kgx forward: ONE fused pass (kgx_gine_run) gathers x_j, forms e_ij from the raw
edge attributes inside the kernel when edge_dim <= 32 (bf16x3-split MFMA,
f32-accurate), applies relu, sums per destination and adds (1 + eps) * x_i; no
[E, F] message or projected edge tensor is written.  edge_dim > 32 projects with
kgx_dense and feeds the same kernel's plain variant; edge_dim=None takes
edge_attr [E, F_in] as it is.  Sum aggregation only; no self loops are added.
The MLP's Dense layers run on kgx_dense.
"""

from __future__ import annotations

from typing import Any

import numpy as np
import torch

from .. import ops as kops
from ._edges import edge_index_tensor, graph_for
from .base import Constant, Dense, Dropout, Sequential, to_device_tensor
from .message_passing import MessagePassing

_KERNEL_EDGE_DIM = 32  # the widest projection edge_mp.hip does itself


class GINEConv(MessagePassing):
    def __init__(
        self,
        output_dim: int,
        mlp_hidden: list[int] | None = None,
        eps_init: float = 0.0,
        train_eps: bool = False,
        edge_dim: int | None = None,
        use_bias: bool = True,
        dropout: float = 0.0,
        kernel_initializer: str = "glorot_uniform",
        bias_initializer: str = "zeros",
        activation: str = "relu",
        **kwargs: Any,
    ) -> None:
        kwargs.pop("aggregator", None)
        super().__init__(aggregator="sum", **kwargs)
        if edge_dim is not None and int(edge_dim) < 1:
            raise ValueError(f"GINEConv: edge_dim must be a positive int or None, got {edge_dim!r}")
        self.output_dim = output_dim
        self.mlp_hidden = list(mlp_hidden) if mlp_hidden is not None else []
        self.eps_init = eps_init
        self.train_eps = train_eps
        self.edge_dim = None if edge_dim is None else int(edge_dim)
        self.use_bias = use_bias
        self.dropout_rate = dropout
        self.kernel_initializer = kernel_initializer
        self.bias_initializer = bias_initializer
        self.activation = activation
        self.mlp = None
        self.eps = None
        self.lin_edge: Dense | None = None

    def build(self, input_shape: Any) -> None:
        node_shape = input_shape[0] if isinstance(input_shape, (list, tuple)) and len(input_shape) >= 1 \
            and isinstance(input_shape[0], (list, tuple)) else input_shape
        if node_shape is None or len(node_shape) < 2 or node_shape[1] is None:
            raise ValueError(f"Expected node features shape (N, F), got {node_shape}")
        input_dim = node_shape[1]
        self.eps = self.add_weight((1,), Constant(self.eps_init), name="eps") if self.train_eps else self.eps_init
        layers = []
        for i, hidden in enumerate(self.mlp_hidden):
            layers.append(Dense(hidden, activation=self.activation, use_bias=self.use_bias,
                                kernel_initializer=self.kernel_initializer,
                                bias_initializer=self.bias_initializer, name=f"mlp_hidden_{i}"))
            if self.dropout_rate > 0:
                layers.append(Dropout(self.dropout_rate))
        layers.append(Dense(self.output_dim, activation=None, use_bias=self.use_bias,
                            kernel_initializer=self.kernel_initializer,
                            bias_initializer=self.bias_initializer, name="mlp_output"))
        self.mlp = Sequential(layers, name="gine_mlp")
        self.mlp._build_device = getattr(self, "_build_device", None)
        self.mlp.build((None, input_dim))
        if self.edge_dim is not None:  # lin_edge: [edge_dim, F_in] and a bias, as PyG's
            self.lin_edge = Dense(input_dim, use_bias=True, kernel_initializer=self.kernel_initializer,
                                  bias_initializer=self.bias_initializer, name="lin_edge")
            self.lin_edge._build_device = getattr(self, "_build_device", None)
            self.lin_edge.build((None, self.edge_dim))
        self.built = True

    def _scale(self) -> float:
        if self.train_eps:
            return float((1 + self.eps.detach()).float().item())
        return float(np.float32(1 + self.eps_init))

    def call(self, inputs, edge_attr=None, training=None):
        if not isinstance(inputs, (list, tuple)) or len(inputs) < 2:
            raise ValueError("Inputs must be a list or tuple containing [x, edge_index] or [x, edge_index, edge_attr]")
        if len(inputs) > 2 and inputs[2] is not None:
            if edge_attr is not None:
                raise ValueError("GINEConv: edge_attr given both as inputs[2] and as a keyword")
            edge_attr = inputs[2]
        if edge_attr is None:
            raise ValueError("GINEConv needs edge_attr (keyword or inputs[2])")
        x = to_device_tensor(inputs[0], torch.float32)
        edge_index = inputs[1]
        N, F = x.shape
        if N == 0:
            return torch.zeros((0, self.output_dim), dtype=x.dtype, device=x.device)
        ei = edge_index_tensor(edge_index, x.device, allow_transpose=False)
        width = F if self.edge_dim is None else self.edge_dim
        ea = to_device_tensor(edge_attr, torch.float32, x.device)
        if ea.dim() != 2 or tuple(ea.shape) != (ei.shape[1], width):
            raise ValueError(f"GINEConv: edge_attr must be [{ei.shape[1]}, {width}] (one row per edge), got "
                             f"{tuple(ea.shape)}")
        eps_live = self.train_eps and torch.is_grad_enabled() and self.eps.requires_grad
        if ei.shape[1] == 0:
            h = (1 + self.eps) * x if self.train_eps else (1 + self.eps_init) * x
            return self.mlp(h, training=training)
        g = graph_for(edge_index, ei, N, N, n_features=F)
        weight = bias = None
        if self.edge_dim is not None:
            if self.edge_dim <= _KERNEL_EDGE_DIM:
                weight, bias = self.lin_edge.kernel, self.lin_edge.bias
            else:
                ea = self.lin_edge(ea)  # kgx_dense; the kernel's plain variant takes the projected rows
        if eps_live:  # trainable eps stays in the autograd graph, as in GINConv
            h = (1 + self.eps) * x + kops.gine_aggregate(g, x, ea, weight=weight, bias=bias)
        else:
            h = kops.gine_aggregate(g, x, ea, weight=weight, bias=bias, xroot=x, gin_scale=self._scale())
        return self.mlp(h, training=training)

    def compute_output_shape(self, input_shape):
        x_shape = input_shape[0] if isinstance(input_shape, (list, tuple)) else input_shape
        return (x_shape[0], self.output_dim)

    def get_config(self) -> dict[str, Any]:
        config = super().get_config()
        config.pop("aggregator", None)
        config.update(
            {
                "output_dim": self.output_dim,
                "mlp_hidden": self.mlp_hidden,
                "eps_init": float(self.eps_init),
                "train_eps": self.train_eps,
                "edge_dim": self.edge_dim,
                "use_bias": self.use_bias,
                "dropout": self.dropout_rate,
                "kernel_initializer": self.kernel_initializer,
                "bias_initializer": self.bias_initializer,
                "activation": self.activation,
            }
        )
        return config
