"""GENConv: the generalized graph convolution of DeeperGCN (Li et al., "DeeperGCN: All You Need to Train
Deeper GCNs"; PyG's GENConv; keras-geometric has no such layer), with its softmax aggregation.

m_ij = relu(x_j + e_ij) + eps
h'_i = MLP( sum_j softmax_j(t * m_ij) * m_ij  +  x_i )          (a softmax per channel, over i's in-edges)

x goes through lin_src (messages) and lin_dst (the residual) when in_channels != out_channels, edge_attr
through lin_edge when edge_dim != out_channels.  The MLP has num_layers Dense layers, the hidden ones
out_channels * expansion wide and followed by norm and ReLU.  t is a float, or a learnt scalar (learn_t).

kgx forward: ONE fused kernel (ops.softmax_aggregate, kgx_softmax_aggr) gathers x_j and the edge row, forms
the message and keeps a running softmax per channel; no [E, F] message, exponential or product is written, and
the backward recomputes the weights instead of keeping them.  The linear maps and the MLP run on kgx_dense.
Softmax aggregation only; no self loops are added; square graphs only.

A layer whose weights were built on the host (layer._build_device = cpu) keeps CPU tensors on the host and
runs the op's composed torch form.
"""

from __future__ import annotations

from typing import Any

import torch

from .. import ops as kops
from ._edges import edge_index_tensor, graph_for
from .base import Constant, Dense, Layer, to_device_tensor
from .message_passing import MessagePassing
from .resgated_conv import _host_csr


class _Norm(Layer):
    """BatchNorm1d ("batch": running statistics in inference, batch statistics when training) or LayerNorm
    ("layer") over the feature axis, with a learnt scale and shift."""

    def __init__(self, kind: str, width: int, **kwargs: Any) -> None:
        super().__init__(**kwargs)
        self.kind, self.width = kind, width
        self.gamma = self.beta = None

    def build(self, input_shape=None) -> None:
        self.gamma = self.add_weight((self.width,), "ones", name="gamma")
        self.beta = self.add_weight((self.width,), "zeros", name="beta")
        if self.kind == "batch":
            self.register_buffer("moving_mean", torch.zeros_like(self.beta))
            self.register_buffer("moving_var", torch.ones_like(self.beta))
        self.built = True

    def forward(self, x, training=None):
        if self.kind == "layer":
            return torch.nn.functional.layer_norm(x, (self.width,), self.gamma, self.beta, 1e-5)
        return torch.nn.functional.batch_norm(x, self.moving_mean, self.moving_var, self.gamma, self.beta,
                                              bool(training), 0.1, 1e-5)


class GENConv(MessagePassing):
    def __init__(
        self,
        in_channels: int,
        out_channels: int,
        aggr: str = "softmax",
        t: float = 1.0,
        learn_t: bool = False,
        norm: str | None = "batch",
        num_layers: int = 2,
        expansion: int = 2,
        eps: float = 1e-7,
        bias: bool = False,
        edge_dim: int | None = None,
        **kwargs: Any,
    ) -> None:
        if aggr != "softmax":
            raise ValueError(f"GENConv: aggr must be 'softmax' (the fused kernel has no other), got aggr={aggr!r}")
        for arg in ("learn_p", "msg_norm", "learn_msg_scale", "semi_grad"):  # PyG's, out of scope here
            if kwargs.pop(arg, False):
                raise ValueError(f"GENConv: {arg} is not supported (softmax aggregation with a scalar t only)")
        if kwargs.pop("p", 1.0) != 1.0:
            raise ValueError("GENConv: p (power-mean aggregation) is not supported")
        if norm not in ("batch", "layer", None):
            raise ValueError(f"GENConv: norm must be 'batch', 'layer' or None, got norm={norm!r}")
        if int(num_layers) < 1 or int(expansion) < 1:
            raise ValueError(f"GENConv: num_layers and expansion must be positive, got {num_layers}, {expansion}")
        if edge_dim is not None and int(edge_dim) < 1:
            raise ValueError(f"GENConv: edge_dim must be a positive int or None, got {edge_dim!r}")
        kwargs.pop("aggregator", None)
        super().__init__(aggregator="sum", **kwargs)
        self.in_channels, self.out_channels = int(in_channels), int(out_channels)
        self.aggr = aggr
        self.initial_t, self.learn_t = float(t), bool(learn_t)
        self.norm, self.num_layers, self.expansion = norm, int(num_layers), int(expansion)
        self.eps, self.use_bias = float(eps), bool(bias)
        self.edge_dim = None if edge_dim is None else int(edge_dim)
        self.t: Any = self.initial_t
        self.lin_src: Dense | None = None
        self.lin_dst: Dense | None = None
        self.lin_edge: Dense | None = None
        self.mlp = torch.nn.ModuleList()

    def _sub(self, layer: Layer, in_dim: int) -> Layer:
        layer._build_device = getattr(self, "_build_device", None)
        layer.build((None, in_dim))
        return layer

    def build(self, input_shape: Any) -> None:
        node_shape = input_shape[0] if isinstance(input_shape, (list, tuple)) and len(input_shape) >= 1 \
            and isinstance(input_shape[0], (list, tuple)) else input_shape
        if node_shape is None or len(node_shape) < 2 or node_shape[1] != self.in_channels:
            raise ValueError(f"GENConv: expected node features of shape (N, {self.in_channels}), got {node_shape}")
        F = self.out_channels
        if self.learn_t:
            self.t = self.add_weight((), Constant(self.initial_t), name="t")
        if self.in_channels != F:
            self.lin_src = self._sub(Dense(F, use_bias=self.use_bias, name="lin_src"), self.in_channels)
            self.lin_dst = self._sub(Dense(F, use_bias=self.use_bias, name="lin_dst"), self.in_channels)
        if self.edge_dim is not None and self.edge_dim != F:
            self.lin_edge = self._sub(Dense(F, use_bias=self.use_bias, name="lin_edge"), self.edge_dim)
        widths = [F] + [F * self.expansion] * (self.num_layers - 1) + [F]
        for i in range(1, len(widths)):
            hidden = i < len(widths) - 1
            # Dense -> norm -> ReLU per hidden layer (the ReLU in kgx_dense's epilogue without a norm between)
            act = "relu" if hidden and self.norm is None else None
            self.mlp.append(self._sub(Dense(widths[i], activation=act, use_bias=self.use_bias, name=f"mlp_{i - 1}"),
                                      widths[i - 1]))
            if hidden and self.norm is not None:
                self.mlp.append(self._sub(_Norm(self.norm, widths[i], name=f"norm_{i - 1}"), widths[i]))
        self.built = True

    def _mlp(self, h, training):
        for layer in self.mlp:
            h = torch.relu(layer(h, training=training)) if isinstance(layer, _Norm) else layer(h)
        return h

    def call(self, inputs, edge_attr=None, training=None):
        if not isinstance(inputs, (list, tuple)) or len(inputs) < 2:
            raise ValueError("Inputs must be a list or tuple containing [x, edge_index] or [x, edge_index, edge_attr]")
        if len(inputs) > 2 and inputs[2] is not None:
            if edge_attr is not None:
                raise ValueError("GENConv: edge_attr given both as inputs[2] and as a keyword")
            edge_attr = inputs[2]
        if (edge_attr is None) != (self.edge_dim is None):
            raise ValueError(f"GENConv(edge_dim={self.edge_dim}): edge_attr "
                             + ("is needed (keyword or inputs[2])" if edge_attr is None else "needs edge_dim"))
        host = isinstance(inputs[0], torch.Tensor) and not inputs[0].is_cuda and not self.mlp[0].kernel.is_cuda
        x = inputs[0].to(torch.float32) if host else to_device_tensor(inputs[0], torch.float32)
        N = x.shape[0]
        if N == 0:
            return torch.zeros((0, self.out_channels), dtype=x.dtype, device=x.device)
        ei = torch.as_tensor(inputs[1]) if host else edge_index_tensor(inputs[1], x.device, allow_transpose=False)
        E = ei.shape[1]
        x_src = x if self.lin_src is None else self.lin_src(x)
        x_dst = x if self.lin_dst is None else self.lin_dst(x)
        if E == 0:  # no message: the residual alone
            return self._mlp(x_dst, training)
        edge = None
        if edge_attr is not None:
            edge = edge_attr.to(torch.float32) if host else to_device_tensor(edge_attr, torch.float32, x.device)
            if edge.dim() != 2 or tuple(edge.shape) != (E, self.edge_dim):
                raise ValueError(f"GENConv: edge_attr must be [{E}, {self.edge_dim}] (one row per edge), got "
                                 f"{tuple(edge.shape)}")
            if self.lin_edge is not None:
                edge = self.lin_edge(edge)
        g = _host_csr(ei, N) if host else graph_for(inputs[1], ei, N, N, n_features=self.out_channels)
        aggr = kops.softmax_aggregate(g, x_src, self.t, edge=edge, edge_order="input", message="gen", eps=self.eps,
                                      exact=self.exact)
        return self._mlp(aggr + x_dst, training)

    def compute_output_shape(self, input_shape):
        x_shape = input_shape[0] if isinstance(input_shape, (list, tuple)) else input_shape
        return (x_shape[0], self.out_channels)

    def get_config(self) -> dict[str, Any]:
        config = super().get_config()
        config.pop("aggregator", None)
        config.update({"in_channels": self.in_channels, "out_channels": self.out_channels, "aggr": self.aggr,
                       "t": self.initial_t, "learn_t": self.learn_t, "norm": self.norm, "num_layers": self.num_layers,
                       "expansion": self.expansion, "eps": self.eps, "bias": self.use_bias, "edge_dim": self.edge_dim})
        return config
