"""NNConv / ECConv: the edge-conditioned convolution of Gilmer et al.'s MPNN (PyG's NNConv;
keras-geometric has no such layer).

h'_i = b + x_i W_root + aggr_{j->i} x_j Theta(e_ij),   Theta(e) = reshape(h_Theta(e), [F_in, F_out])

The edge network h_Theta is `edge_hidden` Dense + ReLU layers (kgx_dense) followed by a linear layer.
That last layer is this layer's `kernel` [D, F_in, F_out] and `kernel_bias` [F_in, F_out], D the last
hidden width (the raw edge_dim with edge_hidden=None), so Theta(e) = kernel_bias + sum_d c_e[d] kernel[d]
for the last hidden activation c_e, and the neighbour sum commutes with the weights:

h'_i = b + x_i W_root + norm_i (sum_d (sum_j c_e[d] x_j) kernel[d] + (sum_j x_j) kernel_bias)

kgx forward: ONE fused pass (kgx_nnconv_run) forms the D + 1 coefficient-weighted neighbour sums of a
tile of nodes in registers and multiplies them with their weights on MFMA; no [E, F_in * F_out] weight
tensor, no [E, F_out] message and no [N, (D + 1) F_in] table is written.  D > 32 or widths the kernel
does not implement take the composed form (a weighted kgx_spmm sum and a kgx_dense product per plane).

Equal to PyG's NNConv(F_in, F_out, nn=Sequential(Linear, ReLU, ..., Linear(D, F_in * F_out)), aggr,
root_weight, bias) with the last Linear's weight transposed and reshaped: kernel = weight.t().view(D,
F_in, F_out), kernel_bias = bias.view(F_in, F_out).  aggregator "sum" / "mean" are PyG's "add" / "mean";
"max" is not a linear reduction and is not offered.  No self loops are added.
"""

from __future__ import annotations

from typing import Any

import torch

from .. import ops as kops
from ._edges import edge_index_tensor, graph_for
from .base import Dense, Layer, to_device_tensor


class NNConv(Layer):
    def __init__(
        self,
        output_dim: int,
        edge_hidden: int | list[int] | tuple[int, ...] | None = None,
        aggregator: str = "sum",
        root_weight: bool = True,
        use_bias: bool = True,
        kernel_initializer: str = "glorot_uniform",
        bias_initializer: str = "zeros",
        **kwargs: Any,
    ) -> None:
        super().__init__(**kwargs)
        if aggregator not in ("sum", "mean"):
            raise ValueError(f"NNConv: aggregator must be 'sum' or 'mean', got {aggregator!r}")
        if edge_hidden is None:
            hidden = []
        elif isinstance(edge_hidden, int):
            hidden = [edge_hidden]
        else:
            hidden = [int(h) for h in edge_hidden]
        if any(h < 1 for h in hidden):
            raise ValueError(f"NNConv: edge_hidden widths must be positive, got {edge_hidden!r}")
        self.output_dim = int(output_dim)
        self.edge_hidden = hidden
        self.aggregator = aggregator
        self.root_weight = root_weight
        self.use_bias = use_bias
        self.kernel_initializer = kernel_initializer
        self.bias_initializer = bias_initializer
        self.edge_net = torch.nn.ModuleList()
        self.kernel = self.kernel_bias = self.root = self.bias = None
        self._F_in: int | None = None

    def build(self, input_shape: Any) -> None:
        node_shape = input_shape[0] if isinstance(input_shape[0], (list, tuple)) else input_shape
        if node_shape is None or len(node_shape) < 2 or node_shape[1] is None:
            raise ValueError(f"Expected node features shape (N, F), got {node_shape}")
        self._F_in = F_in = int(node_shape[1])
        if self.root_weight:
            self.root = self.add_weight((F_in, self.output_dim), self.kernel_initializer, name="root")
        if self.use_bias:
            self.bias = self.add_weight((self.output_dim,), self.bias_initializer, name="bias")
        self.built = True

    def _build_edge_net(self, edge_dim: int) -> None:
        """The edge network's weights, once the width of edge_attr is known."""
        width = edge_dim
        for i, h in enumerate(self.edge_hidden):
            layer = Dense(h, activation="relu", kernel_initializer=self.kernel_initializer,
                          bias_initializer=self.bias_initializer, name=f"edge_hidden_{i}")
            layer._build_device = getattr(self, "_build_device", None)
            layer.build((None, width))
            self.edge_net.append(layer)
            width = h
        self.kernel = self.add_weight((width, self._F_in, self.output_dim), self.kernel_initializer, name="kernel")
        self.kernel_bias = self.add_weight((self._F_in, self.output_dim), self.bias_initializer, name="kernel_bias")

    def call(self, inputs, edge_attr=None, training=None):
        if not isinstance(inputs, (list, tuple)) or len(inputs) < 2:
            raise ValueError("Inputs must be a list or tuple containing [x, edge_index] or [x, edge_index, edge_attr]")
        if len(inputs) > 2 and inputs[2] is not None:
            if edge_attr is not None:
                raise ValueError("NNConv: edge_attr given both as inputs[2] and as a keyword")
            edge_attr = inputs[2]
        if edge_attr is None:
            raise ValueError("NNConv needs edge_attr (keyword or inputs[2])")
        x = to_device_tensor(inputs[0], torch.float32)
        N, F = x.shape
        ei = edge_index_tensor(inputs[1], x.device, allow_transpose=True)
        ea = to_device_tensor(edge_attr, torch.float32, x.device)
        if ea.dim() == 1:
            ea = ea.unsqueeze(1)
        if ea.dim() != 2 or ea.shape[0] != ei.shape[1] or ea.shape[1] < 1:
            raise ValueError(f"NNConv: edge_attr must be [{ei.shape[1]}, edge_dim] (one row per edge), got "
                             f"{tuple(ea.shape)}")
        if self.kernel is None:
            self._build_edge_net(int(ea.shape[1]))
        first = self.edge_net[0].kernel if len(self.edge_net) else self.kernel
        if ea.shape[1] != first.shape[0]:
            raise ValueError(f"NNConv: edge_attr has {ea.shape[1]} columns, the layer was built for {first.shape[0]}")
        if N == 0:
            return torch.zeros((0, self.output_dim), dtype=x.dtype, device=x.device)
        if ei.shape[1] == 0:  # no message: b + x W_root
            out = kops.dense(x, self.root, self.bias) if self.root is not None else x.new_zeros((N, self.output_dim))
            return out + self.bias if self.root is None and self.bias is not None else out
        coef = ea
        for layer in self.edge_net:
            coef = layer(coef)
        g = graph_for(inputs[1], ei, N, N, n_features=F)  # cached on edge_index; the pieces are cached on g
        return kops.nnconv_aggregate(g, x, coef, self.kernel, self.kernel_bias, self.root, self.bias,
                                     aggr=self.aggregator)

    def compute_output_shape(self, input_shape):
        x_shape = input_shape[0] if isinstance(input_shape[0], (list, tuple)) else input_shape
        return (x_shape[0], self.output_dim)

    def get_config(self) -> dict[str, Any]:
        config = super().get_config()
        config.update(
            {
                "output_dim": self.output_dim,
                "edge_hidden": list(self.edge_hidden) if self.edge_hidden else None,
                "aggregator": self.aggregator,
                "root_weight": self.root_weight,
                "use_bias": self.use_bias,
                "kernel_initializer": self.kernel_initializer,
                "bias_initializer": self.bias_initializer,
            }
        )
        return config


ECConv = NNConv
