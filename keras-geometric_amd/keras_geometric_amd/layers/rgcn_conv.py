"""RGCNConv: relational graph convolution (PyG's RGCNConv; keras-geometric has no such layer).

h'_i = b + x_i W_root + sum_r norm_{i,r} sum_{j ->_r i} x_j W_r,   norm = 1 / |N_r(i)| (mean) or 1 (sum)

kgx forward: ONE fused pass (kgx_rgcn_run) walks the relations of a tile of nodes, keeps the
per-relation aggregates in LDS and the output accumulators in registers, so the [N, R * F_in]
table of the composed form is never written.  With num_bases=B the weights are W = comp @ bases,
formed with torch before the op, so autograd carries the decomposition.  Block-diagonal
decomposition is not built; no self loops are added (the root weight plays that role).
"""

from __future__ import annotations

from typing import Any

import torch

from .. import graph as G
from .. import ops as kops
from ._edges import edge_index_tensor
from .base import Layer, to_device_tensor


class RGCNConv(Layer):
    def __init__(
        self,
        output_dim: int,
        num_relations: int,
        num_bases: int | None = None,
        aggregator: str = "mean",
        root_weight: bool = True,
        use_bias: bool = True,
        kernel_initializer: str = "glorot_uniform",
        bias_initializer: str = "zeros",
        **kwargs: Any,
    ) -> None:
        super().__init__(**kwargs)
        if aggregator not in ("mean", "sum"):
            raise ValueError(f"RGCNConv: aggregator must be 'mean' or 'sum', got {aggregator!r}")
        if int(num_relations) < 1 or (num_bases is not None and int(num_bases) < 1):
            raise ValueError("RGCNConv: num_relations and num_bases must be positive")
        self.output_dim = int(output_dim)
        self.num_relations = int(num_relations)
        self.num_bases = None if num_bases is None else int(num_bases)
        self.aggregator = aggregator
        self.root_weight = root_weight
        self.use_bias = use_bias
        self.kernel_initializer = kernel_initializer
        self.bias_initializer = bias_initializer
        self.kernel = self.bases = self.comp = self.root = self.bias = None

    def build(self, input_shape: Any) -> None:
        node_shape = input_shape[0] if isinstance(input_shape[0], (list, tuple)) else input_shape
        if node_shape is None or len(node_shape) < 2 or node_shape[1] is None:
            raise ValueError(f"Expected node features shape (N, F), got {node_shape}")
        F_in, F_out, R = int(node_shape[1]), self.output_dim, self.num_relations
        if self.num_bases is None:
            self.kernel = self.add_weight((R, F_in, F_out), self.kernel_initializer, name="kernel")
        else:
            self.bases = self.add_weight((self.num_bases, F_in, F_out), self.kernel_initializer, name="bases")
            self.comp = self.add_weight((R, self.num_bases), self.kernel_initializer, name="comp")
        if self.root_weight:
            self.root = self.add_weight((F_in, F_out), self.kernel_initializer, name="root")
        if self.use_bias:
            self.bias = self.add_weight((F_out,), self.bias_initializer, name="bias")
        self.built = True

    def call(self, inputs, edge_type=None, training=None):
        if not isinstance(inputs, (list, tuple)) or len(inputs) < 2:
            raise ValueError("Inputs must be a list or tuple containing [x, edge_index] or [x, edge_index, edge_type]")
        if len(inputs) > 2 and inputs[2] is not None:
            if edge_type is not None:
                raise ValueError("RGCNConv: edge_type given both as inputs[2] and as a keyword")
            edge_type = inputs[2]
        if edge_type is None:
            raise ValueError("RGCNConv needs edge_type (keyword or inputs[2])")
        x = to_device_tensor(inputs[0], torch.float32)
        N = x.shape[0]
        if N == 0:
            return torch.zeros((0, self.output_dim), dtype=x.dtype, device=x.device)
        ei = edge_index_tensor(inputs[1], x.device, allow_transpose=True)
        et_obj = edge_type
        et = to_device_tensor(edge_type, torch.int32, x.device).reshape(-1)
        if et.numel() != ei.shape[1]:
            raise ValueError(f"RGCNConv: edge_type must have one entry per edge ({ei.shape[1]}), got {et.numel()}")
        key = G.cache_key(inputs[1], ei.shape[1], N, self.num_relations, "rgcn")
        tkey = G.cache_key(et_obj) if key is not None else None
        rg = G.cached(None if tkey is None else (*key, *tkey), (inputs[1], et_obj),
                      lambda: G.build_relation_csr(ei[0].contiguous(), ei[1].contiguous(), et.contiguous(), N, N,
                                                   self.num_relations))
        W = self.kernel
        if self.num_bases is not None:  # W_r = sum_b comp[r, b] bases[b]
            W = (self.comp @ self.bases.reshape(self.num_bases, -1)).view(self.num_relations, *self.bases.shape[1:])
        return kops.rgcn_aggregate(rg, x, W, self.root, self.bias, aggr=self.aggregator)

    def compute_output_shape(self, input_shape):
        x_shape = input_shape[0] if isinstance(input_shape[0], (list, tuple)) else input_shape
        return (x_shape[0], self.output_dim)

    def get_config(self) -> dict[str, Any]:
        config = super().get_config()
        config.update(
            {
                "output_dim": self.output_dim,
                "num_relations": self.num_relations,
                "num_bases": self.num_bases,
                "aggregator": self.aggregator,
                "root_weight": self.root_weight,
                "use_bias": self.use_bias,
                "kernel_initializer": self.kernel_initializer,
                "bias_initializer": self.bias_initializer,
            }
        )
        return config
