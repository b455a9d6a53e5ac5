"""Edge decoders for link prediction (no reference counterpart)."""

from __future__ import annotations

import torch

from .. import ops as kops
from ..sampling import EdgeBatch
from ._edges import edge_index_tensor, graph_for
from .base import Layer


class DotProductDecoder(Layer):
    """Inner-product edge scores on the fused kgx_edge_dot kernel.

        scores = decoder([z, batch])        # EdgeBatch -> [P, 1 + Q], column 0 the positive
        scores = decoder([z, edge_index])   # [2, E] (src, dst) -> [E]

    z is one table of node embeddings or a pair (z_dst, z_src); the score of
    the edge (s -> d) is z_dst[d] . z_src[s].  The scores are logits
    (sigmoid=True applies the logistic function), differentiable in z through
    deterministic kernels only.  The forward on an EdgeBatch does not
    synchronise: an index outside z gives a NaN score (EdgeBatch.fallbacks()
    reports edge ids the sampler did not know); an edge_index is checked.  The
    first backward of a batch does synchronise: it builds the batch's pair
    graph and its transpose (ops.edge_dot), each with a host read-back, and
    keeps them in batch.extras; a pair with an index outside z is left out of
    that graph and passes no gradient.  The layer has no weights."""

    def __init__(self, sigmoid: bool = False, **kwargs):
        super().__init__(**kwargs)
        self.sigmoid = bool(sigmoid)

    def forward(self, inputs, *args, **kwargs):
        self.built = True  # nothing to build: no weights
        return self.call(inputs, *args, **kwargs)

    def call(self, inputs, training=None):
        if not isinstance(inputs, (list, tuple)) or len(inputs) != 2:
            raise ValueError("DotProductDecoder expects [z, batch] or [z, edge_index]")
        z, edges = inputs
        z_dst, z_src = z if isinstance(z, (list, tuple)) else (z, z)
        if isinstance(edges, EdgeBatch):
            s = kops.edge_dot(z_dst, z_src, edges.a_idx, edges.b_idx, check=False, cache=edges.extras)
        else:
            ei = edge_index_tensor(edges, z_dst.device, allow_transpose=True)
            g = graph_for(edges, ei, z_src.shape[0], z_dst.shape[0])
            s = kops.edge_dot_graph(g, z_dst, z_src)
        return torch.sigmoid(s) if self.sigmoid else s

    def get_config(self):
        config = super().get_config()
        config.update({"sigmoid": self.sigmoid})
        return config
