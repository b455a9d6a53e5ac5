"""keras_geometric_amd — MI355X-native message-passing aggregation engine.

Drop-in for keras-geometric's MessagePassing.propagate() hot path
(GCNConv, GINConv, SAGEConv, GATv2Conv) on hand-written gfx950 HIP kernels
behind the C-ABI in include/kgx.h, registered as torch.ops.kgx.*.
"""

from . import _native, graph, ops
from .graph import Block, CSRGraph, build_csr, clear_cache
from .layers import (
    AggregatorFactory,
    AttentionPooling,
    BatchGlobalPooling,
    DotProductDecoder,
    DynamicEdgeConv,
    EdgeConv,
    GATConv,
    GATv2Conv,
    GCNConv,
    GENConv,
    GINConv,
    GINEConv,
    GlobalPooling,
    MessagePassing,
    PNAConv,
    ResGatedGraphConv,
    RGCNConv,
    NNConv,
    ECConv,
    SAGEConv,
    Set2Set,
    TransformerConv,
    set_random_seed,
)
from .knn import knn, knn_csr, knn_graph, knn_supported
from .sampling import EdgeBatch, NegativeSampler, NeighborSampler, SampledBlocks, SampledSubgraph
from .utils import GraphData, add_self_loops, batch_graphs, compute_gcn_normalization

__version__ = "0.1.0"

__all__ = [
    "AggregatorFactory",
    "AttentionPooling",
    "BatchGlobalPooling",
    "Block",
    "CSRGraph",
    "DotProductDecoder",
    "DynamicEdgeConv",
    "EdgeBatch",
    "EdgeConv",
    "GATConv",
    "GATv2Conv",
    "GCNConv",
    "GENConv",
    "GINConv",
    "GINEConv",
    "GlobalPooling",
    "GraphData",
    "MessagePassing",
    "NegativeSampler",
    "NeighborSampler",
    "PNAConv",
    "RGCNConv",
    "NNConv",
    "ECConv",
    "ResGatedGraphConv",
    "SAGEConv",
    "SampledBlocks",
    "SampledSubgraph",
    "Set2Set",
    "TransformerConv",
    "add_self_loops",
    "batch_graphs",
    "build_csr",
    "clear_cache",
    "compute_gcn_normalization",
    "graph",
    "knn",
    "knn_csr",
    "knn_graph",
    "knn_supported",
    "ops",
    "set_random_seed",
]
