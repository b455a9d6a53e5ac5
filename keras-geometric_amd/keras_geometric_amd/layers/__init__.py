"""Drop-in layer API (mirror of src/keras_geometric/layers/__init__.py)."""

from .aggregators import (
    Aggregator,
    AggregatorFactory,
    MaxAggregator,
    MeanAggregator,
    MinAggregator,
    MultiAggregator,
    PoolingAggregator,
    SoftmaxAggregator,
    StdAggregator,
    SumAggregator,
)
from .attention_pooling import AttentionPooling, Set2Set
from .base import Dense, Layer, Sequential, set_random_seed
from .decoders import DotProductDecoder
from .gat_conv import GATConv
from .gatv2_conv import GATv2Conv
from .gcn_conv import GCNConv
from .gen_conv import GENConv
from .gin_conv import GINConv
from .gine_conv import GINEConv
from .message_passing import MessagePassing
from .pna_conv import PNAConv
from .pooling import BatchGlobalPooling, GlobalPooling
from .resgated_conv import ResGatedGraphConv
from .edge_conv import DynamicEdgeConv, EdgeConv
from .nn_conv import ECConv, NNConv
from .rgcn_conv import RGCNConv
from .sage_conv import SAGEConv
from .transformer_conv import TransformerConv

__all__ = [
    "Aggregator",
    "AggregatorFactory",
    "AttentionPooling",
    "BatchGlobalPooling",
    "Dense",
    "DotProductDecoder",
    "GATConv",
    "GATv2Conv",
    "GCNConv",
    "GENConv",
    "GINConv",
    "GINEConv",
    "GlobalPooling",
    "Layer",
    "MaxAggregator",
    "MeanAggregator",
    "MessagePassing",
    "MinAggregator",
    "MultiAggregator",
    "PNAConv",
    "RGCNConv",
    "NNConv",
    "EdgeConv",
    "DynamicEdgeConv",
    "ECConv",
    "PoolingAggregator",
    "ResGatedGraphConv",
    "SAGEConv",
    "Sequential",
    "Set2Set",
    "SoftmaxAggregator",
    "StdAggregator",
    "SumAggregator",
    "TransformerConv",
    "set_random_seed",
]
