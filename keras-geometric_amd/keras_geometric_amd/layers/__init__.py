"""Drop-in layer API (mirror of src/keras_geometric/layers/__init__.py)."""

from .aggregators import (
    Aggregator,
    AggregatorFactory,
    MaxAggregator,
    MeanAggregator,
    MinAggregator,
    MultiAggregator,
    PoolingAggregator,
    StdAggregator,
    SumAggregator,
)
from .attention_pooling import AttentionPooling, Set2Set
from .base import Dense, Layer, Sequential, set_random_seed
from .decoders import DotProductDecoder
from .gatv2_conv import GATv2Conv
from .gcn_conv import GCNConv
from .gin_conv import GINConv
from .message_passing import MessagePassing
from .pna_conv import PNAConv
from .pooling import BatchGlobalPooling, GlobalPooling
from .sage_conv import SAGEConv
from .transformer_conv import TransformerConv

__all__ = [
    "Aggregator",
    "AggregatorFactory",
    "AttentionPooling",
    "BatchGlobalPooling",
    "Dense",
    "DotProductDecoder",
    "GATv2Conv",
    "GCNConv",
    "GINConv",
    "GlobalPooling",
    "Layer",
    "MaxAggregator",
    "MeanAggregator",
    "MessagePassing",
    "MinAggregator",
    "MultiAggregator",
    "PNAConv",
    "PoolingAggregator",
    "SAGEConv",
    "Sequential",
    "Set2Set",
    "StdAggregator",
    "SumAggregator",
    "TransformerConv",
    "set_random_seed",
]
