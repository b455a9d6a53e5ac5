"""Attention readouts (mirror of src/keras_geometric/layers/pooling/attention_pooling.py).

AttentionPooling (attention_pooling.py:276-461) and Set2Set (:9-273) pool the
nodes of a graph with a softmax over per-node scores:

    out[g, :] = sum_{i in g} softmax_g(s)_i * x[i, :]

The reference runs ops.softmax(scores, axis=0) and ops.sum(weights * inputs,
axis=0) (:175-180, :409-412): x is read twice and an [N, F] product is
written.  Here the softmax and the weighted sum are one kgx_softmax_pool
launch that reads x once (ops.softmax_pool; csrc/softmax_pool.hip), and
Set2Set's score tanh(Dense(concat(x, h))) is split into x . k_x (computed in
that kernel from the row it has loaded) and the per-graph constant h . k_h + b,
so each of its processing_steps + 1 attention passes is one pass over x.

A tensor input pools one graph to [1, .], as the reference does.  A
[x, batch] list pools every graph of a batch to [num_graphs, .]: an extension
with BatchGlobalPooling's conventions (num_graphs = max(batch) + 1, unsorted
ids allowed, ids outside [0, num_graphs) dropped).

Dropout draws from torch's generator, so the random streams differ from
Keras's; the layers' structure (which tensor is dropped, what the pooled sum
reads) is the reference's.
"""

from __future__ import annotations

from typing import Any

import torch

from .. import graph as G
from .. import ops as kops
from .base import Dense, Dropout, Layer, to_device_tensor
from .pooling import segment_graph


def _is_batched(inputs) -> bool:
    """[x, batch]: a two-element list whose first element is itself 2-D."""
    if not isinstance(inputs, (list, tuple)) or len(inputs) != 2:
        return False
    first = inputs[0]
    return hasattr(first, "shape") and len(first.shape) == 2


def _feature_shape(input_shape):
    """The node-feature shape of build()'s argument (a shape, or [x shape, batch shape])."""
    if len(input_shape) == 2 and isinstance(input_shape[0], (list, tuple)):
        return tuple(input_shape[0])
    return tuple(input_shape)


def _check_2d(input_shape) -> None:
    if len(input_shape) != 2:
        raise ValueError(
            f"Expected input shape to be 2D (num_nodes, num_features), got {len(input_shape)}D"
        )


def _segments(inputs):
    """(x, segment graph, segment of every node or None) of a layer input."""
    if _is_batched(inputs):
        x = to_device_tensor(inputs[0], torch.float32)
        batch = to_device_tensor(inputs[1], torch.int32, x.device)
        num_graphs = int(batch.max()) + 1  # global_pooling.py:231's convention
        g = segment_graph(batch, num_graphs)
        return x, g, G.segment_of_node(g)
    x = to_device_tensor(inputs, torch.float32)
    if x.dim() != 2:
        _check_2d(tuple(x.shape))
    return x, G.single_segment_graph(int(x.shape[0]), x.device), None


class AttentionPooling(Layer):
    """Softmax-attention readout (attention_pooling.py:276-461): scores from
    Dense(1)(Dense(attention_dim, tanh)(dropout(x))), pooled sum over the raw x."""

    def __init__(self, attention_dim: int | None = None, dropout: float = 0.0, **kwargs: Any) -> None:
        super().__init__(**kwargs)
        if attention_dim is not None and attention_dim <= 0:
            raise ValueError(f"attention_dim must be positive, got {attention_dim}")
        if not 0.0 <= dropout <= 1.0:
            raise ValueError(f"dropout must be in [0, 1], got {dropout}")
        self.attention_dim = attention_dim
        self.dropout_rate = dropout
        self.attention_dense: Dense | None = None
        self.attention_score: Dense | None = None
        self.dropout_layer: Dropout | None = None

    def build(self, input_shape) -> None:
        shape = _feature_shape(input_shape)
        _check_2d(shape)
        input_dim = shape[1]
        if input_dim is None:
            raise ValueError("Input feature dimension cannot be None")
        attention_dim = self.attention_dim if self.attention_dim is not None else input_dim
        dev = getattr(self, "_build_device", None)
        self.attention_dense = Dense(attention_dim, activation="tanh", kernel_initializer="glorot_uniform",
                                     name="attention_transform")
        self.attention_score = Dense(1, kernel_initializer="glorot_uniform", name="attention_score")
        self.attention_dense._build_device = dev
        self.attention_dense.build((None, input_dim))
        self.attention_score._build_device = dev
        self.attention_score.build((None, attention_dim))
        if self.dropout_rate > 0.0:
            self.dropout_layer = Dropout(self.dropout_rate, name="dropout")
        self.built = True

    def call(self, inputs, training: bool | None = None, **kwargs):
        if self.attention_dense is None or self.attention_score is None:
            raise RuntimeError("Layer not built. Call build() first.")
        x, g, _ = _segments(inputs)
        h = x
        if self.dropout_layer is not None and training:
            h = self.dropout_layer(h, training=training)  # the score path only: the sum reads x (:398-412)
        scores = self.attention_score(self.attention_dense(h)).reshape(-1)
        return kops.softmax_pool(g, x, scores)

    def compute_output_shape(self, input_shape):
        if _is_shape_pair(input_shape):
            _check_2d(input_shape[0])
            return (None, input_shape[0][1])
        _check_2d(input_shape)
        return (1, input_shape[1])

    def get_config(self) -> dict[str, Any]:
        config = super().get_config()
        config.update({"attention_dim": self.attention_dim, "dropout": self.dropout_rate})
        return config

    @classmethod
    def from_config(cls, config: dict[str, Any]) -> "AttentionPooling":
        return cls(**config)


def _is_shape_pair(input_shape) -> bool:
    return (isinstance(input_shape, (list, tuple)) and len(input_shape) == 2
            and isinstance(input_shape[0], (list, tuple)))


def _orthogonal(shape, device):
    return torch.nn.init.orthogonal_(torch.empty(shape, device=device))


def _unit_forget_bias(shape, device):
    """Keras LSTMCell's bias: zeros with the forget gate's slice at one."""
    b = torch.zeros(shape, device=device)
    u = shape[0] // 4
    b[u: 2 * u] = 1.0
    return b


class LSTMCell(Layer):
    """keras.layers.LSTMCell on [num_graphs, .] rows, in torch (the readout's
    state is one row per graph: tiny).  Gates in Keras order i, f, c, o:
        z = x @ kernel + h @ recurrent_kernel + bias
        c' = sigmoid(z_f) * c + sigmoid(z_i) * tanh(z_c);  h' = sigmoid(z_o) * tanh(c')
    kernel [F, 4u] glorot-uniform, recurrent_kernel [u, 4u] orthogonal, bias
    zero with the forget slice at one.  In training, `dropout` masks the input
    and `recurrent_dropout` the previous h (inverted dropout, a fresh mask per
    call)."""

    def __init__(self, units: int, dropout: float = 0.0, recurrent_dropout: float = 0.0, **kwargs: Any) -> None:
        super().__init__(**kwargs)
        self.units = int(units)
        self.dropout = float(dropout)
        self.recurrent_dropout = float(recurrent_dropout)

    def build(self, input_shape) -> None:
        in_dim, u = int(input_shape[-1]), self.units
        self.add_weight((in_dim, 4 * u), "glorot_uniform", name="kernel")
        self.add_weight((u, 4 * u), _orthogonal, name="recurrent_kernel")
        self.add_weight((4 * u,), _unit_forget_bias, name="bias")
        self.built = True

    def call(self, inputs, states, training: bool | None = None):
        h, c = states
        if training and self.dropout > 0.0:
            inputs = torch.nn.functional.dropout(inputs, self.dropout, training=True)
        if training and self.recurrent_dropout > 0.0:
            h = torch.nn.functional.dropout(h, self.recurrent_dropout, training=True)
        z = inputs @ self.kernel + h @ self.recurrent_kernel + self.bias
        zi, zf, zc, zo = torch.split(z, self.units, dim=-1)
        c_new = torch.sigmoid(zf) * c + torch.sigmoid(zi) * torch.tanh(zc)
        h_new = torch.sigmoid(zo) * torch.tanh(c_new)
        return h_new, [h_new, c_new]


class Set2Set(Layer):
    """Set2Set readout (attention_pooling.py:9-273): processing_steps rounds of
    attention over the nodes driven by an LSTM state, then a final attention
    pass; the output is concat(h, pooled) = [., lstm_units + F] (:215)."""

    def __init__(self, output_dim: int, processing_steps: int = 3, lstm_units: int | None = None,
                 dropout: float = 0.0, **kwargs: Any) -> None:
        super().__init__(**kwargs)
        if output_dim <= 0:
            raise ValueError(f"output_dim must be positive, got {output_dim}")
        if processing_steps <= 0:
            raise ValueError(f"processing_steps must be positive, got {processing_steps}")
        if not 0.0 <= dropout <= 1.0:
            raise ValueError(f"dropout must be in [0, 1], got {dropout}")
        self.output_dim = output_dim
        self.processing_steps = processing_steps
        self.lstm_units = lstm_units if lstm_units is not None else output_dim
        self.dropout_rate = dropout
        self.lstm_cell: LSTMCell | None = None
        self.attention_dense: Dense | None = None
        self.dropout_layer: Dropout | None = None

    def build(self, input_shape) -> None:
        shape = _feature_shape(input_shape)
        _check_2d(shape)
        input_dim = shape[1]
        if input_dim is None:
            raise ValueError("Input feature dimension cannot be None")
        dev = getattr(self, "_build_device", None)
        # assignment order is the weight order: LSTM kernel, recurrent kernel, bias, attention kernel, bias
        self.lstm_cell = LSTMCell(self.lstm_units, dropout=self.dropout_rate, recurrent_dropout=self.dropout_rate,
                                  name="lstm_cell")
        self.lstm_cell._build_device = dev
        self.lstm_cell.build((None, input_dim))
        self.attention_dense = Dense(1, activation="tanh", kernel_initializer="glorot_uniform",
                                     name="attention_dense")
        self.attention_dense._build_device = dev
        self.attention_dense.build((None, input_dim + self.lstm_units))
        if self.dropout_rate > 0.0:
            self.dropout_layer = Dropout(self.dropout_rate, name="dropout")
        self.built = True

    def _attend(self, g, seg, x, h, training):
        """One attention pass: softmax over tanh(Dense(concat(x, h_g))) per graph, pooled sum of x."""
        F = x.shape[1]
        if self.dropout_layer is not None and training:
            # the dropped concatenation is the score input (:165-172): scores from torch, then pooled
            h_nodes = h.expand(x.shape[0], -1) if seg is None else h[seg.clamp_min(0).long()]
            att_in = self.dropout_layer(torch.cat([x, h_nodes], dim=-1), training=training)
            return kops.softmax_pool(g, x, self.attention_dense(att_in).reshape(-1))
        K = self.attention_dense.kernel  # [F + u, 1]: rows [0, F) meet x, rows [F, F + u) meet h
        score_c = h @ K[F:, 0] + self.attention_dense.bias[0]
        return kops.softmax_pool(g, x, score_u=K[:F, 0], score_c=score_c, tanh=True)

    def call(self, inputs, training: bool | None = None, **kwargs):
        if self.lstm_cell is None or self.attention_dense is None:
            raise RuntimeError("Layer not built. Call build() first.")
        x, g, seg = _segments(inputs)
        h = torch.zeros((g.n_dst, self.lstm_units), dtype=torch.float32, device=x.device)
        c = torch.zeros_like(h)
        for _step in range(self.processing_steps):
            pooled = self._attend(g, seg, x, h, training)
            _, (h, c) = self.lstm_cell(pooled, states=[h, c], training=training)
        return torch.cat([h, self._attend(g, seg, x, h, training)], dim=-1)

    def compute_output_shape(self, input_shape):
        batched = _is_shape_pair(input_shape)
        shape = input_shape[0] if batched else input_shape
        _check_2d(shape)
        input_dim = shape[1]
        if input_dim is None:
            raise ValueError("Input feature dimension cannot be None")
        return (None if batched else 1, self.lstm_units + input_dim)

    def get_config(self) -> dict[str, Any]:
        config = super().get_config()
        config.update({
            "output_dim": self.output_dim,
            "processing_steps": self.processing_steps,
            "lstm_units": self.lstm_units,
            "dropout": self.dropout_rate,
        })
        return config

    @classmethod
    def from_config(cls, config: dict[str, Any]) -> "Set2Set":
        return cls(**config)
