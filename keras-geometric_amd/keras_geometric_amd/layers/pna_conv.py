"""PNAConv: Principal Neighbourhood Aggregation (Corso et al., NeurIPS 2020).

There is no reference counterpart: keras-geometric has no PNA layer and no
multi-aggregator.  The layer exists because it is the standard user of several
statistics of one neighbourhood, which kgx_multi_aggr computes from ONE gather
of every neighbour row; each statistic is the corresponding reference
aggregator's arithmetic (aggregators.py:48-232).

    A   = concat_r AGG_r { x_j : j -> i }                       [N, R*F]
    z   = concat_s  s_s(d_i) * A                                [N, S*R*F]  (scaler-major)
    out = act(x W_root + z W_aggr + b)

with d_i = max(deg_i, 1) (deg_i the in-degree kept in the CSR) and the degree
scalers identity = 1, amplification = log(d_i + 1) / delta, attenuation =
delta / log(d_i + 1).  delta is the mean over destination rows of
log(deg_i + 1); when not given it is computed from the first graph the layer
sees, then frozen and returned by get_config().  z is never materialised:
z W_aggr = sum_s s_s * (A W_s).  PyG's towers and per-edge pre-MLP are not
implemented.
"""

from __future__ import annotations

from typing import Any

import torch

from .. import ops as kops
from ._edges import edge_index_tensor, graph_for
from .aggregators import MultiAggregator
from .base import get_activation, get_initializer, serialize_activation, serialize_initializer, to_device_tensor
from .message_passing import MessagePassing

_SCALERS = ["identity", "amplification", "attenuation"]


def _name_list(names, what: str) -> list[str]:
    names = [names] if isinstance(names, str) else list(names)
    if not names:
        raise ValueError(f"PNAConv needs at least one {what}")
    if len(set(names)) != len(names):
        raise ValueError(f"PNAConv: repeated {what} in {names}")
    return names


class PNAConv(MessagePassing):
    def __init__(
        self,
        output_dim: int,
        aggregators=("mean", "max", "min", "std"),
        scalers=("identity", "amplification", "attenuation"),
        delta: float | None = None,
        root_weight: bool = True,
        use_bias: bool = True,
        activation: str | None = None,
        kernel_initializer="glorot_uniform",
        bias_initializer="zeros",
        exact: bool | None = None,
        **kwargs: Any,
    ) -> None:
        aggregators = _name_list(aggregators, "aggregator")
        MultiAggregator(aggregators)  # the factory's ValueError for unknown names
        scalers = _name_list(scalers, "scaler")
        for s in scalers:
            if s not in _SCALERS:
                raise ValueError(f"Invalid scaler: {s}. Available scalers: {_SCALERS}")
        super().__init__(aggregator=aggregators, exact=exact, **kwargs)
        self.output_dim = int(output_dim)
        self.aggregators = aggregators
        self.scalers = scalers
        self.delta = None if delta is None else float(delta)
        self.root_weight = root_weight
        self.use_bias = use_bias
        self.activation = get_activation(activation)
        self.kernel_initializer = get_initializer(kernel_initializer)
        self.bias_initializer = get_initializer(bias_initializer)
        self.kernel_root = None
        self.kernel_aggr = None
        self.bias = None

    @staticmethod
    def average_log_degree(edge_index, num_nodes: int) -> float:
        """delta: the mean over the num_nodes destination rows of log(in-degree + 1)."""
        ei = torch.as_tensor(edge_index).detach().cpu().long()
        if ei.dim() == 2 and ei.shape[0] != 2 and ei.shape[1] == 2:
            ei = ei.t()
        if num_nodes <= 0:
            return 0.0
        dst = ei[1] if ei.numel() else ei.new_zeros(0)
        dst = torch.where(dst < 0, dst + num_nodes, dst)
        deg = torch.bincount(dst, minlength=num_nodes)
        return float(torch.log(deg.double() + 1.0).mean())

    def build(self, input_shape) -> None:
        if not isinstance(input_shape, (list, tuple)) or len(input_shape) < 2:
            raise ValueError(f"Expected input_shape to be [(N, F), (2, E)], got {input_shape}")
        node_shape = input_shape[0]
        if node_shape is None or len(node_shape) < 2:
            raise ValueError(f"Expected node shape (N, F), got {node_shape}")
        f_in = int(node_shape[-1])
        if f_in <= 0:
            raise ValueError(f"Input dimension must be positive, got {f_in}")
        if self.root_weight:
            self.kernel_root = self.add_weight((f_in, self.output_dim), self.kernel_initializer, name="kernel_root")
        width = len(self.scalers) * len(self.aggregators) * f_in
        self.kernel_aggr = self.add_weight((width, self.output_dim), self.kernel_initializer, name="kernel_aggr")
        if self.use_bias:
            self.bias = self.add_weight((self.output_dim,), self.bias_initializer, name="bias")
        self.built = True

    def compute_output_shape(self, input_shape) -> tuple:
        node_shape = input_shape[0] if isinstance(input_shape, (list, tuple)) and input_shape else None
        return (node_shape[0] if node_shape else None, self.output_dim)

    def _scaler(self, name: str, log_d: torch.Tensor):
        if name == "amplification":
            return log_d / self.delta
        if name == "attenuation":
            return self.delta / log_d
        return None  # identity

    def call(self, inputs, training=None, mask=None):
        if not isinstance(inputs, (list, tuple)) or len(inputs) < 2:
            raise ValueError("PNAConv expects inputs to be a list/tuple of [node_features, edge_index]")
        x = to_device_tensor(inputs[0], torch.float32)
        edge_index = inputs[1]
        n, f_in = x.shape[0], x.shape[1]
        if n == 0:
            return torch.zeros((0, self.output_dim), dtype=x.dtype, device=x.device)
        ei = edge_index_tensor(edge_index, x.device, allow_transpose=True)
        b = self.bias if self.use_bias else None
        if self.root_weight:
            out = kops.dense(x, self.kernel_root, b)
        else:
            out = torch.zeros((n, self.output_dim), dtype=x.dtype, device=x.device)
            if b is not None:
                out = out + b
        if ei.shape[1] > 0:
            g = graph_for(edge_index, ei, n, n, n_features=f_in)
            deg = g.deg.double()
            if self.delta is None:  # from the first graph seen, then frozen
                self.delta = float(torch.log(deg + 1.0).mean())
            log_d = torch.log(torch.clamp(deg, min=1.0) + 1.0).float().unsqueeze(1)
            A = kops.multi_aggregate(g, x.contiguous(), self.aggregators, exact=self.exact)
            k = len(self.aggregators) * f_in
            for i, name in enumerate(self.scalers):  # z W_aggr = sum_s s_s * (A W_s)
                part = kops.dense(A, self.kernel_aggr[i * k:(i + 1) * k])
                s = self._scaler(name, log_d)
                out = out + (part if s is None else s * part)
        return out if self.activation is None else self.activation(out)

    def get_config(self) -> dict[str, Any]:
        config = super().get_config()
        config.pop("aggregator", None)
        config.update(
            {
                "output_dim": self.output_dim,
                "aggregators": list(self.aggregators),
                "scalers": list(self.scalers),
                "delta": self.delta,
                "root_weight": self.root_weight,
                "use_bias": self.use_bias,
                "activation": serialize_activation(self.activation),
                "kernel_initializer": serialize_initializer(self.kernel_initializer),
                "bias_initializer": serialize_initializer(self.bias_initializer),
                "exact": self.exact,
            }
        )
        return config
