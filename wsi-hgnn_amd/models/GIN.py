"""GIN - drop-in for the reference's ``models/GIN.py:11-177`` (DGL ``GINConv`` around an MLP + BatchNorm1d + ReLU, glob poolings).

``GINConv`` = ``ops.gin_aggregate`` (HIP ``wsi_gin_aggregate_*``: (1 + eps) x + sum | mean | max of the in-neighbours, eps read from its own
device storage, ``graph.message_scale`` honoured) followed by ``apply_func``.  With a sum or mean reducer and in_features > out_features the
first Linear of the MLP runs BEFORE the aggregation (both are linear; ``ops.set_gin_project_first``), as ``GraphConv`` does; max always
aggregates first.  BatchNorm1d is ``ops.masked_batch_norm`` over the graph's live rows - all of them, except on the padded batch of a
``data.BatchSlot``, whose filler rows are dead (the slot keeps the table and the count on the device, ``graph.derive_live_rows``) - and the
ReLU behind each of the three BatchNorms runs inside its passes (``relu=True``: the composite's bits); Linears are ``ops.linear``.  Classes,
constructor signatures, parameter creation order and state_dict keys are the reference's.

One deliberate deviation: ``GIN.py:160`` calls ``self.dropout``, which does not exist (``:123`` defines ``self.drop``), so the reference raises
AttributeError from the second GINConv layer on and runs only with ``num_layers == 2``.  ``self.drop`` is applied at that place, as ``:123``
evidently intends; for ``num_layers == 2`` nothing differs.
"""
from __future__ import annotations

import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import ops
from ..graph import message_scale_of
from .GCN import homo_plan
from .heat_net import make_pool


def _linear(lin: nn.Linear, x: torch.Tensor, with_bias: bool = True) -> torch.Tensor:
    b = lin.bias if with_bias else None
    return ops.linear(x, lin.weight, b) if x.is_cuda else F.linear(x, lin.weight, b)


def _readout(pool: nn.Module, g, h: torch.Tensor) -> torch.Tensor:
    """``pool(g, h)``; for a CPU tensor (the tensor formulation of the whole model: ``ops.gin_aggregate_reference`` and torch's own Linear) the
    same readout with tensor operations, empty graphs giving 0 as the kernels do."""
    if h.is_cuda:
        return pool(g, h)
    bnn = g.batch_num_nodes(g.ntypes[0]).to(h.device).long()
    B = int(bnn.numel())
    seg = torch.repeat_interleave(torch.arange(B, device=h.device), bnn, output_size=h.shape[0])
    zeros = torch.zeros((B, h.shape[1]), dtype=h.dtype, device=h.device)
    kind = type(pool).__name__
    if kind == "GlobalAttentionPooling":
        gate = F.linear(h, pool.gate_nn.weight, pool.gate_nn.bias)
        mx = torch.full((B, 1), float("-inf"), dtype=h.dtype, device=h.device).scatter_reduce(0, seg.view(-1, 1), gate, "amax")
        ex = torch.exp(gate - mx[seg])
        den = torch.zeros((B, 1), dtype=h.dtype, device=h.device).index_add(0, seg, ex)
        return zeros.index_add(0, seg, h * (ex / den[seg]))
    if kind == "MaxPooling":
        idx = seg.view(-1, 1).expand_as(h)
        out = torch.full_like(zeros, float("-inf")).scatter_reduce(0, idx, h, "amax")
        return torch.where((bnn > 0).view(-1, 1), out, zeros)
    out = zeros.index_add(0, seg, h)
    return out / bnn.clamp(min=1).to(h.dtype).view(-1, 1) if kind == "AvgPooling" else out


def live_rows(g, n: int, device):
    """(live [n], the number of live rows as one fp32 word) for ``ops.masked_batch_norm``, kept on the graph next to ``_homo_plan``: ones and
    n, unless the graph is a homogeneous ``data.BatchSlot``'s, which installs its own device tables here and rewrites them behind every fill."""
    c = g.__dict__.get("_gin_live") if g is not None else None
    if c is None or c[0].device != device or c[0].numel() != n:
        c = (torch.ones(n, dtype=torch.float32, device=device), torch.full((1,), float(n), dtype=torch.float32, device=device))
        if g is not None:
            g.__dict__["_gin_live"] = c
    return c


class BatchNorm1d(nn.BatchNorm1d):
    """``nn.BatchNorm1d`` (same parameters, buffers and defaults) whose forward is ``ops.masked_batch_norm`` over the rows ``live`` names
    (``live_rows``; None: every row).  ``relu=True``: followed by ReLU, inside the same passes on the GPU."""

    def forward(self, x, live=None, relu: bool = False):
        if self.training and x.shape[0] < 2:
            raise ValueError(f"Expected more than 1 value per channel when training, got input size {x.size()}")
        live = live if live is not None else live_rows(None, x.shape[0], x.device)
        return ops.masked_batch_norm(x, live[0], live[1], self.weight, self.bias, self.running_mean, self.running_var, self.training,
                                     self.momentum, self.eps, self.num_batches_tracked, relu=relu)


class ApplyNodeFunc(nn.Module):
    """Update the node feature hv with MLP, BN and ReLU (GIN.py:11-22)."""

    def __init__(self, mlp):
        super().__init__()
        self.mlp = mlp
        self.bn = BatchNorm1d(self.mlp.output_dim)

    def first_linear(self) -> nn.Linear:
        return self.mlp.linear if self.mlp.linear_or_not else self.mlp.linears[0]

    def forward(self, h, live=None, projected: bool = False):
        h = self.mlp(h, live, projected)
        return self.bn(h, live, relu=True)


class MLP(nn.Module):
    """MLP with linear output (GIN.py:25-73).  ``projected``: the input already went through the first Linear (bias included)."""

    def __init__(self, num_layers, input_dim, hidden_dim, output_dim):
        super().__init__()
        self.linear_or_not = True
        self.num_layers = num_layers
        self.output_dim = output_dim
        if num_layers < 1:
            raise ValueError("number of layers should be positive!")
        elif num_layers == 1:
            self.linear = nn.Linear(input_dim, output_dim)
        else:
            self.linear_or_not = False
            self.linears = torch.nn.ModuleList()
            self.batch_norms = torch.nn.ModuleList()
            self.linears.append(nn.Linear(input_dim, hidden_dim))
            for layer in range(num_layers - 2):
                self.linears.append(nn.Linear(hidden_dim, hidden_dim))
            self.linears.append(nn.Linear(hidden_dim, output_dim))
            for layer in range(num_layers - 1):
                self.batch_norms.append(BatchNorm1d(hidden_dim))

    def forward(self, x, live=None, projected: bool = False):
        if self.linear_or_not:
            return x if projected else _linear(self.linear, x)
        h = x
        for i in range(self.num_layers - 1):
            z = h if (projected and i == 0) else _linear(self.linears[i], h)
            h = self.batch_norms[i](z, live, relu=True)
        return _linear(self.linears[-1], h)


class GINConv(nn.Module):
    """dgl.nn.pytorch.conv.GINConv(apply_func, aggregator_type, init_eps=0, learn_eps=False): ``eps`` is a Parameter of shape [1] when
    learned and a buffer otherwise."""

    def __init__(self, apply_func=None, aggregator_type="sum", init_eps=0, learn_eps=False):
        super().__init__()
        self.apply_func = apply_func
        if aggregator_type not in ("sum", "max", "mean"):
            raise KeyError("Aggregator type {} not recognized.".format(aggregator_type))
        self._aggregator_type = aggregator_type
        if learn_eps:
            self.eps = nn.Parameter(torch.FloatTensor([init_eps]))
        else:
            self.register_buffer("eps", torch.FloatTensor([init_eps]))

    def project_first(self) -> bool:
        """sum and mean are linear, so the MLP's first Linear may run before them; worth it when it narrows the rows."""
        if not (ops.gin_project_first() and self._aggregator_type in ("sum", "mean") and isinstance(self.apply_func, ApplyNodeFunc)):
            return False
        first = self.apply_func.first_linear()
        return first.in_features > first.out_features

    def forward(self, g, x):
        hp = homo_plan(g)
        scale = message_scale_of(g)                      # graph.message_scale (GNNExplainer): None outside such a block
        if not isinstance(self.apply_func, ApplyNodeFunc):
            rst = ops.gin_aggregate(x, self.eps, hp, self._aggregator_type, edge_scale=scale)
            return self.apply_func(rst) if self.apply_func is not None else rst
        live = live_rows(g, x.shape[0], x.device)
        if self.project_first():
            first = self.apply_func.first_linear()
            rst = ops.gin_aggregate(_linear(first, x, with_bias=False), self.eps, hp, self._aggregator_type, bias=first.bias, edge_scale=scale)
            return self.apply_func(rst, live, projected=True)
        return self.apply_func(ops.gin_aggregate(x, self.eps, hp, self._aggregator_type, edge_scale=scale), live)


class GIN(nn.Module):
    """GIN model (GIN.py:76-177)."""

    def __init__(self, input_dim, hidden_dim, out_dim, num_layers, num_mlp_layers, final_dropout, graph_pooling_type="sum",
                 neighbor_pooling_type="mean", learn_eps=True):
        super().__init__()
        self.num_layers = num_layers
        self.n_layers = num_layers                      # what explainers / localization read (the reference's ExplainGraph: model.n_layers)
        self.learn_eps = learn_eps
        self.layers = torch.nn.ModuleList()
        self.graph_pooling_type = graph_pooling_type
        for layer in range(self.num_layers - 1):
            mlp = MLP(num_mlp_layers, input_dim if layer == 0 else hidden_dim, hidden_dim, hidden_dim)
            self.layers.append(GINConv(ApplyNodeFunc(mlp), neighbor_pooling_type, 0, self.learn_eps))
        self.drop = nn.Dropout(final_dropout)
        self.classify = nn.Linear(hidden_dim, out_dim)
        self.linears_prediction = nn.ModuleList()
        self.pools = nn.ModuleList()
        for layer in range(num_layers + 1):
            self.linears_prediction.append(nn.Linear(input_dim if layer == 0 else hidden_dim, out_dim))
            self.pools.append(make_pool(graph_pooling_type, layer, input_dim, hidden_dim))

    def dead_parameter_names(self):
        """``linears_prediction[num_layers - 1]`` and ``[num_layers]`` (and, for 'att', the gate of ``pools[num_layers - 1]``) are created
        (GIN.py:130-149) and never applied: the loop runs over ``num_layers - 1`` layers and the last readout uses ``pools[-1]`` and ``classify``."""
        dead = [f"linears_prediction.{self.num_layers - 1}.", f"linears_prediction.{self.num_layers}.", f"pools.{self.num_layers - 1}.gate_nn."]
        return [n for n, _ in self.named_parameters() if n.startswith(tuple(dead))]

    def _drop(self, h):
        """``self.drop`` between the layers (GIN.py:160, see the module docstring).  Under an active dropout seed base
        (``ops.dropout_seed_base``) the train-mode draw is counter-based, exactly as ``GCN._drop``."""
        base = ops.current_dropout_seed_base(h.device) if (self.training and self.drop.p > 0.0 and h.is_cuda) else None
        if base is None:
            return self.drop(h)
        return ops.counter_dropout(h, ops.CounterDropout(self.drop.p, ops.next_dropout_seed(), base))

    def forward(self, g, h=None):
        if h is None:
            h = g.ndata["feat"]                                                         # GIN.py:154-155
        if h.is_cuda:
            h = h.to(torch.float32)
        h_list = []
        for i, layer in enumerate(self.layers):                                         # :158-162
            if i != 0:
                h = self._drop(h)
            h_list.append(_linear(self.linears_prediction[i], _readout(self.pools[i], g, h)))
            h = layer(g, h)
        h_list.append(_linear(self.classify, _readout(self.pools[-1], g, h)))                  # :164
        return torch.stack(h_list).sum(0)                                               # :175
