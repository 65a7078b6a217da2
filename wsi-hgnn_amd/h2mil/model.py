"""The H2MIL model (``baselines/H2MIL/code/main_baselines_kfold.py:31-96``, the class the training script builds and calls ``GCN``) over the
packed batch, and one training step of its loop.

  x_y_index * 2 - 1;  norm -> conv1 -> relu -> norm -> dropout -> pool_1 -> readout x1 -> conv2 -> relu -> norm -> dropout -> pool_2 -> readout x2
  x1 + x2 -> lin1 -> relu -> norm -> dropout -> lin2 -> softmax

``norm`` is ONE torch_geometric graph-mode LayerNorm applied to inputs of width in_feats, out_classes and out_classes // 2: over ALL entries
of a slide's current node matrix, (x - mean) / (std(unbiased=False) + 1e-5) * weight + bias.  Its weight and bias have shape [1]:
torch_geometric 2.0.3 (the reference's pinned version) creates them as ``torch.Tensor([in_channels])`` - a one-element tensor - and a
per-channel weight of in_feats entries could not broadcast against the narrower inputs.  In the packed batch the statistics are per slide; for
the [1, out_classes // 2] row of a slide after ``lin1`` they are that row's own.
Excluded, not stubbed: the k-fold, staging and typing scripts around the model (the same model under another ``no_of_class``) and the
``WSI_processing`` pipeline that cuts the slides.
"""
from __future__ import annotations

import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import ops
from .IHPool import IHPool
from .RAConv import RAConv
from .batch import TreeBatch

MPOOL_METHODS = ("global_mean_pool", "global_max_pool", "global_att_pool")


class GraphLayerNorm(nn.Module):
    """torch_geometric's ``LayerNorm(in_channels)`` in graph mode with the [1] parameters of version 2.0.3 (see the module text).
    ``forward(x, slide, num_slides, rp)``: ``slide`` [rows] the slide of every row, ``rp`` the per-slide reduction plan (kernels) or None."""

    def __init__(self, in_channels, eps=1e-5):
        super().__init__()
        self.in_channels, self.eps = in_channels, eps
        self.weight = nn.Parameter(torch.ones(1))
        self.bias = nn.Parameter(torch.zeros(1))

    def forward(self, x, slide, num_slides, rp=None):
        C = x.shape[1]
        if rp is not None:
            ssum = lambda t: ops.segment_reduce(t, rp, "sum").sum(1, keepdim=True)
            cnt = rp.counts() * C
        else:
            ssum = lambda t: torch.zeros((num_slides, 1), dtype=t.dtype, device=t.device).index_add(0, slide, t.sum(1, keepdim=True))
            cnt = torch.zeros((num_slides, 1), dtype=x.dtype, device=x.device).index_add(0, slide, torch.full((x.shape[0], 1), float(C), dtype=x.dtype, device=x.device))
        mean = ssum(x) / cnt
        xc = x - mean[slide]
        std = torch.sqrt(ssum(xc * xc) / cnt)
        return xc / (std + self.eps)[slide] * self.weight + self.bias


class H2MIL(nn.Module):
    """The reference's constructor arguments and defaults (``pool3_ratio`` is accepted and unused, as there) and its ``state_dict`` keys.
    ``forward(batch)`` with ``batch`` a ``TreeBatch`` returns ``(probabilities [B, no_of_class], (cluster_1, cluster_2), (node_type_1,
    node_type_2), (score_1, score_2), (tree_1, tree_2), (x_y_index_1, x_y_index_2), (edge_index_1, edge_index_2))``; every entry of the six
    tuples is a list with one tensor per slide, rows numbered within the slide as the reference numbers them."""

    def __init__(self, in_feats, n_hidden, out_classes, no_of_class, drop_out_ratio=0.2, pool1_ratio=0.2, pool2_ratio=4, pool3_ratio=3,
                 mpool_method="global_mean_pool", kernels=True):
        super().__init__()
        if mpool_method not in MPOOL_METHODS:
            raise ValueError(f"H2MIL: mpool_method {mpool_method!r} is not one of {MPOOL_METHODS}")
        self.kernels = bool(kernels)
        self.mpool_method = mpool_method
        self.conv1 = RAConv(in_channels=in_feats, out_channels=out_classes, kernels=kernels)
        self.conv2 = RAConv(in_channels=out_classes, out_channels=out_classes, kernels=kernels)
        self.pool_1 = IHPool(in_channels=out_classes, ratio=pool1_ratio, select="inter", dis="ou", kernels=kernels)
        self.pool_2 = IHPool(in_channels=out_classes, ratio=pool2_ratio, select="inter", dis="ou", kernels=kernels)
        if mpool_method == "global_att_pool":
            self.mpool = nn.Module()
            self.mpool.gate_nn = nn.Sequential(nn.Linear(out_classes, out_classes // 2), nn.ReLU(), nn.Linear(out_classes // 2, 1))
        self.lin1 = nn.Linear(out_classes, out_classes // 2)
        self.lin2 = nn.Linear(out_classes // 2, no_of_class)
        self.relu = nn.ReLU()
        self.dropout = nn.Dropout(p=drop_out_ratio)
        self.softmax = nn.Softmax(dim=-1)
        self.norm = GraphLayerNorm(in_feats)

    def _linear(self, x, lin):
        return ops.linear(x, lin.weight, lin.bias) if self.kernels else F.linear(x, lin.weight, lin.bias)

    def _norm(self, x, tb: TreeBatch):
        return self.norm(x, tb.slide, tb.num_slides, tb.rp if self.kernels else None)

    def _readout(self, x, tb: TreeBatch):
        B = tb.num_slides
        if self.mpool_method == "global_att_pool":
            g = self.mpool.gate_nn
            gate = self._linear(torch.relu(self._linear(x, g[0])), g[2])
            if self.kernels:
                return ops.bag_softmax_pool(gate, x, tb.rp).reshape(B, -1)
            mx = torch.full((B, 1), -float("inf"), dtype=x.dtype, device=x.device).scatter_reduce(0, tb.slide[:, None], gate.detach(), "amax")
            e = torch.exp(gate - mx[tb.slide])
            a = e / torch.zeros((B, 1), dtype=x.dtype, device=x.device).index_add(0, tb.slide, e)[tb.slide]
            return torch.zeros((B, x.shape[1]), dtype=x.dtype, device=x.device).index_add(0, tb.slide, a * x)
        op = "mean" if self.mpool_method == "global_mean_pool" else "max"
        if self.kernels:
            return ops.segment_reduce(x, tb.rp, op)
        if op == "mean":
            cnt = torch.tensor(tb.sizes, dtype=x.dtype, device=x.device)[:, None]
            return torch.zeros((B, x.shape[1]), dtype=x.dtype, device=x.device).index_add(0, tb.slide, x) / cnt
        return torch.full((B, x.shape[1]), -float("inf"), dtype=x.dtype, device=x.device).scatter_reduce(
            0, tb.slide[:, None].expand_as(x), x, "amax")

    def forward(self, batch: TreeBatch):
        if not isinstance(batch, TreeBatch):
            raise TypeError(f"H2MIL: expected an h2mil.TreeBatch (h2mil.from_slides builds one), got {type(batch).__name__}")
        tb = TreeBatch.__new__(TreeBatch)
        tb.__dict__.update(batch.__dict__)
        tb.x_y_index = batch.x_y_index * 2 - 1
        x = self._norm(batch.x, tb)
        x = self.relu(self.conv1(x, tb, tb.node_type))
        x = self.dropout(self._norm(x, tb))
        x, tb1, cluster_1, score_1 = self.pool_1(x, tb)
        x1 = self._readout(x, tb1)
        x = self.relu(self.conv2(x, tb1, tb1.node_type))
        x = self.dropout(self._norm(x, tb1))
        x, tb2, cluster_2, score_2 = self.pool_2(x, tb1)
        x2 = self._readout(x, tb2)
        x = self.relu(self._linear(x1 + x2, self.lin1))
        rows = torch.arange(tb.num_slides, device=x.device)
        x = self.norm(x, rows, tb.num_slides, None)                  # one row per slide: the statistics are the row's own
        x = self.softmax(self._linear(self.dropout(x), self.lin2))
        return (x, (_rows(tb, tb1, cluster_1), _rows(tb1, tb2, cluster_2)),
                (tb1.per_slide(tb1.node_type), tb2.per_slide(tb2.node_type)), (tb.per_slide(score_1), tb1.per_slide(score_2)),
                (tb1.per_slide(tb1.tree, "tree"), tb2.per_slide(tb2.tree, "tree")), (tb1.per_slide(tb1.x_y_index), tb2.per_slide(tb2.x_y_index)),
                (tb1.edges_per_slide(), tb2.edges_per_slide()))


def _rows(old: TreeBatch, new: TreeBatch, cluster: torch.Tensor):
    """The cluster map cut per slide, new rows numbered within the slide."""
    return [cluster[old.starts[b]:old.starts[b + 1]] - new.starts[b] for b in range(old.num_slides)]


def loss_fn(probs: torch.Tensor, labels: torch.Tensor) -> torch.Tensor:
    """The reference applies ``CrossEntropyLoss`` to the PROBABILITIES of one slide at a time (main_baselines_kfold.py:242,364) and adds the
    slides of a step up: a second log-softmax over the softmax output, summed over the batch."""
    return F.cross_entropy(probs, labels, reduction="sum")


def train_one_step(model: H2MIL, batch: TreeBatch, labels: torch.Tensor, optimizer) -> torch.Tensor:
    """zero_grad, forward, loss, backward, step; returns the detached loss, on the device."""
    model.train()
    optimizer.zero_grad()
    loss = loss_fn(model(batch)[0], labels)
    loss.backward()
    optimizer.step()
    return loss.detach()
