"""DSMIL - drop-in for the reference's ``baselines/ReMix_DSMIL_ABMIL/model/dsmil.py:6-69`` over many bags at once.

``FCLayer``, ``IClassifier``, ``BClassifier``, ``MILNet`` with the reference's constructor signatures, parameter creation order and
``state_dict`` keys (its checkpoints load with ``strict=True``).  Per bag: the critical instance of a class is the FIRST row with the
largest instance score; its query ``q_max`` scores every row of the bag (<Q[r], q_max[c]> / sqrt(128)), a softmax of those scores over
the bag's rows weighs the value rows into B [C, K], and ``fcc`` (a Conv1d whose kernel spans all of K) reads the class scores off B.

Projections: ``ops.linear`` (MFMA GEMM).  Critical instance: the argmax of ``wsi_segment_reduce_fwd`` (op max).  ``q(m_feats)`` equals
``Q[m_idx]`` in value and gradient, so it is taken from Q - as a dense one-hot weighted sum (``ops.bag_scores``), whose backward adds
nothing with atomics: a step stays bit-reproducible when one row is critical for two classes.  Softmax + weighted sum:
``ops.bag_softmax_pool``.  No loop over bags and no host read-back in forward or backward.
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn as nn

from .. import _native as N
from .. import ops
from .bags import rows_and_plan

# the reference divides by torch.sqrt(torch.tensor(128, dtype=torch.float32)) (model/dsmil.py:51): the float32-rounded root
_Q_WIDTH = 128


def score_scale(width: int = _Q_WIDTH) -> float:
    return 1.0 / float(np.sqrt(np.float32(width)))


class FCLayer(nn.Module):
    def __init__(self, in_size, out_size=1):
        super().__init__()
        self.fc = nn.Sequential(nn.Linear(in_size, out_size))

    def forward(self, feats):
        return feats, ops.linear(feats, self.fc[0].weight, self.fc[0].bias)


class IClassifier(nn.Module):
    def __init__(self, feature_extractor, feature_size, output_class):
        super().__init__()
        self.feature_extractor = feature_extractor
        self.fc = nn.Linear(feature_size, output_class)

    def forward(self, x):
        feats = self.feature_extractor(x)
        feats = feats.reshape(feats.shape[0], -1)
        return feats, ops.linear(feats, self.fc.weight, self.fc.bias)


def critical_onehot(c: torch.Tensor, rp: ops.ReducePlan) -> torch.Tensor:
    """[N, C] fp32: 1 where row r is the critical instance of (its bag, class) - the first maximum of the instance scores ``c`` [N, C].
    An empty bag, or a column of -inf / NaN alone, has no critical instance (the reduction reports row -1): no row matches it."""
    _, m_idx = ops._segment_reduce_raw(c.detach().contiguous(), rp, N.WSI_RED_MAX)        # [S, C] int32 global row, -1: none
    rows = torch.arange(c.shape[0], dtype=torch.int32, device=c.device).view(-1, 1)
    return (m_idx.index_select(0, rp.row_segment()) == rows).to(torch.float32)


class BClassifier(nn.Module):
    def __init__(self, input_size, output_class, dropout_v=0.0):
        super().__init__()
        self.q = nn.Linear(input_size, _Q_WIDTH)
        self.v = nn.Sequential(nn.Dropout(dropout_v), nn.Linear(input_size, input_size))
        self.fcc = nn.Conv1d(output_class, output_class, kernel_size=input_size)

    def forward(self, feats, c, bags=None):
        """feats [N, K], c [N, C] -> (C [S, C], A [N, C], B [S, C, K])."""
        feats, rp = rows_and_plan(feats, bags)
        V = ops.linear(self.v[0](feats), self.v[1].weight, self.v[1].bias)                   # [N, K]
        Q = ops.linear(feats, self.q.weight, self.q.bias)                                    # [N, 128]
        scale = score_scale(Q.shape[1])
        scores = ops.bag_scores(Q, critical_onehot(c, rp), rp)                               # [N, C]
        B, _, stats = ops.bag_softmax_pool_lse(scores, V, rp, scale)                         # [S, C, K]
        A = ops.bag_attention(scores, stats, rp, scale)
        n_cls, K = self.fcc.weight.shape[0], self.fcc.weight.shape[2]
        Cb = ops.linear(B.reshape(rp.num_segs, n_cls * K), self.fcc.weight.reshape(n_cls, n_cls * K), self.fcc.bias)
        return Cb, A, B


class MILNet(nn.Module):
    def __init__(self, i_classifier, b_classifier):
        super().__init__()
        self.i_classifier = i_classifier
        self.b_classifier = b_classifier

    def forward(self, x, bags=None):
        """``x`` [N, L] alone: one bag, as the reference takes it.  With ``bags`` (``mil.bag_plan``) ``x`` holds many contiguous bags; a
        homogeneous graph batch is its ``ndata['feat']`` with the graphs as bags.  Returns (classes [N, C], prediction_bag [S, C],
        A [N, C], B [S, C, K]); an empty bag's prediction is ``fcc``'s bias."""
        x, rp = rows_and_plan(x, bags)
        feats, classes = self.i_classifier(x)
        prediction_bag, A, B = self.b_classifier(feats, classes, rp)
        return classes, prediction_bag, A, B
