"""ABMIL - drop-in for the reference's ``baselines/ReMix_DSMIL_ABMIL/model/abmil.py:6-58`` over many bags at once.

``BClassifier`` / ``BClassifier_``: attention = Linear(L, L) -> ReLU -> Linear(L, 1), a softmax of that score over the bag's rows, the
weighted sum of the rows, a Linear classifier.  Same constructor signatures, parameter creation order and ``state_dict`` keys as the
reference, so its checkpoints load with ``strict=True``.  The projections run on the MFMA GEMM (``ops.linear``), softmax + weighted sum
on the bag pooling kernel (``ops.bag_softmax_pool``: C = 1, values = H, scale = 1).  ``GatedAttention`` (an MNIST conv net) is not mirrored.
"""
from __future__ import annotations

import torch
import torch.nn as nn

from .. import ops
from .bags import rows_and_plan


class BClassifier(nn.Module):
    def __init__(self, input_size, num_classes):
        super().__init__()
        self.L = input_size
        self.D = input_size
        self.K = 1
        self.attention = nn.Sequential(nn.Linear(self.L, self.D), nn.ReLU(), nn.Linear(self.D, self.K))
        self.classifier = nn.Sequential(nn.Linear(self.D, num_classes))

    def pooled(self, x, bags=None):
        """(Y [S, classes], H, scores [N, 1], the softmax statistics [S, 1, 2], plan)."""
        H, rp = rows_and_plan(x, bags)
        a = torch.relu(ops.linear(H, self.attention[0].weight, self.attention[0].bias))
        A = ops.linear(a, self.attention[2].weight, self.attention[2].bias)                 # [N, 1]
        M, _, stats = ops.bag_softmax_pool_lse(A, H, rp, 1.0)                                 # [S, 1, L]
        Y = ops.linear(M.reshape(rp.num_segs, self.L), self.classifier[0].weight, self.classifier[0].bias)
        return Y, H, A, stats, rp

    def forward(self, x, bags=None):
        """``x`` [N, L] alone: one bag, as the reference takes it.  With ``bags`` (``mil.bag_plan``) ``x`` holds many contiguous bags; a
        homogeneous graph batch is its ``ndata['feat']`` with the graphs as bags.  Returns [S, classes]; an empty bag gives the classifier's bias."""
        return self.pooled(x, bags)[0]


class BClassifier_(BClassifier):
    def forward(self, x, bags=None):
        return None, self.pooled(x, bags)[0], None, None
