"""``Classifier`` of the GTNMIL baseline (``baselines/GTNMIL/models/GraphTransformer.py:18-103``) over the packed batch: one GCNBlock, a linear
cluster assignment, mincut pooling to ``node_cluster_num`` tokens, a class token in front and the transformer; the objective is the cross
entropy plus the two pooling regularisers.  The reference's ``graphcam_flag`` branch is ``gtn.graphcam.class_maps`` (with
``save_reference_files`` for the files it writes); ``is_print`` is not mirrored."""
from __future__ import annotations

import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import ops
from .ViT import VisionTransformer
from .batch import as_batch
from .gcn import GCNBlock, dense_mincut_pool


class Classifier(nn.Module):
    """The defaults behind ``n_class`` are the values the reference hard-codes.  ``kernels=False`` runs the same model through tensor
    operations (what the tests and the benchmark compare the kernels against)."""

    def __init__(self, n_class, in_feats=1024, embed_dim=64, node_cluster_num=100, depth=3, num_heads=8, kernels=True, fused_attention=None):
        super().__init__()
        self.embed_dim = embed_dim
        self.num_layers = 3
        self.node_cluster_num = node_cluster_num
        self.kernels = bool(kernels)
        self.transformer = VisionTransformer(num_classes=n_class, embed_dim=embed_dim, depth=depth, num_heads=num_heads, kernels=kernels,
                                             fused_attention=fused_attention)
        self.cls_token = nn.Parameter(torch.zeros(1, 1, embed_dim))
        self.bn = 1
        self.add_self = 1
        self.normalize_embedding = 1
        self.conv1 = GCNBlock(in_feats, embed_dim, self.bn, self.add_self, self.normalize_embedding, 0., 0, kernels=kernels)
        self.pool1 = nn.Linear(embed_dim, node_cluster_num)

    def logits(self, batch):
        """(class logits [G, n_class], mincut loss, orthogonality loss)."""
        b = as_batch(batch)
        X = self.conv1(b.x, b)
        s = ops.linear(X, self.pool1.weight, self.pool1.bias) if self.kernels else F.linear(X, self.pool1.weight, self.pool1.bias)
        X, _, mc1, o1 = dense_mincut_pool(X, s, b, kernels=self.kernels)
        X = torch.cat([self.cls_token.repeat(X.shape[0], 1, 1), X], dim=1)
        return self.transformer(X), mc1, o1

    def forward(self, batch, labels):
        """``batch``: a homogeneous ``HeteroGraph`` batch (features in ``ndata['feat']``) or a ``gtn.GraphBatch`` (``gtn.from_dense`` makes one
        from the reference's ``node_feat, adjs, masks``), or a ``gtn.GraphSlot`` - then ``labels=None`` takes the slot's (-100 in unused
        cells, which the cross entropy ignores) and every output has one row per cell.  Returns the reference's (pred, labels, loss,
        softmax(out))."""
        if labels is None:
            labels = as_batch(batch).labels
        out, mc1, o1 = self.logits(batch)
        loss = (ops.cross_entropy(out, labels) if self.kernels else F.cross_entropy(out, labels)) + mc1 + o1
        pred = out.detach().max(1)[1]
        return pred, labels, loss, torch.softmax(out, -1)


def train_one_step(model, batch, labels, optimizer) -> torch.Tensor:
    """zero_grad, forward, backward, step (the loop body of the reference's ``helper.Trainer.train`` / ``main_kfold.py``); returns the detached
    loss, on the device."""
    model.train()
    optimizer.zero_grad()
    loss = model(batch, labels)[2]
    loss.backward()
    optimizer.step()
    return loss.detach()
