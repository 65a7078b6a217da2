"""The multiple-instance-learning baselines of the reference (``baselines/ReMix_DSMIL_ABMIL``): ABMIL and DSMIL over many bags at once.

A slide's patch features are a bag of rows with no edges; a batch is the bags laid one after the other plus a bag plan
(``bag_plan``).  ``abmil`` / ``dsmil`` mirror ``model/abmil.py`` / ``model/dsmil.py``; ``bag_loss`` and ``train_one_step`` mirror the
objective and the loop body of ``train_tcga_k-fold.py``; ``remix`` is how the reference trains them (``reduce.py``, ``train_remix_k-fold.py``):
k-means bag reduction and prototype mixing on the device.  ``slots`` holds the reference's ``dropout_patches`` drawn on the device
(``dropout_patches``, ``patch_counts``), batches of bags in padded slots of fixed shape (``BagSlot``) and a captured training step replayed over
them (``CapturedBagStep``): the one-bag-per-step regime the reference trains in.  ``metrics`` is the reference's ``test()``: the epoch's sigmoid
scores, ROC-optimal thresholds (``multi_label_roc``) and result-table scores kept on the device (``BagEpochMetrics``), eager (``evaluate``) or as
one captured forward per slot (``CapturedBagEval``).  Not built: the k-fold scripts.
"""
from __future__ import annotations

from typing import Optional

import torch
import torch.nn.functional as F

from .. import ops
from . import abmil, dsmil
from .bags import bag_plan, rows_and_plan

__all__ = ["abmil", "dsmil", "remix", "bag_plan", "bag_targets", "bag_loss", "train_one_step", "patch_counts", "dropout_patches",
           "dropout_patches_tensor", "BagSlot", "CapturedBagStep", "slot_step", "BagEpochMetrics", "CapturedBagEval", "evaluate"]


def bag_targets(labels, num_classes: int, device=None) -> torch.Tensor:
    """[S, num_classes] fp32 targets of ``train_tcga_k-fold.py:28-35``: the one-hot row of the label, the all-zero row for a label past
    the last class; with ``num_classes == 1`` the label itself is the value."""
    labels = torch.as_tensor(labels, device=device).reshape(-1)
    if num_classes == 1:
        return labels.to(torch.float32).view(-1, 1)
    return (labels.to(torch.int64).view(-1, 1) == torch.arange(num_classes, device=labels.device).view(1, -1)).to(torch.float32)


def bag_loss(outputs, labels, num_classes: int, model: str, bags: Optional[ops.ReducePlan] = None, weights: Optional[torch.Tensor] = None,
             targets: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The objective of ``train_tcga_k-fold.py:76-82`` (BCEWithLogitsLoss) averaged over the non-empty bags, so one bag gives the reference's
    loss.  ``model`` = 'abmil': the loss of the bag prediction; 'dsmil': 0.5 x that + 0.5 x the loss of the per-bag column maximum of the
    instance scores.  ``outputs``: what the model returned ([S, C], or the reference's 4-tuple); ``bags``: the batch's plan (None: one bag).
    ``weights`` [S, 1] and ``targets`` [S, C] (both or neither; device tensors, as a ``BagSlot`` keeps them): the sum of the per-bag losses
    weighted by ``weights`` against ``targets`` - no host count and no host label enters, ``labels`` is not read."""
    if model not in ("abmil", "dsmil"):
        raise ValueError("bag_loss: model is 'abmil' or 'dsmil'")
    ins, bag = (outputs[0], outputs[1]) if isinstance(outputs, (tuple, list)) else (None, outputs)
    bag = bag.reshape(-1, num_classes)
    if (weights is None) != (targets is None):
        raise ValueError("bag_loss: weights and targets come together")
    target = bag_targets(labels, num_classes, bag.device).to(bag.dtype) if targets is None else targets.to(bag.dtype)
    if target.shape != bag.shape:
        raise ValueError(f"bag_loss: {bag.shape[0]} bags but {target.shape[0]} labels")
    per_bag = F.binary_cross_entropy_with_logits(bag, target, reduction="none").mean(1)
    if model == "dsmil":
        if ins is None:
            raise ValueError("bag_loss: 'dsmil' needs the instance scores (the model's 4-tuple)")
        if bags is None:
            bags = bag_plan([ins.shape[0]], ins.device)
        mx = ops.segment_reduce(ins, bags, "max")                                            # [S, C]
        per_bag = 0.5 * per_bag + 0.5 * F.binary_cross_entropy_with_logits(mx, target, reduction="none").mean(1)
    if weights is not None:
        return (per_bag * weights.view(-1)).sum()
    if bags is None:
        return per_bag.mean()
    live = sum(1 for a, b in bags.ranges if b > a)
    return (per_bag * bags.nonempty().view(-1)).sum() / max(live, 1)


def train_one_step(milnet, optimizer, x, bags, labels) -> torch.Tensor:
    """The body of the reference's ``train`` loop (``train_tcga_k-fold.py:60-84``) for a batch of bags: zero_grad, forward, objective,
    backward, step.  Returns the detached loss (on the device: no read-back here)."""
    milnet.train()
    optimizer.zero_grad()
    x, bags = rows_and_plan(x, bags)
    outputs = milnet(x, bags)
    is_ds = isinstance(milnet, dsmil.MILNet)
    num_classes = (outputs[1] if isinstance(outputs, (tuple, list)) else outputs).shape[-1]
    loss = bag_loss(outputs, labels, num_classes, "dsmil" if is_ds else "abmil", bags)
    loss.backward()
    optimizer.step()
    return loss.detach()


from . import remix  # noqa: E402  (its train_one_step calls the one above)
from .slots import BagSlot, CapturedBagStep, dropout_patches, dropout_patches_tensor, patch_counts, slot_step  # noqa: E402
from .metrics import BagEpochMetrics, CapturedBagEval, evaluate  # noqa: E402
