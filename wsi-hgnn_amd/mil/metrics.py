"""Evaluation of the MIL baselines with the epoch's metrics kept on the device: the reference's ``test()``
(``train_tcga_k-fold.py:98-180``, ``train_remix_k-fold.py:160-232``) without a read-back per bag.

``BagEpochMetrics.update(outputs, targets, weights)`` is ONE launch (``wsi_bag_metrics_update``, csrc/bag_metrics.hip) that allocates nothing and
never synchronises, so it can be the last node of a captured forward (``CapturedBagEval``); ``compute`` runs ``wsi_bag_metrics_finalize`` - per
class the ROC-optimal threshold of ``multi_label_roc`` / ``optimal_thresh`` over the whole epoch's scores, the hard predictions under it, their
counts - and makes the ONE device-to-host copy of the epoch; every score of the two reference scripts is derived on the host, in fp64, from that
block of integers.  The rule of the threshold is stated in ``include/wsi_hgnn.h``.

On a CPU device the same class runs a tensor formulation of both steps (as ``metrics.EpochMetrics`` does): the fixture the kernels are held to.
``evaluate`` is the reference's ``test()`` done eagerly over batches of bags.
"""
from __future__ import annotations

import math
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from .. import _native as N
from .. import capture, ops
from .bags import bag_plan
from .slots import check_bag_slots

HEAD = N.WSI_BAG_METRICS_RESULT_HEAD
MAX_ROWS, MAX_CLASSES = N.WSI_BAG_METRICS_MAX_ROWS, N.WSI_BAG_METRICS_MAX_CLASSES
_FLAG_NAMES = ((N.WSI_BAG_METRICS_BAD_TARGET, "a target other than 0 or 1 in a counted row"),
               (N.WSI_BAG_METRICS_NONFINITE, "a non-finite logit in a counted row"),
               (N.WSI_BAG_METRICS_OVERFLOW, "more counted rows than the capacity (the rows past it were dropped)"),
               (N.WSI_BAG_METRICS_ONE_LABEL, "a class without a positive or without a negative row (its ROC curve is not defined)"))
_PAIR_ROWS = 512          # rows of positives per block of the host formulation's pair counting


def _f64_bits(x: float) -> int:
    return int(np.array([x], dtype=np.float64).view(np.int64)[0])


def _bits_f64(w: int) -> float:
    return float(np.array([w], dtype=np.int64).view(np.float64)[0])


def split_outputs(outputs):
    """(bag prediction [S, C], instance scores [N, C] or None) of what a MIL model returned: [S, C] (``abmil.BClassifier``) or the
    reference's 4-tuple, whose first entry is None for ``abmil.BClassifier_``."""
    if isinstance(outputs, (tuple, list)):
        return outputs[1], outputs[0]
    return outputs, None


def roc_optimum(scores: np.ndarray, positive: np.ndarray):
    """(threshold, tp, fp, P, N) of one class: the rule of ``wsi_bag_metrics_finalize`` (a) with numpy - the host formulation.  ``scores`` fp32
    [n] in [0, 1], ``positive`` bool [n]; both labels must occur."""
    bits = scores.view(np.int32).astype(np.int64)
    order = np.argsort(-bits, kind="stable")
    sb, yb = bits[order], positive[order]
    tpi = np.cumsum(yb.astype(np.int64))
    at = np.nonzero(np.r_[sb[1:] != sb[:-1], True])[0]                 # the last row of every tie group
    tps = tpi[at]
    fps = at + 1 - tps
    P, Nn = int(tps[-1]), int(fps[-1])
    keep = np.ones(len(at), dtype=bool)
    if len(at) > 2:
        keep[1:-1] = (np.diff(fps, 2) != 0) | (np.diff(tps, 2) != 0)
    loss = np.r_[0.0, fps[keep].astype(np.float64) / float(Nn) - tps[keep].astype(np.float64) / float(P)]
    k = int(np.argmin(loss))                                           # the FIRST minimum
    if k == 0:
        return math.inf, 0, 0, P, Nn
    j = np.nonzero(keep)[0][k - 1]
    return float(scores[order[at[j]]]), int(tps[j]), int(fps[j]), P, Nn


def pair_counts(scores: np.ndarray, positive: np.ndarray):
    """(gt, eq): the pairs (positive i, negative j) with s_i > s_j and with s_i == s_j, counted one by one."""
    a, b = scores[positive], scores[~positive]
    gt = eq = 0
    for lo in range(0, len(a), _PAIR_ROWS):
        blk = a[lo:lo + _PAIR_ROWS, None]
        gt += int((blk > b[None, :]).sum())
        eq += int((blk == b[None, :]).sum())
    return gt, eq


class BagEpochMetrics:
    """Accumulator of one epoch's multi-label bag metrics on ``device``.

    Buffers (``include/wsi_hgnn.h``): ``state`` int32 [4] - cursor, flag bits, the fp64 sum of the bags' losses -, ``score_rows`` /
    ``target_rows`` fp32 ``[capacity, C]``, ``result`` int64 ``[4 + 8 C + K K]`` (K = C, or 2 for C = 1).  ``capacity`` <= 4096 rows and
    ``num_classes`` <= 32: one workgroup sorts a class's rows in LDS.

    >>> m = BagEpochMetrics(2, len(test_bags), device)
    >>> for ...: m.update(milnet(x, plan), targets)              # no sync
    >>> stats = m.compute(); m.reset()                           # one read-back per epoch
    """

    def __init__(self, num_classes: int, capacity: int, device):
        from ..graph import _resolve_device
        self.num_classes, self.capacity = int(num_classes), int(capacity)
        if not 1 <= self.num_classes <= MAX_CLASSES:
            raise ValueError(f"BagEpochMetrics: 1 <= num_classes <= {MAX_CLASSES}")
        if not 0 <= self.capacity <= MAX_ROWS:
            raise ValueError(f"BagEpochMetrics: 0 <= capacity <= {MAX_ROWS} (the rows one workgroup ranks in LDS)")
        self.device = dev = _resolve_device(device)
        C, cap = self.num_classes, self.capacity
        self.K = C if C > 1 else 2
        self.state = torch.zeros(N.WSI_BAG_METRICS_STATE_HEAD, dtype=torch.int32, device=dev)
        self.score_rows = torch.zeros((cap, C), dtype=torch.float32, device=dev)
        self.target_rows = torch.zeros((cap, C), dtype=torch.float32, device=dev)
        self.result = torch.zeros(HEAD + 8 * C + self.K * self.K, dtype=torch.int64, device=dev)
        self._loss_sum = self.state[2:4].view(torch.float64)
        self._ones: Dict[int, torch.Tensor] = {}

    # ------------------------------------------------------------------ accumulate
    def reset(self) -> "BagEpochMetrics":
        """Zero the cursor, the flags and the sum, on the current stream (one fill: recordable)."""
        self.state.zero_()
        return self

    def update(self, outputs, targets: torch.Tensor, weights: Optional[torch.Tensor] = None, max_pred: Optional[torch.Tensor] = None) -> None:
        """Append the counted bags of a forward.  ``outputs``: the bag predictions [S, C] fp32 (logits), or what the model returned
        (``split_outputs``; the instance scores are not read here).  ``max_pred`` [S, C]: DSMIL's per-bag column maximum of the instance
        scores - the loss is then 0.5 x bag + 0.5 x max; None: the bag term alone.  ``targets`` [S, C] fp32; ``weights`` [S] or [S, 1]
        fp32: a ``BagSlot``'s weights - > 0 exactly for the real non-empty bags - None: every bag counts.  No sync, no allocation
        (``weights=None`` keeps one vector of ones per S)."""
        C = self.num_classes
        bag = split_outputs(outputs)[0]
        ok = lambda t: (t.dim() == 2 and t.shape[1] == C and t.dtype == torch.float32 and t.is_contiguous() and t.shape[0] == bag.shape[0])
        if not ok(bag) or not ok(targets) or (max_pred is not None and not ok(max_pred)):
            raise ValueError(f"BagEpochMetrics.update: contiguous fp32 predictions and targets [S, {C}]")
        S = bag.shape[0]
        if weights is None:
            weights = self._ones.get(S)
            if weights is None:
                weights = self._ones[S] = torch.ones(S, dtype=torch.float32, device=self.device)
        if weights.dtype != torch.float32 or weights.numel() != S or not weights.is_contiguous():
            raise ValueError("BagEpochMetrics.update: contiguous fp32 weights [S]")
        if any(t is not None and t.device != self.device for t in (bag, targets, weights, max_pred)):
            raise RuntimeError(f"BagEpochMetrics.update: the accumulator lives on {self.device}")
        if S == 0:
            return
        if S * C > 65536:
            raise ValueError("BagEpochMetrics.update: S * C <= 65536")
        if self.device.type != "cuda":
            return self._update_torch(bag.detach(), None if max_pred is None else max_pred.detach(), targets, weights.reshape(-1))
        N.check(N.load().wsi_bag_metrics_update(N.ptr(bag), N.ptr(max_pred), N.ptr(targets), N.ptr(weights), S, C, N.ptr(self.state),
                                                N.ptr(self.score_rows), N.ptr(self.target_rows), self.capacity, N.stream()),
                "wsi_bag_metrics_update")

    def _update_torch(self, x, mx, t, w) -> None:
        """The tensor formulation of ``wsi_bag_metrics_update`` (fp32 sigmoid; the losses and their sum in fp64)."""
        cap = self.capacity
        live = w > 0
        finite = torch.isfinite(x).all(dim=1)
        if mx is not None:
            finite &= torch.isfinite(mx).all(dim=1)
        good = ((t == 0) | (t == 1)).all(dim=1)
        counted = live & finite & good
        pos = int(self.state[0]) + torch.cumsum(counted.to(torch.int64), 0) - 1
        keep = counted & (pos < cap)
        flags = ((N.WSI_BAG_METRICS_NONFINITE if bool((live & ~finite).any()) else 0)
                 | (N.WSI_BAG_METRICS_BAD_TARGET if bool((live & ~good).any()) else 0)
                 | (N.WSI_BAG_METRICS_OVERFLOW if bool((counted & ~keep).any()) else 0))
        self.state[1] |= flags
        k = int(keep.sum())
        if k == 0:
            return
        xs, ts, at = x[keep], t[keep], pos[keep]
        self.score_rows[at] = 1.0 / (1.0 + torch.exp(-xs))
        self.target_rows[at] = ts
        t64 = ts.double()
        bce = lambda v: (torch.clamp(v, min=0) - v * t64 + torch.log1p(torch.exp(-v.abs()))).sum(dim=1) / v.shape[1]
        per_bag = bce(xs.double()) if mx is None else 0.5 * bce(xs.double()) + 0.5 * bce(mx[keep].double())
        self._loss_sum += per_bag.sum()
        self.state[0] += k

    # ------------------------------------------------------------------ read
    def _n(self) -> int:
        return max(0, min(int(self.state[0].item()), self.capacity))

    def scores(self) -> torch.Tensor:
        """Sigmoid scores [n, C] of the counted bags, in the order they came (a device view; reads ``n`` back)."""
        return self.score_rows[:self._n()]

    def targets(self) -> torch.Tensor:
        return self.target_rows[:self._n()]

    def _finalize_host(self) -> None:
        """The tensor formulation of ``wsi_bag_metrics_finalize``: the same integers, the same fp64 operations in the same order."""
        C, K = self.num_classes, self.K
        n = self._n()
        s = self.score_rows[:n].cpu().numpy()
        y = self.target_rows[:n].cpu().numpy() != 0
        nan_bits = _f64_bits(math.nan)
        out = [0] * (HEAD + 8 * C + K * K)
        flags = int(self.state[1])
        thr = np.full(C, np.nan, dtype=np.float64)
        for c in range(C):
            sc, yc = np.ascontiguousarray(s[:, c]), y[:, c]
            P = int(yc.sum())
            Nn = n - P
            if P == 0 or Nn == 0:
                flags |= N.WSI_BAG_METRICS_ONE_LABEL
                out[HEAD + 8 * c:HEAD + 8 * c + 8] = [nan_bits, 0, 0, P, Nn, 0, 0, nan_bits]
                continue
            thr[c], tp, fp, P, Nn = roc_optimum(sc, yc)
            gt, eq = pair_counts(sc, yc)
            auc = np.float64(2 * gt + eq) / np.float64(2 * P * Nn)
            out[HEAD + 8 * c:HEAD + 8 * c + 8] = [_f64_bits(thr[c]), tp, fp, P, Nn, gt, eq, _f64_bits(float(auc))]
        with np.errstate(invalid="ignore"):
            pred = s.astype(np.float64) >= thr[None, :]
        exact = int((pred == y).all(axis=1).sum())
        if C == 1:
            yp, yt = pred[:, 0].astype(np.int64), y[:, 0].astype(np.int64)
        else:
            yp, yt = np.argmax(pred, axis=1), np.argmax(y, axis=1)       # the first 1; an all-zero row decodes to 0
        conf = np.bincount(yt * K + yp, minlength=K * K) if n else np.zeros(K * K, dtype=np.int64)
        out[0], out[1], out[2], out[3] = n, flags, _f64_bits(float(self._loss_sum[0])), exact
        out[HEAD + 8 * C:] = [int(v) for v in conf]
        self.result.copy_(torch.tensor(out, dtype=torch.int64))

    def result_block(self, check: bool = True) -> List[int]:
        """The whole int64 result block of ``wsi_bag_metrics_finalize`` as a host list (include/wsi_hgnn.h): the ONE read-back ``compute``
        makes.  ``check``: raise RuntimeError naming the flags that are set."""
        if self.device.type == "cuda":
            N.check(N.load().wsi_bag_metrics_finalize(N.ptr(self.state), N.ptr(self.score_rows), N.ptr(self.target_rows), self.num_classes,
                                                      self.capacity, N.ptr(self.result), N.stream()), "wsi_bag_metrics_finalize")
            block = self.result.cpu().tolist()
        else:
            self._finalize_host()
            block = self.result.tolist()
        if check and block[1]:
            raise RuntimeError("BagEpochMetrics.compute: " + "; ".join(why for bit, why in _FLAG_NAMES if block[1] & bit))
        return block

    def compute(self) -> dict:
        """The epoch's numbers over the bags accumulated since ``reset``: ``loss`` (mean over bags), ``n``, ``auc[c]`` and ``thresholds[c]``
        (``multi_label_roc``), ``tcga`` = {``avg_score``, ``f1``} (train_tcga_k-fold.py:149-156) and ``remix`` = {``precision``, ``recall``,
        ``accuracy``, ``avg``, ``auc``} (train_remix_k-fold.py:202-208).  ONE device-to-host copy.  Raises RuntimeError when a flag is set
        (a class with one label value among them: the reference's ``roc_auc_score`` raises).  Does not reset."""
        return derive(self.result_block(), self.num_classes)


def derive(block: Sequence[int], C: int) -> dict:
    """Every score of ``compute`` from the integer block, in fp64 on the host - with sklearn's conventions: a ratio with an empty denominator is
    0; macro precision / recall of the decoded labels average over the labels present among the true or the predicted ones; the tcga ``f1`` is
    at C = 1 the macro F1 over the binary classes present, at C > 1 the mean of the C per-column F1 scores; the remix ``auc`` is the AUC of
    the HARD predictions, the mean over classes of (tp / P + tn / N) / 2."""
    K = C if C > 1 else 2
    n = int(block[0])
    cls = [block[HEAD + 8 * c:HEAD + 8 * c + 8] for c in range(C)]
    conf = [block[HEAD + 8 * C + r * K:HEAD + 8 * C + (r + 1) * K] for r in range(K)]
    ratio = lambda a, b: a / b if b > 0 else 0.0
    rows = [sum(conf[l]) for l in range(K)]                                  # true counts of the decoded labels
    cols = [sum(conf[r][l] for r in range(K)) for l in range(K)]             # predicted counts
    present = [l for l in range(K) if rows[l] + cols[l] > 0]
    precision = ratio(sum(ratio(conf[l][l], cols[l]) for l in present), len(present))
    recall = ratio(sum(ratio(conf[l][l], rows[l]) for l in present), len(present))
    accuracy = ratio(sum(conf[l][l] for l in range(K)), n)
    if C == 1:
        f1 = ratio(sum(ratio(2.0 * conf[l][l], rows[l] + cols[l]) for l in present), len(present))
    else:
        f1 = sum(ratio(2.0 * tp, P + tp + fp) for _, tp, fp, P, _, _, _, _ in cls) / C
    hard = [(ratio(tp, P) + ratio(Nn - fp, Nn)) / 2 if P > 0 and Nn > 0 else math.nan for _, tp, fp, P, Nn, _, _, _ in cls]
    return {"loss": _bits_f64(block[2]) / n if n > 0 else math.nan, "n": n,
            "auc": [_bits_f64(w[7]) for w in cls], "thresholds": [_bits_f64(w[0]) for w in cls],
            "tcga": {"avg_score": ratio(block[3], n), "f1": f1},
            "remix": {"precision": precision, "recall": recall, "accuracy": accuracy, "avg": ((precision + recall) + accuracy) / 3,
                      "auc": sum(hard) / C}}


# ---------------------------------------------------------------------------------------------------------------------------------------------
def _bag_max(ins: torch.Tensor, plan: ops.ReducePlan) -> torch.Tensor:
    """[S, C]: per bag the column maximum of the instance scores (an empty bag: 0, as ``ops.segment_reduce``)."""
    if ins.is_cuda:
        return ops.segment_reduce(ins, plan, "max")
    return torch.stack([ins[a:b].max(dim=0).values if b > a else ins.new_zeros(ins.shape[1]) for a, b in plan.ranges])


def forward_update(milnet, rows: torch.Tensor, plan: ops.ReducePlan, targets: torch.Tensor, weights: Optional[torch.Tensor],
                   metrics: BagEpochMetrics) -> torch.Tensor:
    """One forward over the bags of ``plan`` and one ``metrics.update``: what ``evaluate`` runs per batch and ``CapturedBagEval`` records per
    slot.  A model that returns instance scores (DSMIL) is scored as the reference scores DSMIL: 0.5 x bag + 0.5 x max.  Returns the bag
    predictions [S, C]."""
    bag, ins = split_outputs(milnet(rows, plan))
    bag = bag.reshape(plan.num_segs, -1)
    metrics.update(bag, targets, weights, None if ins is None else _bag_max(ins, plan))
    return bag


def evaluate(milnet, bags: Sequence[torch.Tensor], labels, metrics: Optional[BagEpochMetrics] = None, batch_size: int = 8) -> dict:
    """The reference's ``test()`` done eagerly: eval mode, ``no_grad``, the bags ``batch_size`` at a time through ``bag_plan``, one
    ``metrics.update`` per batch and no read-back per bag; returns ``metrics.compute()``.  ``bags``: tensors [n_i, feats] on one device,
    ``labels``: one host label per bag (``mil.bag_targets`` makes the target rows).  ``metrics=None`` builds a ``BagEpochMetrics`` for
    ``len(bags)`` rows; one that is passed is reset first.  An empty bag is not counted (the reference has none)."""
    from . import bag_targets
    bags = list(bags)
    labels = [float(v) for v in (labels.tolist() if isinstance(labels, torch.Tensor) else labels)]
    if len(labels) != len(bags) or not bags:
        raise ValueError(f"evaluate: {len(bags)} bags but {len(labels)} labels")
    dev = bags[0].device
    with capture.eval_mode(milnet):
        for lo in range(0, len(bags), max(1, int(batch_size))):
            part = bags[lo:lo + batch_size]
            sizes = [int(t.shape[0]) for t in part]
            rows = torch.cat([t.to(torch.float32) for t in part])
            plan = bag_plan(sizes, dev)
            if metrics is None:                                    # (the number of classes: from a forward of the first batch)
                probe = split_outputs(milnet(rows, plan))[0]
                metrics = BagEpochMetrics(probe.reshape(len(part), -1).shape[1], len(bags), dev)
            if lo == 0:
                metrics.reset()
            targets = bag_targets(labels[lo:lo + batch_size], metrics.num_classes, dev).contiguous()
            weights = torch.tensor([1.0 if n > 0 else 0.0 for n in sizes], dtype=torch.float32, device=dev) if 0 in sizes else None
            forward_update(milnet, rows, plan, targets, weights, metrics)
    return metrics.compute()


class CapturedBagEval:
    """The forward of an evaluation pass captured once per ``BagSlot`` and replayed over the evaluation set: what the reference does after every
    epoch of every fold, one bag at a time with one read-back per bag.  Each slot's graph records, in eval mode under ``no_grad``, the forward
    over the slot's tables ending in ``metrics.update(outputs, slot.targets, slot.weights)``; the filler, the unused and the empty bags of a
    slot have weight 0 and are not counted.  Protocol: ``capture.py``, slot by slot (warm up, then capture, then the next slot); a batch no
    slot fits runs the same forward and the same ``update`` eagerly on the unpadded bags (``eager_batches``).

    The recorded forward reads the LIVE parameters - ``ops.linear`` packs nothing ahead of time - so an optimizer step (a ``CapturedBagStep``
    on slots of its own beside this one) between two epochs changes the result as it must.  Refused: slots with ``dropout_patch > 0`` (the
    reference's ``test`` does not drop), slots off the GPU, models other than ABMIL / DSMIL.  A model with ``torch.nn.Dropout`` is fine: eval
    mode makes it the identity.  ``metrics=None`` builds a ``BagEpochMetrics`` of the supported capacity."""

    def __init__(self, milnet: torch.nn.Module, slots, metrics: Optional[BagEpochMetrics] = None, warmup: int = 1, warmup_batches=None):
        slots, dev = check_bag_slots("CapturedBagEval", milnet, slots)
        if len({(s.feats, s.num_classes) for s in slots}) != 1:
            raise ValueError("CapturedBagEval: the slots must agree on feats and num_classes")
        if any(s.dropout_patch > 0 for s in slots):
            raise ValueError("CapturedBagEval: a slot with dropout_patch > 0 - the reference's test() does not drop patches; build the "
                             "evaluation slots without it")
        if metrics is None:
            metrics = BagEpochMetrics(slots[0].num_classes, MAX_ROWS, dev)
        elif metrics.device != dev or metrics.num_classes != slots[0].num_classes:
            raise RuntimeError(f"CapturedBagEval: metrics= must live on the slots' device ({dev}) and count their {slots[0].num_classes} classes")
        self.milnet, self.metrics = milnet, metrics
        self.slots, warmup_batches = capture.smallest_first(slots, lambda s: s.row_cap, warmup_batches)
        self.replays, self.eager_batches = 0, 0
        self.graphs, self.outputs = [], []
        with capture.eval_mode(milnet):
            for i, slot in enumerate(self.slots):
                capture.load_warm_up_batch("CapturedBagEval", i, slot, warmup_batches)
                body = lambda: forward_update(self.milnet, slot.rows, slot.plan, slot.targets, slot.weights, self.metrics)
                capture.warm_up(dev, warmup, body)
                torch.cuda.synchronize(dev)
                cg, out = capture.record("CapturedBagEval", body, self.graphs[-1].pool() if self.graphs else None,
                                         "the forward could not be captured into a hipGraph; evaluate eagerly (mil.evaluate) instead")
                self.graphs.append(cg)
                self.outputs.append(out)
            metrics.reset()                                        # (the warm-up forwards counted their rows)

    def slot_for(self, sizes: Sequence[int]):
        """Index of the smallest slot the batch fits, or None."""
        return capture.first_fit(self.slots, sizes)

    def run(self, bags: Sequence[torch.Tensor], labels) -> torch.Tensor:
        """The bag predictions ``[len(bags), C]`` of the bags ``bags`` (device tensors [n_i, feats]) with host labels ``labels`` (a device
        tensor; those of a replay are overwritten by the next replay of the same slot), their rows appended to ``metrics``."""
        bags = list(bags)
        sizes = [int(t.shape[0]) for t in bags]
        i = self.slot_for(sizes)
        if i is None:
            from . import bag_targets
            with capture.eval_mode(self.milnet):
                dev = self.slots[0].device
                rows = torch.cat([t.to(torch.float32) for t in bags])
                labels = [float(v) for v in (labels.tolist() if isinstance(labels, torch.Tensor) else labels)]
                targets = bag_targets(labels, self.metrics.num_classes, dev).contiguous()
                weights = torch.tensor([1.0 if n > 0 else 0.0 for n in sizes], dtype=torch.float32, device=dev)
                self.eager_batches += 1
                return forward_update(self.milnet, rows, bag_plan(sizes, dev), targets, weights, self.metrics)
        slot = self.slots[i]
        slot.load(bags, labels)
        self.graphs[i].replay()
        self.replays += 1
        return self.outputs[i][:slot.num_real]

    def run_epoch(self, batches) -> dict:
        """``metrics.reset()``, every ``(bags, labels)`` of ``batches`` through ``run``, ``metrics.compute()``: one read-back.  The model's
        training flag is what it was on return."""
        with capture.eval_mode(self.milnet):
            self.metrics.reset()
            for bags, labels in batches:
                self.run(bags, labels)
            return self.metrics.compute()
