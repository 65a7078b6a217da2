"""Epoch metrics accumulated on the device: the reference's per-epoch accuracy / precision / recall / F1 / AUC and mean cross entropy
(trainer/train_gnn.py:73-79,104-108 over the training predictions; evaluator/eval_homo_graph.py:61-95 over an evaluation set; utils.py:37-47)
without a read-back per step.

``EpochMetrics.update(logits, labels)`` is ONE launch (``wsi_metrics_update``, csrc/metrics.hip) that allocates nothing and never synchronises, so it
can be the last node of a captured step (``trainer.CapturedSlotStep(..., metrics=)``) or of a captured forward (``trainer.CapturedSlotEval``);
``compute`` runs ``wsi_metrics_finalize`` and makes the ONE device-to-host copy of the epoch.  A label of -100 - what ``data.BatchSlot`` gives its
filler and its empty graphs - is not counted.

The AUC ranks the softmax PROBABILITIES, as the reference does (``prob_list`` into ``metrics``, train_gnn.py:67,108; eval_homo_graph.py:54,90).
On a CPU device the same class runs a tensor formulation of both steps (as ``data.BatchSlot`` and ``transforms`` do): the fixture the kernels are
compared with.
"""
from __future__ import annotations

from typing import Dict

import torch

from . import _native as N

IGNORE_INDEX = -100
KEYS = ("precision", "recall", "f1", "auc")
_FLAG_NAMES = ((N.WSI_METRICS_BAD_LABEL, "a label outside [0, num_classes) other than -100"),
               (N.WSI_METRICS_NONFINITE, "a non-finite logit in a counted row"),
               (N.WSI_METRICS_OVERFLOW, "more counted rows than the capacity (the rows past it were dropped)"))
_PAIR_TILE = 256          # csrc/metrics.hip::METRICS_TILE


class EpochMetrics:
    """Accumulator of one epoch's classification metrics on ``device``.

    Buffers (``include/wsi_hgnn.h``): ``state`` int32 ``[4 + C * C]`` - cursor, flag bits, the fp64 sum of the cross entropies, the confusion
    matrix ``conf[label, prediction]`` -, ``probs`` fp32 ``[capacity, C]``, ``row_labels`` / ``row_preds`` int64 ``[capacity]``.

    >>> m = EpochMetrics(2, len(loader.items), device)
    >>> for ...: m.update(logits, labels)              # no sync
    >>> stats = m.compute("binary"); m.reset()          # one read-back per epoch
    """

    def __init__(self, num_classes: int, capacity: int, device):
        from .graph import _resolve_device
        self.num_classes, self.capacity = int(num_classes), int(capacity)
        if not 1 <= self.num_classes <= 32:
            raise ValueError("EpochMetrics: 1 <= num_classes <= 32")
        if self.capacity < 0:
            raise ValueError("EpochMetrics: capacity >= 0")
        self.device = dev = _resolve_device(device)
        C, cap = self.num_classes, self.capacity
        self.state = torch.zeros(N.WSI_METRICS_STATE_HEAD + C * C, dtype=torch.int32, device=dev)
        self.probs = torch.zeros((cap, C), dtype=torch.float32, device=dev)
        self.row_labels = torch.zeros(cap, dtype=torch.int64, device=dev)
        self.row_preds = torch.zeros(cap, dtype=torch.int64, device=dev)
        self.result = torch.zeros(N.WSI_METRICS_RESULT_HEAD + 4 * C, dtype=torch.float64, device=dev)
        self._partials = torch.zeros(max(C * ((cap + _PAIR_TILE - 1) // _PAIR_TILE) * 2, 1), dtype=torch.int64, device=dev)
        # views of the state block (the fp64 sum lies 8 bytes in: the block itself is aligned as every torch allocation)
        self.confusion = self.state[N.WSI_METRICS_STATE_HEAD:].view(C, C)
        self._loss_sum = self.state[2:4].view(torch.float64)

    # ------------------------------------------------------------------ accumulate
    def reset(self) -> "EpochMetrics":
        """Zero the cursor, the flags, the confusion matrix and the sum, on the current stream (one fill: recordable)."""
        self.state.zero_()
        return self

    def update(self, logits: torch.Tensor, labels: torch.Tensor) -> None:
        """Append the counted rows of ``logits`` [B, C] fp32 against int64 ``labels`` [B].  No sync, no allocation."""
        C = self.num_classes
        if (logits.dim() != 2 or logits.shape[1] != C or logits.dtype != torch.float32 or labels.dtype != torch.int64 or labels.dim() != 1
                or labels.shape[0] != logits.shape[0] or not logits.is_contiguous() or not labels.is_contiguous()):
            raise ValueError(f"EpochMetrics.update: contiguous logits [B, {C}] fp32 and int64 labels [B]")
        if logits.device != self.device or labels.device != self.device:
            raise RuntimeError(f"EpochMetrics.update: the accumulator lives on {self.device}")
        B = logits.shape[0]
        if B == 0:
            return
        if B * C > 65536:
            raise ValueError("EpochMetrics.update: B * C <= 65536")
        if self.device.type != "cuda":
            return self._update_torch(logits.detach(), labels)
        N.check(N.load().wsi_metrics_update(N.ptr(logits), N.ptr(labels), B, C, N.ptr(self.state), N.ptr(self.probs), N.ptr(self.row_labels),
                                            N.ptr(self.row_preds), self.capacity, N.stream()), "wsi_metrics_update")

    def _update_torch(self, x: torch.Tensor, y: torch.Tensor) -> None:
        """The tensor formulation of ``wsi_metrics_update`` (fp32 softmax with the maximum subtracted, fp64 sum)."""
        C, cap = self.num_classes, self.capacity
        ignored = y == IGNORE_INDEX
        bad = ~ignored & ((y < 0) | (y >= C))
        finite = torch.isfinite(x).all(dim=1)
        nonfinite = ~ignored & ~bad & ~finite
        counted = ~ignored & ~bad & finite
        pos = int(self.state[0]) + torch.cumsum(counted.to(torch.int64), 0) - 1
        keep = counted & (pos < cap)
        flags = ((N.WSI_METRICS_BAD_LABEL if bool(bad.any()) else 0) | (N.WSI_METRICS_NONFINITE if bool(nonfinite.any()) else 0)
                 | (N.WSI_METRICS_OVERFLOW if bool((counted & ~keep).any()) else 0))
        self.state[1] |= flags
        k = int(keep.sum())
        if k == 0:
            return
        xs, ys, at = x[keep], y[keep], pos[keep]
        mx = xs.max(dim=1, keepdim=True).values
        e = torch.exp(xs - mx)
        den = e.sum(dim=1, keepdim=True)
        self.probs[at] = e / den
        self.row_labels[at] = ys
        pred = xs.argmax(dim=1)                                  # (the first maximum)
        self.row_preds[at] = pred
        self.confusion.view(-1).index_add_(0, ys * C + pred, torch.ones(k, dtype=torch.int32))
        ce = (torch.log(den) + mx).reshape(-1) - xs.gather(1, ys.reshape(-1, 1)).reshape(-1)
        self._loss_sum += ce.double().sum()
        self.state[0] += k

    # ------------------------------------------------------------------ read
    def _n(self) -> int:
        return max(0, min(int(self.state[0].item()), self.capacity))

    def probabilities(self) -> torch.Tensor:
        """Softmax probabilities [n, C] of the counted rows, in row order (a device view; reads ``n`` back)."""
        return self.probs[:self._n()]

    def labels(self) -> torch.Tensor:
        return self.row_labels[:self._n()]

    def predictions(self) -> torch.Tensor:
        return self.row_preds[:self._n()]

    def _finalize_torch(self) -> None:
        """The tensor formulation of ``wsi_metrics_finalize``: the same integers, the same fp64 operations in the same order."""
        C = self.num_classes
        n = self._n()
        conf = self.confusion.tolist()
        s, y = self.probs[:n], self.row_labels[:n]
        out = [0.0] * (N.WSI_METRICS_RESULT_HEAD + 4 * C)
        nan = float("nan")
        ratio = lambda a, b: a / b if b > 0 else 0.0
        cls = []
        for c in range(C):
            tp, row, col = conf[c][c], sum(conf[c]), sum(conf[k][c] for k in range(C))
            p, r = ratio(tp, col), ratio(tp, row)
            f = 2 * p * r / (p + r) if p + r > 0 else 0.0
            isc = y == c
            a, b = s[isc, c], s[~isc, c]
            gt = int((a[:, None] > b[None, :]).sum())
            eq = int((a[:, None] == b[None, :]).sum())
            P, Nn = row, n - row
            cls.append((p, r, f, (2 * gt + eq) / (2 * P * Nn) if P > 0 and Nn > 0 else nan))
            out[N.WSI_METRICS_RESULT_HEAD + 4 * c:N.WSI_METRICS_RESULT_HEAD + 4 * c + 4] = cls[c]
        out[0], out[1] = float(n), float(int(self.state[1]))
        out[2] = sum(conf[k][k] for k in range(C)) / n if n > 0 else nan
        out[3] = float(self._loss_sum[0]) / n if n > 0 else nan
        binary = [0.0, 0.0, 0.0, nan]
        if C > 1:
            binary[:3] = cls[1][:3]
            tp, P, col = conf[1][1], sum(conf[1]), sum(conf[k][1] for k in range(C))
            Nn, fp, fn = n - P, col - tp, P - tp
            tn = Nn - fp
            if P > 0 and Nn > 0:
                binary[3] = (2 * tp * tn + tp * fp + tn * fn) / (2 * P * Nn)
        out[4:8] = binary
        out[8:12] = [sum(cls[c][k] for c in range(C)) / C for k in range(4)]
        self.result.copy_(torch.tensor(out, dtype=torch.float64))

    def compute(self, average: str = "binary") -> Dict[str, float]:
        """``{"loss", "accuracy", "precision", "recall", "f1", "auc", "n"}`` over the rows accumulated since ``reset`` (the keys of
        ``io.evaluate``): ``average`` 'binary' - class 1, the AUC of the hard predictions - or 'macro' - unweighted class means, the one-vs-rest
        AUC of the probabilities (utils.py:37-47).  ONE device-to-host copy.  Raises RuntimeError when a flag is set.  Does not reset."""
        if average not in ("binary", "macro"):
            raise ValueError("EpochMetrics.compute: average is 'binary' or 'macro'")
        block = self.result_block()
        at = 4 if average == "binary" else 8
        out = {"loss": block[3], "accuracy": block[2]}
        out.update(zip(KEYS, block[at:at + 4]))
        out["n"] = int(block[0])
        return out

    def result_block(self) -> list:
        """The whole fp64 result block of ``wsi_metrics_finalize`` as a host list (per-class numbers behind the aggregates, include/wsi_hgnn.h);
        the read-back ``compute`` makes, with the same check of the flags."""
        if self.device.type == "cuda":
            N.check(N.load().wsi_metrics_finalize(N.ptr(self.state), N.ptr(self.probs), N.ptr(self.row_labels), self.num_classes, self.capacity,
                                                  N.ptr(self._partials), N.ptr(self.result), N.stream()), "wsi_metrics_finalize")
            block = self.result.cpu().tolist()
        else:
            self._finalize_torch()
            block = self.result.tolist()
        flags = int(block[1])
        if flags:
            raise RuntimeError("EpochMetrics.compute: " + "; ".join(why for bit, why in _FLAG_NAMES if flags & bit))
        return block
