"""Shared fixture of tests/test_epoch_metrics.py and tests/test_epoch_metrics_gpu.py: update sequences for metrics.EpochMetrics and the float64
references they are held against.  Logits lie in [-10, 10]; updates alternate between 1 and 3 rows until 40 rows are counted.

Cases and what each is there for:
  c2        C = 2: duplicated logit rows (tied scores in both columns), rows with two equal maxima (first-maximum prediction), rows labelled -100
            with NaN logits interleaved (not counted, not flagged)
  c5        C = 5, every class occurs: the same edge rows
  c5_absent C = 5, class 4 never occurs: its AUC and the macro AUC are NaN, everything else finite
  empty     n = 0: only ignored rows
  ties257   C = 3, ONE update of 300 rows of which 257 count, logits from {-1, 0, 1}: many ties; crosses the 256-row step of the update kernel and
            the 256-row tile of the pair kernel
"""
import math

import torch

IGNORE = -100
P_TOL, LOSS_TOL, EXACT_TOL = 1e-6, 1e-5, 1e-12


def _sequence(C, seed, classes, n=40):
    gen = torch.Generator().manual_seed(seed)
    ups, rows, k = [], [], 0
    while len(rows) < n:
        B = 3 if k % 5 == 4 else (1, 3)[k % 2]
        x = torch.rand((B, C), generator=gen) * 20.0 - 10.0
        y = torch.tensor(classes)[torch.randint(0, len(classes), (B,), generator=gen)]
        if k % 7 == 3 and rows:                              # a duplicate of an earlier row, under whatever label it draws: tied scores
            x[0] = rows[len(rows) // 2]
        if k % 6 == 2:                                       # two equal maxima: the prediction is the first
            x[0, C - 1] = x[0, 0] = min(float(x[0].max()) + 0.5, 10.0)
        if k % 9 == 5 and C > 2:
            x[0, 1] = x[0, 2] = min(float(x[0].max()) + 1.0, 10.0)
        if k % 5 == 4:                                       # a -100 row in the middle of an update, carrying NaN and inf
            y[1] = IGNORE
            x[1, 0], x[1, C - 1] = float("nan"), float("inf")
        for b in range(B):
            if int(y[b]) != IGNORE:
                if len(rows) < n:
                    rows.append(x[b].clone())
                else:
                    y[b] = IGNORE                            # (exactly n rows count)
        ups.append((x, y))
        k += 1
    return ups


def cases():
    gen = torch.Generator().manual_seed(99)
    x257 = torch.randint(-1, 2, (300, 3), generator=gen).to(torch.float32)
    y257 = torch.randint(0, 3, (300,), generator=gen)
    y257[torch.randperm(300, generator=gen)[:43]] = IGNORE
    return {
        "c2": dict(C=2, capacity=48, updates=_sequence(2, 1, [0, 1])),
        "c5": dict(C=5, capacity=40, updates=_sequence(5, 2, [0, 1, 2, 3, 4])),
        "c5_absent": dict(C=5, capacity=64, updates=_sequence(5, 3, [0, 1, 2, 3])),
        "empty": dict(C=2, capacity=4, updates=[(torch.full((3, 2), float("nan")), torch.full((3,), IGNORE, dtype=torch.int64))]),
        "ties257": dict(C=3, capacity=257, updates=[(x257, y257)]),
    }


def feed(metrics, case, device):
    for x, y in case["updates"]:
        metrics.update(x.to(device), y.to(device))
    return metrics


def counted_rows(case):
    """(logits [n, C] fp32, labels [n]) of the rows that count, in row order."""
    x = torch.cat([u[0] for u in case["updates"]])
    y = torch.cat([u[1] for u in case["updates"]])
    keep = y != IGNORE
    return x[keep], y[keep]


def close(a, b, tol):
    return (math.isnan(a) and math.isnan(b)) or abs(a - b) <= tol


def reference(case):
    """float64 softmax, cross entropies, first-maximum predictions and the confusion matrix of the counted rows."""
    x, y = counted_rows(case)
    C = case["C"]
    p = torch.softmax(x.double(), dim=1)
    ce = -torch.log(p.gather(1, y.reshape(-1, 1))).reshape(-1) if len(y) else torch.zeros(0, dtype=torch.float64)
    pred = torch.from_numpy(x.numpy().argmax(axis=1)) if len(y) else torch.zeros(0, dtype=torch.int64)
    conf = torch.zeros((C, C), dtype=torch.int32)
    for a, b in zip(y.tolist(), pred.tolist()):
        conf[a, b] += 1
    return dict(x=x, y=y, p=p, ce=ce, pred=pred, conf=conf)


def brute_auc(scores, pos):
    """The Mann-Whitney statistic by two Python loops over exact integers."""
    P, Nn = int(pos.sum()), int((~pos).sum())
    if P == 0 or Nn == 0:
        return float("nan")
    s = scores.tolist()
    twice = sum((2 if s[i] > s[j] else (1 if s[i] == s[j] else 0)) for i in range(len(s)) if pos[i] for j in range(len(s)) if not pos[j])
    return twice / (2 * P * Nn)


def check_against_references(metrics, case, with_brute=True):
    """Everything ``compute`` returns against io.classification_metrics fed the accumulator's OWN stored probabilities (1e-12), the stored rows
    against float64 (1e-6 / 1e-5), integers exactly.  Prints each figure before it asserts."""
    from wsi_hgnn_amd import io
    ref = reference(case)
    C, n = case["C"], len(ref["y"])
    probs, labels, preds = metrics.probabilities().cpu(), metrics.labels().cpu(), metrics.predictions().cpu()
    assert probs.shape == (n, C) and torch.equal(labels, ref["y"]) and torch.equal(preds, ref["pred"])
    assert torch.equal(metrics.confusion.cpu(), ref["conf"]) and int(metrics.state[0]) == n and int(metrics.state[1]) == 0
    perr = (probs.double() - ref["p"]).abs().max().item() if n else 0.0
    print("probabilities", perr)
    assert perr <= P_TOL
    block = metrics.result_block()
    for average in ("binary", "macro"):
        got = metrics.compute(average)
        assert got["n"] == n
        mean_ce = ref["ce"].mean().item() if n else float("nan")
        acc = (ref["pred"] == ref["y"]).double().mean().item() if n else float("nan")
        print(average, got, "loss ref", mean_ce, "accuracy ref", acc)
        assert close(got["loss"], mean_ce, LOSS_TOL) and close(got["accuracy"], acc, EXACT_TOL)
        if n == 0:
            assert got["precision"] == got["recall"] == got["f1"] == 0.0 and math.isnan(got["auc"])
            continue
        p, r, f, a = io.classification_metrics(probs.double(), labels, average)
        assert close(got["precision"], p, EXACT_TOL) and close(got["recall"], r, EXACT_TOL) and close(got["f1"], f, EXACT_TOL)
        if average == "macro" or C == 2:
            assert close(got["auc"], a, EXACT_TOL), (got["auc"], a)
        else:                               # C > 2: class 1 against the rest from the confusion matrix, (TPR + TNR) / 2
            pos, hit = labels == 1, preds == 1
            P, Nn = int(pos.sum()), int((~pos).sum())
            want = (int((pos & hit).sum()) / P + int((~pos & ~hit).sum()) / Nn) / 2 if P and Nn else float("nan")
            assert close(got["auc"], want, EXACT_TOL), (got["auc"], want)
    if with_brute and n:
        for c in range(C):
            want = brute_auc(probs[:, c], labels == c)
            assert close(block[12 + 4 * c + 3], want, EXACT_TOL), (c, block[12 + 4 * c + 3], want)
    return block
