#!/usr/bin/env python
"""One evaluation pass of the MIL baselines on one GPU: DSMIL and ABMIL (feats 1024, 2 classes, fp32 GEMMs) over 64 bags of
6 000 - 12 000 rows, every form ending in the epoch's numbers on the host:

    plain PyTorch   the reference's regime restated: one bag per forward, the loss read back and the sigmoid scores copied to the host per bag
                    (``.cpu().numpy()``), then sklearn on the host - roc_curve and the first minimum of fpr - tpr per class, the thresholded
                    predictions, f1 / precision / recall / accuracy / AUC
    evaluate        mil.evaluate, one bag per forward (batch_size 1), and eight bags per forward (batch_size 8)
    one slot        mil.CapturedBagEval over one BagSlot that holds the largest bag
    three slots     the same over three slots by size
    eight per slot  the same over one slot of eight bags (the batch of evaluate's batch_size 8, padded to the largest such batch)

interleaved, medians and min / max over the repeats (ms per pass).  Then ``BagEpochMetrics.update`` (one bag) and ``wsi_bag_metrics_finalize``
alone by device events at n = 64 and n = 4096.  Prints one JSON line and writes it to --out.

    python tools/bag_eval_bench.py --repeats 7 --inner 2 --out profiles/r23_bag_eval.json
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np
import torch

import __graft_entry__
import mil_bench as MB
from bag_slot_bench import BAGS, CLASSES, FEATS, SLOT_CAPS, _model, _sizes


def _host_metrics(scores, labels):
    """What the reference's test() derives on the host from the epoch's scores, by the rule (sklearn does the curves and the scores)."""
    from sklearn.metrics import accuracy_score, f1_score, precision_score, recall_score, roc_auc_score, roc_curve
    C = scores.shape[1]
    hard, aucs, thr = scores.copy(), [], []
    for c in range(C):
        fpr, tpr, t = roc_curve(labels[:, c], scores[:, c])
        k = int(np.argmin(fpr - tpr))
        thr.append(t[k])
        aucs.append(roc_auc_score(labels[:, c], scores[:, c]))
        hard[:, c] = scores[:, c] >= t[k]
    y_pred, y_true = hard.argmax(1), labels.argmax(1)
    return {"auc": aucs, "thresholds": thr, "avg_score": float((hard == labels).all(1).mean()),
            "f1": f1_score(labels, hard, average="macro", zero_division=0),
            "precision": precision_score(y_true, y_pred, average="macro", zero_division=0),
            "recall": recall_score(y_true, y_pred, average="macro", zero_division=0), "accuracy": accuracy_score(y_true, y_pred),
            "hard_auc": roc_auc_score(labels, hard, average="macro")}


def passes(res, args, dev):
    from wsi_hgnn_amd import mil
    sizes = _sizes()
    bags = [torch.randn(n, FEATS, device=dev) for n in sizes]
    labels = [i % 2 for i in range(BAGS)]
    targets = mil.bag_targets(labels, CLASSES, dev)
    host_targets = targets.cpu().numpy()
    bce = torch.nn.BCEWithLogitsLoss()
    big = max(range(BAGS), key=lambda i: sizes[i])
    res["bag_rows"] = {"min": min(sizes), "median": int(statistics.median(sizes)), "max": max(sizes)}
    for name in ("dsmil", "abmil"):
        m = _model(name, dev).eval()
        params = {k: q.detach() for k, q in m.named_parameters()}
        out = {}

        def plain():
            total, rows = 0.0, []
            with torch.no_grad():
                for i in range(BAGS):
                    if name == "dsmil":
                        ins, pred = MB.torch_dsmil(params, bags[i])
                        loss = 0.5 * bce(pred, targets[i:i + 1]) + 0.5 * bce(ins.max(0)[0].view(1, -1), targets[i:i + 1])
                    else:
                        pred = MB.torch_abmil(params, bags[i])
                        loss = bce(pred, targets[i:i + 1])
                    total += loss.item()
                    rows.append(torch.sigmoid(pred).squeeze().cpu().numpy())
            out["plain_pytorch"] = dict(_host_metrics(np.array(rows), host_targets), loss=total / BAGS)

        acc = mil.BagEpochMetrics(CLASSES, BAGS, dev)

        def evaluate(bs):
            out[f"evaluate_b{bs}"] = mil.evaluate(m, bags, labels, metrics=acc, batch_size=bs)

        legs = {"plain_pytorch": plain, "evaluate_b1": lambda: evaluate(1), "evaluate_b8": lambda: evaluate(8)}
        keep = {}
        for leg, caps in (("one_slot", SLOT_CAPS[-1:]), ("three_slots", SLOT_CAPS)):
            slots = [mil.BagSlot(FEATS, cap, 1, CLASSES, dev) for cap in caps]
            warm = [([bags[next(i for i in range(BAGS) if s.fits([sizes[i]]) and (i == big or s is not slots[-1]))]], [1]) for s in slots]
            cap = keep[leg] = mil.CapturedBagEval(m, slots, mil.BagEpochMetrics(CLASSES, BAGS, dev), warmup=2, warmup_batches=warm)
            batches = [([bags[i]], [labels[i]]) for i in range(BAGS)]
            legs[leg] = lambda cap=cap, leg=leg, batches=batches: out.__setitem__(leg, cap.run_epoch(batches))
        groups = [list(range(lo, lo + 8)) for lo in range(0, BAGS, 8)]
        wide = mil.BagSlot(FEATS, max(sum(sizes[i] for i in g) for g in groups) + 1, 8, CLASSES, dev)
        cap8 = keep["eight_per_slot"] = mil.CapturedBagEval(m, wide, mil.BagEpochMetrics(CLASSES, BAGS, dev), warmup=2,
                                                            warmup_batches=[([bags[i] for i in groups[0]], [labels[i] for i in groups[0]])])
        batches8 = [([bags[i] for i in g], [labels[i] for i in g]) for g in groups]
        legs["eight_per_slot"] = lambda: out.__setitem__("eight_per_slot", cap8.run_epoch(batches8))
        med, spread = MB._interleaved(legs, args.repeats, args.inner, warmup=2)
        row = {k: {"ms": med[k], "min_max_ms": spread[k]} for k in legs}
        for k in ("evaluate_b1", "evaluate_b8", "one_slot", "three_slots", "eight_per_slot"):
            row[k]["over_plain_pytorch"] = round(med[k] / med["plain_pytorch"], 3)
            row[k]["over_evaluate_b1"] = round(med[k] / med["evaluate_b1"], 3)
        row["eight_per_slot"]["over_evaluate_b8"] = round(med["eight_per_slot"] / med["evaluate_b8"], 3)
        row["eager_batches"] = {leg: c.eager_batches for leg, c in keep.items()}
        # the forms agree: thresholds and AUCs of the device against sklearn on the plain leg's scores (different GEMMs: not bit-equal inputs)
        row["agreement"] = {"auc_abs_diff_vs_plain": max(abs(a - b) for a, b in zip(out["three_slots"]["auc"], out["plain_pytorch"]["auc"])),
                            "loss": {k: out[k]["loss"] for k in out},
                            "three_slots_equals_evaluate_b1": out["three_slots"] == out["evaluate_b1"],
                            "eight_per_slot_equals_evaluate_b8": out["eight_per_slot"] == out["evaluate_b8"]}
        res["passes"][name] = row
        del legs, keep
        torch.cuda.empty_cache()


def kernels_alone(res, dev):
    from wsi_hgnn_amd import mil
    rng = np.random.RandomState(3)
    for n in (64, 4096):
        acc = mil.BagEpochMetrics(CLASSES, n, dev)
        y = torch.from_numpy((rng.rand(n, CLASSES) < 0.5).astype(np.float32)).to(dev)
        x = torch.from_numpy(rng.randn(n, CLASSES).astype(np.float32)).to(dev)
        for lo in range(0, n, 1024):
            acc.update(x[lo:lo + 1024], y[lo:lo + 1024], None, x[lo:lo + 1024])
        one = lambda: (acc.state[0].fill_(n - 1), acc.update(x[:1], y[:1], None, x[:1]))          # (the cursor put back: the row is rewritten)
        fin = lambda: mil.metrics.N.check(mil.metrics.N.load().wsi_bag_metrics_finalize(
            mil.metrics.N.ptr(acc.state), mil.metrics.N.ptr(acc.score_rows), mil.metrics.N.ptr(acc.target_rows), CLASSES, n,
            mil.metrics.N.ptr(acc.result), mil.metrics.N.stream()), "finalize")
        fill = lambda: acc.state[0].fill_(n - 1)
        row = {}
        for key, fn in (("cursor_fill_us", fill), ("fill_and_update_us", one), ("finalize_us", fin)):
            for _ in range(10):
                fn()
            samples = [MB._window(fn, 200) * 1e3 for _ in range(5)]
            row[key] = {"median": round(statistics.median(samples), 2), "min_max": [round(min(samples), 2), round(max(samples), 2)]}
        res["kernels"][f"n{n}"] = row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--inner", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bag_eval_bench.py measures on the GPU; none is visible")
    __graft_entry__.build()
    from wsi_hgnn_amd import ops
    dev = torch.device("cuda:0")
    res = {"workload": "MIL evaluation pass with the epoch's metrics on the device", "feats": FEATS, "classes": CLASSES, "bags": BAGS,
           "gemm": ops.gemm_precision(), "repeats": args.repeats, "inner": args.inner, "slot_caps": list(SLOT_CAPS), "passes": {}, "kernels": {}}
    passes(res, args, dev)
    torch.cuda.empty_cache()
    kernels_alone(res, dev)
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
