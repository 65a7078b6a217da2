#!/usr/bin/env python
"""Fixture produced by EXECUTING the reference's own ``multi_label_roc`` / ``optimal_thresh`` (baselines/ReMix_DSMIL_ABMIL/
train_tcga_k-fold.py:158-180 and train_remix_k-fold.py:211-232) and ``inverse_convert_label`` (train_remix_k-fold.py:60-68) over the cases of
tests/bag_metrics_cases.py, followed by the sklearn calls of the two ``test()`` functions on the thresholded predictions (train_tcga_k-fold.py:
136-154, train_remix_k-fold.py:189-207), made here line for line.  mil/reference_bag_metrics.json records, per case, the builder's arguments with
checksums of the scores and labels it gave, and the results: the optimal thresholds (as the bits of the fp64 value: +inf occurs), the per-class
AUC, tp / fp at the threshold, P, N, the pair counts, the exact-match count, the confusion matrix of the decoded labels and the scores the two
scripts return.  Data only; no reference source travels.

The functions are taken out of the reference's files by name and executed with numpy and scikit-learn alone (1.7.2 here: the first threshold
of ``roc_curve`` is +inf).  Re-run where the reference is checked out:
``python tests/golden/make_reference_bag_metrics_fixture.py <reference checkout>``."""
import ast
import copy
import json
import os
import sys
import warnings

import numpy as np
import sklearn
from sklearn.metrics import accuracy_score, confusion_matrix, f1_score, precision_score, recall_score, roc_auc_score, roc_curve

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import bag_metrics_cases as BM  # noqa: E402

TCGA = ("baselines", "ReMix_DSMIL_ABMIL", "train_tcga_k-fold.py")
REMIX = ("baselines", "ReMix_DSMIL_ABMIL", "train_remix_k-fold.py")


def load(reference: str, rel, names):
    path = os.path.join(reference, *rel)
    tree = ast.parse(open(path).read(), path)
    fns = [node for node in tree.body if isinstance(node, ast.FunctionDef) and node.name in names]
    assert len(fns) == len(names), (path, names)
    scope = {"np": np, "roc_curve": roc_curve, "roc_auc_score": roc_auc_score}
    exec(compile(ast.Module(body=fns, type_ignores=[]), path, "exec"), scope)
    return scope


def bits(x) -> int:
    return int(np.array([x], dtype=np.float64).view(np.int64)[0])


def threshold_predictions(test_predictions, thresholds_optimal, num_classes):
    """train_tcga_k-fold.py:137-148 = train_remix_k-fold.py:190-201"""
    if num_classes == 1:
        class_prediction_bag = copy.deepcopy(test_predictions)
        class_prediction_bag[test_predictions >= thresholds_optimal[0]] = 1
        class_prediction_bag[test_predictions < thresholds_optimal[0]] = 0
        return class_prediction_bag
    test_predictions = test_predictions.copy()
    for i in range(num_classes):
        class_prediction_bag = copy.deepcopy(test_predictions[:, i])
        class_prediction_bag[test_predictions[:, i] >= thresholds_optimal[i]] = 1
        class_prediction_bag[test_predictions[:, i] < thresholds_optimal[i]] = 0
        test_predictions[:, i] = class_prediction_bag
    return test_predictions


def main():
    tcga = load(sys.argv[1], TCGA, ("multi_label_roc", "optimal_thresh"))
    remix = load(sys.argv[1], REMIX, ("multi_label_roc", "optimal_thresh", "inverse_convert_label"))
    cases = []
    for name, n, C, family, seed, absent in BM.case_list():
        scores, labels = BM.build(n, C, family, seed, absent)
        n = scores.shape[0]
        # what test() holds after its loop: predictions [n, C] - [n] at C = 1, the per-bag arrays were squeezed - and labels [n, C]
        test_predictions = scores[:, 0].copy() if C == 1 else scores.copy()
        test_labels = labels.astype(np.float64)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            aucs, curves, thr = tcga["multi_label_roc"](test_labels, test_predictions, C, pos_label=1)
            aucs_r, _, thr_r = remix["multi_label_roc"](test_labels.reshape(n, -1), test_predictions, C)
            assert [bits(a) for a in thr] == [bits(a) for a in thr_r] and [bits(a) for a in aucs] == [bits(a) for a in aucs_r]
            hard = threshold_predictions(test_predictions, thr, C)
            y_true_rows = np.squeeze(test_labels) if C == 1 else test_labels
            # train_tcga_k-fold.py:149-154
            bag_score = 0
            for i in range(n):
                bag_score = np.array_equal(y_true_rows[i], hard[i]) + bag_score
            avg_score = bag_score / n
            f1 = f1_score(y_pred=hard, y_true=y_true_rows, average="macro")
            # train_remix_k-fold.py:202-207
            y_pred, y_true = remix["inverse_convert_label"](hard), remix["inverse_convert_label"](y_true_rows)
            p = precision_score(y_true, y_pred, average="macro")
            r = recall_score(y_true, y_pred, average="macro")
            acc = accuracy_score(y_true, y_pred)
            avg = np.mean([p, r, acc])
            c_auc = roc_auc_score(y_score=hard, y_true=y_true_rows, multi_class="ovr", average="macro")
        K = C if C > 1 else 2
        hard2, lab2 = hard.reshape(n, C) != 0, labels != 0
        gt = [int((scores[lab2[:, c], c][:, None] > scores[~lab2[:, c], c][None, :]).sum()) for c in range(C)]
        eq = [int((scores[lab2[:, c], c][:, None] == scores[~lab2[:, c], c][None, :]).sum()) for c in range(C)]
        cases.append({"name": name, "n": n, "C": C, "family": family, "seed": seed, "absent": absent,
                      "score_bits_sum": int(scores.view(np.int32).astype(np.int64).sum()), "label_sum": [int(v) for v in lab2.sum(0)],
                      "threshold_bits": [bits(t) for t in thr], "auc": [float(a) for a in aucs],
                      "roc_points": [int(len(t)) for t in curves], "distinct_scores": [int(len(np.unique(scores[:, c]))) for c in range(C)],
                      "tp": [int((hard2[:, c] & lab2[:, c]).sum()) for c in range(C)], "fp": [int((hard2[:, c] & ~lab2[:, c]).sum()) for c in range(C)],
                      "P": [int(lab2[:, c].sum()) for c in range(C)], "N": [int((~lab2[:, c]).sum()) for c in range(C)], "gt": gt, "eq": eq,
                      "exact": int(bag_score), "confusion": confusion_matrix(y_true, y_pred, labels=list(range(K))).tolist(),
                      "labels_present": sorted(int(v) for v in set(np.unique(y_true)) | set(np.unique(y_pred))),
                      "tcga": {"avg_score": float(avg_score), "f1": float(f1)},
                      "remix": {"precision": float(p), "recall": float(r), "accuracy": float(acc), "avg": float(avg), "auc": float(c_auc)}})
    os.makedirs(os.path.join(HERE, "mil"), exist_ok=True)
    path = os.path.join(HERE, "mil", "reference_bag_metrics.json")
    with open(path, "w") as f:
        json.dump({"functions": ["/".join(TCGA) + ":multi_label_roc,optimal_thresh", "/".join(REMIX) + ":multi_label_roc,optimal_thresh,inverse_convert_label"],
                   "sklearn": sklearn.__version__, "cases": cases}, f, indent=0)
        f.write("\n")
    print("wrote", path, os.path.getsize(path), "bytes,", len(cases), "cases;", sum(1 for c in cases if float("inf") in
          [float(np.array([b], dtype=np.int64).view(np.float64)[0]) for b in c["threshold_bits"]]), "with a +inf optimum;",
          sum(1 for c in cases if any(p < d + 1 for p, d in zip(c["roc_points"], c["distinct_scores"]))), "with dropped points")


if __name__ == "__main__":
    main()
