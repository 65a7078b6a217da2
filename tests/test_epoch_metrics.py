"""metrics.EpochMetrics on the CPU (the tensor formulation of wsi_metrics_update / wsi_metrics_finalize, the fixture the kernels are compared
with): against io.classification_metrics fed the accumulator's own stored probabilities - confusion-derived numbers and AUCs within 1e-12, both
sides being exact integer or half-integer counts until one fp64 division - and against a float64 softmax / cross entropy computed here:
probabilities within 1e-6, mean loss within 1e-5 (a few fp32 roundings of values bounded by 1 and by about 13).  Fixture: tests/metrics_cases.py."""
import math

import pytest
import torch

import metrics_cases as M

CPU = torch.device("cpu")


def _metrics(C, capacity):
    from wsi_hgnn_amd.metrics import EpochMetrics
    return EpochMetrics(C, capacity, CPU)


@pytest.mark.parametrize("name", ["c2", "c5", "c5_absent", "empty", "ties257"])
def test_tensor_formulation_against_classification_metrics_and_float64(name):
    case = M.cases()[name]
    m = M.feed(_metrics(case["C"], case["capacity"]), case, CPU)
    block = M.check_against_references(m, case)
    if name == "c5_absent":                                 # a class that never occurs: its AUC and the macro AUC are NaN, the rest finite
        macro = m.compute("macro")
        assert math.isnan(macro["auc"]) and math.isnan(block[12 + 4 * 4 + 3])
        assert all(math.isfinite(macro[k]) for k in ("loss", "accuracy", "precision", "recall", "f1"))
        assert all(math.isfinite(block[12 + 4 * c + 3]) for c in range(4))
    if name == "c5":
        assert math.isfinite(m.compute("macro")["auc"])
    if name == "c2":                                        # the fixture holds what it promises: tied scores between the classes, equal maxima
        x, y = M.counted_rows(case)
        assert int((x[:, 0] == x[:, 1]).sum()) >= 3
        s = m.probabilities()[:, 1]
        assert any(float(a) == float(b) for a in s[y == 1] for b in s[y == 0])
    # compute does not reset; reset does
    assert m.compute("macro")["n"] == len(M.counted_rows(case)[1])
    assert m.reset().compute("binary")["n"] == 0 and int(m.confusion.sum()) == 0


def test_overflow_drops_the_row_and_raises():
    m = _metrics(2, 8)
    x = torch.linspace(-9, 9, 18).reshape(9, 2)
    y = torch.tensor([0, 1, 0, 1, 1, 0, 1, 0, 1])
    m.update(x[:4], y[:4])
    m.update(x[4:8], y[4:8])
    assert m.compute("binary")["n"] == 8
    before = (m.probs.clone(), m.row_labels.clone(), m.row_preds.clone(), m.confusion.clone(), m._loss_sum.clone())
    m.update(x[8:], y[8:])                                   # the 9th counted row
    with pytest.raises(RuntimeError, match="capacity"):
        m.compute("binary")
    assert m.probabilities().shape[0] == 8 and int(m.confusion.sum()) == 8
    for a, b in zip(before, (m.probs, m.row_labels, m.row_preds, m.confusion, m._loss_sum)):
        assert torch.equal(a, b)


def test_bad_label_and_non_finite_logits_raise_but_not_in_an_ignored_row():
    x = torch.tensor([[1.0, 2.0, 0.5], [0.0, float("nan"), 1.0], [3.0, 1.0, 2.0]])
    m = _metrics(3, 8)
    m.update(x, torch.tensor([0, M.IGNORE, 2]))              # the NaN sits in a -100 row: not looked at
    assert m.compute("macro")["n"] == 2
    m.update(x, torch.tensor([0, 1, 2]))                     # the same NaN in a counted row: skipped, flagged
    with pytest.raises(RuntimeError, match="non-finite"):
        m.compute("macro")
    assert m.probabilities().shape[0] == 4
    m = _metrics(3, 8)
    m.update(x[[0, 2]], torch.tensor([3, 1]))                # a label of C
    with pytest.raises(RuntimeError, match="label"):
        m.compute("macro")
    assert m.probabilities().shape[0] == 1 and m.labels().tolist() == [1]
    m = _metrics(3, 8)
    m.update(x[[0, 2]], torch.tensor([-1, 1]))
    with pytest.raises(RuntimeError, match="label"):
        m.compute("binary")


def test_arguments_are_checked():
    from wsi_hgnn_amd.metrics import EpochMetrics
    with pytest.raises(ValueError):
        EpochMetrics(33, 4, CPU)
    m = _metrics(2, 4)
    with pytest.raises(ValueError):
        m.update(torch.zeros(2, 3), torch.zeros(2, dtype=torch.int64))
    with pytest.raises(ValueError):
        m.update(torch.zeros(2, 2), torch.zeros(2, dtype=torch.int32))
    with pytest.raises(ValueError):
        m.compute("micro")
