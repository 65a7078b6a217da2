"""metrics.EpochMetrics through the kernels of csrc/metrics.hip: the cases of tests/test_epoch_metrics.py (fixture: tests/metrics_cases.py).  Integer
buffers, labels and predictions equal the CPU formulation exactly; probabilities within 1e-6 and the mean loss within 1e-5 of float64; every
``compute`` output within 1e-12 of io.classification_metrics fed the kernel's own stored probabilities.  ``ties257`` crosses the 256-row tile
of the pair kernel (and the 256-row step of the update).  Two runs from ``reset`` leave the same bits; ``update`` and ``reset`` record into a graph."""
import pytest
import torch

import metrics_cases as M

pytestmark = pytest.mark.gpu

CPU = torch.device("cpu")


def _dev():
    return torch.device("cuda", torch.cuda.current_device())


def _metrics(C, capacity, device=None):
    from wsi_hgnn_amd.metrics import EpochMetrics
    return EpochMetrics(C, capacity, _dev() if device is None else device)


def _bits(m):
    n = m.probabilities().shape[0]
    return [m.state.cpu(), m.probs[:n].cpu().view(torch.int32), m.row_labels[:n].cpu(), m.row_preds[:n].cpu()]


@pytest.mark.parametrize("name", ["c2", "c5", "c5_absent", "empty", "ties257"])
def test_kernels_against_the_cpu_formulation_and_the_references(name):
    case = M.cases()[name]
    g = M.feed(_metrics(case["C"], case["capacity"]), case, _dev())
    c = M.feed(_metrics(case["C"], case["capacity"], CPU), case, CPU)
    # cursor, flags, confusion matrix exactly (the fp64 sum: words 2..3, held against float64 below); labels and predictions exactly
    assert torch.equal(g.state[:2].cpu(), c.state[:2]) and torch.equal(g.confusion.cpu(), c.confusion)
    assert torch.equal(g.labels().cpu(), c.labels()) and torch.equal(g.predictions().cpu(), c.predictions())
    block = M.check_against_references(g, case)
    first = _bits(g) + [torch.tensor(block, dtype=torch.float64).view(torch.int64)]
    # a second run from reset(): bit-identical buffers and result block
    M.feed(g.reset(), case, _dev())
    again = _bits(g) + [torch.tensor(g.result_block(), dtype=torch.float64).view(torch.int64)]
    for a, b in zip(first, again):
        assert torch.equal(a, b)


def test_flags_on_the_device():
    dev = _dev()
    m = _metrics(2, 8)
    x = torch.linspace(-9, 9, 18).reshape(9, 2).to(dev)
    y = torch.tensor([0, 1, 0, 1, 1, 0, 1, 0, 1], device=dev)
    m.update(x[:4].contiguous(), y[:4].contiguous())
    m.update(x[4:8].contiguous(), y[4:8].contiguous())
    assert m.compute("binary")["n"] == 8
    before = _bits(m)
    m.update(x[8:].contiguous(), y[8:].contiguous())
    with pytest.raises(RuntimeError, match="capacity"):
        m.compute("binary")
    after = _bits(m)
    assert int(after[0][1]) == 4 and torch.equal(before[0][2:], after[0][2:]) and all(torch.equal(a, b) for a, b in zip(before[1:], after[1:]))
    x = torch.tensor([[1.0, 2.0, 0.5], [0.0, float("nan"), 1.0], [3.0, 1.0, 2.0]], device=dev)
    m = _metrics(3, 8)
    m.update(x, torch.tensor([0, M.IGNORE, 2], device=dev))
    assert m.compute("macro")["n"] == 2
    m.update(x, torch.tensor([0, 1, 2], device=dev))
    with pytest.raises(RuntimeError, match="non-finite"):
        m.compute("macro")
    assert m.probabilities().shape[0] == 4
    m = _metrics(3, 8)
    m.update(x[[0, 2]], torch.tensor([3, 1], device=dev))
    with pytest.raises(RuntimeError, match="label"):
        m.compute("macro")
    assert m.labels().tolist() == [1]


def test_update_and_reset_record_into_a_graph():
    """Three replays of a recorded update accumulate what three eager calls do; a recorded reset zeroes the accumulator."""
    dev = _dev()
    case = M.cases()["c5"]
    x = torch.cat([u[0] for u in case["updates"]])[:12].to(dev)
    y = torch.cat([u[1] for u in case["updates"]])[:12].to(dev)
    eager, rec = _metrics(5, 40), _metrics(5, 40)
    for _ in range(3):
        eager.update(x, y)
    rec.update(x, y)                                          # (dirty: the recorded reset has something to clear)
    torch.cuda.synchronize()
    g_reset, g_update = torch.cuda.CUDAGraph(), torch.cuda.CUDAGraph()
    with torch.cuda.graph(g_reset):
        rec.reset()
    with torch.cuda.graph(g_update):
        rec.update(x, y)
    g_reset.replay()
    assert rec.compute("macro")["n"] == 0
    for _ in range(3):
        g_update.replay()
    for a, b in zip(_bits(eager), _bits(rec)):
        assert torch.equal(a, b)
    assert torch.equal(torch.tensor(eager.result_block(), dtype=torch.float64).view(torch.int64), torch.tensor(rec.result_block(), dtype=torch.float64).view(torch.int64))
    assert rec.compute("macro")["n"] == 3 * int((y != M.IGNORE).sum())
