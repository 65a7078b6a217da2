"""trainer.CapturedSlotEval and CapturedSlotStep(metrics=) on the GPU: the recorded forward against eager no-grad forwards on the
slots' own graphs bit for bit, a whole evaluation pass against io.classification_metrics over logits collected here, the recorded forward
following the live parameters (exact fp32 and packed fp16x3 weights), and a training capture with metrics beside an evaluation capture on one
model.  Fixture: tests/slot_cases.py."""
import contextlib
import math

import pytest
import torch

import metrics_cases as M
import slot_cases as C

pytestmark = pytest.mark.gpu

CONFIGS = [("HEATNet2", 64, "fp32", False), ("HEATNet4", 64, "fp32", False), ("HEATNet4", 128, "fp16x3", True)]
EXPLICIT = [[2, 6], [3, 4], [5, 1], C.NO_FIT]              # all 8 slides once: three replays ([3, 4] in the small slot), one eager run
SEQUENCE = [[0, 1], [2], [3, 4], [5, 3], [1, 2], [6, 4]]
WARM = [[2, 6], [4]]


def _dev():
    return torch.device("cuda", torch.cuda.current_device())


@pytest.fixture(scope="module")
def ld():
    return C.loader(_dev())


@contextlib.contextmanager
def _switches(gemm, collapse):
    from wsi_hgnn_amd import ops
    ops.set_gemm_precision(gemm)
    if collapse:
        ops.set_value_collapse(True, min_work=0.0)
    try:
        yield
    finally:
        ops.set_gemm_precision("fp32")
        ops.set_value_collapse(True, min_work=4.0e9)


def _make(name="HEATNet4", hidden=64, readout="mean"):
    from wsi_hgnn_amd import models
    torch.manual_seed(3)
    return getattr(models, name)(C.IN_DIM, hidden, 2, 2, 4, C.ND, 0.0, readout).to(_dev()).eval()


def _slots(ld):
    from wsi_hgnn_amd.data import BatchSlot
    return [BatchSlot(ld, C.BIG), BatchSlot(ld, C.SMALL)]


@torch.no_grad()
def _eager_logits(ld, m, twins, idxs):
    """An eager no-grad forward of the batch the way CapturedSlotEval routes it: on the smallest twin slot that fits, else on the loader's batch."""
    big, small = twins
    slot = small if small.fits(idxs) else (big if big.fits(idxs) else None)
    if slot is None:
        G, _, _ = ld._assemble(idxs, 0)
        return m(G).clone()
    slot.load(idxs)
    return m(slot.graph)[:len(idxs)].clone()


def _expected(logits, labels, average):
    """The numbers of io.evaluate's keys over collected logits: float64 softmax into io.classification_metrics, float64 loss, exact accuracy."""
    from wsi_hgnn_amd import io
    x = logits.double().cpu()
    y = torch.tensor(labels)
    p, r, f, a = io.classification_metrics(torch.softmax(x, dim=1), y, average)
    return {"loss": torch.nn.functional.cross_entropy(x, y).item(), "accuracy": (x.argmax(1) == y).double().mean().item(),
            "precision": p, "recall": r, "f1": f, "auc": a, "n": len(labels)}


def _agree(got, want):
    print(got, want)
    assert got["n"] == want["n"] and M.close(got["loss"], want["loss"], M.LOSS_TOL)
    for k in ("accuracy", "precision", "recall", "f1", "auc"):
        assert M.close(got[k], want[k], M.EXACT_TOL), (k, got[k], want[k])


@pytest.mark.parametrize("name,hidden,gemm,collapse", CONFIGS)
def test_run_replays_the_eager_forward_bit_for_bit(ld, name, hidden, gemm, collapse):
    """(a) the logits of ``run`` equal an eager no-grad forward on a slot's own graph after the same load, bit for bit; under exact fp32 they lie
    within 1e-4 of the loader's unpadded batch (tile and chunk boundaries move with the capacities: not bitwise)."""
    from wsi_hgnn_amd.trainer import CapturedSlotEval
    with _switches(gemm, collapse):
        m = _make(name, hidden)
        ev = CapturedSlotEval(m, _slots(ld))
        twins = _slots(ld)
        assert not m.training and ev.metrics.capacity == 8 and ev.metrics.num_classes == 2
        for idxs in ([0, 1], [2], [3, 4], [5, 3], [4], [0, 1]):
            got = ev.run(idxs).clone()
            ref = _eager_logits(ld, m, twins, idxs)
            assert got.shape == (len(idxs), 2) and torch.equal(got, ref), idxs
            if gemm == "fp32":
                with torch.no_grad():
                    G, _, _ = ld._assemble(idxs, 0)
                    err = (m(G) - got).abs().max().item()
                print(idxs, "padded against unpadded", err)
                assert err <= 1e-4
        assert ev.replays == 6 and ev.eager_runs == 0
        assert ev.slot_for([3, 4]) == 0 and ev.slot_for([0, 1]) == 1 and ev.slot_for(C.NO_FIT) is None


@pytest.mark.parametrize("name,hidden,gemm,collapse", CONFIGS)
def test_evaluate_equals_the_metrics_of_collected_logits(ld, name, hidden, gemm, collapse):
    """(b) a pass over the default batches and one over explicit batches with a batch no slot fits: the result equals io.classification_metrics,
    accuracy and a float64 loss over logits collected by eager forwards here; no row of a filler or an empty graph counts; the counters and the
    model's training flag are as expected."""
    from wsi_hgnn_amd.trainer import CapturedSlotEval
    with _switches(gemm, collapse):
        m = _make(name, hidden).train()
        ev = CapturedSlotEval(m, _slots(ld))
        assert m.training
        twins = _slots(ld)
        m.eval()
        default = [[0, 1], [2, 3], [4, 5], [6, 7]]
        assert ev.batches() == default
        collected = {tuple(b): _eager_logits(ld, m, twins, b) for b in default + EXPLICIT}
        m.train()
        for batches, replays, eager_runs in ((None, 4, 0), (EXPLICIT, 3, 1)):
            order = default if batches is None else batches
            logits = torch.cat([collected[tuple(b)] for b in order])
            labels = [C.LABELS[i] for b in order for i in b]
            before = (ev.replays, ev.eager_runs)
            for average in ("binary", "macro"):
                got = ev.evaluate(batches, average)
                assert got["n"] == 8
                _agree(got, _expected(logits, labels, average))
            assert (ev.replays - before[0], ev.eager_runs - before[1]) == (2 * replays, 2 * eager_runs)
            assert ev.metrics.labels().tolist() == labels
        assert m.training


@pytest.mark.parametrize("name,hidden,gemm,collapse", CONFIGS[1:])
def test_recorded_forward_follows_the_live_parameters(ld, name, hidden, gemm, collapse):
    """(c) evaluate, one optimizer step on the model, evaluate again: the second result equals a fresh eager evaluation of the stepped model (its
    logits bit for bit) and differs from the first - under exact fp32 and under fp16x3, whose recorded projections pack their own weights."""
    from wsi_hgnn_amd.trainer import CapturedSlotEval
    with _switches(gemm, collapse):
        m = _make(name, hidden)
        ev = CapturedSlotEval(m, _slots(ld))
        twins = _slots(ld)
        first = ev.evaluate(EXPLICIT, "macro")
        first_logits = ev.run([2, 6]).clone()
        opt = torch.optim.SGD(m.parameters(), lr=0.05)
        G, y, _ = ld._assemble([0, 1], 0)
        torch.nn.functional.cross_entropy(m(G), y).backward()
        opt.step()
        opt.zero_grad(set_to_none=True)
        second = ev.evaluate(EXPLICIT, "macro")
        collected = [_eager_logits(ld, m, twins, b) for b in EXPLICIT]
        _agree(second, _expected(torch.cat(collected), [C.LABELS[i] for b in EXPLICIT for i in b], "macro"))
        for b, ref in zip(EXPLICIT, collected):
            assert torch.equal(ev.run(b), ref), b
        assert second["loss"] != first["loss"] and not torch.equal(first_logits, collected[0])


def test_training_capture_with_metrics_beside_an_evaluation_capture(ld):
    """(d) a CapturedSlotStep with ``metrics=`` and a CapturedSlotEval interleaved on one model: the loss trajectory and the final state_dict equal
    those of the run without any metrics, bit for bit; the training metrics equal io.classification_metrics over the collected logits."""
    from wsi_hgnn_amd.metrics import EpochMetrics
    from wsi_hgnn_amd.trainer import CapturedSlotEval, CapturedSlotStep
    lf = torch.nn.CrossEntropyLoss()

    def make():
        m = _make("HEATNet4", 64)
        return m, torch.optim.Adam(m.parameters(), lr=1e-3, weight_decay=5e-3, capturable=True)

    m1, o1 = make()
    plain = CapturedSlotStep(m1, o1, lf, _slots(ld), warmup=1, warmup_batches=WARM)
    want = [plain.step(idxs)[0].item() for idxs in SEQUENCE + [C.NO_FIT]]
    m2, o2 = make()
    tm = EpochMetrics(2, 32, _dev())
    step = CapturedSlotStep(m2, o2, lf, _slots(ld), warmup=1, warmup_batches=WARM, metrics=tm)
    assert tm.compute("binary")["n"] == 3                   # the warm-up steps are steps: [4] and [2, 6]
    ev = CapturedSlotEval(m2, _slots(ld))
    tm.reset()
    got, logits, evals = [], [], []
    for k, idxs in enumerate(SEQUENCE + [C.NO_FIT]):
        loss, pred = step.step(idxs)
        got.append(loss.item())
        logits.append(pred.clone())
        if k % 2 == 1:
            evals.append(ev.evaluate()["loss"])
    assert got == want, (got, want)
    for (k, a), (_, b) in zip(m1.state_dict().items(), m2.state_dict().items()):
        assert torch.equal(a, b), k
    labels = [C.LABELS[i] for b in SEQUENCE + [C.NO_FIT] for i in b]
    for average in ("binary", "macro"):
        _agree(tm.compute(average), _expected(torch.cat(logits), labels, average))
    assert step.replays == 6 and step.eager_steps == 1 and ev.metrics.compute()["n"] == 8
    assert len(set(evals)) == 3 and all(math.isfinite(v) for v in evals)      # the evaluation saw the model move


def test_unsupported_setups_are_refused(ld):
    """(e) HGT, the attention readout, a slot over a loader with a transform."""
    from wsi_hgnn_amd import models, transforms as T
    from wsi_hgnn_amd.data import BatchSlot, GraphBatchLoader
    from wsi_hgnn_amd.trainer import CapturedSlotEval
    slot = BatchSlot(ld, C.BIG)
    ed = {r: i for i, r in enumerate(slot.layout.rels)}
    hgt = models.HGT(C.ND, ed, C.IN_DIM, 64, 2, 2, 4, graph_pooling_type="mean").to(_dev())
    with pytest.raises(RuntimeError, match="HGT"):
        CapturedSlotEval(hgt, slot)
    with pytest.raises(RuntimeError, match="att"):
        CapturedSlotEval(_make("HEATNet4", 64, "att"), slot)
    aug = GraphBatchLoader(C.slides(), C.LABELS, 2, _dev(), shuffle=False, resident=True, transform=T.Compose([T.DropEdge(0.2)]))
    with pytest.raises(RuntimeError, match="transform"):
        CapturedSlotEval(_make("HEATNet4", 64), BatchSlot(aug, C.BIG))
