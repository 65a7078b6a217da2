"""``mil.CapturedBagEval`` on the GPU: an epoch replayed over two bag slots against an eager twin that runs the same forward over slots of its own
without capture - the whole result block and the stored scores bit-equal -, the stored scores against ``mil.evaluate`` on the unpadded bags
(error <= 1e-4 x the largest float64 entry: the bound of tests/test_bag_slot_gpu.py), a second epoch, the eager batch, the training flag, what it
refuses, and an evaluation after ``CapturedBagStep`` steps on the same model: the parameters are read in place."""
import pytest
import torch

import bag_slot_cases as BC

pytestmark = pytest.mark.gpu

DEV = "cuda"
TOL = 1e-4
C = 2
SIZES = (5, 40, 17, 120, 300, 64, 9, 250, 90)
LABELS = (0, 1, 1, 0, 1, 0, 2, 0, 1)                      # (2: past the last class - an all-zero target row)
# batches of 1, 3 and 2 bags: the second fills the small slot's three bags, the third leaves a bag of the large slot unused, the last fits no slot
BATCHES = ((0,), (1, 2, 6), (3, 5), (8,), (4, 7))
MODELS = (("dsmil", 22), ("dsmil", 64), ("abmil", 22), ("abmil", 64))


def _make(model, feats, seed, dropout=0.0):
    from wsi_hgnn_amd.mil import abmil, dsmil
    torch.manual_seed(seed)
    if model == "dsmil":
        m = dsmil.MILNet(dsmil.FCLayer(feats, C), dsmil.BClassifier(feats, C, dropout_v=dropout))
    else:
        m = abmil.BClassifier(feats, C)
    with torch.no_grad():                                  # (sharper than the initialisation: scores spread over (0, 1))
        for p in m.parameters():
            p.mul_(2.5)
    return m.to(DEV)


def _slots(feats):
    from wsi_hgnn_amd import mil
    return [mil.BagSlot(feats, 400, 3, num_classes=C, device=DEV), mil.BagSlot(feats, 128, 3, num_classes=C, device=DEV)]     # (largest first: sorted)


def _data(feats, seed=30):
    bags = BC.make_bags(SIZES, feats, seed, DEV)
    return bags, [([bags[i] for i in ix], [LABELS[i] for i in ix]) for ix in BATCHES]


def _warm(feats):
    return [(BC.make_bags((200,), feats, 91, DEV), [1]), (BC.make_bags((50, 20), feats, 92, DEV), [0, 1])]


def _twin_epoch(m, feats):
    """What ``CapturedBagEval.run_epoch`` does, eagerly, on slots and an accumulator of its own."""
    from wsi_hgnn_amd import mil
    from wsi_hgnn_amd.mil import metrics as M
    slots = sorted(_slots(feats), key=lambda s: s.row_cap)
    acc = mil.BagEpochMetrics(C, M.MAX_ROWS, DEV)
    was = m.training
    m.eval()
    with torch.no_grad():
        for bags, labels in _data(feats)[1]:
            sizes = [int(t.shape[0]) for t in bags]
            slot = next((s for s in slots if s.fits(sizes)), None)
            if slot is not None:
                slot.load(bags, labels)
                M.forward_update(m, slot.rows, slot.plan, slot.targets, slot.weights, acc)
            else:
                w = torch.ones(len(bags), device=DEV)
                M.forward_update(m, torch.cat(list(bags)), mil.bag_plan(sizes, DEV), mil.bag_targets(labels, C, DEV).contiguous(), w, acc)
    m.train(was)
    acc.result_block()
    return acc


@pytest.mark.parametrize("model,feats", MODELS)
def test_captured_epoch_equals_the_eager_twin(model, feats):
    from wsi_hgnn_amd import mil
    m = _make(model, feats, 60 + feats, dropout=0.25 if (model, feats) == ("dsmil", 22) else 0.0)     # (eval mode: a Dropout is the identity)
    m.train()
    cap = mil.CapturedBagEval(m, _slots(feats), warmup_batches=_warm(feats))
    assert m.training and [s.row_cap for s in cap.slots] == [128, 400]
    assert int(cap.metrics.state[0]) == 0                                  # (the warm-up rows were reset)
    bags, batches = _data(feats)
    got = cap.run_epoch(batches)
    assert m.training                                                      # the flag is restored
    assert cap.replays == 4 and cap.eager_batches == 1 and got["n"] == len(SIZES)
    s = cap.metrics.scores()
    assert 0.0 < float(s.min()) and float(s.max()) < 1.0 and len(torch.unique(s)) == s.numel()      # (no saturated and no repeated score)
    twin = _twin_epoch(m, feats)
    assert torch.equal(cap.metrics.result, twin.result)
    assert torch.equal(cap.metrics.scores().view(torch.int32), twin.scores().view(torch.int32))
    assert torch.equal(cap.metrics.state, twin.state)
    # against the eager evaluation of the unpadded bags, in the order the batches took them
    order = [i for ix in BATCHES for i in ix]
    acc = mil.BagEpochMetrics(C, len(SIZES), DEV)
    ref = mil.evaluate(m, [bags[i] for i in order], [LABELS[i] for i in order], metrics=acc, batch_size=4)
    want = acc.scores().double()
    err = float((cap.metrics.scores().double() - want).abs().max())
    print(f"{model} feats {feats}: scores error / bound {err / (TOL * float(want.abs().max())):.3e}")
    assert err <= TOL * float(want.abs().max())
    assert torch.equal(cap.metrics.targets(), acc.targets()) and ref["n"] == got["n"]
    assert abs(ref["loss"] - got["loss"]) <= TOL * abs(ref["loss"])
    # a second epoch reproduces the first bit for bit
    first = cap.metrics.result.clone()
    again = cap.run_epoch(batches)
    assert torch.equal(cap.metrics.result, first) and again == got
    assert cap.replays == 8 and cap.eager_batches == 2
    m.eval()
    cap.run_epoch(batches)
    assert not m.training


@pytest.mark.parametrize("model,feats", [("dsmil", 64), ("abmil", 22)])
def test_evaluation_sees_the_weights_a_captured_step_wrote(model, feats):
    from wsi_hgnn_amd import mil, optim
    m = _make(model, feats, 80 + feats)
    cap = mil.CapturedBagEval(m, _slots(feats), warmup_batches=_warm(feats))
    bags, batches = _data(feats)
    cap.run_epoch(batches)
    before = cap.metrics.result.clone()
    opt = optim.Adam(m.parameters(), lr=5e-3, betas=(0.5, 0.9), weight_decay=5e-3, capturable=True)
    step = mil.CapturedBagStep(m, opt, [mil.BagSlot(feats, 400, 3, num_classes=C, device=DEV)], warmup_batches=[_warm(feats)[0]])
    for b, l in batches[:4]:
        step.step(b, l)
    assert step.replays == 4
    cap.run_epoch(batches)
    assert not torch.equal(cap.metrics.scores(), torch.zeros_like(cap.metrics.scores()))
    assert not torch.equal(cap.metrics.result, before)                     # the replay read the stepped parameters
    twin = _twin_epoch(m, feats)
    assert torch.equal(cap.metrics.result, twin.result) and torch.equal(cap.metrics.scores().view(torch.int32), twin.scores().view(torch.int32))


def test_refusals():
    from wsi_hgnn_amd import mil
    m = _make("abmil", 22, 3)
    with pytest.raises(ValueError, match="dropout_patch"):
        mil.CapturedBagEval(m, mil.BagSlot(22, 100, 1, num_classes=C, device=DEV, dropout_patch=0.25))
    with pytest.raises(ValueError, match="no batch to warm up"):
        mil.CapturedBagEval(m, mil.BagSlot(22, 100, 1, num_classes=C, device=DEV))
    with pytest.raises(RuntimeError, match="GPU"):
        mil.CapturedBagEval(m, mil.BagSlot(22, 100, 1, num_classes=C, device="cpu"))
    with pytest.raises(RuntimeError, match="not supported"):
        mil.CapturedBagEval(torch.nn.Linear(22, C).to(DEV), mil.BagSlot(22, 100, 1, num_classes=C, device=DEV))
    with pytest.raises(ValueError, match="no slot"):
        mil.CapturedBagEval(m, [])
    with pytest.raises(RuntimeError, match="classes"):
        mil.CapturedBagEval(m, mil.BagSlot(22, 100, 1, num_classes=C, device=DEV), metrics=mil.BagEpochMetrics(3, 16, DEV))
