"""GIN over padded batch slots without a GPU, float64 through the slot's tensor-formulation fill: the model on a slot graph
whose filler holds more rows than the real slides against the same model on the loader's unpadded batch - the BatchNorms must not see the
filler - the two-live-rows rule of ``CapturedSlotStep.slot_for``, and what ``_check_slots`` admits and refuses.  Slides: tests/gin_slot_cases.py."""
import copy

import pytest
import torch

import gin_slot_cases as S

BATCHES = [[0], [0, 5], [2, 3]]


@pytest.fixture(scope="module")
def homo():
    from wsi_hgnn_amd.data import BatchSlot
    ld = S.loader("cpu")
    return ld, BatchSlot(ld, S.WIDE)


def _run(m, graph, labels, train):
    m.train(train)
    m.zero_grad(set_to_none=True)
    logits = m(graph, graph.ndata["feat"].double())
    logits.retain_grad()
    loss = torch.nn.CrossEntropyLoss()(logits, labels)
    loss.backward()
    grads = {k: (None if p.grad is None else p.grad.clone()) for k, p in m.named_parameters()}
    stats = {k: v.clone() for k, v in m.state_dict().items() if "running_" in k or k.endswith("num_batches_tracked")}
    return logits, loss.detach().clone(), grads, stats


@pytest.mark.parametrize("train", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("idxs", BATCHES)
@pytest.mark.parametrize("neighbor,readout", S.SETTINGS)
def test_the_filler_enters_no_statistic_no_logit_and_no_gradient(homo, neighbor, readout, idxs, train):
    """Bound: 1e-12 of the largest entry of each tensor - both runs add the same float64 numbers, the padded one with exact zeros (dead rows,
    the filler's readout segment) in between.  The filler's graph and the empty ones carry label -100, so the gradient that reaches their
    logits is exactly zero.  On a tree whose BatchNorms run over all rows of the slot's table this fails: the filler, most of the table,
    enters every mean, variance and running statistic."""
    ld, slot = homo
    slot.load(idxs)
    lay = slot.layout
    assert lay.N - sum(S.SIZES[i] for i in idxs) > sum(S.SIZES[i] for i in idxs)       # the filler holds more rows than the real slides
    G, y, _ = ld._assemble(idxs, 0)
    ma = S.model(neighbor, readout, True).double()
    mb = copy.deepcopy(ma)
    la, lossa, ga, sa = _run(ma, G, y, train)
    lb, lossb, gb, sb = _run(mb, slot.graph, slot.labels, train)
    rel = lambda a, b: (a - b).abs().max().item() / max(b.abs().max().item(), 1e-300)
    B = len(idxs)
    assert lb.shape == (lay.graphs, S.CLASSES) and torch.isfinite(lb).all()
    assert rel(lb.detach()[:B], la.detach()) <= 1e-12 and rel(lossb, lossa) <= 1e-12
    assert not lb.grad[B:].any() and lb.grad[:B].any()
    for k, a in ga.items():
        b = gb[k]
        assert (a is None) == (b is None), k
        if a is None:
            continue
        if S.cancelling(k, train):
            # 0 in exact arithmetic: rounding noise, held against the scale of the same Linear's weight gradient
            top = ga[k[:-4] + "weight"].abs().max().item()
            assert top > 0 and (b - a).abs().max().item() <= 1e-12 * top, k
        elif a.abs().max() > 0:
            assert rel(b, a) <= 1e-12, k
        else:
            assert not b.any(), k
    assert set(sa) == set(sb) and len(sa) == 6                   # two BatchNorms: the MLP's hidden one and ApplyNodeFunc's
    for k, a in sa.items():
        if k.endswith("num_batches_tracked"):
            assert int(a) == int(sb[k]) == (1 if train else 0), k
        else:
            assert rel(sb[k], a) <= 1e-12, k
    if train:
        assert any(rel(v, S.model(neighbor, readout, True).state_dict()[k].double()) > 1e-3 for k, v in sa.items() if "running_" in k)


def _bare_step(slots, gnn):
    """``CapturedSlotStep`` as far as ``slot_for`` reads it (the class itself needs a GPU to capture on)."""
    from wsi_hgnn_amd.models import GIN
    from wsi_hgnn_amd.trainer import CapturedSlotStep
    step = CapturedSlotStep.__new__(CapturedSlotStep)
    step.slots, step.gnn, step.two_rows = list(slots), gnn, type(gnn) is GIN
    return step


def test_slot_for_keeps_two_live_rows_for_gin_in_train_mode():
    from wsi_hgnn_amd import models
    from wsi_hgnn_amd.data import BatchSlot
    from wsi_hgnn_amd.trainer import two_live_rows
    gin = S.model("mean", "att", True)
    plain = BatchSlot(S.loader("cpu"), S.WIDE)
    step = _bare_step([plain], gin.train())
    assert plain.fits([S.ONE]) and not two_live_rows(plain, [S.ONE]) and step.slot_for([S.ONE]) is None       # n = 1
    assert step.slot_for([S.ONE, 0]) == 0 and step.slot_for([0]) == 0 and step.slot_for([S.N37]) == 0
    assert _bare_step([plain], gin.eval()).slot_for([S.ONE]) == 0                                             # eval mode normalises with the running statistics
    gcn = models.GCN(S.IN_DIM, 8, 2, 2, torch.nn.functional.relu, 0.0, "mean").train()
    assert _bare_step([plain], gcn).slot_for([S.ONE]) == 0                                                    # the rule is GIN's
    # augmented, node drop probability 0.5: (n + 1) / 2^n <= 2^-32 from n = 38 on
    aug = BatchSlot(S.loader("cpu", augment=True), S.WIDE)
    assert aug.spec.node_thr == 32768
    step = _bare_step([aug], gin.train())
    assert aug.fits([S.N37]) and aug.fits([S.N38])
    assert not two_live_rows(aug, [S.N37]) and two_live_rows(aug, [S.N38])
    assert step.slot_for([S.N37]) is None and step.slot_for([S.N38]) == 0 and step.slot_for([S.N37, S.ONE]) == 0
    assert 38 * 0.5 ** 37 > 2.0 ** -32 >= 39 * 0.5 ** 38
    # quotas: the node quotas must leave two rows as well
    ld = S.loader("cpu", augment=True)
    tight = BatchSlot(ld, S.WIDE, quota=lambda i: ([1 if i == 1 else S.SIZES[i]], [5 * S.SIZES[i]]))
    assert tight.fits([1]) and not two_live_rows(tight, [1]) and two_live_rows(tight, [1, 3]) and two_live_rows(tight, [3])


def test_slot_checks_admit_gin_over_homogeneous_slots_only(homo):
    """``_check_slots`` up to the device test (CPU slots)."""
    import slot_cases as C
    from wsi_hgnn_amd.data import BatchSlot
    from wsi_hgnn_amd.trainer import _check_slots
    ld, slot = homo
    for neighbor, readout in S.SETTINGS:
        for learn in (True, False):
            with pytest.raises(RuntimeError, match="on the GPU"):                      # everything before the device test passed
                _check_slots("t", "step", S.model(neighbor, readout, learn), slot)
    gin = S.model("mean", "att", True)
    with pytest.raises(RuntimeError, match="GIN needs homogeneous slots"):
        _check_slots("t", "step", gin, BatchSlot(C.loader("cpu"), C.BIG))
    with pytest.raises(ValueError, match="type_mask"):
        _check_slots("t", "evaluate", gin, BatchSlot(ld, S.WIDE, type_mask=True))
    with pytest.raises(RuntimeError, match="GCN / GIN over homogeneous slots"):
        _check_slots("t", "step", torch.nn.Linear(2, 2), slot)


def test_gin_is_counter_based_for_the_capture_protocol():
    from wsi_hgnn_amd import capture
    from wsi_hgnn_amd.models import GIN
    m = S.model("sum", "sum", False, dropout=0.2).train()
    assert capture.counter_dropout_only("Who", m, (GIN,)) is True
    with pytest.raises(RuntimeError, match="outside"):
        capture.counter_dropout_only("Who", m, (torch.nn.Linear,))
