"""Padded batch slots on the GPU: the fill kernel (csrc/slot.hip) against graph.slot_fill_torch bit for bit, and one captured step
per slot (trainer.CapturedSlotStep) replayed over new slides against eager steps on the same slots.  Fixture: tests/slot_cases.py."""
import pytest
import torch

import slot_cases as C

pytestmark = pytest.mark.gpu


def _dev():
    return torch.device("cuda", torch.cuda.current_device())


@pytest.fixture(scope="module")
def ld():
    return C.loader(_dev())


def _reference(slot, ld, idxs):
    from wsi_hgnn_amd import graph as G
    its = [ld.items[i] for i in idxs]
    T = slot.layout.T
    return G.slot_fill_torch(slot.layout, [it.pieces for it in its], [it.label for it in its], [it.feat for it in its],
                             [[it.feat_scale(t) for t in range(T)] for it in its], _dev())


def test_slot_fill_kernel_equals_the_tensor_operations_bit_for_bit(ld):
    """wsi_slot_fill against graph.slot_fill_torch on every case - plan tables, sim, orders, labels, features, row scales, the per-edge segment
    table and the readout plan's tables - filling the SAME slots again and again, big batches before small ones (a stale tail would show).  The
    filler's parts are closed forms in the kernel and sorts in the reference."""
    from wsi_hgnn_amd import ops
    from wsi_hgnn_amd.data import BatchSlot
    big, small = BatchSlot(ld, C.BIG), BatchSlot(ld, C.SMALL)
    for bufs in (big.bufs, small.bufs):
        for v in bufs.values():                              # poison: every element must be written by every fill
            v.view(torch.uint8).fill_(0xA5)
    for slot, idxs in [(big, c) for c in C.CASES] + [(small, c) for c in C.SMALL_CASES] + [(big, [0, 1]), (big, [4])]:
        slot.load(idxs)
        ref = _reference(slot, ld, idxs)
        for k, v in ref.items():
            if k != "batch":
                got = slot.bufs[k]
                assert got.dtype == v.dtype and got.shape == v.shape, (idxs, k)
                assert torch.equal(got.view(torch.int32) if got.dtype == torch.float32 else got, v.view(torch.int32) if v.dtype == torch.float32 else v), (idxs, k)
        assert torch.equal(slot.bufs["scales"], ops.row_absmax(slot.bufs["feat"])), idxs      # a valid scale on every row, the zero rows included
        assert slot.num_real == len(idxs) and slot.labels.tolist()[:len(idxs)] == [C.LABELS[i] for i in idxs]


def _make(name="HEATNet4", hidden=64, drop=0.0, train=False):
    from wsi_hgnn_amd import models
    torch.manual_seed(3)
    m = getattr(models, name)(C.IN_DIM, hidden, 2, 2, 4, C.ND, drop, "mean").to(_dev())
    m = m.train() if train else m.eval()
    return m, torch.optim.Adam(m.parameters(), lr=1e-3, weight_decay=5e-3, capturable=True)


SEQUENCE = [[0, 1], [2], [3, 4], [5, 3], [1, 2], [6, 4]]          # [3, 4] goes to the small slot
WARM = [[2, 6], [4]]                                               # big slot, small slot


def _eager_twin(ld, m, o, lf, sequence, base=None, extra=None):
    """Eager steps on slot.graph after load: the warm-up steps CapturedSlotStep takes (small slot first), then the sequence."""
    from wsi_hgnn_amd import ops
    from wsi_hgnn_amd.data import BatchSlot
    big, small = BatchSlot(ld, C.BIG), BatchSlot(ld, C.SMALL)
    losses = []

    def one(G, y):
        o.zero_grad(set_to_none=True)
        with ops.dropout_seed_base(base):
            l = lf(m(G), y)
            l.backward()
        o.step()
        if base is not None:
            ops.advance_dropout_seed_base(base)
        return l.item()

    for slot, idxs in ((small, WARM[1]), (big, WARM[0])):
        slot.load(idxs)
        one(slot.graph, slot.labels)
    for idxs in sequence:
        slot = small if small.fits(idxs) else big
        slot.load(idxs)
        losses.append(one(slot.graph, slot.labels))
    if extra is not None:
        G, y, ready = ld._assemble(extra, 0)
        losses.append(one(G, y))
    return losses


@pytest.mark.parametrize("name,hidden,gemm,collapse", [("HEATNet2", 64, "fp32", False), ("HEATNet4", 64, "fp32", False),
                                                        ("HEATNet4", 128, "fp32", True), ("HEATNet4", 128, "fp16x3", True)])
def test_captured_slot_step_replays_the_eager_trajectory_over_new_batches(ld, name, hidden, gemm, collapse):
    """Six different batches through two captured slots (one batch goes to the small one), then a batch that fits neither: the loss trajectory
    and the final state_dict equal those of eager steps on the slots' graphs, bit for bit; the no-fit batch took the loader's eager path.
    ``collapse``: the last layer's value-collapse path at this small size (it reads the per-edge segment table, which the fill rewrites);
    fp16x3: the scaled GEMMs, which read the features' row scales and column statistics the slot keeps current (column statistics in line in
    both twins: a capture cannot use the statistics stream)."""
    from wsi_hgnn_amd import ops
    from wsi_hgnn_amd.data import BatchSlot
    from wsi_hgnn_amd.trainer import CapturedSlotStep
    lf = torch.nn.CrossEntropyLoss()
    ops.set_gemm_precision(gemm)
    ops.set_side_column_statistics(gemm == "fp32")
    if collapse:
        ops.set_value_collapse(True, min_work=0.0)
    try:
        m1, o1 = _make(name, hidden)
        eager = _eager_twin(ld, m1, o1, lf, SEQUENCE, extra=C.NO_FIT)
        m2, o2 = _make(name, hidden)
        step = CapturedSlotStep(m2, o2, lf, [BatchSlot(ld, C.BIG), BatchSlot(ld, C.SMALL)], warmup=1, warmup_batches=WARM)
        assert [s.layout.N for s in step.slots] == [sum(C.SMALL[0]), sum(C.BIG[0])]
        got = []
        for idxs in SEQUENCE:
            loss, logits = step.step(idxs)
            assert logits.shape == (len(idxs), 2)
            got.append(loss.item())
        assert step.slot_for([3, 4]) == 0 and step.slot_for([0, 1]) == 1 and step.slot_for(C.NO_FIT) is None
        loss, logits = step.step(C.NO_FIT)
        got.append(loss.item())
    finally:
        ops.set_gemm_precision("fp32")
        ops.set_side_column_statistics(True)
        ops.set_value_collapse(True, min_work=4.0e9)
    assert step.replays == 6 and step.eager_steps == 1 and logits.shape == (2, 2)
    assert got == eager, (got, eager)
    assert len(set(got)) == len(got)
    for (k, a), (_, b) in zip(m1.state_dict().items(), m2.state_dict().items()):
        assert torch.equal(a, b), k


def test_captured_slot_step_in_training_mode_with_dropout(ld, monkeypatch):
    """The reference's training configuration (feat_drop = 0.2, train mode): the slots' captures share ONE device word, every replay of either
    slot advances it, and the trajectory equals eager steps that draw through the same word with the same host seeds."""
    from wsi_hgnn_amd import ops
    from wsi_hgnn_amd.data import BatchSlot
    from wsi_hgnn_amd.trainer import CapturedSlotStep
    lf = torch.nn.CrossEntropyLoss()
    calls = {"n": 0}

    def seeds():                                   # the host seeds of a step: the same two values at every step (what a capture freezes them to)
        calls["n"] += 1
        return 1000 + (calls["n"] % 2)

    monkeypatch.setattr(ops, "next_dropout_seed", seeds)
    m2, o2 = _make("HEATNet4", 128, 0.2, train=True)
    torch.manual_seed(77)
    step = CapturedSlotStep(m2, o2, lf, [BatchSlot(ld, C.BIG), BatchSlot(ld, C.SMALL)], warmup=1, warmup_batches=WARM)
    first = int(step.seed_base.item()) - 2 * ops.SEED_STRIDE           # the word before the two warm-up steps
    got = [step.step(idxs)[0].item() for idxs in SEQUENCE]
    assert (int(step.seed_base.item()) - first - 8 * ops.SEED_STRIDE) % (1 << 32) == 0
    m1, o1 = _make("HEATNet4", 128, 0.2, train=True)
    base = torch.tensor([((first + (1 << 31)) % (1 << 32)) - (1 << 31)], dtype=torch.int32, device=_dev())
    eager = _eager_twin(ld, m1, o1, lf, SEQUENCE, base=base)
    assert got == eager, (got, eager)
    for (k, a), (_, b) in zip(m1.state_dict().items(), m2.state_dict().items()):
        assert torch.equal(a, b), k


@pytest.mark.parametrize("idxs", [[0, 1], [2], [5, 3]])
def test_padded_step_matches_the_unpadded_batch(ld, idxs):
    """One step's logits, loss and gradients on slot.graph against the loader's ordinary batch of the same slides, under exact fp32 GEMMs: logits
    and loss within 1e-4, every gradient within 1e-4 of the tensor's largest entry.  Not bitwise: tile and chunk boundaries move with
    the slot's capacities, so sums associate differently."""
    from wsi_hgnn_amd import ops
    from wsi_hgnn_amd.data import BatchSlot
    ops.set_gemm_precision("fp32")
    lf = torch.nn.CrossEntropyLoss()
    m, _ = _make("HEATNet4")
    slot = BatchSlot(ld, C.BIG).load(idxs)
    G, y, _ = ld._assemble(idxs, 0)
    res = []
    for graph, lab in ((G, y), (slot.graph, slot.labels)):
        m.zero_grad(set_to_none=True)
        logits = m(graph)
        loss = lf(logits, lab)
        loss.backward()
        res.append((logits.detach()[:len(idxs)].clone(), loss.item(), {k: p.grad.clone() for k, p in m.named_parameters() if p.grad is not None}))
    (la, lossa, ga), (lb, lossb, gb) = res
    print("logits", (la - lb).abs().max().item(), "loss", abs(lossa - lossb))
    assert (la - lb).abs().max().item() <= 1e-4 and abs(lossa - lossb) <= 1e-4
    assert set(ga) == set(gb)
    for k in ga:
        err, top = (ga[k] - gb[k]).abs().max().item(), ga[k].abs().max().item()
        print(k, err, top)
        assert err <= 1e-4 * top, (k, err, top)


def test_hgt_and_uncapturable_setups_are_refused(ld):
    from wsi_hgnn_amd import models
    from wsi_hgnn_amd.data import BatchSlot
    from wsi_hgnn_amd.trainer import CapturedSlotStep
    lf = torch.nn.CrossEntropyLoss()
    slot = BatchSlot(ld, C.BIG)
    ed = {r: i for i, r in enumerate(slot.layout.rels)}
    hgt = models.HGT(C.ND, ed, C.IN_DIM, 64, 2, 2, 4, graph_pooling_type="mean").to(_dev())
    with pytest.raises(RuntimeError, match="HGT"):
        CapturedSlotStep(hgt, torch.optim.Adam(hgt.parameters(), lr=1e-3, capturable=True), lf, slot)
    m, _ = _make("HEATNet4")
    with pytest.raises(RuntimeError, match="capturable"):
        CapturedSlotStep(m, torch.optim.Adam(m.parameters(), lr=1e-3), lf, slot)
    m, o = _make("HEATNet4", drop=0.2, train=True)
    m.gcs[0].counter_dropout = False
    with pytest.raises(RuntimeError, match="dropout"):
        CapturedSlotStep(m, o, lf, slot)
