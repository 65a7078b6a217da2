"""Augmented slides in padded batch slots on the GPU: the device fill (csrc/slot_aug.hip: draw, scans, layout kernel, push, pull,
feature gather - no read-back) against the CPU tensor route bit for bit, its determinism, one step on the slot against the eager augmented route,
and trainer.CapturedSlotStep replaying over a fresh draw every step against an eager twin.  Fixture: tests/slot_cases.py."""
import pytest
import torch

import slot_cases as C
from test_batch_slot_augment import SEED, aug_loader, draws_of, pipelines, same

pytestmark = pytest.mark.gpu

TABLES = ("rowptr", "colptr", "node_seg", "src", "csc_eid", "csc_dst", "order_dst", "order_src", "sim", "inv_rd", "readout_ptr", "labels", "feat",
          "edge_seg", "row_seg", "chunk_row", "chunk_seg", "seg_chunk", "seg_counts", "seg_inv_counts", "seg_nonempty")


def _dev():
    return torch.device("cuda", torch.cuda.current_device())


def _poison(slot):
    for k in TABLES + ("scales",):
        slot.bufs[k].view(torch.uint8).fill_(0xA5)


def _compare(gpu, cpu, idxs, draws, tag):
    from wsi_hgnn_amd import ops
    gpu.load_augmented(idxs, draws)
    cpu.load_augmented(idxs, draws)
    for k in TABLES:
        assert same(gpu.bufs[k], cpu.bufs[k]), (tag, idxs, k)
    assert torch.equal(gpu.bufs["scales"], ops.row_absmax(gpu.bufs["feat"])), (tag, idxs)
    assert gpu.counts() == cpu.counts(), (tag, idxs)
    assert gpu.num_real == len(idxs) and gpu.labels.tolist()[:len(idxs)] == [C.LABELS[i] for i in idxs]


@pytest.mark.parametrize("name", ["REF", "HARD", "EDGE_FIRST"])
def test_device_fill_equals_the_tensor_route_bit_for_bit(name):
    """Every table of the slot - plan, sim, orders (by the restriction rule), labels, features as bit patterns, the per-edge segment table, the
    readout plan's tables - after the device fill against the CPU slot filled through the tensor formulation with the same draws; the SAME two
    slots again and again after poisoning, big batches before small ones (a stale tail would show), counters 0-2.  HARD goes through
    load_augmented (fits refuses it): a whole node type emptied ([3, 4] and [4] at counter 0: nf = n_cap), a slide without edges ([5, 3] at 1)."""
    from wsi_hgnn_amd.data import BatchSlot
    pipe = pipelines()[name]
    lg, lc = aug_loader(_dev(), pipe), aug_loader("cpu", pipe)
    big, small, cbig, csmall = BatchSlot(lg, C.BIG), BatchSlot(lg, C.SMALL), BatchSlot(lc, C.BIG), BatchSlot(lc, C.SMALL)
    _poison(big); _poison(small)
    seq = [(big, cbig, c, 0) for c in C.CASES] + [(small, csmall, c, 0) for c in C.SMALL_CASES] + [(big, cbig, [0, 1], 1), (big, cbig, [4], 0)]
    seq += [(big, cbig, [5, 3], 1), (big, cbig, [4], 2), (small, csmall, [3, 4], 2), (big, cbig, [2, 6], 2)]
    for g, c, idxs, counter in seq:
        _compare(g, c, idxs, draws_of(counter, idxs), (name, counter))
    if name == "REF":                                          # the public path: load() with explicit and with default draws
        big.load([0, 1], draws=draws_of(2, [0, 1])); cbig.load([0, 1], draws=draws_of(2, [0, 1]))
        assert all(same(big.bufs[k], cbig.bufs[k]) for k in TABLES)
        lg._batches_drawn = lc._batches_drawn = 5
        big.load([2]); cbig.load([2])
        assert big.draws == draws_of(5, [2]) and lg._batches_drawn == 6 and all(same(big.bufs[k], cbig.bufs[k]) for k in TABLES)
        with pytest.raises(RuntimeError, match="device only"):
            big.graph.batch_num_nodes("0")
        with pytest.raises(RuntimeError, match="device only"):
            big.graph.edges(big.graph.canonical_etypes[0])
        assert big.graph.batch_size == 3


def test_device_fill_narrow_features():
    """in_dim = 50: no 16-byte row alignment - the element path of the feature gather."""
    from wsi_hgnn_amd import synthetic
    from wsi_hgnn_amd.data import BatchSlot, GraphBatchLoader
    pipe = pipelines()["REF"]
    gs = [synthetic.hetero_graph(n, 50, seed=940 + i) for i, n in enumerate((150, 90))]
    mk = lambda dev: BatchSlot(GraphBatchLoader(gs, [1, 0], 2, dev, shuffle=False, resident=True, seed=SEED, transform=pipe))
    g, c = mk(_dev()), mk("cpu")
    _poison(g)
    for counter, idxs in ((0, [0, 1]), (1, [1]), (2, [1, 0])):
        _compare_plain(g, c, idxs, draws_of(counter, idxs))


def _compare_plain(gpu, cpu, idxs, draws):
    from wsi_hgnn_amd import ops
    gpu.load_augmented(idxs, draws)
    cpu.load_augmented(idxs, draws)
    for k in TABLES:
        assert same(gpu.bufs[k], cpu.bufs[k]), (idxs, k)
    assert torch.equal(gpu.bufs["scales"], ops.row_absmax(gpu.bufs["feat"])), idxs


def test_the_same_fill_twice_gives_identical_bytes():
    from wsi_hgnn_amd.data import BatchSlot
    pipe = pipelines()["REF"]
    ld = aug_loader(_dev(), pipe)
    a, b = BatchSlot(ld, C.BIG), BatchSlot(ld, C.BIG)
    _poison(a); _poison(b)
    for idxs in ([0, 1], [6, 4]):
        d = draws_of(1, idxs)
        a.load_augmented(idxs, d)
        first = {k: a.bufs[k].clone() for k in TABLES + ("scales",)}
        a.load_augmented([2], draws_of(0, [2]))
        a.load_augmented(idxs, d)
        b.load_augmented(idxs, d)
        for k, v in first.items():
            assert torch.equal(a.bufs[k].view(torch.uint8), v.view(torch.uint8)) and torch.equal(b.bufs[k].view(torch.uint8), v.view(torch.uint8)), (idxs, k)


def _make(hidden=64, drop=0.0, train=False):
    from wsi_hgnn_amd import models
    torch.manual_seed(3)
    m = models.HEATNet4(C.IN_DIM, hidden, 2, 2, 4, C.ND, drop, "mean").to(_dev())
    m = m.train() if train else m.eval()
    return m, torch.optim.Adam(m.parameters(), lr=1e-3, weight_decay=5e-3, capturable=True)


@pytest.mark.parametrize("idxs", [[0, 1], [2]])
def test_step_on_the_augmented_slot_matches_the_eager_route(idxs):
    """One step's logits, loss and gradients on slot.graph against the parent route - graph.batch of the fused REF(slide, draw) - under exact
    fp32 GEMMs: logits and loss within 1e-4, every gradient within 1e-4 of its tensor's largest entry (not bitwise: tile and chunk
    boundaries move with the slot's capacities)."""
    from wsi_hgnn_amd import ops
    from wsi_hgnn_amd.data import BatchSlot
    ops.set_gemm_precision("fp32")
    lf = torch.nn.CrossEntropyLoss()
    m, _ = _make()
    pipe = pipelines()["REF"]
    ld, ld2 = aug_loader(_dev(), pipe), aug_loader(_dev(), pipe)
    slot = BatchSlot(ld, C.BIG).load(idxs)
    G, y = ld2._augmented(idxs)                                # the same counter (0) under the same seed: the same draws
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


SEQUENCE = [[0, 1], [2], [3, 4], [0, 1], [0, 1], [5, 3], [1, 2], [3, 4]]      # [3, 4]: the small slot; [5, 3]: fits no augmented slot (24 nodes of type 2)
WARM = [[2, 6], [3, 4]]                                                       # big slot, small slot


def _eager_twin(m, o, lf, sequence, base=None):
    """Eager steps on slot.graph after load with the loader's own draws: the warm-up steps CapturedSlotStep takes (small slot first), then the
    sequence; a batch that fits no slot through the loader's eager augmented route."""
    from wsi_hgnn_amd import ops
    from wsi_hgnn_amd.data import BatchSlot
    ld = aug_loader(_dev(), pipelines()["REF"])
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
        slot = small if small.fits(idxs) else (big if big.fits(idxs) else None)
        if slot is None:
            losses.append(one(*ld._augmented(idxs)))
        else:
            slot.load(idxs)
            losses.append(one(slot.graph, slot.labels))
    return losses, ld._batches_drawn


@pytest.mark.parametrize("gemm", ["fp32", "fp16x3"])
def test_captured_step_replays_over_a_fresh_draw_every_step(gemm):
    """CapturedSlotStep over augmented BIG + SMALL (HEATNet4, hidden 128, eval mode): batches for both slots, a repeated batch, one batch no slot
    fits.  Loss trajectory and final state_dict equal the eager twin's bit for bit; both advanced the loader's batch counter once per step."""
    from wsi_hgnn_amd import ops
    from wsi_hgnn_amd.data import BatchSlot
    from wsi_hgnn_amd.trainer import CapturedSlotStep
    lf = torch.nn.CrossEntropyLoss()
    ops.set_gemm_precision(gemm)
    ops.set_side_column_statistics(gemm == "fp32")
    try:
        m1, o1 = _make(128)
        eager, drawn = _eager_twin(m1, o1, lf, SEQUENCE)
        m2, o2 = _make(128)
        ld = aug_loader(_dev(), pipelines()["REF"])
        step = CapturedSlotStep(m2, o2, lf, [BatchSlot(ld, C.BIG), BatchSlot(ld, C.SMALL)], warmup=1, warmup_batches=WARM)
        assert step.slot_for([3, 4]) == 0 and step.slot_for([0, 1]) == 1 and step.slot_for([5, 3]) is None
        got = []
        for idxs in SEQUENCE:
            loss, logits = step.step(idxs)
            assert logits.shape == (len(idxs), 2)
            got.append(loss.item())
    finally:
        ops.set_gemm_precision("fp32")
        ops.set_side_column_statistics(True)
    assert step.replays == len(SEQUENCE) - 1 and step.eager_steps == 1
    assert ld._batches_drawn == drawn == 2 + len(SEQUENCE)
    assert got == eager, (got, eager)
    assert got[3] != got[4]                                    # the repeated batch [0, 1]: another draw (and another model) every time
    for (k, a), (_, b) in zip(m1.state_dict().items(), m2.state_dict().items()):
        assert torch.equal(a, b), k


def test_captured_step_in_training_mode_with_dropout(monkeypatch):
    """feat_drop = 0.2, train mode: the captures share one device word for the dropout draw and every replay fills its slot with a new
    augmentation draw in front; trajectory and weights equal the eager twin's."""
    from wsi_hgnn_amd import ops
    from wsi_hgnn_amd.data import BatchSlot
    from wsi_hgnn_amd.trainer import CapturedSlotStep
    lf = torch.nn.CrossEntropyLoss()
    calls = {"n": 0}

    def seeds():                                   # the host seeds of a step: the same two values at every step (what a capture freezes them to)
        calls["n"] += 1
        return 1000 + (calls["n"] % 2)

    monkeypatch.setattr(ops, "next_dropout_seed", seeds)
    m2, o2 = _make(128, 0.2, train=True)
    torch.manual_seed(77)
    ld = aug_loader(_dev(), pipelines()["REF"])
    step = CapturedSlotStep(m2, o2, lf, [BatchSlot(ld, C.BIG), BatchSlot(ld, C.SMALL)], warmup=1, warmup_batches=WARM)
    first = int(step.seed_base.item()) - 2 * ops.SEED_STRIDE           # the word before the two warm-up steps
    seq = [s for s in SEQUENCE if s != [5, 3]]                         # (the eager route draws host seeds of its own; the replayed steps are what is compared)
    got = [step.step(idxs)[0].item() for idxs in seq]
    m1, o1 = _make(128, 0.2, train=True)
    base = torch.tensor([((first + (1 << 31)) % (1 << 32)) - (1 << 31)], dtype=torch.int32, device=_dev())
    eager, _ = _eager_twin(m1, o1, lf, seq, base=base)
    assert got == eager, (got, eager)
    for (k, a), (_, b) in zip(m1.state_dict().items(), m2.state_dict().items()):
        assert torch.equal(a, b), k


def test_refusals_stay():
    from wsi_hgnn_amd import models
    from wsi_hgnn_amd.data import BatchSlot
    from wsi_hgnn_amd.trainer import CapturedSlotStep
    lf = torch.nn.CrossEntropyLoss()
    slot = BatchSlot(aug_loader(_dev(), pipelines()["REF"]), C.BIG)
    ed = {r: i for i, r in enumerate(slot.layout.rels)}
    hgt = models.HGT(C.ND, ed, C.IN_DIM, 64, 2, 2, 4, graph_pooling_type="mean").to(_dev())
    with pytest.raises(RuntimeError, match="HGT"):
        CapturedSlotStep(hgt, torch.optim.Adam(hgt.parameters(), lr=1e-3, capturable=True), lf, slot)
    m = models.HEATNet4(C.IN_DIM, 64, 2, 2, 4, C.ND, 0.0, "att").to(_dev())
    with pytest.raises(RuntimeError, match="attention readout"):
        CapturedSlotStep(m, torch.optim.Adam(m.parameters(), lr=1e-3, capturable=True), lf, slot)
    m, _ = _make()
    with pytest.raises(RuntimeError, match="capturable"):
        CapturedSlotStep(m, torch.optim.Adam(m.parameters(), lr=1e-3), lf, slot)
    m, o = _make(drop=0.2, train=True)
    m.gcs[0].counter_dropout = False
    with pytest.raises(RuntimeError, match="dropout"):
        CapturedSlotStep(m, o, lf, slot)
