"""Survivor quotas of augmented batch slots on the GPU: the device fill under quotas (csrc/augment.hip clamps, csrc/slot_aug.hip
reads the final decision and range-checks its scattered stores) against the CPU slot bit for bit - quotas that do not bind and quotas that do -
with the overflow words, the order tables, HGT's derived plan, one step against the eager augmented route and trainer.CapturedSlotStep over two
quota slots against an eager twin.  Helpers: tests/quota_cases.py."""
import pytest
import torch

import quota_cases as Q
import slot_cases as C
from test_batch_slot_augment_gpu import TABLES, _dev, _make, _poison

pytestmark = pytest.mark.gpu

NAMES = ["REF", "HARD", "EDGE_FIRST"]


def _compare(gpu, cpu, idxs, draws, tag):
    from wsi_hgnn_amd import ops
    gpu.load_augmented(idxs, draws)
    cpu.load_augmented(idxs, draws)
    for k in TABLES:
        assert Q.same(gpu.bufs[k], cpu.bufs[k]), (tag, idxs, k)
    assert torch.equal(gpu.bufs["scales"], ops.row_absmax(gpu.bufs["feat"])), (tag, idxs)
    assert gpu.counts() == cpu.counts(), (tag, idxs)
    for k in ("order_dst", "order_src"):
        assert torch.equal(torch.sort(gpu.bufs[k].long()).values.cpu(), torch.arange(gpu.layout.N)), (tag, idxs, k)
    assert gpu.overflows() == cpu.overflows() and gpu.overflow_excess() == cpu.overflow_excess(), (tag, idxs)


@pytest.mark.parametrize("name", NAMES)
def test_device_fill_under_the_bound_quota_equals_the_cpu_slot(name):
    """quota="bound", derived capacities (below the stored counts of every two-slide batch): every table against the CPU quota slot, the same
    two slots refilled after poisoning, big batches before small ones, counters 0-2; no quota binds."""
    from wsi_hgnn_amd.data import BatchSlot
    pipe = Q.pipelines()[name]
    lg, lc = Q.aug_loader(_dev(), pipe), Q.aug_loader("cpu", pipe)
    g, c = BatchSlot(lg, quota="bound"), BatchSlot(lc, quota="bound")
    assert g.layout.n_cap == c.layout.n_cap and g.layout.e_cap == c.layout.e_cap and g.layout.N < sum(C.BIG[0])
    _poison(g)
    for counter in range(3):
        for idxs in C.CASES + [[0, 7]]:
            _compare(g, c, idxs, Q.draws_of(counter, idxs), (name, counter))
        _poison(g)
    assert g.overflows() == 0 and g.overflow_excess() == (0, 0)


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("case", Q.BINDING)
def test_device_fill_under_binding_quotas_equals_the_cpu_slot(name, case):
    """Each binding quota (a callable) on the batch of the two largest slides, two draws, a non-binding fill of another batch in between: tables,
    truncated counts, permutation orders and the overflow words against the CPU slot, whose own test holds them against the contract."""
    from wsi_hgnn_amd.data import BatchSlot
    pipe = Q.pipelines()[name]
    lg, lc = Q.aug_loader(_dev(), pipe), Q.aug_loader("cpu", pipe)
    table = {}
    fn = lambda i: table[i] if i in table else Q.stored_quota(lc, i)
    g, c = BatchSlot(lg, C.BIG, quota=fn), BatchSlot(lc, C.BIG, quota=fn)
    _poison(g)
    fills = 0
    for counter in range(2):
        draws = Q.draws_of(counter, Q.BATCH)
        quotas, xn, xe = Q.binding_quotas(lc, pipe, Q.BATCH, draws, case)
        table.clear(); table.update(quotas); g._quotas.clear(); c._quotas.clear()
        _compare(g, c, Q.BATCH, draws, (name, case, counter))
        fills += int(xn > 0 or xe > 0)
        assert g.overflows() == fills, (name, case, counter)
        _compare(g, c, [2], Q.draws_of(counter, [2]), (name, case, counter, "plain"))
        _poison(g)
    if name == "REF":
        assert fills == 2


def test_the_same_truncated_fill_twice_gives_identical_bytes():
    from wsi_hgnn_amd.data import BatchSlot
    pipe = Q.pipelines()["REF"]
    ld, lc = Q.aug_loader(_dev(), pipe), Q.aug_loader("cpu", pipe)
    d = Q.draws_of(1, Q.BATCH)
    quotas = Q.binding_quotas(lc, pipe, Q.BATCH, d, "both")[0]
    a, b = BatchSlot(ld, C.BIG, quota=Q.quota_fn(lc, quotas)), BatchSlot(ld, C.BIG, quota=Q.quota_fn(lc, quotas))
    _poison(a); _poison(b)
    a.load_augmented(Q.BATCH, d)
    first = {k: a.bufs[k].clone() for k in TABLES + ("scales",)}
    a.load_augmented([2], Q.draws_of(0, [2]))
    a.load_augmented(Q.BATCH, d)
    b.load_augmented(Q.BATCH, d)
    for k, v in first.items():
        assert torch.equal(a.bufs[k].view(torch.uint8), v.view(torch.uint8)) and torch.equal(b.bufs[k].view(torch.uint8), v.view(torch.uint8)), k
    assert a.overflows() == 2 and b.overflows() == 1


def test_truncated_fill_with_narrow_features():
    """in_dim = 50 (the element path of the feature gather) under quotas that bind (a quarter of the stored nodes, an eighth of the edges) and
    under the bound quota with derived capacities."""
    from wsi_hgnn_amd import synthetic
    from wsi_hgnn_amd.data import BatchSlot, GraphBatchLoader
    pipe = Q.pipelines()["REF"]
    gs = [synthetic.hetero_graph(n, 50, seed=940 + i) for i, n in enumerate((150, 90))]
    lg, lc = (GraphBatchLoader(gs, [1, 0], 2, dev, shuffle=False, resident=True, seed=Q.SEED, transform=pipe) for dev in (_dev(), "cpu"))
    tight = lambda i: ([n // 4 for n in Q.stored_quota(lc, i)[0]], [e // 8 for e in Q.stored_quota(lc, i)[1]])
    for quota in (tight, "bound"):
        g, c = BatchSlot(lg, quota=quota), BatchSlot(lc, quota=quota)
        _poison(g)
        for counter, idxs in ((0, [0, 1]), (1, [1]), (2, [1, 0])):
            draws = Q.draws_of(counter, idxs)
            g.load_augmented(idxs, draws); c.load_augmented(idxs, draws)
            for k in TABLES:
                assert Q.same(g.bufs[k], c.bufs[k]), (idxs, k)
            assert g.counts() == c.counts()
        assert g.overflows() == c.overflows() == (3 if quota is tight else 0) and g.overflow_excess() == c.overflow_excess()


def test_hgt_plan_of_a_truncated_slot():
    """per_relation_src=True under a binding quota: the tables the slot re-derives behind the fill equal the tensor formulation over the filled
    tables (their shapes are functions of the capacities, a quota changes none)."""
    from wsi_hgnn_amd import graph as G
    from wsi_hgnn_amd.data import BatchSlot
    pipe = Q.pipelines()["REF"]
    ld, lc = Q.aug_loader(_dev(), pipe), Q.aug_loader("cpu", pipe)
    for case in ("both", "node_zero"):
        d = Q.draws_of(0, Q.BATCH)
        quotas = Q.binding_quotas(lc, pipe, Q.BATCH, d, case)[0]
        slot = BatchSlot(ld, C.BIG, per_relation_src=True, quota=Q.quota_fn(lc, quotas))
        plan = slot.graph.plan(per_relation_src=True)
        for k in ("src", "colptr", "csc_eid", "csc_dst"):
            slot.rel[k].fill_(0x5A5A5A5A)
        slot.load_augmented(Q.BATCH, d)
        assert slot.overflows() == 1
        ref = G.plan_by_relation_torch(slot.layout.hd, slot.graph.plan())
        for k in ("src", "colptr", "csc_eid", "csc_dst"):
            assert getattr(plan, k) is slot.rel[k] and torch.equal(slot.rel[k], getattr(ref, k)), (case, k)
    bound = BatchSlot(ld, per_relation_src=True, quota="bound").load([0, 7])
    ref = G.plan_by_relation_torch(bound.layout.hd, bound.graph.plan())
    for k in ("src", "colptr", "csc_eid", "csc_dst"):
        assert torch.equal(bound.rel[k], getattr(ref, k)), k


@pytest.mark.parametrize("idxs", [[0, 1], [2]])
def test_step_on_the_quota_slot_matches_the_eager_route(idxs):
    """One step's logits, loss and gradients on a quota slot (quota="bound", derived capacities, nothing binds) against the eager augmented
    route under exact fp32 GEMMs, with the tolerance of the augmented slot's own test: 1e-4, gradients relative to their largest entry."""
    from wsi_hgnn_amd import ops
    from wsi_hgnn_amd.data import BatchSlot
    ops.set_gemm_precision("fp32")
    lf = torch.nn.CrossEntropyLoss()
    m, _ = _make()
    pipe = Q.pipelines()["REF"]
    ld, ld2 = Q.aug_loader(_dev(), pipe), Q.aug_loader(_dev(), pipe)
    slot = BatchSlot(ld, quota="bound").load(idxs)
    G, y = ld2._augmented(idxs)
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
    assert set(ga) == set(gb) and slot.overflows() == 0
    for k in ga:
        err, top = (ga[k] - gb[k]).abs().max().item(), ga[k].abs().max().item()
        print(k, err, top)
        assert err <= 1e-4 * top, (k, err, top)


SEQUENCE = [[0, 1], [2], [3, 4], [0, 1], [0, 7], [1, 2], [3, 4]]              # [3, 4]: the small slot; [0, 7]: only a quota slot holds it
WARM = [[2, 6], [3, 4]]                                                       # derived slot, small slot


def _quota_slots(ld):
    from wsi_hgnn_amd.data import BatchSlot
    return BatchSlot(ld, quota="bound"), BatchSlot(ld, C.SMALL, quota="bound")


def _eager_twin(m, o, lf, sequence, base=None):
    """Eager steps on the quota slots' graphs after load with the loader's own draws: the warm-up steps of CapturedSlotStep (small slot first),
    then the sequence."""
    from wsi_hgnn_amd import ops
    ld = Q.aug_loader(_dev(), Q.pipelines()["REF"])
    big, small = _quota_slots(ld)
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
    return losses, ld._batches_drawn


@pytest.mark.parametrize("gemm", ["fp32", "fp16x3"])
def test_captured_step_replays_over_quota_slots(gemm):
    """CapturedSlotStep over two quota slots of different capacity (HEATNet4, hidden 128, eval mode): loss trajectory and final state_dict
    equal the eager twin's bit for bit; every step is a replay, no quota binds."""
    from wsi_hgnn_amd import ops
    from wsi_hgnn_amd.trainer import CapturedSlotStep
    lf = torch.nn.CrossEntropyLoss()
    ops.set_gemm_precision(gemm)
    ops.set_side_column_statistics(gemm == "fp32")
    try:
        m1, o1 = _make(128)
        eager, drawn = _eager_twin(m1, o1, lf, SEQUENCE)
        m2, o2 = _make(128)
        ld = Q.aug_loader(_dev(), Q.pipelines()["REF"])
        step = CapturedSlotStep(m2, o2, lf, list(_quota_slots(ld)), warmup=1, warmup_batches=WARM)
        assert step.slots[0].layout.N < step.slots[1].layout.N < sum(C.BIG[0])
        assert step.slot_for([3, 4]) == 0 and step.slot_for([0, 1]) == 1 and step.slot_for([0, 7]) == 1
        got = []
        for idxs in SEQUENCE:
            loss, logits = step.step(idxs)
            assert logits.shape == (len(idxs), 2)
            got.append(loss.item())
    finally:
        ops.set_gemm_precision("fp32")
        ops.set_side_column_statistics(True)
    assert step.replays == len(SEQUENCE) and step.eager_steps == 0 and step.overflows() == 0
    assert ld._batches_drawn == drawn == 2 + len(SEQUENCE)
    assert got == eager, (got, eager)
    for (k, a), (_, b) in zip(m1.state_dict().items(), m2.state_dict().items()):
        assert torch.equal(a, b), k


def test_captured_step_over_quota_slots_in_training_mode_with_dropout(monkeypatch):
    """feat_drop = 0.2, train mode, as the augmented slot's own test: trajectory and weights equal the eager twin's."""
    from wsi_hgnn_amd import ops
    from wsi_hgnn_amd.trainer import CapturedSlotStep
    lf = torch.nn.CrossEntropyLoss()
    calls = {"n": 0}

    def seeds():                                   # the host seeds of a step: the same two values at every step (what a capture freezes them to)
        calls["n"] += 1
        return 1000 + (calls["n"] % 2)

    monkeypatch.setattr(ops, "next_dropout_seed", seeds)
    m2, o2 = _make(128, 0.2, train=True)
    torch.manual_seed(77)
    ld = Q.aug_loader(_dev(), Q.pipelines()["REF"])
    step = CapturedSlotStep(m2, o2, lf, list(_quota_slots(ld)), warmup=1, warmup_batches=WARM)
    first = int(step.seed_base.item()) - 2 * ops.SEED_STRIDE           # the word before the two warm-up steps
    got = [step.step(idxs)[0].item() for idxs in SEQUENCE]
    assert step.replays == len(SEQUENCE) and step.overflows() == 0
    m1, o1 = _make(128, 0.2, train=True)
    base = torch.tensor([((first + (1 << 31)) % (1 << 32)) - (1 << 31)], dtype=torch.int32, device=_dev())
    eager, _ = _eager_twin(m1, o1, lf, SEQUENCE, base=base)
    assert got == eager, (got, eager)
    for (k, a), (_, b) in zip(m1.state_dict().items(), m2.state_dict().items()):
        assert torch.equal(a, b), k
