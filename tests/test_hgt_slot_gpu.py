"""HGT in captured batch slots on the GPU: the per-relation-source plan derived on the device for loader batches and re-derived by
a slot behind every fill; trainer.CapturedSlotStep / CapturedSlotEval over ``BatchSlot(..., per_relation_src=True)`` against eager twins on the
slots' own graphs, bit for bit; padded against unpadded batches by the project's 1e-4 rule.  Fixture: tests/slot_cases.py, exact fp32 GEMMs."""
import pytest
import torch

import slot_cases as C
from test_batch_slot_augment import aug_loader, pipelines

pytestmark = pytest.mark.gpu

# hidden 40 = 4 heads x 10: padded per head to 32 (models.HGT.padded_head_dim, the path of the reference's hidden 200); hidden 128 with LayerNorm
CONFIGS = [(40, False), (128, True)]
SEQUENCE = [[0, 1], [2], [3, 4], [5, 3], [1, 2], [6, 4]]          # [3, 4] goes to the small slot
WARM = [[2, 6], [4]]                                               # big slot, small slot


def _dev():
    return torch.device("cuda", torch.cuda.current_device())


@pytest.fixture(scope="module")
def ld():
    from wsi_hgnn_amd import ops
    ops.set_gemm_precision("fp32")
    return C.loader(_dev())


def _make(ld, hidden, use_norm, train=False, readout="mean", cls="HGT"):
    from wsi_hgnn_amd import models
    rels = ld.items[0].rels
    ed = {tuple(r): i for i, r in enumerate(rels)}
    torch.manual_seed(3)
    m = getattr(models, cls)(C.ND, ed, C.IN_DIM, hidden, 2, 2, 4, use_norm=use_norm, graph_pooling_type=readout).to(_dev())
    m = m.train() if train else m.eval()
    return m, torch.optim.Adam(m.parameters(), lr=1e-3, weight_decay=5e-3, capturable=True)


def _slots(loader):
    from wsi_hgnn_amd.data import BatchSlot
    return [BatchSlot(loader, C.BIG, per_relation_src=True), BatchSlot(loader, C.SMALL, per_relation_src=True)]


def _eager_twin(loader, m, o, lf, sequence, base=None, warm=WARM):
    """Eager steps on slot.graph after load: the warm-up steps CapturedSlotStep takes (small slot first), then the sequence."""
    from wsi_hgnn_amd import ops
    big, small = _slots(loader)
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

    for slot, idxs in ((small, warm[1]), (big, warm[0])):
        slot.load(idxs)
        one(slot.graph, slot.labels)
    for idxs in sequence:
        slot = small if small.fits(idxs) else big
        slot.load(idxs)
        losses.append(one(slot.graph, slot.labels))
    return losses


def _same_state(m1, m2):
    for (k, a), (_, b) in zip(m1.state_dict().items(), m2.state_dict().items()):
        assert torch.equal(a, b), k


@pytest.mark.parametrize("hidden,use_norm", CONFIGS)
def test_loader_batch_on_the_derived_plan_equals_the_plan_built_from_coo(ld, monkeypatch, hidden, use_norm):
    """(a) table for table; HGT's logits and every gradient on the two plans bit for bit (batches without hub destinations: there the hub
    prefix an assembled plan carries and the one ``finish_plan`` picks select the same kernels)."""
    from wsi_hgnn_amd import graph as G
    lf = torch.nn.CrossEntropyLoss()
    m, _ = _make(ld, hidden, use_norm)
    for idxs in ([0, 1], [2], [5, 3], [6, 4]):
        res = []
        for derive in (True, False):
            monkeypatch.setattr(G, "DERIVE_REL_PLAN", derive)
            batch, y, _ = ld._assemble(idxs, 0)
            plan = batch.plan(per_relation_src=True)
            assert (batch._edges_store is None) == derive
            res.append((batch, y, plan))
        (g1, y, p1), (g2, _, p2) = res
        for k in ("rowptr", "src", "colptr", "csc_eid", "csc_dst", "order_src"):
            assert torch.equal(getattr(p1, k), getattr(p2, k)), (idxs, k)
        assert p1.num_src_rows == p2.num_src_rows and p1.rel_rows == p2.rel_rows and p1.num_edges == p2.num_edges
        base = g1.plan()
        assert p1.order_dst is base.order_dst and p1.num_heavy == base.num_heavy
        if idxs == [6, 4]:
            continue
        assert p1.num_heavy == p2.num_heavy == 0
        out = []
        for g in (g1, g2):
            m.zero_grad(set_to_none=True)
            logits = m(g)
            lf(logits, y).backward()
            out.append((logits.detach().clone(), {k: p.grad.clone() for k, p in m.named_parameters() if p.grad is not None}))
        assert torch.equal(out[0][0], out[1][0]), idxs
        assert set(out[0][1]) == set(out[1][1]) and len(out[0][1]) > 10
        for k in out[0][1]:
            assert torch.equal(out[0][1][k], out[1][1][k]), (idxs, k)


@pytest.mark.parametrize("hidden,use_norm", CONFIGS)
def test_captured_slot_step_replays_the_eager_trajectory_over_new_batches(ld, hidden, use_norm):
    """(b) six different batches through two captured slots: the loss of every step and the final state_dict equal those of eager steps on the
    slots' own graphs, bit for bit; a batch no slot fits takes the loader's eager path (on the derived plan)."""
    from wsi_hgnn_amd.trainer import CapturedSlotStep
    lf = torch.nn.CrossEntropyLoss()
    m1, o1 = _make(ld, hidden, use_norm)
    eager = _eager_twin(ld, m1, o1, lf, SEQUENCE)
    m2, o2 = _make(ld, hidden, use_norm)
    step = CapturedSlotStep(m2, o2, lf, _slots(ld), warmup=1, warmup_batches=WARM)
    got = []
    for idxs in SEQUENCE:
        loss, logits = step.step(idxs)
        assert logits.shape == (len(idxs), 2)
        got.append(loss.item())
    assert step.replays == 6 and step.eager_steps == 0
    assert got == eager, (got, eager)
    assert len(set(got)) == len(got)
    _same_state(m1, m2)
    loss, logits = step.step(C.NO_FIT)
    assert step.eager_steps == 1 and logits.shape == (2, 2) and bool(torch.isfinite(loss))


def test_layer_mask_under_a_seed_base_is_the_specified_draw(ld):
    """The kernel's mask for the layer against ``ops.dropout_keep_mask``; another value of the device word gives another mask."""
    from wsi_hgnn_amd import ops
    m, _ = _make(ld, 40, False, train=True)
    layer = m.gcs[0]
    h = torch.randn(333, 40, device=_dev())
    base = torch.tensor([-77], dtype=torch.int32, device=_dev())
    torch.manual_seed(11)
    seed = ops.next_dropout_seed()
    torch.manual_seed(11)
    with ops.dropout_seed_base(base):
        mask = layer._dropout_mask(h)
        want = ops.dropout_keep_mask(ops.CounterDropout(0.2, seed, base), 333, 40, _dev()).to(torch.float32) * 1.25
        assert torch.equal(mask, want)
        ops.advance_dropout_seed_base(base)
        torch.manual_seed(11)
        assert not torch.equal(layer._dropout_mask(h), mask)


def test_captured_slot_step_in_training_mode_with_dropout(ld, monkeypatch):
    """(b) train mode, the layer's dropout 0.2: the captures share ONE device word that every replay advances, so a replay draws masks no
    earlier one drew; the trajectory equals eager steps that draw through the same word with the same host seed - forward and backward of a
    step share one mask in both.  The same batch twice in a row gives two different losses."""
    from wsi_hgnn_amd import ops
    from wsi_hgnn_amd.trainer import CapturedSlotStep
    lf = torch.nn.CrossEntropyLoss()
    monkeypatch.setattr(ops, "next_dropout_seed", lambda: 1000)       # the host seed of every step: what a capture freezes it to
    seq = SEQUENCE + [[6, 4]]
    m2, o2 = _make(ld, 128, True, train=True)
    step = CapturedSlotStep(m2, o2, lf, _slots(ld), warmup=1, warmup_batches=WARM)
    first = int(step.seed_base.item()) - 2 * ops.SEED_STRIDE           # the word before the two warm-up steps
    got = [step.step(idxs)[0].item() for idxs in seq]
    assert (int(step.seed_base.item()) - first - (2 + len(seq)) * ops.SEED_STRIDE) % (1 << 32) == 0
    assert got[-1] != got[-2]
    m1, o1 = _make(ld, 128, True, train=True)
    base = torch.tensor([((first + (1 << 31)) % (1 << 32)) - (1 << 31)], dtype=torch.int32, device=_dev())
    eager = _eager_twin(ld, m1, o1, lf, seq, base=base)
    assert got == eager, (got, eager)
    _same_state(m1, m2)


@pytest.mark.parametrize("hidden,use_norm", CONFIGS)
@pytest.mark.parametrize("idxs", [[0, 1], [2], [5, 3]])
def test_padded_step_matches_the_unpadded_batch(ld, hidden, use_norm, idxs):
    """(c) logits, loss and gradients on slot.graph against the loader's ordinary batch of the same slides: logits and loss within 1e-4, every
    gradient within 1e-4 of the tensor's largest entry (not bitwise: tile and chunk boundaries move with the capacities)."""
    from wsi_hgnn_amd.data import BatchSlot
    lf = torch.nn.CrossEntropyLoss()
    m, _ = _make(ld, hidden, use_norm)
    slot = BatchSlot(ld, C.BIG, per_relation_src=True).load(idxs)
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


def test_captured_step_over_an_augmented_slot(ld):
    """(d) slots over a loader with the reference's training transform: every step fills its slot with a fresh draw taken on the device, the
    slot re-derives HGT's plan behind it, the replay equals the eager twin on the slot graph under the same draws."""
    from wsi_hgnn_amd.trainer import CapturedSlotStep
    lf = torch.nn.CrossEntropyLoss()
    seq = [[0, 1], [2], [3, 4], [0, 1], [1, 2], [3, 4]]               # batches an augmented slot takes (enough nodes of every type)
    warm = [[2, 6], [3, 4]]
    m1, o1 = _make(ld, 128, True)
    l1 = aug_loader(_dev(), pipelines()["REF"])
    eager = _eager_twin(l1, m1, o1, lf, seq, warm=warm)
    m2, o2 = _make(ld, 128, True)
    l2 = aug_loader(_dev(), pipelines()["REF"])
    step = CapturedSlotStep(m2, o2, lf, _slots(l2), warmup=1, warmup_batches=warm)
    got = [step.step(idxs)[0].item() for idxs in seq]
    assert step.replays == len(seq) and step.eager_steps == 0 and l1._batches_drawn == l2._batches_drawn == 2 + len(seq)
    assert got == eager, (got, eager)
    assert got[0] != got[3]                                            # the repeated batch [0, 1]: another draw, another model
    _same_state(m1, m2)


@pytest.mark.parametrize("hidden,use_norm", CONFIGS)
def test_captured_slot_eval_gives_the_metrics_of_io_evaluate(ld, hidden, use_norm):
    """(e) ``CapturedSlotEval.evaluate`` over the default batches against ``io.evaluate`` over the same loader.  Replayed logits equal eager
    forwards on twin slots bit for bit; against the loader's unpadded batches they move by at most 1e-4 (the padded-batch rule), so the loss
    agrees within 2e-4 (cross entropy moves by at most twice the largest logit change) and the counts behind accuracy, precision, recall, F1
    and the binary AUC are equal as long as no slide's two logits lie closer than 2e-4 - asserted."""
    from wsi_hgnn_amd import io
    from wsi_hgnn_amd.trainer import CapturedSlotEval
    m, _ = _make(ld, hidden, use_norm)
    ev = CapturedSlotEval(m, _slots(ld))
    big, small = _slots(ld)
    rows = []
    for idxs in ev.batches():
        got = ev.run(idxs).clone()
        slot = (small if small.fits(idxs) else big).load(idxs)
        with torch.no_grad():
            assert torch.equal(got, m(slot.graph)[:len(idxs)]), idxs
        rows.append(got)
    logits = torch.cat(rows)
    assert float((logits[:, 0] - logits[:, 1]).abs().min()) > 2e-4
    got = ev.evaluate()
    want = io.evaluate(m, ld)
    print(got, want)
    assert got["n"] == 8 and ev.eager_runs == 0
    assert abs(got["loss"] - want["loss"]) <= 2e-4
    for k in ("accuracy", "precision", "recall", "f1", "auc"):
        assert abs(got[k] - want[k]) <= 1e-12, (k, got[k], want[k])


def test_refusals_that_stay(ld):
    """(f) HGT on a default slot, on a mix of slots, HGT + ASAP, HeteroRGCN and the attention readout."""
    from wsi_hgnn_amd import models
    from wsi_hgnn_amd.data import BatchSlot
    from wsi_hgnn_amd.trainer import CapturedSlotEval, CapturedSlotStep
    lf = torch.nn.CrossEntropyLoss()
    plain, rel = BatchSlot(ld, C.BIG), BatchSlot(ld, C.BIG, per_relation_src=True)
    assert plain.rel is None and "_plan_rel" not in plain.graph.__dict__ and rel.graph.plan(per_relation_src=True).num_src_rows == rel.layout.hd.rel_rows_total
    adam = lambda m: torch.optim.Adam(m.parameters(), lr=1e-3, capturable=True)
    hgt, _ = _make(ld, 40, False)
    for slots in (plain, [rel, plain]):
        with pytest.raises(RuntimeError, match="HGT.*per_relation_src=True"):
            CapturedSlotStep(hgt, adam(hgt), lf, slots)
        with pytest.raises(RuntimeError, match="HGT.*per_relation_src=True"):
            CapturedSlotEval(hgt, slots)
    ed = {tuple(r): i for i, r in enumerate(ld.items[0].rels)}
    torch.manual_seed(3)
    asap = models.HGTASAP(C.ND, ed, C.IN_DIM, 64, 2, 2, 4).to(_dev())
    rgcn = models.HeteroRGCN(C.IN_DIM, 64, 2, 2, {r: str(i) for r, i in ed.items()}, C.ND).to(_dev())
    for m in (asap, rgcn):
        with pytest.raises(RuntimeError, match="not supported"):
            CapturedSlotStep(m, adam(m), lf, rel)
    att, _ = _make(ld, 40, False, readout="att")
    with pytest.raises(RuntimeError, match="attention readout"):
        CapturedSlotStep(att, adam(att), lf, rel)
    with pytest.raises(RuntimeError, match="attention readout"):
        CapturedSlotEval(att, rel)
