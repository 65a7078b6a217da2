"""GIN in captured batch slots on the GPU: trainer.CapturedSlotStep / CapturedSlotEval over GIN - every neighbour reducer, a
sum / attention / mean readout, eps learned and fixed - against an eager twin stepping on the same padded slot graphs, bit for bit, and
against eager steps on the loader's unpadded batches by the 1e-4 rule of tests/test_att_slot_gpu.py; an augmented slot whose live count
changes between fills; a batch under the two-live-rows rule; the BatchNorm + ReLU fusion against the composite.  Slides: tests/gin_slot_cases.py
(40-90 nodes, in_dim 16, hidden 8, 2 layers, 2-layer MLPs), exact fp32 GEMMs."""
import pytest
import torch

import gin_slot_cases as S

pytestmark = pytest.mark.gpu

WARM = [5, 3]
SEQUENCE = [[0, 1], [2], [0, 1]]              # three steps over two different batches
LR, WD = 1e-3, 5e-3


def _dev():
    return torch.device("cuda", torch.cuda.current_device())


@pytest.fixture(scope="module")
def ld():
    from wsi_hgnn_amd import ops
    ops.set_gemm_precision("fp32")
    return S.loader(_dev())


def _make(neighbor, readout, learn, train):
    from wsi_hgnn_amd import optim
    m = S.model(neighbor, readout, learn, dropout=0.2).to(_dev())
    m.train(train)
    return m, optim.Adam(m.parameters(), lr=LR, weight_decay=WD, capturable=True)


def _eager(m, o, batches):
    """Eager optimisation steps on ``batches`` (an iterable of (graph, labels, real graphs)): per step (loss, the real slides' logits)."""
    lf, out = torch.nn.CrossEntropyLoss(), []
    for graph, labels, B in batches:
        o.zero_grad(set_to_none=True)
        logits = m(graph)
        loss = lf(logits, labels)
        loss.backward()
        o.step()
        out.append((loss.item(), logits.detach()[:B].clone()))
    return out


def _padded(ld, sequence):
    from wsi_hgnn_amd.data import BatchSlot
    slot = BatchSlot(ld, S.WIDE)
    for idxs in sequence:
        slot.load(idxs)
        yield slot.graph, slot.labels, len(idxs)


def _unpadded(ld, sequence):
    for idxs in sequence:
        G, y, _ = ld._assemble(idxs, 0)
        yield G, y, len(idxs)


@pytest.mark.parametrize("learn", [True, False], ids=["eps learned", "eps fixed"])
@pytest.mark.parametrize("neighbor,readout", S.SETTINGS)
def test_captured_slot_step_replays_the_eager_trajectory(ld, neighbor, readout, learn):
    """Train mode, ``optim.Adam(capturable=True)``, dropout 0.2 (with two layers GIN draws none: the module is there, and the step carries
    its seed word).  Bit for bit against the twin on the padded graphs: losses, logits, gradients of the last step and the whole state.
    Against eager steps on the unpadded batches: logits and loss within 1e-4, every gradient within 1e-4 of the tensor's largest entry (the
    exactly-cancelling biases - tests/gin_slot_cases.py: cancelling - against their weight's gradient), running statistics and parameters
    after the steps within 1e-4 of the tensor's largest entry.  (The weight decay keeps Adam's step of a bias whose own gradient is rounding
    noise well defined: what it normalises is wd * b, not the noise.)"""
    from wsi_hgnn_amd.data import BatchSlot
    from wsi_hgnn_amd.trainer import CapturedSlotStep
    m1, o1 = _make(neighbor, readout, learn, True)
    twin = _eager(m1, o1, _padded(ld, [WARM] + SEQUENCE))[1:]
    m2, o2 = _make(neighbor, readout, learn, True)
    step = CapturedSlotStep(m2, o2, torch.nn.CrossEntropyLoss(), BatchSlot(ld, S.WIDE), warmup=1, warmup_batches=[WARM])
    assert step.seed_base is not None
    got = []
    for idxs in SEQUENCE:
        loss, logits = step.step(idxs)
        assert logits.shape == (len(idxs), S.CLASSES)
        got.append((loss.item(), logits.clone()))
    assert step.replays == 3 and step.eager_steps == 0
    assert [a for a, _ in got] == [a for a, _ in twin] and len({a for a, _ in got}) == 3
    assert all(torch.equal(a, b) for (_, a), (_, b) in zip(got, twin))
    for (k, a), (_, b) in zip(m1.state_dict().items(), m2.state_dict().items()):
        assert torch.equal(a, b), k
    for (k, p), (_, q) in zip(m1.named_parameters(), m2.named_parameters()):
        assert (p.grad is None) == (q.grad is None) and (p.grad is None or torch.equal(p.grad, q.grad)), k
    assert int(m2.state_dict()["layers.0.apply_func.bn.num_batches_tracked"]) == 4
    if learn:
        assert m2.layers[0].eps.grad is not None and abs(m2.layers[0].eps.item() - 0.3) > 1e-4         # eps is stepped

    m3, o3 = _make(neighbor, readout, learn, True)
    plain = _eager(m3, o3, _unpadded(ld, [WARM] + SEQUENCE))[1:]
    for (la, za), (lb, zb) in zip(plain, twin):
        print("loss", abs(la - lb), "logits", (za - zb).abs().max().item())
        assert abs(la - lb) <= 1e-4 and (za - zb).abs().max().item() <= 1e-4
    ga = {k: p.grad for k, p in m3.named_parameters() if p.grad is not None}
    gb = {k: p.grad for k, p in m1.named_parameters() if p.grad is not None}
    assert set(ga) == set(gb)
    for k in ga:
        top = ga[k[:-4] + "weight" if S.cancelling(k, True) else k].abs().max().item()
        err = (ga[k] - gb[k]).abs().max().item()
        print("grad", k, err, top)
        assert err <= 1e-4 * top, (k, err, top)
    sa, sb = m3.state_dict(), m1.state_dict()
    for k in sa:
        if k.endswith("num_batches_tracked"):
            assert int(sa[k]) == int(sb[k]) == 4
            continue
        err, top = (sa[k] - sb[k]).abs().max().item(), sa[k].abs().max().item()
        print("state", k, err, top)
        assert err <= 1e-4 * top, (k, err, top)


@pytest.mark.parametrize("neighbor,readout", S.SETTINGS)
def test_captured_slot_eval_replays_the_eager_forward(ld, neighbor, readout):
    """Replayed logits equal the eager no-grad forward on a twin slot bit for bit, and the unpadded batch's within 1e-4: eval-mode BatchNorm +
    ReLU from the running statistics, the filler's rows written as zeros."""
    from wsi_hgnn_amd.data import BatchSlot
    from wsi_hgnn_amd.trainer import CapturedSlotEval
    m, _ = _make(neighbor, readout, True, False)
    ev = CapturedSlotEval(m, BatchSlot(ld, S.WIDE))
    twin = BatchSlot(ld, S.WIDE)
    for idxs in ([0, 1], [2], [S.ONE], [5, 3]):
        got = ev.run(idxs).clone()
        twin.load(idxs)
        G, _, _ = ld._assemble(idxs, 0)
        with torch.no_grad():
            assert torch.equal(got, m(twin.graph)[:len(idxs)]), idxs
            assert (got - m(G)).abs().max().item() <= 1e-4, idxs
    assert ev.replays == 4 and ev.eager_runs == 0


def test_augmented_slot_counts_its_live_rows_on_the_device():
    """An augmented slot (``reference_train_transform()``: nodes dropped at 0.5): the number of live rows differs from fill to fill, exists on
    the device only, and is what ``slot.counts()`` - the explicit read-back - reports; the live table is 1 on exactly those rows.  GIN then
    steps on it through ``CapturedSlotStep``; a batch of 37 stored nodes fails the two-live-rows rule and is stepped eagerly."""
    from wsi_hgnn_amd.data import BatchSlot
    from wsi_hgnn_amd.trainer import CapturedSlotStep
    ald = S.loader(_dev(), augment=True)
    slot = BatchSlot(ald, S.WIDE)
    seen = []
    for draws in ([11, 12], [13, 14]):
        slot.load([1, 3], draws)
        n = int(sum(sum(c) for c in slot.counts()[0]))
        live, rows = slot.live_rows
        assert rows.item() == float(n) and 2 <= n < S.SIZES[1] + S.SIZES[3]
        assert live[:n].eq(1).all() and not live[n:].any() and torch.equal(live, (slot.bufs["row_seg"] < slot.layout.b_cap).float())
        seen.append(n)
    assert seen[0] != seen[1]
    m, o = _make("mean", "att", True, True)
    step = CapturedSlotStep(m, o, torch.nn.CrossEntropyLoss(), slot, warmup=1, warmup_batches=[[1, 3]])
    loss, logits = step.step([0, 4])
    assert step.replays == 1 and step.eager_steps == 0 and bool(torch.isfinite(loss)) and bool(torch.isfinite(logits).all())
    assert step.slots[0].live_rows[1].item() == float(sum(sum(c) for c in step.slots[0].counts()[0]))
    assert slot.fits([S.N37]) and step.slot_for([S.N37]) is None and step.slot_for([S.N38]) == 0
    loss, logits = step.step([S.N37])
    assert step.replays == 1 and step.eager_steps == 1 and bool(torch.isfinite(loss)) and logits.shape == (1, S.CLASSES)
    assert all(bool(torch.isfinite(v).all()) for v in m.state_dict().values())


@pytest.mark.parametrize("train", [True, False], ids=["train", "eval"])
def test_fusion_switch_changes_no_bit(ld, train):
    """One step on a padded slot graph with the BatchNorm + ReLU fusion on against ``ops.set_fused_bn_relu(False)``: loss, logits, every
    gradient, the running statistics and the stepped parameters, bit for bit."""
    from wsi_hgnn_amd import ops
    res = []
    for fused in (True, False):
        ops.set_fused_bn_relu(fused)
        try:
            m, o = _make("mean", "att", True, train)
            out = _eager(m, o, _padded(ld, [[0, 1]]))
        finally:
            ops.set_fused_bn_relu(True)
        res.append((out, m))
    (oa, ma), (ob, mb) = res
    assert oa[0][0] == ob[0][0] and torch.equal(oa[0][1], ob[0][1])
    for (k, p), (_, q) in zip(ma.named_parameters(), mb.named_parameters()):
        assert (p.grad is None) == (q.grad is None) and (p.grad is None or torch.equal(p.grad, q.grad)), k
    for (k, a), (_, b) in zip(ma.state_dict().items(), mb.state_dict().items()):
        assert torch.equal(a, b), k
