"""The attention readout ('att') and GCN in captured batch slots on the GPU: trainer.CapturedSlotStep / CapturedSlotEval over
GCN ('att', homogeneous slots), HEATNet4 ('att') and HGT ('att', ``per_relation_src`` slots) against eager twins on the slots' own graphs, bit
for bit, and against the unpadded batches by the project's 1e-4 rule; one augmented + quota + ``type_mask`` slot for HEATNet4 ('att')
under a draw that leaves the batch without a node type; the degree-norm launch against torch.  Fixtures: tests/slot_cases.py and
tests/type_mask_cases.py, exact fp32 GEMMs.  ('att' sizes pools[0]'s gate for in_dim and the heterogeneous models apply it to their hidden
states, models/HEATNet4.py:182-187 and :219: they run with hidden = in_dim.)"""
import ctypes

import pytest
import torch
import torch.nn.functional as F

import slot_cases as C
import type_mask_cases as M

pytestmark = pytest.mark.gpu

MODELS = ["GCN", "HEATNet4", "HGT"]
WARM = [5, 3]
SEQUENCE = [[0, 1], [2], [0, 1]]              # three steps over two different batches


def _dev():
    return torch.device("cuda", torch.cuda.current_device())


@pytest.fixture(scope="module")
def loaders():
    """name -> loader: the slides of tests/slot_cases.py, for GCN as ``graph.to_homogeneous`` output with self-loops."""
    from wsi_hgnn_amd import graph as G, ops
    from wsi_hgnn_amd.data import GraphBatchLoader
    ops.set_gemm_precision("fp32")
    het = C.loader(_dev())
    homo = GraphBatchLoader([G.to_homogeneous(g, add_self_loop=True) for g in C.slides()], C.LABELS, 2, _dev(), shuffle=False, resident=True)
    return {"GCN": homo, "HEATNet4": het, "HGT": het}


def _slot(name, ld):
    from wsi_hgnn_amd.data import BatchSlot
    return BatchSlot(ld) if name == "GCN" else BatchSlot(ld, C.BIG, per_relation_src=(name == "HGT"))


def _make(name, ld, drop=0.0, train=False):
    from wsi_hgnn_amd import models
    torch.manual_seed(3)
    if name == "GCN":
        m = models.GCN(C.IN_DIM, 64, 2, 2, F.relu, drop, "att")
    elif name == "HEATNet4":
        m = models.HEATNet4(C.IN_DIM, C.IN_DIM, 2, 2, 4, C.ND, drop, "att")
    else:
        ed = {tuple(r): i for i, r in enumerate(ld.items[0].rels)}
        m = models.HGT(C.ND, ed, C.IN_DIM, C.IN_DIM, 2, 2, 4, use_norm=False, graph_pooling_type="att")
    m = m.to(_dev())
    m = m.train() if train else m.eval()
    return m, torch.optim.Adam(m.parameters(), lr=1e-3, weight_decay=5e-3, capturable=True)


def _eager_twin(name, ld, m, o, sequence, base=None):
    """Eager steps on a twin slot's own graph: the warm-up step CapturedSlotStep takes, then the sequence."""
    from wsi_hgnn_amd import ops
    lf = torch.nn.CrossEntropyLoss()
    slot, losses = _slot(name, ld), []
    for idxs in [WARM] + list(sequence):
        slot.load(idxs)
        o.zero_grad(set_to_none=True)
        with ops.dropout_seed_base(base):
            l = lf(m(slot.graph), slot.labels)
            l.backward()
        o.step()
        if base is not None:
            ops.advance_dropout_seed_base(base)
        losses.append(l.item())
    return losses[1:]


def _same_state(m1, m2):
    for (k, a), (_, b) in zip(m1.state_dict().items(), m2.state_dict().items()):
        assert torch.equal(a, b), k


def test_refusals_are_lifted_and_the_readout_reads_the_slot_tables(loaders):
    from wsi_hgnn_amd.pooling.readout import slot_plan
    slot = _slot("HEATNet4", loaders["HEATNet4"]).load([0, 1])
    m, _ = _make("HEATNet4", loaders["HEATNet4"])
    assert slot_plan(slot.graph) is slot.readout_plan and m.pools[0].fused(slot.graph)
    G, _, _ = loaders["HEATNet4"]._assemble([0, 1], 0)
    assert slot_plan(G) is None and not m.pools[0].fused(G)                   # an ordinary batch keeps the composite path


@pytest.mark.parametrize("name", MODELS)
def test_switch_on_an_ordinary_batch_matches_the_composite_readout(loaders, name):
    """``ops.set_fused_attention_readout(True)`` on the loader's unpadded batch - for the heterogeneous models one launch over the all-types
    plan built from host-side node counts - against the composite default: logits and loss within 1e-4."""
    from wsi_hgnn_amd import ops
    ld = loaders[name]
    m, _ = _make(name, ld)
    G, y, _ = ld._assemble([0, 1], 0)
    lf = torch.nn.CrossEntropyLoss()
    with torch.no_grad():
        composite = m(G)
        ops.set_fused_attention_readout(True)
        try:
            fused = m(G)
        finally:
            ops.set_fused_attention_readout(False)
    assert (fused - composite).abs().max().item() <= 1e-4 and abs(lf(fused, y).item() - lf(composite, y).item()) <= 1e-4
    assert bool(torch.isfinite(fused).all())


@pytest.mark.parametrize("name", MODELS)
def test_captured_slot_step_replays_the_eager_trajectory(loaders, name):
    from wsi_hgnn_amd.trainer import CapturedSlotStep
    ld = loaders[name]
    lf = torch.nn.CrossEntropyLoss()
    m1, o1 = _make(name, ld)
    eager = _eager_twin(name, ld, m1, o1, SEQUENCE)
    m2, o2 = _make(name, ld)
    step = CapturedSlotStep(m2, o2, lf, _slot(name, ld), warmup=1, warmup_batches=[WARM])
    got = []
    for idxs in SEQUENCE:
        loss, logits = step.step(idxs)
        assert logits.shape == (len(idxs), 2)
        got.append(loss.item())
    assert step.replays == 3 and step.eager_steps == 0
    assert got == eager, (got, eager)
    assert len(set(got)) == 3                                                  # the repeated batch meets another model
    _same_state(m1, m2)


def test_gcn_dropout_is_drawn_anew_by_every_replay(loaders, monkeypatch):
    """GCN in train mode, inter-layer dropout 0.2: under the captured step the draw is counter-based through ONE device word that every replay
    advances; the trajectory equals eager steps that draw through the same word with the same host seed, and the same batch twice in a row
    gives two different losses.  Outside a seed base the module still calls nn.Dropout."""
    from wsi_hgnn_amd import ops
    from wsi_hgnn_amd.trainer import CapturedSlotStep
    ld = loaders["GCN"]
    lf = torch.nn.CrossEntropyLoss()
    monkeypatch.setattr(ops, "next_dropout_seed", lambda: 1000)               # the host seed of every draw: what a capture freezes it to
    seq = SEQUENCE + [[0, 1]]
    m2, o2 = _make("GCN", ld, 0.2, train=True)
    step = CapturedSlotStep(m2, o2, lf, _slot("GCN", ld), warmup=1, warmup_batches=[WARM])
    first = int(step.seed_base.item()) - ops.SEED_STRIDE                       # the word before the warm-up step
    got = [step.step(idxs)[0].item() for idxs in seq]
    assert (int(step.seed_base.item()) - first - (1 + len(seq)) * ops.SEED_STRIDE) % (1 << 32) == 0
    assert got[-1] != got[-2]
    m1, o1 = _make("GCN", ld, 0.2, train=True)
    base = torch.tensor([((first + (1 << 31)) % (1 << 32)) - (1 << 31)], dtype=torch.int32, device=_dev())
    assert got == _eager_twin("GCN", ld, m1, o1, seq, base=base)
    _same_state(m1, m2)
    called = []
    monkeypatch.setattr(m1.dropout, "forward", lambda h: called.append(1) or h)
    m1._drop(torch.ones(4, 4, device=_dev()))
    assert called == [1]


@pytest.mark.parametrize("idxs", [[0, 1], [2]])
@pytest.mark.parametrize("name", MODELS)
def test_padded_step_matches_the_unpadded_batch(loaders, name, idxs):
    """Logits, loss and gradients on slot.graph (fused readout, the slot's tables) against the loader's ordinary batch of the same slides
    (composite readout, host-side node counts): logits and loss within 1e-4, every gradient within 1e-4 of the tensor's largest entry.
    Two kinds of bias have a gradient that is 0 in exact arithmetic - what is left is rounding noise (1e-13 here) without a scale of its own:
    the gate's (a softmax ignores a shift of its gates) and HGT's key projections' (a key bias shifts every score of one (destination,
    relation) softmax by the same <q, W b>, models/HGT.py:92-101).  They are held against the scale of their weight's gradient, the other
    half of the same Linear's gradient.  Largest error / bound such a bias reached on an MI355X: 0.86 (HEATNet4's gate, batch [2], where the
    gate's weight gradient itself is 8e-6 at most); every other tensor stays under 0.3."""
    ld = loaders[name]
    lf = torch.nn.CrossEntropyLoss()
    m, _ = _make(name, ld)
    slot = _slot(name, ld).load(idxs)
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
    assert set(ga) == set(gb) and any(k.endswith("gate_nn.weight") for k in ga)
    for k in ga:
        zero = k.endswith("gate_nn.bias") or (name == "HGT" and ".k_linears." in k and k.endswith(".bias"))
        top = ga[k[:-4] + "weight" if zero else k].abs().max().item()
        err = (ga[k] - gb[k]).abs().max().item()
        print(k, err, top)
        assert err <= 1e-4 * top, (k, err, top)


@pytest.mark.parametrize("name", MODELS)
def test_captured_slot_eval_replays_the_eager_forward(loaders, name):
    """Replayed logits equal the eager no-grad forward on a twin slot bit for bit, and the unpadded batch's within 1e-4."""
    from wsi_hgnn_amd.trainer import CapturedSlotEval
    ld = loaders[name]
    m, _ = _make(name, ld)
    ev = CapturedSlotEval(m, _slot(name, ld))
    twin = _slot(name, ld)
    for idxs in ([0, 1], [2], [5, 3]):
        got = ev.run(idxs).clone()
        twin.load(idxs)
        G, _, _ = ld._assemble(idxs, 0)
        with torch.no_grad():
            assert torch.equal(got, m(twin.graph)[:len(idxs)]), idxs
            assert (got - m(G)).abs().max().item() <= 1e-4, idxs
    assert ev.replays == 3 and ev.eager_runs == 0


def test_augmented_quota_type_mask_slot_on_a_batch_that_lacks_a_type():
    """HEATNet4 ('att') over an augmented slot with survivor quotas and a presence table, under the draw that empties type 2 of the three-node
    slide: the absent type's readout segments are empty - 0 out of the readout, zero gradient back - the replayed step is bit-equal to the eager
    step on a twin slot under the same gates, and the gated parameters are not stepped."""
    from wsi_hgnn_amd import models, optim
    from wsi_hgnn_amd.data import BatchSlot
    from wsi_hgnn_amd.trainer import CapturedSlotStep
    lf = torch.nn.CrossEntropyLoss()
    draw = M.found_draws()[0]
    idxs, warm = [M.THREE], [[0, 1]]

    def make():
        torch.manual_seed(3)
        m = models.HEATNet4(M.IN_DIM, M.IN_DIM, 2, 2, 4, M.ND, 0.0, "att").to(_dev()).eval()
        return m, optim.Adam(m.parameters(), lr=1e-3, weight_decay=5e-3, capturable=True)

    ald = M.loader(_dev(), augment=True)
    m2, o2 = make()
    slot = BatchSlot(ald, M.BIG, quota="bound", type_mask=True)
    step = CapturedSlotStep(m2, o2, lf, slot, warmup=1, warmup_batches=warm)
    slot.load(idxs, [draw])
    step.graphs[0].replay()
    loss, logits = step.outputs[0]
    assert slot.type_present.tolist() == [1.0, 1.0, 0.0] and slot.counts()[0][0][M.RARE] == 0 and slot.overflows() == 0
    assert bool(torch.isfinite(loss)) and bool(torch.isfinite(logits).all())

    ld2 = M.loader(_dev(), augment=True)
    m1, o1 = make()
    twin = BatchSlot(ld2, M.BIG, quota="bound", type_mask=True)
    for t, ps in enumerate(m1.type_gated_parameters()):
        o1.gate(ps, twin.type_present, t)
    for batch, draws in ((warm[0], None), (idxs, [draw])):
        twin.load(batch, draws)
        o1.zero_grad(set_to_none=True)
        l1 = lf(m1(twin.graph), twin.labels)
        l1.backward()
        o1.step()
    assert loss.item() == l1.item()
    _same_state(m1, m2)
    assert {float(o2.state[p]["step"]) for p in m2.type_gated_parameters()[M.RARE]} == {1.0}
    # the absent type's segments of the real slides are empty: exact zeros out of the readout
    with torch.no_grad():
        _, hcat, pooled, B = m1.encode(twin.graph, predict=False)
    assert B == 3 and not pooled[M.RARE * B:M.RARE * B + 2].any() and pooled[:2].any()


def test_degree_norm_launch_matches_torch_bit_for_bit(loaders):
    from wsi_hgnn_amd import _native as N
    from wsi_hgnn_amd.models.GCN import homo_plan
    slot = _slot("GCN", loaders["GCN"])
    for v in slot.degree_norms:
        v.fill_(-7.5)
    for idxs in ([0, 1], [4], [5, 3]):
        slot.load(idxs)
        n = slot.layout.N
        rowptr, colptr = slot.bufs["rowptr"], slot.bufs["colptr"]
        want_in = (rowptr[1:n + 1] - rowptr[:n]).to(torch.float32).clamp(min=1).pow(-0.5)
        want_out = (colptr[1:n + 1] - colptr[:n]).to(torch.float32).clamp(min=1).pow(-0.5)
        hp = homo_plan(slot.graph)
        assert hp.in_norm is slot.bufs["in_norm"] and torch.equal(hp.in_norm, want_in) and torch.equal(hp.out_norm, want_out), idxs
        assert int((rowptr[1:n + 1] - rowptr[:n]).max()) > 1 and int((rowptr[1:n + 1] - rowptr[:n]).min()) >= 0
    lib = N.load()
    P = ctypes.c_void_p(1 << 40)          # a fake device address: the calls below fail their argument check before touching it
    assert lib.wsi_degree_norms(P, P, -1, P, P, None) == N.WSI_EINVAL
    for args in ((None, P, 4, P, P), (P, None, 4, P, P), (P, P, 4, None, P), (P, P, 4, P, None)):
        assert lib.wsi_degree_norms(*args, None) == N.WSI_EINVAL
    assert lib.wsi_degree_norms(None, None, 0, None, None, None) == 0
