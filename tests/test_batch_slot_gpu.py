"""Padded batch slots on the GPU: the fill kernel (csrc/segment_table.hip) against graph.slot_fill_torch bit for bit, its descriptor
contract (include/wsi_hgnn.h, graph.SegmentTable) by hand, and one captured step per slot (trainer.CapturedSlotStep) replayed over new slides
against eager steps on the same slots.  Fixture: tests/slot_cases.py."""
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


POISON = -0x5A5A5A5B                          # int32 0xA5A5A5A5: what an element no segment owns must still hold


def _hand_table(out):
    """A SegmentTable by hand over ``out`` (int32, poisoned) and what the header's formulas give for it, evaluated directly: mode 0 in the four
    combinations of in1 and in2 + tab, modes 1 and 2; lengths at the 1024-element block edges, interleaved; one unowned element between any two
    segments.  Two lookup tables, the second behind the first, so that ``tab_off`` differs from the handle's offset alone."""
    from wsi_hgnn_amd import graph as G
    dev = out.device
    tb = G.SegmentTable("test")
    lut = [7, -3, 100]
    far = [1000, 2000, -4000, 8000]
    h_lut, h_far = tb.table("lut", lut), tb.table("far", far)
    assert (h_lut, h_far) == (0, 3)
    words = lut + far
    exp = torch.full((out.numel(),), POISON, dtype=torch.int64)
    gen = torch.Generator().manual_seed(5)
    keep = []                                 # the sources stay alive until the caller has synchronised
    lengths = [1, 1023, 1024, 1025, 2049]
    nan, neg0 = 0x7FC12345, -0x80000000       # a quiet NaN with a payload; -0.0 as the signed word graph._float_bits gives
    off = 1
    for k in range(12):
        n, kind = lengths[(2 * k + k // 6) % 5], k % 6
        i = torch.arange(n, dtype=torch.int64)
        if kind < 4:                          # mode 0: add + i * stride + in1[i] + tab[key + in2[i]]
            add, stride = 11 + k, 3 - k
            in1 = torch.randint(-500, 500, (n,), generator=gen, dtype=torch.int64) if kind & 1 else None
            v = add + i * stride + (in1 if in1 is not None else 0)
            kw = {}
            if kind & 2:
                tab, key, size = ((h_lut, 1, 3) if k < 6 else (h_far, 2, 4))
                in2 = torch.randint(0, size - key, (n,), generator=gen, dtype=torch.int64)
                v = v + torch.tensor(words, dtype=torch.int64)[tab + key + in2]
                kw = dict(in2=in2.to(dev), tab=tab, key=key)
                keep.append(kw["in2"])
            if in1 is not None:
                kw["in1"] = in1.to(dev)
                keep.append(kw["in1"])
            tb.seg(out, off, n, add=add, stride=stride, mode=0, **kw)
        elif kind == 4:                       # mode 1: the same 32 bits, whatever float they spell
            bits = torch.randint(-2 ** 31, 2 ** 31, (n,), generator=gen, dtype=torch.int64)
            bits[0], bits[n - 1] = nan, neg0
            v = bits
            src = bits.to(torch.int32).view(torch.float32).to(dev)
            keep.append(src)
            tb.seg(out, off, n, in1=src, mode=1)
        else:                                 # mode 2: the low 32 bits of add
            add = nan if k < 6 else neg0
            v = torch.full((n,), add, dtype=torch.int64)
            tb.seg(out, off, n, add=add, mode=2)
        before = tb.nsegs
        tb.seg(out, off, 0, add=1)            # n = 0: no row
        assert tb.nsegs == before == k + 1
        exp[off:off + n] = v
        off += n + 1
    assert off <= out.numel()
    wrap = lambda x: ((x + 2 ** 31) % 2 ** 32 - 2 ** 31).to(torch.int32)
    assert tb.blocks == sum((s_[7] + 1023) // 1024 for s_ in tb.segs) and {s_[7] for s_ in tb.segs} == set(lengths)
    return tb, wrap(exp), keep


def test_segment_descriptor_contract_through_both_entry_points(ld):
    """The descriptor contract of include/wsi_hgnn.h itself, not through the graph functions: one hand-built table launched through
    wsi_plan_assemble and through wsi_slot_fill into separate outputs; both equal the direct evaluation of the header's formulas and each other,
    exactly (every unowned element still poisoned).  An empty table is OK without a launch; a segment that leaves its output raises before
    anything is launched, in assemble_plan and in ReducePlan.row_segment as well."""
    from wsi_hgnn_amd import _native as N, graph as G, ops
    dev = _dev()
    lib = N.load()
    total = 12 + 2 * (1 + 1023 + 1024 + 1025 + 2049) + 2049 + 8
    outs = {}
    for name in ("wsi_plan_assemble", "wsi_slot_fill"):
        out = torch.full((total,), POISON, dtype=torch.int32, device=dev)
        tb, exp, keep = _hand_table(out)          # (keep: the sources, alive until the synchronise below)
        desc = tb.upload(dev)
        N.check(getattr(lib, name)(N.ptr(desc), tb.nsegs, tb.blocks, N.stream()), name)
        torch.cuda.synchronize()
        outs[name] = out.cpu()
        assert torch.equal(outs[name], exp), name
        # nothing to do: OK, and nothing written
        empty = G.SegmentTable("test")
        empty.seg(out, 0, 0)
        assert empty.nsegs == 0 and empty.blocks == 0
        assert getattr(lib, name)(None, 0, 0, N.stream()) == 0
        torch.cuda.synchronize()
        assert torch.equal(out.cpu(), exp), name
        with pytest.raises(RuntimeError, match="leaves the table"):
            tb.seg(out, total - 4, 5, add=1)
        with pytest.raises(RuntimeError, match="reads past its source"):
            tb.seg(out, 0, 5, in1=torch.zeros(4, dtype=torch.int64, device=dev))
    assert torch.equal(outs["wsi_plan_assemble"], outs["wsi_slot_fill"])
    # the two callers that launched unchecked pointers: pieces larger than the header they are assembled under ...
    small, large = ld.items[4], ld.items[0]
    hd = G.PlanHeader(small.ntypes, small.rels, list(small.num_nodes))
    with pytest.raises(RuntimeError, match="plan_assemble: a segment leaves the table"):
        G.assemble_plan(hd, [large.pieces], dev, [[n] for n in small.num_nodes])
    # ... and a row range past the plan's rows
    rp = ops.ReducePlan.from_ptr([0, 5, 1030], dev)
    rp.ranges[-1] = (5, 1031)
    with pytest.raises(RuntimeError, match="row_segment: a segment leaves the table"):
        rp.row_segment()
    assert rp._row_seg is None


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
