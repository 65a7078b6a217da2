"""Batch slots with a device-side presence table on the CPU: the ``fits`` rules under ``type_mask``, the presence table of the
tensor route against node counts of the unpadded batch, and the refusals of ``optim.gate`` and of the captured classes' checks.
Fixture: tests/type_mask_cases.py."""
import pytest
import torch

import type_mask_cases as M


@pytest.fixture(scope="module")
def ld():
    return M.loader("cpu")


@pytest.fixture(scope="module")
def ald():
    return M.loader("cpu", augment=True)


def test_fits_takes_a_batch_without_a_node_type_only_under_type_mask(ld):
    from wsi_hgnn_amd.data import BatchSlot
    masked, plain = BatchSlot(ld, M.BIG, type_mask=True), BatchSlot(ld, M.BIG)
    assert plain.type_mask is False and plain.type_present is None and not hasattr(plain.graph, "_type_present")
    assert masked.type_mask is True and masked.graph._type_present is masked.type_present
    assert masked.type_present.dtype == torch.float32 and tuple(masked.type_present.shape) == (3,)
    assert masked.fits([M.TYPELESS]) and not plain.fits([M.TYPELESS])
    assert masked.fits([M.TYPELESS, 6]) and not plain.fits([M.TYPELESS, 6])
    with pytest.raises(ValueError, match="does not fit"):
        plain.load([M.TYPELESS])
    for slot in (masked, plain):                                      # what stays: a batch with the type somewhere, capacity, b_cap, membership
        assert slot.fits([1, M.TYPELESS]) and slot.fits([0, 1])
        assert not slot.fits(M.NO_FIT) and not slot.fits([1, 5, 3]) and not slot.fits([]) and not slot.fits([99])
    small = BatchSlot(ld, M.SMALL, type_mask=True)
    assert small.fits([M.TYPELESS]) and small.fits([M.THREE]) and not small.fits([0]) and not small.fits([M.TYPELESS, 5])


def test_augmented_fits_drops_the_emptying_rule_only_under_type_mask(ald):
    from wsi_hgnn_amd.data import BatchSlot
    masked, plain = BatchSlot(ald, M.BIG, type_mask=True), BatchSlot(ald, M.BIG)
    assert masked.fits([M.THREE]) and not plain.fits([M.THREE])       # 0.5 ** 3 > 2 ** -32
    assert masked.fits([M.TYPELESS]) and not plain.fits([M.TYPELESS])
    assert masked.fits([0, 1]) and plain.fits([0, 1])                 # 64 nodes of the rarest type
    for slot in (masked, plain):
        assert not slot.fits(M.NO_FIT) and not slot.fits([1, 5, 3]) and not slot.fits([99])


def test_a_caller_table_is_used_and_checked(ld):
    from wsi_hgnn_amd.data import BatchSlot
    table = torch.full((3,), 7.0)
    a, b = BatchSlot(ld, M.BIG, type_mask=table), BatchSlot(ld, M.SMALL, type_mask=table)
    assert a.type_present is table and b.type_present is table and a.graph._type_present is table
    a.load([M.TYPELESS, 6])
    assert table.tolist() == [1.0, 1.0, 0.0]
    b.load([5])
    assert table.tolist() == [1.0, 1.0, 1.0]
    for bad in (torch.ones(2), torch.ones(3, dtype=torch.float64), torch.ones(3, 1), torch.ones(6)[::2], "yes"):
        with pytest.raises(ValueError, match="type_mask"):
            BatchSlot(ld, M.BIG, type_mask=bad)
    with pytest.raises(RuntimeError, match="without type_mask"):
        BatchSlot(ld, M.BIG).share_type_table(table)


def test_presence_table_of_plain_fills_against_the_unpadded_counts(ld):
    """Every plain case, a present batch behind an absent one, a poison value in the table before every fill."""
    from wsi_hgnn_amd.data import BatchSlot
    slot = BatchSlot(ld, M.BIG, type_mask=True)
    seen = set()
    for idxs, what in M.PLAIN + M.PLAIN[:2]:
        slot.type_present.fill_(-3.0)
        slot.load(idxs)
        want = M.expected_present([M.stored_graph(ld, i) for i in idxs])
        assert slot.type_present.tolist() == want, (idxs, what)
        assert want == [1.0 if sum(ld.items[i].num_nodes[t] for i in idxs) else 0.0 for t in range(3)]
        seen.add(tuple(want))
    assert seen == {(1.0, 1.0, 1.0), (1.0, 1.0, 0.0)}


def test_presence_table_of_augmented_fills_against_the_unpadded_counts(ald):
    """The emptying and the sparing draw of the three-node slide, alone and beside a slide that keeps the type, and the type-less slide."""
    from wsi_hgnn_amd.data import BatchSlot
    emptying, sparing = M.found_draws()
    slot = BatchSlot(ald, M.BIG, type_mask=True)
    for idxs, draws, want2 in (([M.THREE], [emptying], 0.0), ([M.THREE], [sparing], 1.0), ([M.THREE, M.TYPELESS], [emptying, 5], 0.0),
                               ([M.THREE, 1], [emptying, 5], 1.0), ([M.TYPELESS], [9], 0.0), ([M.THREE], [sparing], 1.0)):
        slot.type_present.fill_(-3.0)
        slot.load(idxs, draws)
        graphs = M.unpadded_augmented(ald, idxs, draws)
        want = M.expected_present(graphs)
        assert want[M.RARE] == want2 and want[:2] == [1.0, 1.0], (idxs, draws, [g.num_nodes("2") for g in graphs])
        assert slot.type_present.tolist() == want, (idxs, draws)
        assert slot.counts()[0] == [[g.num_nodes(t) for t in g.ntypes] for g in graphs]


def test_presence_table_under_a_quota_that_truncates_the_type_to_zero(ald):
    from wsi_hgnn_amd.data import BatchSlot
    _, sparing = M.found_draws()
    limits = {}

    def quota(i):
        qn, qe = M.stored_quota(ald, i)
        return [min(q, limits.get((i, t), q)) for t, q in enumerate(qn)], qe

    limits[(M.THREE, M.RARE)] = 0
    slot = BatchSlot(ald, M.BIG, quota=quota, type_mask=True)
    for idxs, draws, want2 in (([M.THREE], [sparing], 0.0), ([M.THREE, 5], [sparing, 3], 1.0), ([M.THREE, M.TYPELESS], [sparing, 3], 0.0)):
        slot.type_present.fill_(-3.0)
        slot.load(idxs, draws)
        graphs = M.unpadded_augmented(ald, idxs, draws, [slot.quota_of(i) for i in idxs])
        want = M.expected_present(graphs)
        assert want[M.RARE] == want2, (idxs, [g.num_nodes("2") for g in graphs])
        assert slot.type_present.tolist() == want, idxs
    assert slot.overflows() == 3                                       # the sparing draw keeps a node of the type: the zero quota bound every time


def test_gate_refuses_a_host_count_and_a_bad_table():
    from wsi_hgnn_amd import optim
    p = [torch.nn.Parameter(torch.zeros(4)), torch.nn.Parameter(torch.zeros(2))]
    table = torch.ones(3)
    for cls in (optim.Adam, optim.Adagrad):
        with pytest.raises(RuntimeError, match="capturable=True"):
            cls(p, lr=1e-3).gate(p[:1], table, 0)
        o = cls(p, lr=1e-3, capturable=True)
        with pytest.raises(ValueError, match="on the GPU"):          # (the count is on the device; this table is not)
            o.gate(p[:1], table, 0)
        o.gate(p[:1], None)                                            # unbinding nothing is fine
    o = optim.SGD(p[:1], lr=1e-3, momentum=0.9)
    with pytest.raises(ValueError, match="does not step"):
        o.gate(p[1:], table, 0)
    with pytest.raises(ValueError, match="dampening"):
        optim.SGD(p, lr=1e-3, momentum=0.9, dampening=0.5).gate(p[:1], table, 0)


def test_the_captured_classes_checks_refuse_mixed_slots_and_a_torch_optimizer(ld):
    from wsi_hgnn_amd import models, optim
    from wsi_hgnn_amd.data import BatchSlot
    from wsi_hgnn_amd.trainer import _check_slots, _gate_by_type, _share_type_table
    m = models.HEATNet4(M.IN_DIM, 32, 2, 2, 4, M.ND, 0.0, "mean")
    masked, plain = BatchSlot(ld, M.BIG, type_mask=True), BatchSlot(ld, M.SMALL)
    with pytest.raises(ValueError, match="with and without type_mask"):
        _check_slots("CapturedSlotStep", "step", m, [masked, plain])
    with pytest.raises(RuntimeError, match="must live on the GPU"):   # (all with, all without: on to the next check)
        _check_slots("CapturedSlotStep", "step", m, [masked, BatchSlot(ld, M.SMALL, type_mask=True)])
    with pytest.raises(RuntimeError, match="must live on the GPU"):
        _check_slots("CapturedSlotStep", "step", m, [plain])
    with pytest.raises(RuntimeError, match="cannot skip a tensor"):
        _gate_by_type("CapturedSlotStep", m, torch.optim.Adam(m.parameters(), lr=1e-3, capturable=True), masked.type_present)
    with pytest.raises(RuntimeError, match="capturable=True"):
        _gate_by_type("CapturedSlotStep", m, optim.Adam(m.parameters(), lr=1e-3), masked.type_present)
    o = optim.Adam(m.parameters(), lr=1e-3, capturable=True)          # binding happens on the host: the order of gate()'s checks lets a CPU
    with pytest.raises(ValueError, match="on the GPU"):                # table through as far as the table check, after every refusal above
        _gate_by_type("CapturedSlotStep", m, o, masked.type_present)
    other = BatchSlot(ld, M.SMALL, type_mask=True)
    assert _share_type_table([plain]) is None
    assert _share_type_table([masked, other]) is masked.type_present and other.type_present is masked.type_present
    assert other.graph._type_present is masked.type_present


def test_type_gated_parameters_name_the_heads_of_each_type():
    """One list per node type; HEATNet4's fused path leaves the absent type's projection and block out of the step, the other forms run every
    projection as a group of one GEMM (exact zeros, not None - the GPU test holds each set against an eager step)."""
    from wsi_hgnn_amd import models
    rels = M.slides()[0].canonical_etypes
    m4 = models.HEATNet4(M.IN_DIM, 32, 2, 2, 4, M.ND, 0.0, "mean")
    names = {id(p): k for k, p in m4.named_parameters()}
    assert [[names[id(p)] for p in ps] for ps in m4.type_gated_parameters()] == [
        [f"linears_prediction.{t}.weight", f"linears_prediction.{t}.bias", f"attn.{t}.op.weight"] for t in "012"]
    for t in "012":
        m4.attn[t].normalize_attn = False
    assert [[names[id(p)] for p in ps] for ps in m4.type_gated_parameters()] == [[f"attn.{t}.op.weight"] for t in "012"]
    m2 = models.HEATNet2(M.IN_DIM, 32, 2, 2, 4, M.ND, 0.0, "mean")
    hgt = models.HGT(M.ND, {tuple(r): i for i, r in enumerate(rels)}, M.IN_DIM, 32, 2, 2, 4)
    assert m2.type_gated_parameters() == [[], [], []] and hgt.type_gated_parameters() == [[], [], []]
