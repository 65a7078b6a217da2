"""wsi_plan_by_relation (csrc/plan_rel.hip) against the tensor formulation graph.plan_by_relation_torch, bit for bit, on the cases
of tests/plan_rel_cases.py; its buffers' margins, its determinism, the empty-input contract and the relation limit of the C ABI."""
import pytest
import torch

import plan_rel_cases as P
import slot_cases as C

pytestmark = pytest.mark.gpu

CASES = P.cases()
POISON = -0x5A5A5A5B
MARGIN = 64
OWNED = ("src", "colptr", "csc_eid", "csc_dst", "order_src")


def _dev():
    return torch.device("cuda", torch.cuda.current_device())


def _guarded(hd, E):
    """``plan_rel_buffers`` whose five tables are the middles of poisoned allocations: (out, {name: whole allocation})."""
    from wsi_hgnn_amd import graph as G
    out = G.plan_rel_buffers(hd, E, _dev())
    whole = {}
    for k in OWNED + ("scratch",):
        n = out[k].numel()
        whole[k] = torch.full((n + 2 * MARGIN,), POISON, dtype=torch.int32, device=_dev())
        out[k] = whole[k][MARGIN:MARGIN + n]
    return out, whole


def _margins_intact(whole):
    for k, w in whole.items():
        assert bool((w[:MARGIN] == POISON).all()) and bool((w[-MARGIN:] == POISON).all()), k


def _check(hd, base):
    from wsi_hgnn_amd import graph as G
    ref = G.plan_by_relation_torch(hd, base)
    out, whole = _guarded(hd, base.num_edges)
    got = G.plan_by_relation(hd, base, out)
    first = {k: out[k].clone() for k in OWNED}
    for k in OWNED:
        assert getattr(got, k) is out[k]
        assert torch.equal(out[k], getattr(ref, k)), k
    _margins_intact(whole)
    assert got.num_src_rows == ref.num_src_rows == hd.rel_rows_total and got.order_dst is base.order_dst
    G.plan_by_relation(hd, base, out)                          # the same call again: the same bits
    for k in OWNED:
        assert torch.equal(out[k], first[k]), k
    _margins_intact(whole)
    return got


@pytest.mark.parametrize("name,build", CASES, ids=[n for n, _ in CASES])
def test_kernel_equals_the_tensor_formulation(name, build):
    g = build().to(_dev())
    _check(P.header(g), g.plan())


def test_kernel_on_slot_tables_with_one_filler_source():
    """A slot's tables after a fill, ONE filler node of type 0 carrying 300 filler edges; then the plan built from the explicit padded batch."""
    from wsi_hgnn_amd import graph as G
    from wsi_hgnn_amd.data import BatchSlot
    ld = C.loader(_dev())
    slot = BatchSlot(ld, C.BIG)
    for idxs in ([0, 1], [2], [5, 3]):
        slot.load(idxs)
        got = _check(slot.layout.hd, slot.graph.plan())
        g, nf, ef = P.explicit_padded(ld, slot, idxs, _dev())
        ref = G._build_plan(g, per_relation_src=True)
        for k in ("rowptr", "src", "colptr", "csc_eid", "csc_dst", "order_src"):
            assert torch.equal(getattr(got, k), getattr(ref, k)), (idxs, k)


def test_slot_rederives_its_per_relation_tables_behind_every_fill():
    """``BatchSlot(per_relation_src=True)``: after every ``load`` the installed plan's tables equal the tensor formulation over the slot's
    current tables, plain and augmented fills alike; poisoned in between, so every element is written by every derivation."""
    from test_batch_slot_augment import aug_loader, pipelines
    from wsi_hgnn_amd import graph as G
    from wsi_hgnn_amd.data import BatchSlot
    for ld, cases in ((C.loader(_dev()), C.CASES[:5]), (aug_loader(_dev(), pipelines()["REF"]), [[0, 1], [2], [1, 2]])):
        slot = BatchSlot(ld, C.BIG, per_relation_src=True)
        plan = slot.graph.plan(per_relation_src=True)
        for sort in (False, True):
            slot.rel_sorted = sort
            for idxs in cases:
                for k in OWNED:
                    slot.rel[k].fill_(POISON)
                slot.load(idxs)
                ref = G.plan_by_relation_torch(slot.layout.hd, slot.graph.plan())
                for k in ("src", "colptr", "csc_eid", "csc_dst") + (("order_src",) if sort else ()):
                    assert getattr(plan, k) is slot.rel[k] and torch.equal(slot.rel[k], getattr(ref, k)), (idxs, k)
                if not sort:
                    assert torch.equal(plan.order_src, torch.arange(plan.num_src_rows, dtype=torch.int32, device=_dev()))


def test_loader_batch_derives_instead_of_rebuilding_the_coo(monkeypatch):
    """``plan(per_relation_src=True)`` of a loader batch: derived (the COO is never materialised), equal to the plan built from the COO."""
    from wsi_hgnn_amd import graph as G
    ld = C.loader(_dev())
    for idxs in ([0, 1], [6, 4], [5]):
        batch, _, _ = ld._assemble(idxs, 0)
        got = batch.plan(per_relation_src=True)
        assert batch._edges_store is None and got is batch.plan(per_relation_src=True)
        ref = G._build_plan(batch, per_relation_src=True)
        for k in ("rowptr", "src", "colptr", "csc_eid", "csc_dst", "order_src"):
            assert torch.equal(getattr(got, k), getattr(ref, k)), (idxs, k)
        assert got.num_src_rows == ref.num_src_rows and got.rel_rows == ref.rel_rows
    monkeypatch.setattr(G, "DERIVE_REL_PLAN", False)
    batch, _, _ = ld._assemble([0, 1], 0)
    batch.plan(per_relation_src=True)
    assert batch._edges_store is not None


def test_empty_input_and_relation_limit_of_the_c_abi():
    from wsi_hgnn_amd import _native as N
    lib = N.load()
    dev = _dev()
    NS, T, NR = 37, 2, 3
    words = 5 * T + 5 * NR + 8
    colptr = torch.full((NS + 1 + 2 * MARGIN,), POISON, dtype=torch.int32, device=dev)
    mid = colptr[MARGIN:MARGIN + NS + 1]
    # E = 0 with NULL arrays: colptr_rel = 0, nothing else is touched (no header, no scratch needed)
    rc = lib.wsi_plan_by_relation(None, None, None, None, None, 20, 0, 30, None, words, T, NR, NS, 2, None, N.ptr(mid), None, None, None, 0, N.stream())
    assert rc == 0
    torch.cuda.synchronize()
    assert not mid.any() and bool((colptr[:MARGIN] == POISON).all()) and bool((colptr[-MARGIN:] == POISON).all())
    # 33 relations leaving one node type: refused before anything is launched
    mid.fill_(POISON)
    assert N.WSI_PLAN_REL_MAX_RELS == 32 and N.WSI_PLAN_REL_TILE == P.TILE
    rc = lib.wsi_plan_by_relation(None, None, None, None, None, 20, 0, 30, None, words, T, NR, NS, 33, None, N.ptr(mid), None, None, None, 0, N.stream())
    assert rc == N.WSI_EINVAL and b"33 relations" in lib.wsi_last_error()
    # a header table of another schema's size, a missing colptr_rel, edges without arrays
    assert lib.wsi_plan_by_relation(None, None, None, None, None, 20, 0, 30, None, words + 1, T, NR, NS, 2, None, N.ptr(mid), None, None, None, 0, N.stream()) == N.WSI_EINVAL
    assert lib.wsi_plan_by_relation(None, None, None, None, None, 20, 0, 30, None, words, T, NR, NS, 2, None, None, None, None, None, 0, N.stream()) == N.WSI_EINVAL
    assert lib.wsi_plan_by_relation(None, None, None, None, None, 20, 5, 30, None, words, T, NR, NS, 2, None, N.ptr(mid), None, None, None, 0, N.stream()) == N.WSI_EINVAL
    torch.cuda.synchronize()
    assert bool((mid == POISON).all())
    assert lib.wsi_plan_by_relation_scratch_words(NS) == NS + 2 and lib.wsi_plan_by_relation_scratch_words(2 * P.TILE + 1) == 2 * P.TILE + 1 + 4
