"""The per-relation-source plan (HGT's) derived from the ordinary plan (graph.plan_by_relation_torch) against the plan built from
the COO (graph._build_plan(per_relation_src=True)): every integer table element for element."""
import pytest
import torch

import plan_rel_cases as P
import slot_cases as C

CASES = P.cases()


def _equal_plans(got, ref, tables=P.TABLES):
    for k in tables:
        a, b = getattr(got, k), getattr(ref, k)
        assert a.dtype == b.dtype == torch.int32 and a.shape == b.shape, k
        assert torch.equal(a, b), k
    assert got.num_src_rows == ref.num_src_rows and got.num_edges == ref.num_edges and got.rel_rows == ref.rel_rows


@pytest.mark.parametrize("name,build", CASES, ids=[n for n, _ in CASES])
def test_derived_plan_equals_the_plan_built_from_coo(name, build):
    from wsi_hgnn_amd import graph as G
    g = build()
    hd = P.header(g)
    base = g.plan()
    ref = G._build_plan(g, per_relation_src=True)
    got = G.plan_by_relation_torch(hd, base)
    _equal_plans(got, ref)
    assert got.num_heavy == ref.num_heavy and got.num_src_rows == hd.rel_rows_total
    # shared with the base plan, not copied
    for k in ("rowptr", "node_seg", "inv_rd", "order_dst", "readout_ptr"):
        assert getattr(got, k) is getattr(base, k), k
    assert (got.heavy_degree, got.locality, got.batch_size) == (base.heavy_degree, base.locality, base.batch_size)
    # what the cases are there for
    outdeg = (ref.colptr[1:] - ref.colptr[:-1])
    if name.startswith("hub-"):
        assert int(outdeg.max()) >= int(name[4:]) // 6
        assert int((base.colptr[1:] - base.colptr[:-1]).max()) >= int(name[4:])
    if name == "some-relations-empty":
        assert any(int(ref.colptr[b] - ref.colptr[a]) == 0 for a, b in ref.rel_rows)
    if name == "no-edges":
        assert got.num_edges == 0 and not got.colptr.any()
    if name.startswith("rows-"):
        assert hd.rel_rows_total - P.TILE * (2 if "2-tiles" in name else 1) == {"rows-tile": 0, "rows-tile-minus-1": -1}.get(name, 1)


def test_derived_plan_into_caller_owned_tables():
    """``out=``: the tables are written into the caller's buffers, and the plan's tables ARE those buffers."""
    from wsi_hgnn_amd import graph as G
    g = P.hub_source(300)
    hd = P.header(g)
    out = G.plan_rel_buffers(hd, g.num_edges(), "cpu")
    got = G.plan_by_relation(hd, g.plan(), out)                 # (a CPU plan: the tensor formulation)
    _equal_plans(got, G._build_plan(g, per_relation_src=True))
    for k in ("src", "colptr", "csc_eid", "csc_dst", "order_src"):
        assert getattr(got, k) is out[k], k
    assert out["header"].dtype == torch.int32 and out["header"].numel() == 5 * 3 + 5 * 18 + 8 and hd.max_src_rels == 6


def test_padded_slot_batch_with_one_filler_source_carrying_every_filler_edge():
    """The padded batch of a slot, [slides.., empty graph.., filler]: batch [0, 1] of the big slot leaves ONE filler node of type 0 and 300
    filler edges into it, all from that node.  The plan derived from the slot's tables equals the plan built from the same batch as a graph."""
    from wsi_hgnn_amd import graph as G
    from wsi_hgnn_amd.data import BatchSlot
    ld = C.loader("cpu")
    for idxs in ([0, 1], [2], [5, 3]):
        slot = BatchSlot(ld, C.BIG).load(idxs)
        g, nf, ef = P.explicit_padded(ld, slot, idxs)
        if idxs == [0, 1]:
            assert nf[0] == 1 and ef[0] == 300
        base = slot.graph.plan()
        got = G.plan_by_relation_torch(slot.layout.hd, base)
        ref = G._build_plan(g, per_relation_src=True)
        _equal_plans(got, ref, ("rowptr", "src", "colptr", "csc_eid", "csc_dst", "order_src"))
        assert got.order_dst is base.order_dst and got.num_heavy == base.num_heavy == 0


def test_slot_with_the_per_relation_tables_rederives_them_at_every_load():
    """``BatchSlot(per_relation_src=True)`` on the CPU: the installed plan's own tables are the slot's buffers, current after every ``load`` -
    equal to the plan built from the explicit padded batch; the source order is the rows' own (``rel_sorted`` off) or ``finish_plan``'s."""
    from wsi_hgnn_amd import graph as G
    from wsi_hgnn_amd.data import BatchSlot
    ld = C.loader("cpu")
    slot = BatchSlot(ld, C.BIG, per_relation_src=True)
    plan = slot.graph.plan(per_relation_src=True)
    NS = slot.layout.hd.rel_rows_total
    assert plan.num_src_rows == NS and plan.src is slot.rel["src"] and plan.colptr.numel() == NS + 1 and plan.order_dst is slot.bufs["order_dst"]
    for sort in (False, True):
        slot.rel_sorted = sort
        for idxs in ([0, 1], [4], [5, 3]):
            slot.load(idxs)
            assert slot.graph.plan(per_relation_src=True) is plan
            ref = G._build_plan(P.explicit_padded(ld, slot, idxs)[0], per_relation_src=True)
            _equal_plans(plan, ref, ("rowptr", "src", "colptr", "csc_eid", "csc_dst") + (("order_src",) if sort else ()))
            if not sort:
                assert torch.equal(plan.order_src, torch.arange(NS, dtype=torch.int32))
    plain = BatchSlot(ld, C.BIG)
    assert plain.rel is None and "_plan_rel" not in plain.graph.__dict__


def test_cpu_graphs_and_coo_graphs_keep_the_build_from_coo(monkeypatch):
    """``HeteroGraph.plan(per_relation_src=True)`` derives only on a GPU graph without COO; everything else goes through ``_build_plan``."""
    from wsi_hgnn_amd import graph as G
    calls = []
    real = G._build_plan
    monkeypatch.setattr(G, "_build_plan", lambda g, per_relation_src=False: calls.append(per_relation_src) or real(g, per_relation_src))
    monkeypatch.setattr(G, "plan_by_relation", lambda *a, **k: pytest.fail("derived on the CPU"))
    g = P.rand_graph(3, (9, 8, 7), P.ALL18, 11)
    g.plan(per_relation_src=True)
    ld = C.loader("cpu")
    batch, _, _ = ld._assemble([3, 4], 0)
    assert batch._edges_store is None
    batch.plan(per_relation_src=True)
    assert calls.count(True) == 2
