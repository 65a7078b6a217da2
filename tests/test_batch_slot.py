"""Padded batch slots on the CPU: the slot's tables (graph.slot_fill_torch) against the plan assembled from the explicit graphs
[real slides..., empty graphs..., filler]; the filler adds nothing to logits, loss or gradients (oracle model, float64); the capacity rules; and
the kernel's closed forms (csrc/slot_math.h) against a sort, as a stand-alone host program under the address and undefined-behaviour sanitizers."""
import os
import subprocess
from collections import OrderedDict

import pytest
import torch

import slot_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def data():
    from wsi_hgnn_amd.data import BatchSlot
    ld = C.loader("cpu")
    return ld, BatchSlot(ld, C.BIG), BatchSlot(ld, C.SMALL)


def _explicit(ld, slot, idxs):
    """The padded batch spelled out: the real slides' stored graphs, empty graphs up to b_cap, the filler as a graph of its own."""
    from wsi_hgnn_amd import graph as G
    from wsi_hgnn_amd.data import StoredGraph
    lay = slot.layout
    its = [ld.items[i] for i in idxs]
    n = [sum(it.num_nodes[t] for it in its) for t in range(lay.T)]
    e = [sum(it.pieces.ecount[t] for it in its) for t in range(lay.T)]
    nf, ef = [lay.n_cap[t] - n[t] for t in range(lay.T)], [lay.e_cap[t] - e[t] for t in range(lay.T)]
    filler = G.filler_graph(lay.ntypes, lay.rels, nf, ef, C.IN_DIM)
    empty = G.filler_graph(lay.ntypes, lay.rels, [0] * lay.T, [0] * lay.T, C.IN_DIM)
    graphs = [empty] * (lay.b_cap - len(idxs)) + [filler]
    return its + [StoredGraph(g, -100, torch.device("cpu"), True) for g in graphs], graphs, nf, ef


@pytest.mark.parametrize("which,idxs", [("big", c) for c in C.CASES] + [("small", c) for c in C.SMALL_CASES])
def test_slot_tables_equal_the_plan_of_the_explicit_padded_batch(data, which, idxs):
    from wsi_hgnn_amd import graph as G
    ld, big, small = data
    slot = big if which == "big" else small
    lay = slot.layout
    assert slot.fits(idxs)
    its = [ld.items[i] for i in idxs]
    out = G.slot_fill_torch(lay, [it.pieces for it in its], [it.label for it in its], [it.feat for it in its])
    padded, _, nf, ef = _explicit(ld, slot, idxs)
    counts = [[it.num_nodes[t] for it in padded] for t in range(lay.T)]
    assert [sum(c) for c in counts] == lay.n_cap
    hd = G.PlanHeader(lay.ntypes, lay.rels, lay.n_cap)
    ref, sim = G.assemble_plan_torch(hd, [it.pieces for it in padded], "cpu", counts)
    for k in ("rowptr", "src", "colptr", "csc_eid", "csc_dst", "node_seg", "inv_rd", "readout_ptr"):
        assert torch.equal(out[k], getattr(ref, k)), k
    assert torch.equal(out["sim"], sim)
    assert ref.num_edges == lay.E and out["src"].numel() == lay.E
    # processing orders: permutations; the real nodes in the relative order of the UNPADDED batch's plan; the filler's nodes last
    real = [ld.items[i] for i in idxs]
    ucounts = [[it.num_nodes[t] for it in real] for t in range(lay.T)]
    uhd = G.PlanHeader(lay.ntypes, lay.rels, [sum(c) for c in ucounts])
    uplan, _ = G.assemble_plan_torch(uhd, [it.pieces for it in real], "cpu", ucounts)
    shift = torch.zeros(uhd.N, dtype=torch.int64)                      # unpadded global id -> padded global id
    for t in range(lay.T):
        shift[uhd.type_off[t]:uhd.type_off[t + 1]] = hd.type_off[t] - uhd.type_off[t]
    is_filler = torch.zeros(lay.N, dtype=torch.bool)
    for t in range(lay.T):
        is_filler[hd.type_off[t + 1] - nf[t]:hd.type_off[t + 1]] = True
    for k in ("order_dst", "order_src"):
        o = out[k].long()
        assert torch.equal(torch.sort(o).values, torch.arange(lay.N)), k
        assert not is_filler[o[:uhd.N]].any() and is_filler[o[uhd.N:]].all(), k
        u = getattr(uplan, k).long()
        assert torch.equal(o[:uhd.N], u + shift[u]), k
    # labels, features, the derived per-edge segment table and the readout plan's row -> segment table
    assert out["labels"].tolist() == [ld.items[i].label for i in idxs] + [-100] * (lay.graphs - len(idxs))
    for t in range(lay.T):
        a = hd.type_off[t]
        rows = torch.cat([it.feat[t] for it in real])
        assert torch.equal(out["feat"][a:a + rows.shape[0]], rows) and not out["feat"][a + rows.shape[0]:hd.type_off[t + 1]].any()
    rp = out["rowptr"].long()
    assert torch.equal(out["edge_seg"].long(), torch.repeat_interleave(torch.arange(lay.S), rp[1:] - rp[:-1]))
    ptr = out["readout_ptr"].long()
    assert torch.equal(out["row_seg"].long(), torch.repeat_interleave(torch.arange(lay.num_segs), ptr[1:] - ptr[:-1]))
    # the edge cases the batches are there for
    if which == "big" and idxs == [0, 1]:
        assert nf == [1, 5, 10] and ef == [300, 0, 5]
    if idxs == [2]:
        assert counts[0][1] == 0


def test_slot_graph_is_the_explicit_padded_batch(data):
    """BatchSlot on the CPU: slot.graph's node counts, features, labels and (rebuilt on demand) per-relation COO and sim are those of
    graph.batch over the explicit graphs; a second load into the same slot leaves nothing of the first behind."""
    import wsi_hgnn_amd as W
    from wsi_hgnn_amd import graph as G
    ld, big, _ = data
    for idxs in ([0, 1], [4], [5, 3]):
        big.load(idxs)
        _, extra, nf, ef = _explicit(ld, big, idxs)
        ref = W.batch(_slide_graphs(idxs) + extra)
        g = big.graph
        assert big.num_real == len(idxs) and g.batch_size == 3
        assert big.labels.tolist() == [C.LABELS[i] for i in idxs] + [-100] * (3 - len(idxs))
        for t in g.ntypes:
            assert g.batch_num_nodes(t).tolist() == ref.batch_num_nodes(t).tolist()
            assert torch.equal(g.nodes[t].data["feat"], ref.nodes[t].data["feat"])
        for r in g.canonical_etypes:
            assert torch.equal(g.edges(r)[0], ref.edges(r)[0]) and torch.equal(g.edges(r)[1], ref.edges(r)[1]), r
            assert torch.equal(g.edata["sim"][r], ref.edata["sim"][r])
        fresh = G.slot_fill_torch(big.layout, [ld.items[i].pieces for i in idxs], [C.LABELS[i] for i in idxs], [ld.items[i].feat for i in idxs])
        for k, v in fresh.items():
            if k != "batch" and k != "scales":
                assert torch.equal(big.bufs[k], v), k


_SLIDES = {}


def _slide_graphs(idxs):
    if not _SLIDES:
        _SLIDES.update(enumerate(C.slides()))
    return [_SLIDES[i] for i in idxs]


def _double(g):
    for t in g.ntypes:
        g.nodes[t].data["feat"] = g.nodes[t].data["feat"].double()
    for r in g.canonical_etypes:
        g._eframes[r]["sim"] = g._eframes[r]["sim"].double()
    return g


@pytest.mark.parametrize("idxs", [[0, 1], [2], [5, 3], [1, 2]])
def test_filler_changes_no_logit_no_loss_and_no_gradient(data, idxs):
    """Oracle HEATNet4 in float64 (hidden 64, 2 layers, 4 heads), padded against unpadded batch: the real slides' logits, the loss (the filler
    and the empty graphs carry ignore_index) and every parameter gradient agree to float64 round-off.  Bound: 1e-12, relative to the largest
    entry of the tensor compared (the two runs sum the same numbers, the padded one with exact zeros in between)."""
    import wsi_hgnn_amd as W
    from oracle import models as OM
    ld, big, _ = data
    _, extra, nf, ef = _explicit(ld, big, idxs)
    torch.manual_seed(11)
    m = OM.HEATNet4(C.IN_DIM, 64, 2, 2, 4, C.ND, 0.0, "mean").double()
    lf = torch.nn.CrossEntropyLoss()
    y = torch.tensor([C.LABELS[i] for i in idxs])
    plain = _double(W.batch(_slide_graphs(idxs)))
    padded = _double(W.batch(_slide_graphs(idxs) + extra))
    out = {}
    for name, g, lab in (("plain", plain, y), ("padded", padded, torch.cat([y, torch.full((3 - len(idxs),), -100)]))):
        m.zero_grad(set_to_none=True)
        logits = m(g)
        loss = lf(logits, lab)
        loss.backward()
        out[name] = (logits.detach()[:len(idxs)].clone(), loss.detach().clone(), {k: (None if p.grad is None else p.grad.clone()) for k, p in m.named_parameters()})
    rel = lambda a, b: (a - b).abs().max().item() / max(b.abs().max().item(), 1e-300)
    assert out["padded"][0].shape == out["plain"][0].shape
    assert rel(out["padded"][0], out["plain"][0]) <= 1e-12
    assert rel(out["padded"][1], out["plain"][1]) <= 1e-12
    for k, gp in out["plain"][2].items():
        gq = out["padded"][2][k]
        assert (gp is None) == (gq is None), k
        if gp is not None and gp.abs().max() > 0:
            assert rel(gq, gp) <= 1e-12, k
        elif gp is not None:
            assert not gq.any(), k


def test_fits_follows_the_capacity_rules(data):
    from wsi_hgnn_amd.data import BatchSlot
    ld, big, small = data
    assert big.fits([0, 1]) and not big.fits(C.NO_FIT) and not big.fits([0, 1, 2]) and not big.fits([])
    assert not small.fits([2]) and small.fits([3, 4])
    with pytest.raises(ValueError, match="does not fit"):
        big.load(C.NO_FIT)
    # nf[t] = 0 does not fit: the filler keeps one node of every type; ef[t] = 0 does; one edge too few does not
    n, e = [350, 210, 140], [2800, 1680, 1120]                       # slides 0 + 1 exactly
    assert not BatchSlot(ld, (n, e, 2)).fits([0, 1])
    assert not BatchSlot(ld, ([351, 211, 140], e, 2)).fits([0, 1])
    assert BatchSlot(ld, ([351, 211, 141], e, 2)).fits([0, 1])
    assert not BatchSlot(ld, ([351, 211, 141], [2800, 1679, 1120], 2)).fits([0, 1])
    assert not big.fits([5])                                          # no slide of the batch has a node of type 2: stepped eagerly (see SlotBatch.fits)
    # capacity=None: per type the batch_size largest counts, plus one node - every batch of the loader fits except those without some node type
    auto = BatchSlot(ld)
    assert auto.layout.n_cap == [210 + 200 + 1, 126 + 120 + 1, 84 + 80 + 1] and auto.layout.b_cap == 2
    assert all(auto.fits([i, j]) for i in range(8) for j in range(8) if i != j)


def test_refusals(data):
    from wsi_hgnn_amd.data import BatchSlot, GraphBatchLoader
    gs = C.slides()[:2]
    with pytest.raises(RuntimeError, match="transform"):
        BatchSlot(GraphBatchLoader(gs, [0, 1], 2, "cpu", resident=True, transform=lambda g, draw=0: g))
    pinned = GraphBatchLoader(gs, [0, 1], 2, "cpu", resident=True)
    pinned.resident = False                  # (a pinned-host loader proper needs a GPU to pin for)
    with pytest.raises(RuntimeError, match="resident"):
        BatchSlot(pinned)


def test_filler_closed_forms_against_a_sort_under_sanitizers(tmp_path):
    """csrc/slot_math.h is what the fill kernel computes the filler's rowptr / src / colptr / CSC entries with; the same header, compiled for the
    host into tests/slot_math_check.cpp, must reproduce a stable sort of the filler's explicit edge list on 4000 random shapes (ASan + UBSan)."""
    exe = str(tmp_path / "slot_math_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "wsi-hgnn_amd", "csrc"), os.path.join(ROOT, "tests", "slot_math_check.cpp"), "-o", exe])
    res = subprocess.run([exe], capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr
    assert " 0 mismatches" in res.stdout
