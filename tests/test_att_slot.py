"""The attention readout ('att') and GCN over padded batch slots, on the CPU, with the shapes of tests/slot_cases.py:
the padded batch [real slides..., empty graphs..., filler] against the unpadded one under the float64 oracle models (as tests/test_batch_slot.py
does for 'mean'); the filler's share of every gradient; the degree-norm tables of a homogeneous slot against ``models.GCN.HomoPlan``."""
import pytest
import torch
import torch.nn.functional as F

import slot_cases as C

BATCHES = [[0, 1], [2], [5, 3], [1, 2]]
GRAPHS = 3                    # b_cap + 1: two slides at most, the filler


def _double(g):
    for t in g.ntypes:
        g.nodes[t].data["feat"] = g.nodes[t].data["feat"].double()
    for r in g.canonical_etypes:
        if "sim" in g._eframes[r]:
            g._eframes[r]["sim"] = g._eframes[r]["sim"].double()
    return g


@pytest.fixture(scope="module")
def hetero():
    """(slides, a function idxs -> the graphs that pad the batch to the BIG slot of tests/slot_cases.py)."""
    from wsi_hgnn_amd import graph as G
    from wsi_hgnn_amd.data import BatchSlot
    slides = C.slides()
    lay = BatchSlot(C.loader("cpu"), C.BIG).layout

    def extra(idxs):
        n = [sum(slides[i].num_nodes(t) for i in idxs) for t in lay.ntypes]
        e = [0] * lay.T
        for i in idxs:
            for (s, _, d) in slides[i].canonical_etypes:
                e[lay.ntypes.index(d)] += slides[i].num_edges((s, _, d))
        nf, ef = [lay.n_cap[t] - n[t] for t in range(lay.T)], [lay.e_cap[t] - e[t] for t in range(lay.T)]
        empty = G.filler_graph(lay.ntypes, lay.rels, [0] * lay.T, [0] * lay.T, C.IN_DIM)
        return [empty] * (lay.b_cap - len(idxs)) + [G.filler_graph(lay.ntypes, lay.rels, nf, ef, C.IN_DIM)]

    return slides, extra


@pytest.fixture(scope="module")
def homo():
    """The same slides as ``graph.to_homogeneous`` output with self-loops (no ``sim`` field), their loader and a slot sized for any two."""
    from wsi_hgnn_amd import graph as G
    from wsi_hgnn_amd.data import BatchSlot, GraphBatchLoader
    slides = [G.to_homogeneous(g, add_self_loop=True) for g in C.slides()]
    ld = GraphBatchLoader(slides, C.LABELS, 2, "cpu", shuffle=False, resident=True)
    slot = BatchSlot(ld)
    lay = slot.layout

    def extra(idxs):
        nf = [lay.n_cap[0] - sum(slides[i].num_nodes() for i in idxs)]
        ef = [lay.e_cap[0] - sum(slides[i].num_edges() for i in idxs)]
        empty = G.filler_graph(lay.ntypes, lay.rels, [0], [0], C.IN_DIM)
        return [empty] * (lay.b_cap - len(idxs)) + [G.filler_graph(lay.ntypes, lay.rels, nf, ef, C.IN_DIM)]

    return slides, extra, ld, slot


def _models():
    from oracle import models as OM
    torch.manual_seed(11)
    # ('att' sizes pools[0]'s gate for in_dim and HEATNet4 applies it to the hidden states: hidden = in_dim, models/HEATNet4.py:182-187, :219)
    return {"HEATNet4": OM.HEATNet4(C.IN_DIM, C.IN_DIM, 2, 2, 4, C.ND, 0.0, "att").double(),
            "GCN": OM.GCN(C.IN_DIM, 64, 2, 2, F.relu, 0.0, "att").double()}


def _run(m, g, labels):
    m.zero_grad(set_to_none=True)
    logits = m(g)
    logits.retain_grad()
    loss = torch.nn.CrossEntropyLoss()(logits, labels)
    loss.backward()
    return logits, loss.detach().clone(), {k: (None if p.grad is None else p.grad.clone()) for k, p in m.named_parameters()}


@pytest.mark.parametrize("idxs", BATCHES)
@pytest.mark.parametrize("name", ["GCN", "HEATNet4"])
def test_filler_changes_no_logit_no_loss_and_no_gradient_under_att(hetero, homo, name, idxs):
    """Bound: 1e-12 relative to the largest entry of the tensor compared - the two runs sum the same float64 numbers, the padded one with exact
    zeros in between.  The filler's rows stay finite through GraphConv / the HEAT layers and the softmax of the readout (its logits are
    finite), its graph and the empty graphs carry label -100, and so the gradient that reaches their logits is exactly zero - as is every
    parameter gradient of a loss over those graphs alone."""
    import wsi_hgnn_amd as W
    slides, extra = (homo if name == "GCN" else hetero)[:2]
    m = _models()[name]
    y = torch.tensor([C.LABELS[i] for i in idxs])
    ypad = torch.cat([y, torch.full((GRAPHS - len(idxs),), -100)])
    plain = _double(W.batch([slides[i] for i in idxs]))
    padded = _double(W.batch([slides[i] for i in idxs] + extra(idxs)))
    lp, lossp, gp = _run(m, plain, y)
    lq, lossq, gq = _run(m, padded, ypad)
    rel = lambda a, b: (a - b).abs().max().item() / max(b.abs().max().item(), 1e-300)
    assert lq.shape == (GRAPHS, 2) and torch.isfinite(lq).all()
    assert rel(lq.detach()[:len(idxs)], lp.detach()) <= 1e-12 and rel(lossq, lossp) <= 1e-12
    assert not lq.grad[len(idxs):].any() and lq.grad[:len(idxs)].any()               # what reaches the filler's and the empty graphs' logits
    for k, a in gp.items():
        b = gq[k]
        assert (a is None) == (b is None), k
        if a is not None and k.endswith("gate_nn.bias"):
            # a softmax ignores a shift of its gates: this gradient is 0 up to rounding (1e-19 here) and has no scale of its own - it is held
            # against the scale of the gate's weight gradient, the other half of g_w | g_b
            top = gp[k[:-4] + "weight"].abs().max().item()
            assert top > 0 and (b - a).abs().max().item() <= 1e-12 * top, k
        elif a is not None and a.abs().max() > 0:
            assert rel(b, a) <= 1e-12, k
        elif a is not None:
            assert not b.any(), k
    # the filler alone: a loss over the graphs labelled -100 gives exactly zero in every parameter gradient
    m.zero_grad(set_to_none=True)
    torch.nn.CrossEntropyLoss(reduction="sum")(m(padded)[len(idxs):], ypad[len(idxs):]).backward()
    for k, p in m.named_parameters():
        assert p.grad is None or not p.grad.any(), k


@pytest.mark.parametrize("idxs", BATCHES)
def test_degree_norm_tables_equal_the_plan_of_the_padded_graph(homo, idxs):
    import wsi_hgnn_amd as W
    from wsi_hgnn_amd.models.GCN import HomoPlan, homo_plan
    slides, extra, ld, slot = homo
    slot.load([0, 1]).load(idxs)                      # (over a larger batch: nothing of it may stay)
    ref = HomoPlan(W.batch([slides[i] for i in idxs] + extra(idxs)))
    hp = homo_plan(slot.graph)
    assert hp.num_nodes == slot.layout.N == ref.num_nodes and hp.num_edges == slot.layout.E == ref.num_edges
    assert hp.in_norm is slot.bufs["in_norm"] and hp.out_norm is slot.bufs["out_norm"]
    assert torch.equal(hp.in_norm, ref.in_norm) and torch.equal(hp.out_norm, ref.out_norm)
    assert torch.isfinite(hp.in_norm).all() and (hp.in_norm <= 1).all() and (hp.out_norm <= 1).all()
    assert torch.equal(hp.rowptr, ref.rowptr) and torch.equal(hp.colptr, ref.colptr)


def test_a_slide_without_sim_is_stored_with_zeros(homo):
    slides, _, ld, _ = homo
    assert all("sim" not in slides[0]._eframes[r] for r in slides[0].canonical_etypes)
    it = ld.items[0]
    assert all(not s.any() and s.numel() == slides[0].num_edges(r) for r, s in it.sims.items())


def test_slot_checks_admit_att_and_gcn_and_keep_the_other_refusals(homo):
    """``_check_slots`` up to the device test (CPU slots): GCN wants homogeneous slots, 'att' wants a gate as wide as the states it pools."""
    from wsi_hgnn_amd import models
    from wsi_hgnn_amd.data import BatchSlot
    from wsi_hgnn_amd.trainer import _check_slots
    _, _, _, hslot = homo
    het = BatchSlot(C.loader("cpu"), C.BIG)
    gcn = models.GCN(C.IN_DIM, 64, 2, 2, F.relu, 0.0, "att")
    with pytest.raises(RuntimeError, match="homogeneous"):
        _check_slots("t", "step", gcn, het)
    with pytest.raises(RuntimeError, match="on the GPU"):                              # everything before the device test passed
        _check_slots("t", "step", gcn, hslot)
    with pytest.raises(RuntimeError, match="on the GPU"):
        _check_slots("t", "step", models.HEATNet4(C.IN_DIM, C.IN_DIM, 2, 2, 4, C.ND, 0.0, "att"), het)
    with pytest.raises(RuntimeError, match="attention readout.*in_dim == hidden_dim"):
        _check_slots("t", "step", models.HEATNet4(C.IN_DIM, 64, 2, 2, 4, C.ND, 0.0, "att"), het)
    with pytest.raises(RuntimeError, match="not supported"):
        _check_slots("t", "step", models.GAT(2, C.IN_DIM, 8, 2, [2, 2, 1], F.leaky_relu, 0.0, 0.0, 0.2, False, "att"), hslot)
