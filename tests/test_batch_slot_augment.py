"""Augmented slides in padded batch slots on the CPU: the tensor route of ``BatchSlot.load`` over a loader with ``transform=`` - the
slot's tables against ``graph.slot_fill_torch`` over the augmented slides stored anew, the processing orders against the restriction rule, the
filler against a float64 oracle model, the ``fits`` rule and the refusals, the default draws, and the layout header (csrc/slot_layout.h) as a
stand-alone host program under the address and undefined-behaviour sanitizers.  Fixture: tests/slot_cases.py."""
import os
import subprocess
from collections import OrderedDict

import pytest
import torch

import slot_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 611


def pipelines():
    from wsi_hgnn_amd import transforms as T
    return {"REF": T.reference_train_transform(),
            "HARD": T.Compose([T.DropNode(0.9), T.DropEdge(0.5), T.NodeShuffle(), T.FeatMask(0.5, node_feat_names=["feat"])]),
            "EDGE_FIRST": T.Compose([T.DropEdge(0.3), T.NodeShuffle(), T.DropNode(0.5)])}


def aug_loader(device, pipe, seed=SEED):
    from wsi_hgnn_amd.data import GraphBatchLoader
    return GraphBatchLoader(_slides(), C.LABELS, 2, device, shuffle=False, resident=True, seed=seed, transform=pipe)


_CACHE = {}


def _slides():
    if "slides" not in _CACHE:
        _CACHE["slides"] = C.slides()
    return _CACHE["slides"]


def draws_of(counter, idxs):
    from wsi_hgnn_amd.data import augment_draw
    return [augment_draw(SEED, counter, i) for i in idxs]


def augmented_slide(ld, pipe, i, draw):
    """Slide i of the loader through the tensor formulation of the pipeline: (augmented graph, DropNode's keep flags per node type)."""
    from wsi_hgnn_amd.data import slot_augment_spec
    from wsi_hgnn_amd.graph import HeteroGraph
    it = ld.items[i]
    g = HeteroGraph.from_coo(OrderedDict(zip(it.ntypes, it.num_nodes)), it.edges, feat=dict(zip(it.ntypes, it.feat)), sim=it.sims)
    return pipe(g, draw=draw, fused=False), slot_augment_spec(pipe).node_keep(draw, it.num_nodes, ld.device)


def expected_tables(ld, slot, pipe, idxs, draws):
    """The contract, spelled out: slot_fill_torch over the augmented slides stored anew; the two orders by the restriction rule, from the
    UNAUGMENTED fill's order tables and the keep flags of the draw contract."""
    from wsi_hgnn_amd import graph as G
    from wsi_hgnn_amd.data import StoredGraph
    lay, T = slot.layout, slot.layout.T
    its = [ld.items[i] for i in idxs]
    got = [augmented_slide(ld, pipe, i, d) for i, d in zip(idxs, draws)]
    aug = [StoredGraph(g, it.label, ld.device, True) for (g, _), it in zip(got, its)]
    out = G.slot_fill_torch(lay, [a.pieces for a in aug], [a.label for a in aug], [a.feat for a in aug], None, ld.device, allow_empty_type=True)
    sb = out["batch"]
    plain = G.slot_fill_torch(lay, [it.pieces for it in its], [it.label for it in its], [it.feat for it in its], None, ld.device)
    pb = plain["batch"]
    to_aug = torch.full((lay.N,), -1, dtype=torch.int64)                   # id in the unaugmented padded batch -> id in the augmented one
    for b, (_, keep) in enumerate(got):
        for t in range(T):
            k = keep[t].cpu()
            a = pb.node_tab[b * T + t]
            to_aug[a:a + k.numel()] = torch.where(k, sb.node_tab[b * T + t] + torch.cumsum(k.long(), 0) - 1, torch.full((k.numel(),), -1))
    filler = torch.cat([sb.fb[t] + torch.arange(sb.nf[t]) for t in range(T)])
    for key in ("order_dst", "order_src"):
        m = to_aug[plain[key].long().cpu()[:sum(pb.n)]]
        out[key] = torch.cat([m[m >= 0], filler]).to(torch.int32)
    return out


def same(a, b):
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    if a.dtype == torch.float32:
        a, b = a.contiguous().view(torch.int32), b.contiguous().view(torch.int32)
    return torch.equal(a.cpu(), b.cpu())


@pytest.fixture(scope="module")
def slots():
    from wsi_hgnn_amd.data import BatchSlot
    out = {}
    for name, pipe in pipelines().items():
        ld = aug_loader("cpu", pipe)
        out[name] = (ld, pipe, BatchSlot(ld, C.BIG), BatchSlot(ld, C.SMALL))
    return out


@pytest.mark.parametrize("name", ["REF", "HARD", "EDGE_FIRST"])
@pytest.mark.parametrize("which,idxs", [("big", c) for c in C.CASES] + [("small", c) for c in C.SMALL_CASES])
def test_cpu_slot_tables_are_those_of_the_augmented_padded_batch(slots, name, which, idxs):
    ld, pipe, big, small = slots[name]
    slot = big if which == "big" else small
    N = slot.layout.N
    for counter in range(3):
        draws = draws_of(counter, idxs)
        slot.load_augmented(idxs, draws)
        ref = expected_tables(ld, slot, pipe, idxs, draws)
        for k, v in ref.items():
            if k != "batch":
                assert same(slot.bufs[k], v), (name, idxs, counter, k)
        for k in ("order_dst", "order_src"):
            assert torch.equal(torch.sort(slot.bufs[k].long()).values, torch.arange(N)), (name, idxs, counter, k)
        n, e = slot.counts()
        sb = ref["batch"]
        assert [sum(x[t] for x in n) for t in range(3)] == sb.n and [sum(x[t] for x in e) for t in range(3)] == sb.e
        share = slot.padded_share()
        assert share == (sum(sb.nf) / N, sum(sb.ef) / slot.layout.E)


def test_the_fixture_draws_hit_the_edge_cases(slots):
    """What the cases are there for (computed once at seed 611): HARD empties a whole node type of a slide, a relation's destination type, and
    every edge of a slide; REF empties nothing."""
    ld, pipe, big, _ = slots["HARD"]
    big.load_augmented([3, 4], draws_of(0, [3, 4]))
    n, e = big.counts()
    assert n == [[4, 5, 1], [0, 5, 1]] and e[0][2] == 0
    big.load_augmented([5, 3], draws_of(1, [5, 3]))
    assert big.counts()[1][0] == [0, 0, 0]
    big.load_augmented([4], draws_of(2, [4]))
    assert big.counts()[0][0][1] == 0
    ld, pipe, big, _ = slots["REF"]
    for counter in range(3):
        for idxs in ([0, 1], [2]):
            big.load_augmented(idxs, draws_of(counter, idxs))
            assert all(x > 0 for row in big.counts()[0] for x in row)


def _double(g):
    for t in g.ntypes:
        g.nodes[t].data["feat"] = g.nodes[t].data["feat"].double()
    for r in g.canonical_etypes:
        g._eframes[r]["sim"] = g._eframes[r]["sim"].double()
    return g


@pytest.mark.parametrize("name,idxs", [("REF", [0, 1]), ("REF", [2]), ("EDGE_FIRST", [1, 2]), ("HARD", [0, 1])])
def test_filler_of_an_augmented_slot_changes_no_logit_no_loss_and_no_gradient(slots, name, idxs):
    """Oracle HEATNet4 in float64 on the padded augmented batch against the unpadded augmented batch: logits, loss and every parameter gradient
    agree to 1e-12 relative to the tensor's largest entry (the two runs sum the same numbers, the padded one with exact zeros in between); a
    gradient that is numerically zero in one run must be so in the other (see the comment at the assertion)."""
    import wsi_hgnn_amd as W
    from wsi_hgnn_amd import graph as G
    from oracle import models as OM
    ld, pipe, big, _ = slots[name]
    lay = big.layout
    draws = draws_of(0, idxs)
    big.load_augmented(idxs, draws)
    sb = big.batch
    mk = lambda: [augmented_slide(ld, pipe, i, d)[0] for i, d in zip(idxs, draws)]
    extra = lambda: [G.filler_graph(lay.ntypes, lay.rels, [0] * lay.T, [0] * lay.T, C.IN_DIM)] * (lay.b_cap - len(idxs)) + \
        [G.filler_graph(lay.ntypes, lay.rels, sb.nf, sb.ef, C.IN_DIM)]
    torch.manual_seed(11)
    m = OM.HEATNet4(C.IN_DIM, 64, 2, 2, 4, C.ND, 0.0, "mean").double()
    lf = torch.nn.CrossEntropyLoss()
    y = torch.tensor([C.LABELS[i] for i in idxs])
    plain, padded = _double(W.batch(mk())), _double(W.batch(mk() + extra()))
    assert [padded.num_nodes(t) for t in padded.ntypes] == lay.n_cap
    # the slot's own graph IS that padded batch: node counts, features, COO
    for t in padded.ntypes:
        assert big.graph.batch_num_nodes(t).tolist() == padded.batch_num_nodes(t).tolist()
        assert torch.equal(big.graph.nodes[t].data["feat"].double(), padded.nodes[t].data["feat"])
    for r in padded.canonical_etypes:
        assert torch.equal(big.graph.edges(r)[0], padded.edges(r)[0]) and torch.equal(big.graph.edges(r)[1], padded.edges(r)[1]), r
    out = {}
    for key, g, lab in (("plain", plain, y), ("padded", padded, torch.cat([y, torch.full((3 - len(idxs),), -100)]))):
        m.zero_grad(set_to_none=True)
        logits = m(g)
        loss = lf(logits, lab)
        loss.backward()
        out[key] = (logits.detach()[:len(idxs)].clone(), loss.detach().clone(), {k: (None if p.grad is None else p.grad.clone()) for k, p in m.named_parameters()})
    rel = lambda a, b: (a - b).abs().max().item() / max(b.abs().max().item(), 1e-300)
    assert rel(out["padded"][0], out["plain"][0]) <= 1e-12
    assert rel(out["padded"][1], out["plain"][1]) <= 1e-12
    top = max(gp.abs().max().item() for gp in out["plain"][2].values() if gp is not None)       # the model's gradient scale
    for k, gp in out["plain"][2].items():
        gq = out["padded"][2][k]
        assert (gp is None) == (gq is None), k
        if gp is not None:
            print(k, "largest entry", gp.abs().max().item(), "difference", (gq - gp).abs().max().item())
    # A gradient can cancel to zero: the softmax over a destination's ONE edge has p = 1 and passes p (g - p g) on.  Such a tensor is exactly 0 in
    # one run and round-off of the cancelled terms in the other (other matrix shapes, other blocking on another CPU: 5e-26 was seen beside
    # gradients of 1e-1), and has no entry of its own to be relative to.  The terms that cancel are of the model's gradient scale `top`, so a
    # tensor whose largest entry is below ONE float64 round-off unit of that scale (2 ** -52 * top) is numerically zero, and the other run's must
    # be numerically zero too; every other tensor keeps the 1e-12 of its own largest entry.
    floor = 2.0 ** -52 * top
    for k, gp in out["plain"][2].items():
        gq = out["padded"][2][k]
        if gp is None:
            continue
        if gp.abs().max().item() > floor:
            assert rel(gq, gp) <= 1e-12, k
        else:
            assert gq.abs().max().item() <= floor, (k, gq.abs().max().item(), floor)


def test_fits_rule_and_refusals(slots):
    from wsi_hgnn_amd import transforms as T
    from wsi_hgnn_amd.data import BatchSlot, GraphBatchLoader
    _, _, big, small = slots["REF"]
    assert big.fits([0, 1]) and big.fits([2])
    assert not big.fits([4]) and not big.fits([5, 3])            # 12 and 24 nodes of type 2: 0.5 ** n > 2 ** -32
    assert small.fits([3, 4]) and not small.fits([3])
    with pytest.raises(ValueError, match="does not fit"):
        big.load([4])
    _, _, hard, hard_small = slots["HARD"]                        # 0.9 ** n <= 2 ** -32 needs n >= 211
    assert not any(hard.fits(c) for c in C.CASES) and not any(hard_small.fits(c) for c in C.SMALL_CASES)
    nodrop = BatchSlot(aug_loader("cpu", T.Compose([T.DropEdge(0.5), T.FeatMask(0.5, node_feat_names=["feat"])])), C.BIG)
    assert nodrop.fits([4]) and nodrop.fits([5, 3])               # without DropNode the rule is always true
    gs = _slides()[:2]
    mk = lambda tr: GraphBatchLoader(gs, [0, 1], 2, "cpu", resident=True, transform=tr)
    for tr in (lambda g, draw=0: g, T.Compose([T.DropEdge(0.5), T.DropNode(0.5), T.DropEdge(0.2)]), T.Compose([T.FeatMask(0.5, edge_feat_names=["sim"])]),
               T.Compose([T.DropNode(0.5), lambda g: g]), T.DropNode(0.5), T.Compose([T.FeatMask(0.5, node_feat_names=["feat", "x"])])):
        with pytest.raises(RuntimeError, match="transform"):
            BatchSlot(mk(tr))
    with pytest.raises(ValueError, match="draws"):
        BatchSlot(C.loader("cpu"), C.BIG).load([0, 1], draws=[1, 2])


def test_default_draws_follow_the_loaders_batch_counter():
    """draws=None: augment_draw(seed, running batch counter, slide) - two loaders under one seed fill the same tables, a second load of the same
    batch another draw; the eager route (_augmented) advances the same counter, so slot fills and eager batches interleave on one sequence."""
    from wsi_hgnn_amd.data import BatchSlot
    pipe = pipelines()["REF"]
    l1, l2 = aug_loader("cpu", pipe), aug_loader("cpu", pipe)
    s1, s2 = BatchSlot(l1, C.BIG), BatchSlot(l2, C.BIG)
    s1.load([0, 1]); s2.load([0, 1])
    assert s1.draws == draws_of(0, [0, 1]) and l1._batches_drawn == 1
    first = {k: v.clone() for k, v in s1.bufs.items()}
    assert all(same(v, s2.bufs[k]) for k, v in first.items())
    s1.load([0, 1])
    assert s1.draws == draws_of(1, [0, 1]) and not same(first["feat"], s1.bufs["feat"]) and not same(first["src"], s1.bufs["src"])
    l2._augmented([0, 1])                                          # the eager route takes draw 1 of the other loader
    s2.load([2]); s1.load([2])
    assert s1.draws == s2.draws == draws_of(2, [2]) and all(same(v, s2.bufs[k]) for k, v in s1.bufs.items())
    explicit = BatchSlot(aug_loader("cpu", pipe), C.BIG).load([2], draws=draws_of(2, [2]))
    assert all(same(v, explicit.bufs[k]) for k, v in s1.bufs.items()) and explicit.loader._batches_drawn == 0


def test_layout_header_against_a_plain_reimplementation_under_sanitizers(tmp_path):
    """csrc/slot_layout.h is what the layout kernel turns the device-side counts into offsets, filler block, readout pointers, chunk tables and
    segment counts with; compiled for the host into tests/slot_aug_check.cpp it must reproduce graph.SlotBatch's arithmetic, re-implemented
    plainly, on 4000 random count tables - zeros, empty (slide, type) segments, B < b_cap - without touching a guard word (ASan + UBSan)."""
    exe = str(tmp_path / "slot_aug_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "wsi-hgnn_amd", "csrc"), os.path.join(ROOT, "tests", "slot_aug_check.cpp"), "-o", exe])
    res = subprocess.run([exe], capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "4000 count tables, 0 mismatches" in res.stdout
