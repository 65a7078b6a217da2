"""Survivor quotas of augmented batch slots on the CPU: the "bound" quota against a plain restatement and against 300 draws per
slide, a quota slot whose quotas do not bind against today's slot, binding quotas (set through a callable) against ``graph.slot_fill_torch``
over the truncated tensor formulation with the overflow words, the padded truncated batch against the unpadded one in float64, and ``fits``
with the derived capacities.  Helpers: tests/quota_cases.py; slides: tests/slot_cases.py."""
import pytest
import torch

import quota_cases as Q
import slot_cases as C

NAMES = ["REF", "HARD", "EDGE_FIRST"]


@pytest.fixture(scope="module")
def loaders():
    return {name: (Q.aug_loader("cpu", pipe), pipe) for name, pipe in Q.pipelines().items()}


@pytest.fixture(scope="module")
def bound_slots(loaders):
    from wsi_hgnn_amd.data import BatchSlot
    return {name: BatchSlot(ld, quota="bound") for name, (ld, _) in loaders.items()}


# ------------------------------------------------------------------ 1. the bound
@pytest.mark.parametrize("name", NAMES)
def test_bound_quota_is_the_stated_rule(loaders, name):
    from wsi_hgnn_amd import transforms as T
    from wsi_hgnn_amd.data import slot_augment_spec, slot_quota_bound
    ld, pipe = loaders[name]
    spec = slot_augment_spec(pipe)
    pn, pe = Q.stage_probabilities(pipe)
    for i, it in enumerate(ld.items):
        qn, qe = slot_quota_bound(it, spec)
        assert (qn, qe) == Q.restated_bound(Q.stored_graph(ld, i), pn, pe), (name, i)
        sn, se = Q.stored_quota(ld, i)
        assert all(0 <= a <= b for a, b in zip(qn, sn)) and all(0 <= a <= b for a, b in zip(qe, se)), (name, i)
        assert slot_quota_bound(it, spec) is slot_quota_bound(it, spec)                   # cached per slide and spec
    # without DropNode the node quota is the stored count, and a node quota has no effect on the pipeline
    nodrop = T.Compose([T.DropEdge(0.5), T.NodeShuffle(), T.FeatMask(0.5, node_feat_names=["feat"])])
    spec0 = slot_augment_spec(nodrop)
    for i in (0, 4, 5):
        assert slot_quota_bound(ld.items[i], spec0)[0] == list(ld.items[i].num_nodes)
        assert slot_quota_bound(ld.items[i], spec0)[1] == Q.restated_bound(Q.stored_graph(ld, i), None, 0.5)[1]
        g = Q.stored_graph(ld, i)
        a, b = nodrop(g, draw=77, fused=False), nodrop(g, draw=77, quota=([0, 0, 0], None))
        for t in a.ntypes:
            assert a.num_nodes(t) == b.num_nodes(t) and torch.equal(a.nodes[t].data["feat"], b.nodes[t].data["feat"])
        for r in a.canonical_etypes:
            assert torch.equal(a.edges(r)[0], b.edges(r)[0]) and torch.equal(a.edges(r)[1], b.edges(r)[1])


@pytest.mark.parametrize("i", range(8))
def test_no_bound_quota_binds_in_300_draws_of_the_reference_pipeline(loaders, i):
    """A condition, not a measurement: the bound makes a binding draw a 2 ** -32 event per table."""
    from collections import OrderedDict
    from wsi_hgnn_amd.data import augment_draw, slot_augment_spec, slot_quota_bound
    from wsi_hgnn_amd.graph import HeteroGraph
    ld, pipe = loaders["REF"]
    it = ld.items[i]
    qn, qe = slot_quota_bound(it, slot_augment_spec(pipe))
    worst_n, worst_e = [0] * len(qn), [0] * len(qe)
    topo = HeteroGraph.from_coo(OrderedDict(zip(it.ntypes, it.num_nodes)), it.edges)          # the counts need no feature rows
    for counter in range(300):
        g = pipe(topo, draw=augment_draw(Q.SEED, counter, i), fused=False)
        n, e = [g.num_nodes(t) for t in g.ntypes], [int(g.edges(r)[0].numel()) for r in g.canonical_etypes]
        worst_n, worst_e = [max(a, b) for a, b in zip(worst_n, n)], [max(a, b) for a, b in zip(worst_e, e)]
    print("slide", i, "quota", qn, qe, "largest drawn", worst_n, worst_e)
    assert all(a <= q for a, q in zip(worst_n, qn)) and all(a <= q for a, q in zip(worst_e, qe)), i


def _plainly_truncated(pipe, g, draw, qn, qe):
    """The contract by another route: DropNode as ``graph.remove_nodes`` of (the drawn nodes and the kept ones of rank >= quota), one type after
    the other; every other stage as it stands; at the end the first ``qe[j]`` edges of every relation."""
    from collections import OrderedDict
    from wsi_hgnn_amd import graph as G, ops, transforms as T
    seed = int(draw) & 0xffffffff
    for k, t in enumerate(pipe.transforms):
        if not isinstance(t, T.DropNode):
            g = t.apply(g, seed, k)
            continue
        for j, nt in enumerate(g.ntypes):
            gone, kept = [], 0
            drawn = ops.augment_drawn(g.num_nodes(nt), ops.augment_subseed(seed, k, j), t.threshold, "cpu").tolist()
            for i, d in enumerate(drawn):
                if d or kept >= qn[j]:
                    gone.append(i)
                else:
                    kept += 1
            g = G.remove_nodes(g, torch.tensor(gone, dtype=torch.int64), nt)
    edges = OrderedDict((r, (g.edges(r)[0][:qe[j]], g.edges(r)[1][:qe[j]])) for j, r in enumerate(g.canonical_etypes))
    out = G.HeteroGraph.from_coo(OrderedDict((t, g.num_nodes(t)) for t in g.ntypes), edges, feat={t: g.nodes[t].data["feat"] for t in g.ntypes},
                                 sim={r: g._eframes[r]["sim"][:qe[j]] for j, r in enumerate(g.canonical_etypes)})
    return out


@pytest.mark.parametrize("name", NAMES)
def test_truncated_pipeline_is_the_stated_semantics(loaders, name):
    """transforms.truncated against the contract spelled out with graph.remove_nodes, under quotas that bind (a third of the stored nodes, a
    twentieth of the edges), that bind in part, and that do not bind (then: the pipeline as drawn, bit for bit)."""
    from wsi_hgnn_amd import transforms as T
    ld, pipe = loaders[name]
    for i in (0, 3, 5, 6):
        sn, se = Q.stored_quota(ld, i)
        for qn, qe in (([n // 3 for n in sn], [e // 20 for e in se]), ([sn[0] // 3, sn[1], sn[2]], se), (sn, [se[0] // 20] + se[1:]), (sn, se)):
            draw = 1000 + i
            got, xn, xe = T.truncated(pipe, Q.stored_graph(ld, i), draw, qn, qe)
            ref = _plainly_truncated(pipe, Q.stored_graph(ld, i), draw, qn, qe)
            assert pipe(Q.stored_graph(ld, i), draw=draw, quota=(qn, qe)).num_edges() == got.num_edges()
            if (qn, qe) == (sn, se):
                ref = pipe(Q.stored_graph(ld, i), draw=draw, fused=False)
                assert not any(xn) and not any(xe)
            for t in ref.ntypes:
                assert got.num_nodes(t) == ref.num_nodes(t) and Q.same(got.nodes[t].data["feat"], ref.nodes[t].data["feat"]), (name, i, t)
            for r in ref.canonical_etypes:
                assert torch.equal(got.edges(r)[0], ref.edges(r)[0]) and torch.equal(got.edges(r)[1], ref.edges(r)[1]), (name, i, r)
                assert Q.same(got._eframes[r]["sim"], ref._eframes[r]["sim"]), (name, i, r)


# ------------------------------------------------------------------ 2. a quota that does not bind
def _live(slot, B):
    """The real slides' part of a CPU slot in a form that does not depend on its capacities: node counts, feature rows, per-relation COO (ids
    count inside the node type) and sim of the real edges, labels."""
    from wsi_hgnn_amd import graph
    G = slot.graph
    n, e = slot.counts()
    out = {"counts": (n, e), "labels": slot.labels[:B].clone()}
    real = {t: sum(x[j] for x in n) for j, t in enumerate(G.ntypes)}
    for t in G.ntypes:
        out["nodes", t] = G.batch_num_nodes(t)[:B].clone()
        out["feat", t] = G.nodes[t].data["feat"][:real[t]].clone()
    sb = slot.batch
    fg = graph.filler_graph(G.ntypes, G.canonical_etypes, sb.nf, sb.ef, 0)
    for r in G.canonical_etypes:
        u, v = G.edges(r)
        k = u.numel() - fg.edges(r)[0].numel()
        out["edges", r] = (u[:k].clone(), v[:k].clone())
    return out


@pytest.mark.parametrize("name", NAMES)
def test_a_quota_that_does_not_bind_changes_nothing(loaders, bound_slots, name):
    from wsi_hgnn_amd.data import BatchSlot
    ld, pipe = loaders[name]
    quota, today = bound_slots[name], BatchSlot(ld, C.BIG)
    lay = quota.layout
    assert lay.N < today.layout.N and lay.E < today.layout.E
    for idxs in C.CASES:
        for counter in range(3):
            draws = Q.draws_of(counter, idxs)
            quota.load_augmented(idxs, draws)
            today.load_augmented(idxs, draws)
            a, b = _live(quota, len(idxs)), _live(today, len(idxs))
            assert a.keys() == b.keys()
            for k in a:
                if k == "counts":
                    assert a[k] == b[k], (name, idxs, counter)
                elif k[0] == "edges":
                    assert torch.equal(a[k][0], b[k][0]) and torch.equal(a[k][1], b[k][1]), (name, idxs, counter, k)
                else:
                    assert Q.same(a[k], b[k]), (name, idxs, counter, k)
            ref = Q.expected_tables(ld, quota, pipe, idxs, draws)          # every table, in the quota slot's own layout
            for k, v in ref.items():
                if k != "batch":
                    assert Q.same(quota.bufs[k], v), (name, idxs, counter, k)
            sq, st = quota.padded_share(), today.padded_share()
            assert sq[0] < st[0] and sq[1] < st[1], (name, idxs, counter, sq, st)
    assert quota.overflows() == 0 and quota.overflow_excess() == (0, 0)


# ------------------------------------------------------------------ 3. binding quotas
@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("case", Q.BINDING)
def test_binding_quotas_truncate_as_the_tensor_formulation_says(loaders, name, case):
    from wsi_hgnn_amd.data import BatchSlot
    ld, pipe = loaders[name]
    idxs = Q.BATCH
    fills, worst_n, worst_e = 0, 0, 0
    table = {}
    slot = BatchSlot(ld, C.BIG, quota=lambda i: table[i])
    N = slot.layout.N
    for counter in range(2):
        draws = Q.draws_of(counter, idxs)
        quotas, xn, xe = Q.binding_quotas(ld, pipe, idxs, draws, case)
        table.clear(); table.update(quotas); slot._quotas.clear()              # (another draw, other survivors: other limits)
        slot.load_augmented(idxs, draws)
        ref = Q.expected_tables(ld, slot, pipe, idxs, draws)
        for k, v in ref.items():
            if k != "batch":
                assert Q.same(slot.bufs[k], v), (name, case, counter, k)
        for k in ("order_dst", "order_src"):
            assert torch.equal(torch.sort(slot.bufs[k].long()).values, torch.arange(N)), (name, case, counter, k)
        sb = ref["batch"]
        n, e = slot.counts()
        assert [sum(x[t] for x in n) for t in range(3)] == sb.n and [sum(x[t] for x in e) for t in range(3)] == sb.e
        for b, i in enumerate(idxs):                                            # the truncated counts respect every quota
            assert all(a <= q for a, q in zip(n[b], quotas[i][0])) or Q.stage_probabilities(pipe)[0] is None
        fills += int(xn > 0 or xe > 0)
        worst_n, worst_e = max(worst_n, xn), max(worst_e, xe)
        assert slot.overflows() == fills and slot.overflow_excess() == (worst_n, worst_e), (name, case, counter)
        if case == "node_zero":
            assert sb.n[2] == 0 and sb.nf[2] == slot.layout.n_cap[2]
    if name == "REF":
        assert fills == 2                                                       # at these sizes every REF case does bind
        assert (worst_n > 0) == (case not in ("edge_minus_one", "edge_zero")) and (worst_e > 0) == (case in ("edge_minus_one", "edge_zero", "both"))
    if case in ("node_minus_one", "edge_minus_one") and name == "REF":
        assert (worst_n, worst_e) == ((1, 0) if case == "node_minus_one" else (0, 1))


# ------------------------------------------------------------------ 4. float64 oracle
def _double(g):
    for t in g.ntypes:
        g.nodes[t].data["feat"] = g.nodes[t].data["feat"].double()
    for r in g.canonical_etypes:
        g._eframes[r]["sim"] = g._eframes[r]["sim"].double()
    return g


@pytest.mark.parametrize("name,case", [("REF", "both"), ("REF", "node_half"), ("EDGE_FIRST", "edge_minus_one")])
def test_filler_of_a_truncated_slot_changes_no_logit_no_loss_and_no_gradient(loaders, name, case):
    """Oracle HEATNet4 in float64 on the padded truncated batch against the unpadded truncated batch at 1e-12 relative to the tensor's largest
    entry, the bound (and the rule for gradients that cancel to zero) of the augmented slot's own oracle test."""
    import wsi_hgnn_amd as W
    from wsi_hgnn_amd import graph as G
    from wsi_hgnn_amd.data import BatchSlot
    from oracle import models as OM
    ld, pipe = loaders[name]
    idxs = Q.BATCH
    draws = Q.draws_of(0, idxs)
    quotas, xn, xe = Q.binding_quotas(ld, pipe, idxs, draws, case)
    assert xn > 0 or xe > 0
    slot = BatchSlot(ld, C.BIG, quota=Q.quota_fn(ld, quotas))
    lay = slot.layout
    slot.load_augmented(idxs, draws)
    sb = slot.batch
    mk = lambda: [Q.truncated_slide(ld, pipe, i, d, slot.quota_of(i))[0] for i, d in zip(idxs, draws)]
    extra = lambda: [G.filler_graph(lay.ntypes, lay.rels, [0] * lay.T, [0] * lay.T, C.IN_DIM)] * (lay.b_cap - len(idxs)) + \
        [G.filler_graph(lay.ntypes, lay.rels, sb.nf, sb.ef, C.IN_DIM)]
    torch.manual_seed(11)
    m = OM.HEATNet4(C.IN_DIM, 64, 2, 2, 4, C.ND, 0.0, "mean").double()
    lf = torch.nn.CrossEntropyLoss()
    y = torch.tensor([C.LABELS[i] for i in idxs])
    plain, padded = _double(W.batch(mk())), _double(W.batch(mk() + extra()))
    assert [padded.num_nodes(t) for t in padded.ntypes] == lay.n_cap
    for t in padded.ntypes:                                      # the slot's own graph IS that padded batch
        assert slot.graph.batch_num_nodes(t).tolist() == padded.batch_num_nodes(t).tolist()
        assert torch.equal(slot.graph.nodes[t].data["feat"].double(), padded.nodes[t].data["feat"])
    for r in padded.canonical_etypes:
        assert torch.equal(slot.graph.edges(r)[0], padded.edges(r)[0]) and torch.equal(slot.graph.edges(r)[1], padded.edges(r)[1]), r
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
    top = max(gp.abs().max().item() for gp in out["plain"][2].values() if gp is not None)
    floor = 2.0 ** -52 * top                                     # a gradient below one round-off unit of the model's gradient scale is numerically zero
    for k, gp in out["plain"][2].items():
        gq = out["padded"][2][k]
        assert (gp is None) == (gq is None), k
        if gp is None:
            continue
        if gp.abs().max().item() > floor:
            assert rel(gq, gp) <= 1e-12, k
        else:
            assert gq.abs().max().item() <= floor, (k, gq.abs().max().item(), floor)


# ------------------------------------------------------------------ 5. fits and capacities
def test_fits_and_derived_capacities(loaders, bound_slots):
    from wsi_hgnn_amd import transforms as T
    from wsi_hgnn_amd.data import BatchSlot, GraphBatchLoader, slot_augment_spec, slot_quota_bound
    ld, pipe = loaders["REF"]
    slot = bound_slots["REF"]
    lay, spec = slot.layout, slot_augment_spec(pipe)
    qs = [slot_quota_bound(it, spec) for it in ld.items]
    dst = [lay.hd.tindex[r[2]] for r in lay.rels]
    top2 = lambda xs: sum(sorted(xs, reverse=True)[:2])
    assert lay.n_cap == [top2([q[0][t] for q in qs]) + 1 for t in range(3)]
    assert lay.e_cap == [top2([sum(x for x, d in zip(q[1], dst) if d == t) for q in qs]) for t in range(3)] and lay.b_cap == 2
    assert slot.fits([0, 7]) and slot.fits([0, 1]) and slot.fits([2])           # every pair of the bucket fits the derived capacities
    assert not slot.fits([4]) and not slot.fits([5, 3])                         # the type-present rule of the augmented slot stays
    assert not slot.fits([]) and not slot.fits([0, 1, 2]) and not slot.fits([99])
    with pytest.raises(ValueError, match="does not fit"):
        slot.load([4])
    # explicit capacity: the quota sums decide, not the stored counts
    small = BatchSlot(ld, C.SMALL, quota="bound")
    sums = lambda idxs: [sum(qs[i][0][t] for i in idxs) for t in range(3)]
    assert sums([3]) [0] + 1 <= C.SMALL[0][0] and small.fits([3, 4]) == all(a + 1 <= c for a, c in zip(sums([3, 4]), C.SMALL[0]))
    assert not small.fits([0]) and sums([0])[0] + 1 > C.SMALL[0][0]             # quota sums above the capacity: no fit
    with pytest.raises(ValueError, match="does not fit"):
        small.load_augmented([0], Q.draws_of(0, [0]))
    # stored counts above the capacity, quotas below: fits (and fills)
    table = {i: ([n // 3 for n in Q.stored_quota(ld, i)[0]], [e // 8 for e in Q.stored_quota(ld, i)[1]]) for i in (0, 7)}
    tight = BatchSlot(ld, C.BIG, quota=Q.quota_fn(ld, table))
    assert not BatchSlot(ld, C.BIG).fits(C.NO_FIT) and tight.fits(C.NO_FIT)
    tight.load(C.NO_FIT, draws=Q.draws_of(0, C.NO_FIT))
    n, e = tight.counts()
    assert all(a <= q for b, i in enumerate(C.NO_FIT) for a, q in zip(n[b], table[i][0]))
    # quota=None: today's slot - no quota state, no overflow table, the stored counts decide
    plain = BatchSlot(ld, C.BIG)
    assert plain.quota is None and not hasattr(plain, "_overflow") and plain.overflows() == 0 and plain.overflow_excess() == (0, 0)
    assert plain.layout.n_cap == list(C.BIG[0]) and plain._counts([0]) == ([ld.items[0].num_nodes], [ld.items[0].pieces.ecount])
    default = BatchSlot(ld)
    assert default.layout.n_cap == [top2([it.num_nodes[t] for it in ld.items]) + 1 for t in range(3)]
    # refusals: quotas need a transform; the quota argument's forms
    with pytest.raises(RuntimeError, match="transform"):
        BatchSlot(C.loader("cpu"), C.BIG, quota="bound")
    with pytest.raises(ValueError, match="quota"):
        BatchSlot(ld, C.BIG, quota="tight")
    with pytest.raises(ValueError, match="one node quota per node type"):
        BatchSlot(ld, C.BIG, quota=lambda i: ([1], [1])).fits([0])
    gs = Q._slides()[:2]
    with pytest.raises(RuntimeError, match="transform"):
        BatchSlot(GraphBatchLoader(gs, [0, 1], 2, "cpu", resident=True, transform=T.DropNode(0.5)), quota="bound")
