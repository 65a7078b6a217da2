"""Train-time graph augmentation (wsi_hgnn_amd/transforms.py: DropNode, DropEdge, NodeShuffle, FeatMask, Compose - the pipeline of the reference's
data.py:16-23) in its tensor formulation on the CPU: semantics against ``graph.remove_nodes`` and against the draw contract of include/wsi_hgnn.h
replayed here with Python integers, edge cases, replay, rates, refusals and the loader's ``transform=`` route."""
import math
from collections import OrderedDict

import pytest
import torch

import wsi_hgnn_amd as W
from wsi_hgnn_amd import data, ops, synthetic, transforms as TR
from wsi_hgnn_amd.graph import HeteroGraph, remove_nodes, to_homogeneous

SEED = 0x1234ABCD


def _fmix(h):
    h &= 0xffffffff
    h ^= h >> 16
    h = (h * 0x85EBCA6B) & 0xffffffff
    h ^= h >> 13
    h = (h * 0xC2B2AE35) & 0xffffffff
    return h ^ (h >> 16)


def _hash(i, seed, k, j):
    """h(i) of the contract, in Python integers (independent of ops.augment_hash's tensor arithmetic)."""
    sub = _fmix(_fmix(seed + (k + 1) * 0x9E3779B1) + (j + 1) * 0x85EBCA6B)
    return _fmix(i * 0x9E3779B1 + sub)


def _drawn(n, seed, k, j, p):
    thr = int(round(p * 65536))
    return torch.tensor([(_hash(i, seed, k, j) & 0xffff) < thr for i in range(n)], dtype=torch.bool)


def _equal(a: HeteroGraph, b: HeteroGraph, fields=True):
    assert a.ntypes == b.ntypes and a.canonical_etypes == b.canonical_etypes
    assert [a.num_nodes(t) for t in a.ntypes] == [b.num_nodes(t) for t in b.ntypes]
    for r in a.canonical_etypes:
        assert torch.equal(a.edges(r)[0], b.edges(r)[0]) and torch.equal(a.edges(r)[1], b.edges(r)[1]), r
        if fields:
            assert set(a._eframes[r]) == set(b._eframes[r])
            for k in a._eframes[r]:
                assert torch.equal(a._eframes[r][k], b._eframes[r][k]), (r, k)
    if fields:
        for t in a.ntypes:
            assert set(a._nframes[t]) == set(b._nframes[t]), t
            for k in a._nframes[t]:
                assert torch.equal(a._nframes[t][k], b._nframes[t][k]), (t, k)


def _snapshot(g):
    return ({t: {k: x.clone() for k, x in g._nframes[t].items()} for t in g.ntypes},
            {r: ({k: x.clone() for k, x in g._eframes[r].items()}, g.edges(r)[0].clone(), g.edges(r)[1].clone()) for r in g.canonical_etypes})


def _unchanged(g, snap):
    nodes, rels = snap
    for t in g.ntypes:
        assert set(g._nframes[t]) == set(nodes[t])
        for k, x in nodes[t].items():
            assert torch.equal(g._nframes[t][k], x)
    for r in g.canonical_etypes:
        fr, u, v = rels[r]
        assert torch.equal(g.edges(r)[0], u) and torch.equal(g.edges(r)[1], v)
        for k, x in fr.items():
            assert torch.equal(g._eframes[r][k], x)


@pytest.fixture(scope="module")
def graph():
    g = synthetic.hetero_graph(300, 6, seed=5)
    for t in g.ntypes:
        g.nodes[t].data["tag"] = torch.arange(g.num_nodes(t))
    return g


def test_tensor_hash_matches_the_contract():
    for (k, j) in ((0, 0), (3, 2), (1, 65536 + 32768 + 5)):
        sub = ops.augment_subseed(SEED, k, j)
        assert ops.augment_hash(50, sub).tolist() == [_hash(i, SEED, k, j) for i in range(50)]
    assert ops.augment_threshold(0.5) == 32768 and ops.augment_threshold(1.0) == 65536 and ops.augment_threshold(0.0) == 0


def test_dropnode_equals_remove_nodes_type_by_type(graph):
    snap = _snapshot(graph)
    out = TR.DropNode(0.5)(graph, draw=SEED)
    ref = graph
    for j, t in enumerate(graph.ntypes):
        gone = torch.nonzero(_drawn(graph.num_nodes(t), SEED, 0, j, 0.5)).reshape(-1)
        assert 0 < gone.numel() < graph.num_nodes(t)
        ref = remove_nodes(ref, gone, ntype=t)
    _equal(out, ref)
    assert all(torch.equal(out.nodes[t].data["tag"], torch.nonzero(~_drawn(graph.num_nodes(t), SEED, 0, j, 0.5)).reshape(-1))
               for j, t in enumerate(graph.ntypes))
    _unchanged(graph, snap)


def test_dropedge_keeps_exactly_the_undrawn_edges_in_order(graph):
    snap = _snapshot(graph)
    out = TR.DropEdge(0.5)(graph, draw=SEED)
    for j, r in enumerate(graph.canonical_etypes):
        u, v = graph.edges(r)
        m = ~_drawn(u.numel(), SEED, 0, j, 0.5)
        assert 0 < int(m.sum()) < u.numel()
        assert torch.equal(out.edges(r)[0], u[m]) and torch.equal(out.edges(r)[1], v[m])
        assert torch.equal(out.edata["sim"][r], graph.edata["sim"][r][m])
    assert [out.num_nodes(t) for t in out.ntypes] == [graph.num_nodes(t) for t in graph.ntypes]
    _unchanged(graph, snap)


def test_nodeshuffle_permutes_rows_by_the_argsort_of_the_keys(graph):
    g = W.apply_locality_order(graph)
    snap = _snapshot(g)
    out = TR.NodeShuffle()(g, draw=SEED)
    moved = 0
    for j, t in enumerate(g.ntypes):
        keys = [_hash(i, SEED, 0, j) for i in range(g.num_nodes(t))]
        perm = torch.tensor(sorted(range(len(keys)), key=lambda i: (keys[i], i)))
        assert sorted(perm.tolist()) == list(range(g.num_nodes(t)))
        assert torch.equal(out.nodes[t].data["feat"], g.nodes[t].data["feat"][perm])
        assert torch.equal(out.nodes[t].data["tag"], g.nodes[t].data["tag"][perm])
        assert "_pos" not in out.nodes[t].data and "_pos" in g.nodes[t].data
        moved += int((perm != torch.arange(perm.numel())).sum())
    assert moved > 0
    for r in g.canonical_etypes:
        assert torch.equal(out.edges(r)[0], g.edges(r)[0]) and torch.equal(out.edges(r)[1], g.edges(r)[1])
        assert torch.equal(out.edata["sim"][r], g.edata["sim"][r])
    _unchanged(g, snap)


def test_featmask_zeroes_the_drawn_columns_per_type():
    g = synthetic.hetero_graph(60, 64, seed=9)
    for r in g.canonical_etypes:
        g._eframes[r]["w"] = torch.rand(g.num_edges(r), 8) + 1.0
    snap = _snapshot(g)
    out = TR.FeatMask(0.5, node_feat_names=["missing", "feat"], edge_feat_names=["w"])(g, draw=SEED)
    sets = []
    for j, t in enumerate(g.ntypes):
        z = _drawn(64, SEED, 0, 65536 * 1 + j, 0.5)           # "feat" is name number 1 of the list; "missing" is skipped
        x, y = g.nodes[t].data["feat"], out.nodes[t].data["feat"]
        assert 0 < int(z.sum()) < 64
        assert float(y[:, z].abs().max()) == 0.0 and torch.equal(y[:, ~z], x[:, ~z])
        sets.append(tuple(z.tolist()))
    assert len(set(sets)) == len(sets), "every node type draws its own columns"
    for j, r in enumerate(g.canonical_etypes):
        z = _drawn(8, SEED, 0, 32768 + j, 0.5)
        assert torch.equal(out._eframes[r]["w"][:, ~z], g._eframes[r]["w"][:, ~z]) and float(out._eframes[r]["w"][:, z].abs().sum()) == 0.0
        assert torch.equal(out.edata["sim"][r], g.edata["sim"][r])
    _equal(out, g, fields=False)
    _unchanged(g, snap)


def test_p0_returns_an_equal_graph(graph):
    for t in (TR.DropNode(0.0), TR.DropEdge(0.0), TR.FeatMask(0.0, node_feat_names=["feat"])):
        _equal(t(graph, draw=SEED), graph)


def test_p1_leaves_the_schema_and_heatnet2_still_runs(graph):
    from oracle import models as OM
    out = TR.DropNode(1.0)(graph, draw=SEED)
    assert out.ntypes == graph.ntypes and out.canonical_etypes == graph.canonical_etypes
    assert out.num_nodes() == 0 and out.num_edges() == 0
    assert all(out.nodes[t].data["feat"].shape == (0, 6) for t in out.ntypes)
    e = TR.DropEdge(1.0)(graph, draw=SEED)
    assert e.num_edges() == 0 and e.num_nodes() == graph.num_nodes()
    torch.manual_seed(0)
    m = OM.HEATNet2(6, 16, 2, 1, 2, {"0": 0, "1": 1, "2": 2}, 0.0, "mean")
    y = m(e)
    assert y.shape == (1, 2) and bool(torch.isfinite(y).all())
    y0 = m(out)           # runs; HEATNet2.py:189-194 skips every type without nodes, so what is left is the empty sum
    assert isinstance(y0, int) and y0 == 0
    z = TR.FeatMask(1.0, node_feat_names=["feat"])(graph, draw=SEED)
    assert all(float(z.nodes[t].data["feat"].abs().max()) == 0.0 for t in z.ntypes)


def test_empty_type_empty_relation_and_parallel_edges():
    nn_ = OrderedDict([("a", 0), ("b", 40)])
    e0 = torch.empty(0, dtype=torch.int64)
    u = torch.tensor([0, 0, 0, 5, 5, 7, 7, 7, 39, 39])
    v = torch.tensor([1, 1, 1, 6, 6, 7, 7, 8, 0, 0])              # parallel edges and self loops
    g = HeteroGraph.from_coo(nn_, OrderedDict([(("a", "x", "b"), (e0, e0)), (("b", "y", "b"), (u, v)), (("b", "z", "a"), (e0, e0))]),
                             feat={"a": torch.zeros(0, 4), "b": torch.rand(40, 4)},
                             sim={("a", "x", "b"): torch.empty(0), ("b", "y", "b"): torch.arange(10.0), ("b", "z", "a"): torch.empty(0)})
    pipe = TR.reference_train_transform()
    out = pipe(g, draw=SEED)
    assert out.ntypes == g.ntypes and out.canonical_etypes == g.canonical_etypes and out.num_nodes("a") == 0
    assert out.num_edges(("a", "x", "b")) == 0 and out.edata["sim"][("a", "x", "b")].numel() == 0
    dn = TR.DropNode(0.5)(g, draw=SEED)
    keep = ~_drawn(40, SEED, 0, 1, 0.5)
    m = keep[u] & keep[v]
    assert torch.equal(dn.edata["sim"][("b", "y", "b")], torch.arange(10.0)[m])   # parallel edges stand or fall together, in order
    de = TR.DropEdge(0.5)(g, draw=SEED)
    assert torch.equal(de.edata["sim"][("b", "y", "b")], torch.arange(10.0)[~_drawn(10, SEED, 0, 1, 0.5)])   # ... and are drawn one by one


def test_homogeneous_graph_then_self_loops():
    g = synthetic.homogeneous_graph(200, 4, self_loops=False)
    out = TR.Compose([TR.DropNode(0.5), TR.DropEdge(0.5), TR.NodeShuffle(), TR.FeatMask(0.5, node_feat_names=["feat"])])(g, draw=SEED)
    assert out.is_homogeneous and 0 < out.num_nodes() < 200
    h = to_homogeneous(out, add_self_loop=True)                   # the reference's order: augment first, then add the self loops
    n, e = out.num_nodes(), out.num_edges()
    assert h.num_edges() == e + n
    u, v = h.edges()
    assert torch.equal(u[e:], torch.arange(n)) and torch.equal(v[e:], torch.arange(n))
    assert torch.equal(h.ndata["feat"], out.ndata["feat"])


def test_replay_and_manual_seed(graph):
    pipe = TR.reference_train_transform()
    a, b, c = pipe(graph, draw=SEED), pipe(graph, draw=SEED), pipe(graph, draw=SEED + 1)
    _equal(a, b)
    assert [a.num_nodes(t) for t in a.ntypes] != [c.num_nodes(t) for t in c.ntypes] or a.num_edges() != c.num_edges() or \
        not all(torch.equal(a.nodes[t].data["feat"], c.nodes[t].data["feat"]) for t in a.ntypes)
    torch.manual_seed(77)
    d1, d2 = pipe(graph), pipe(graph)
    torch.manual_seed(77)
    _equal(pipe(graph), d1)
    _equal(pipe(graph), d2)
    assert d1.num_edges() != d2.num_edges() or d1.num_nodes() != d2.num_nodes() or \
        not all(torch.equal(d1.nodes[t].data["feat"], d2.nodes[t].data["feat"]) for t in d1.ntypes)


def test_rates_within_five_sigma():
    n = 4096
    g = HeteroGraph.from_coo(OrderedDict([("a", n)]), OrderedDict([(("a", "e", "a"), (torch.arange(n), torch.arange(n)))]),
                             feat={"a": torch.ones(n, 1)})
    tol = 5 * math.sqrt(0.25 / n)
    assert abs(TR.DropNode(0.5)(g, draw=SEED).num_nodes() / n - 0.5) <= tol
    assert abs(TR.DropEdge(0.5)(g, draw=SEED).num_edges() / n - 0.5) <= tol
    w = HeteroGraph.from_coo(OrderedDict([("a", 2)]), OrderedDict([(("a", "e", "a"), (torch.zeros(0, dtype=torch.int64),) * 2)]),
                             feat={"a": torch.ones(2, 1024)})
    kept = float(TR.FeatMask(0.5, node_feat_names=["feat"])(w, draw=SEED).nodes["a"].data["feat"][0].sum()) / 1024
    assert abs(kept - 0.5) <= 5 * math.sqrt(0.25 / 1024)


def test_compose_equals_its_members_one_after_another(graph):
    members = [TR.DropNode(0.5), TR.DropEdge(0.5), TR.NodeShuffle(), TR.FeatMask(0.5, node_feat_names=["feat"])]
    for order in ([0, 1, 2, 3], [2, 1, 3, 0], [1, 0]):
        seq = [members[i] for i in order]
        ref = graph
        for k, t in enumerate(seq):
            ref = t(ref, draw=SEED, index=k)
        _equal(TR.Compose(seq)(graph, draw=SEED), ref)
    # behind DropNode, DropEdge indexes the SURVIVING edges: position in the graph it receives
    dn = members[0](graph, draw=SEED, index=0)
    both = TR.Compose(members[:2])(graph, draw=SEED)
    for j, r in enumerate(graph.canonical_etypes):
        m = ~_drawn(dn.num_edges(r), SEED, 1, j, 0.5)
        assert torch.equal(both.edges(r)[0], dn.edges(r)[0][m]) and torch.equal(both.edata["sim"][r], dn.edata["sim"][r][m])
    # foreign callables are applied one by one
    seen = []
    out = TR.Compose([members[1], lambda g: (seen.append(g.num_edges()), g)[1], members[3]])(graph, draw=SEED)
    assert seen == [members[1](graph, draw=SEED, index=0).num_edges()]
    _equal(out, members[3](members[1](graph, draw=SEED, index=0), draw=SEED, index=2))


def test_refusals(graph):
    b = W.batch([graph, graph])
    for t in (TR.DropNode(), TR.DropEdge(), TR.NodeShuffle(), TR.FeatMask(node_feat_names=["feat"]), TR.reference_train_transform()):
        with pytest.raises(ValueError, match="single graphs"):
            t(b, draw=SEED)
    _equal(TR.FeatMask(0.5, node_feat_names=["nope"], edge_feat_names=["nope"])(graph, draw=SEED), graph)   # unknown names are skipped, as DGL skips
    with pytest.raises(ValueError):
        TR.DropNode(1.5)
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.augment_graph(graph, [TR.DropNode().stage(0)], SEED)


def test_loader_with_a_transform_on_the_cpu():
    gs = [synthetic.hetero_graph(60 + 10 * i, 4, seed=20 + i) for i in range(4)]
    labels = [0, 1, 1, 0]
    mk = lambda tr, seed=3: data.GraphBatchLoader(gs, labels, 2, "cpu", shuffle=True, seed=seed, resident=True, passes=2, transform=tr)
    a, b = list(mk(TR.reference_train_transform())), list(mk(TR.reference_train_transform()))
    assert len(a) == len(b) == 4
    for (ga, ya), (gb, yb) in zip(a, b):
        _equal(ga, gb)
        assert torch.equal(ya, yb) and ga.batch_size == 2
        for t in ga.ntypes:
            assert int(ga.batch_num_nodes(t).sum()) == ga.num_nodes(t) == ga.nodes[t].data["feat"].shape[0]
    sizes = [(g.num_nodes(), g.num_edges()) for g, _ in a]
    assert len(set(sizes)) > 2, "the second pass draws other graphs than the first"
    assert all(g.num_nodes() < sum(x.num_nodes() for x in gs) for g, _ in a)
    # the draw is a function of (loader seed, batch counter, slide index)
    g0, _ = next(iter(mk(TR.DropNode(0.5))))
    first = next(iter(mk(None)))[0]
    # transform=None: the stored slides, batched - what the loader is specified to yield
    slides = [gs[i] for n0 in first.batch_num_nodes("0").tolist() for i in range(4) if gs[i].num_nodes("0") == n0]
    ref = W.batch(slides)
    _equal(first, ref)
    assert torch.equal(first.cat_edata_csr("sim"), ref.cat_edata_csr("sim")) and torch.equal(first.plan().src, ref.plan().src)
    want = W.batch([TR.DropNode(0.5)(s, draw=data.augment_draw(3, 0, gs.index(s))) for s in slides])
    _equal(g0, want)
