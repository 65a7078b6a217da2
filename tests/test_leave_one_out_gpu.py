"""The device path of graph.leave_one_out_batch (csrc/loo.hip through ops.leave_one_out_batch) against the composition it replaces,
``batch([remove_nodes(g, [i], t) for i in nids])`` built on the CPU and moved to the device.  Index arithmetic and row copies only, so every
comparison is ``torch.equal``: counts, ``batch_num_nodes``, edges, every node and edge field.  Each case also runs with ``check=True`` (the
kernel's per-copy counts against the tables' prediction).

The heterogeneous graph (300 nodes, 2930 edges, F = 8) is the smallest that reaches every path: a t->t relation of 2300 edges (three 1024-edge
scan tiles, so a copy's output segment spans tile boundaries) with self loops and duplicates, a relation that does not touch the type, a relation
without edges, a one-node type (its removal leaves 0 nodes and empties two relations), an isolated node (the last of type '0') and a hub that is
the source of EVERY edge of one relation (that copy's relation becomes empty).  Node fields: fp32 [n, 8] (gather kernel), an fp32 [n, 8] view
with non-unit column stride, int64 ``_ID`` and an [n, 2, 3] field (indexing); edge fields: fp32 ``sim`` (written by the kernel) and an int64 tag
(carried through the original edge index)."""
from collections import OrderedDict

import pytest
import torch

pytestmark = pytest.mark.gpu

COUNTS = OrderedDict([("0", 200), ("1", 99), ("2", 1)])
HUB = 7


def _dev():
    return torch.device("cuda:0")


_CACHE = {}


def _hetero():
    """(CPU graph, device graph), built once and never modified."""
    if "het" not in _CACHE:
        from wsi_hgnn_amd.graph import HeteroGraph
        gen = torch.Generator().manual_seed(2024)
        ri = lambda hi, m: torch.randint(0, hi, (m,), generator=gen)
        n0, n1 = COUNTS["0"], COUNTS["1"]
        au, av = ri(n0 - 1, 2300), ri(n0 - 1, 2300)                 # node n0 - 1 stays isolated
        au[:40], av[:40] = torch.arange(40) * 3, torch.arange(40) * 3      # self loops
        au[40:60], av[40:60] = au[60:80], av[60:80]                 # duplicates
        au[1023:1026], av[1023:1026] = torch.tensor([HUB, 0, HUB]), torch.tensor([HUB, HUB, 1])    # removed edges on both sides of a tile boundary
        edges = OrderedDict([
            (("0", "a", "0"), (au, av)),
            (("0", "c", "1"), (ri(n0 - 1, 300), ri(n1, 300))),
            (("0", "hub", "1"), (torch.full((100,), HUB), ri(n1, 100))),
            (("1", "b", "1"), (ri(n1, 150), ri(n1, 150))),
            (("1", "e", "0"), (torch.empty(0, dtype=torch.int64), torch.empty(0, dtype=torch.int64))),
            (("1", "f", "2"), (ri(n1, 30), torch.zeros(30, dtype=torch.int64))),
            (("2", "d", "0"), (torch.zeros(50, dtype=torch.int64), ri(n0 - 1, 50))),
        ])
        g = HeteroGraph.from_coo(COUNTS, edges, feat={t: torch.rand(c, 8, generator=gen) for t, c in COUNTS.items()},
                                 sim={r: torch.rand(u.numel(), generator=gen) - 0.5 for r, (u, v) in edges.items()})
        for t, c in COUNTS.items():
            g.nodes[t].data["nc"] = torch.rand(8, c, generator=gen).t()         # [n, 8], column stride n: dense, so .to(device) keeps the strides
            g.nodes[t].data["_ID"] = torch.arange(c) + 1000
            g.nodes[t].data["hr"] = torch.rand(c, 2, 3, generator=gen)
        for r in g.canonical_etypes:
            g._eframes[r]["tag"] = torch.arange(g.num_edges(r)) * 7 + 1
        assert g.num_nodes() == 300 and g.num_edges() == 2930
        gd = g.to(_dev())
        assert gd.nodes["0"].data["nc"].stride(1) != 1 and gd.nodes["0"].data["feat"].is_contiguous()
        _CACHE["het"] = (g, gd)
    return _CACHE["het"]


def _nid_sets(n):
    if n == 1:
        return {"first": [0], "last": [0], "seven": [0] * 7, "sixteen": [0] * 16}
    return {"first": [0], "last": [n - 1], "seven": [n - 2, HUB, 3, 64, HUB, 0, n - 1], "sixteen": list(range(16))}


def _want(key, g, nids, t):
    """The composition, on the CPU, moved to the device (computed once per case)."""
    if key not in _CACHE:
        import wsi_hgnn_amd as W
        _CACHE[key] = W.batch([W.remove_nodes(g, torch.tensor([i]), t) for i in nids]).to(_dev())
    return _CACHE[key]


def _assert_same(a, b):
    assert a.ntypes == b.ntypes and a.canonical_etypes == b.canonical_etypes and a.batch_size == b.batch_size
    for t in b.ntypes:
        assert a.num_nodes(t) == b.num_nodes(t), t
        assert torch.equal(a.batch_num_nodes(t), b.batch_num_nodes(t)), t
        assert set(a._nframes[t]) == set(b._nframes[t]), t
        for k, x in b._nframes[t].items():
            y = a._nframes[t][k]
            assert y.is_cuda and y.dtype == x.dtype and y.shape == x.shape and torch.equal(y, x), (t, k)
    for r in b.canonical_etypes:
        assert a.num_edges(r) == b.num_edges(r), r
        for x, y in zip(a.edges(r), b.edges(r)):
            assert x.is_cuda and x.dtype == y.dtype and torch.equal(x, y), r
        assert set(a._eframes[r]) == set(b._eframes[r]), r
        for k, x in b._eframes[r].items():
            y = a._eframes[r][k]
            assert y.dtype == x.dtype and y.shape == x.shape and torch.equal(y, x), (r, k)


@pytest.mark.parametrize("which", ["first", "last", "seven", "sixteen"])
@pytest.mark.parametrize("t", ["0", "1", "2"])
def test_heterogeneous_batch_equals_the_composition(t, which):
    from wsi_hgnn_amd import graph as G
    g, gd = _hetero()
    nids = _nid_sets(g.num_nodes(t))[which]
    want = _want(("het", t, which), g, nids, t)
    tables = G.leave_one_out_tables(gd, t)
    _assert_same(G.leave_one_out_batch(gd, nids, t, tables=tables), want)
    _assert_same(G.leave_one_out_batch(gd, nids, t, check=True), want)          # tables built on demand + the kernel's counts checked
    if t == "0" and which == "seven":                                           # the hub's copy (second of the batch) lost the whole relation
        got = G.leave_one_out_batch(gd, [HUB], t, tables=tables, check=True)
        assert got.num_edges(("0", "hub", "1")) == 0 and got.num_edges(("0", "c", "1")) > 0
    if t == "2":                                                                # the only node of its type: 0 nodes left in every copy
        assert want.num_nodes("2") == 0 and want.num_edges(("1", "f", "2")) == 0 and want.num_edges(("2", "d", "0")) == 0


def test_tables_from_the_device_equal_the_host_ones():
    from wsi_hgnn_amd import graph as G
    g, gd = _hetero()
    for t in g.ntypes:
        a, b = G.leave_one_out_tables(gd, t), G.leave_one_out_tables(g, t)
        assert a.num_edges == b.num_edges
        for x, y in zip(a.out_degree + a.in_degree + a.self_loops, b.out_degree + b.in_degree + b.self_loops):
            assert (x is None) == (y is None) and (x is None or (not x.is_cuda and torch.equal(x, y)))


def test_check_mode_reports_wrong_tables():
    """Tables that predict one survivor too few for one copy: the kernel stays inside the ranges they give and check=True raises."""
    from wsi_hgnn_amd import graph as G
    g, gd = _hetero()
    tables = G.leave_one_out_tables(gd, "0")
    j = g.canonical_etypes.index(("0", "c", "1"))
    tables._removed[j, 3] += 1                                  # predicts one survivor too few for node 3
    with pytest.raises(RuntimeError, match="predict"):
        G.leave_one_out_batch(gd, [3, 5], "0", tables=tables, check=True)


def test_homogeneous_batch_equals_the_composition():
    import wsi_hgnn_amd as W
    from wsi_hgnn_amd import graph as G, synthetic
    hg = synthetic.homogeneous_graph(40, 16, seed=5)
    hd = hg.to(_dev())
    for nids in ([0], [39], [38, 2, 17, 2, 0, 39, 21], list(range(12, 28))):
        want = W.batch([W.remove_nodes(hg, torch.tensor([i])) for i in nids]).to(_dev())
        _assert_same(G.leave_one_out_batch(hd, nids), want)
        _assert_same(G.leave_one_out_batch(hd, nids, check=True), want)


def _model_and_graph():
    if "model" not in _CACHE:
        from wsi_hgnn_amd import models, synthetic
        from wsi_hgnn_amd.explainers.gem import collapse_relations
        gc = collapse_relations(synthetic.hetero_graph(60, 16, seed=21, dst_mode="hub"))
        torch.manual_seed(611)
        m = models.HEATNet4(16, 64, 2, 2, 4, {"0": 0, "1": 1, "2": 2}, 0.0, "mean").to(_dev()).eval()
        _CACHE["model"] = (m, gc, gc.to(_dev()))
    return _CACHE["model"]


def test_model_forward_on_the_batch_equals_the_forward_on_the_composition():
    """The same graph gives the same kernel plan, hence the same bits."""
    import wsi_hgnn_amd as W
    from wsi_hgnn_amd import graph as G
    m, gc, gd = _model_and_graph()
    for t in gc.ntypes:
        n = gc.num_nodes(t)
        nids = [n - 1, 1, 4, 1, 0, n // 2, 2]
        want = W.batch([W.remove_nodes(gc, torch.tensor([i]), t) for i in nids]).to(_dev())
        got = G.leave_one_out_batch(gd, nids, t, check=True)
        _assert_same(got, want)
        with torch.no_grad():
            a, b = m(got), m(want)
        assert a.shape == (7, 2) and torch.equal(a, b), t


def test_het_gem_explainer_takes_the_device_path(monkeypatch):
    """With graph.remove_nodes made to raise, the explainer still completes on a GPU graph (no host composition is left in its loop), and its masks
    equal the explicit remove_nodes + batch loop with the same batch size (same batches, same plans; only the read-back moved): within 1e-6."""
    import wsi_hgnn_amd as W
    from wsi_hgnn_amd import graph as G, synthetic
    from wsi_hgnn_amd.explainers import HetGemExplainer
    m, gc, gd = _model_and_graph()
    label = torch.tensor([1], device=_dev())
    bs = 16
    want = {}
    with torch.no_grad():
        loss = torch.nn.functional.cross_entropy(m(gd), label)
        for t in gd.ntypes:
            n = gd.num_nodes(t)
            want[t] = torch.zeros(n)
            for start in range(0, n, bs):
                end = min(start + bs, n)
                bg = W.batch([W.remove_nodes(gd, torch.tensor([i]), t) for i in range(start, end)])
                want[t][start:end] = (loss - torch.nn.functional.cross_entropy(m(bg), label.expand(end - start), reduction="none")).cpu()

    def refuse(*a, **k):
        raise AssertionError("remove_nodes was called on the device path")
    monkeypatch.setattr(G, "remove_nodes", refuse)
    mask = HetGemExplainer(synthetic.hetero_graph(60, 16, seed=21, dst_mode="hub").to(_dev()), m, label, batch_size=bs).explain_node()
    assert list(mask) == gd.ntypes
    for t in gd.ntypes:
        assert not mask[t].is_cuda and mask[t].shape == want[t].shape
        assert (mask[t] - want[t]).abs().max().item() <= 1e-6, t
