"""graph.leave_one_out_tables / graph.leave_one_out_batch on CPU graphs, and the GEM explainers on top of them.

The tables must predict, for every node of every type, exactly the per-relation edge counts of ``remove_nodes`` (the device path sizes its
outputs from them and never asks the device); a CPU batch IS ``batch([remove_nodes(g, [i], t) for i in nids])``; the explainers' masks equal
an explicit one-node-per-forward loop.  The model is a tiny torch-only stand-in (graph -> logits), so nothing here needs a GPU."""
from collections import OrderedDict

import numpy as np
import pytest
import torch

import wsi_hgnn_amd as W
from wsi_hgnn_amd import graph as G
from wsi_hgnn_amd.explainers import GemExplainer, HetGemExplainer
from wsi_hgnn_amd.explainers.gem import collapse_relations


def _hand_graph():
    """3 node types; relation ('a','aa','a') with self loops (0->0 twice, 3->3) and duplicate edges (1->2 twice), relations into and out of 'a',
    one that does not touch 'a', one without edges; node 4 of 'a' is isolated."""
    nn_ = OrderedDict([("a", 5), ("b", 3), ("c", 1)])
    edges = OrderedDict([
        (("a", "aa", "a"), (torch.tensor([0, 0, 1, 1, 2, 3, 3, 0]), torch.tensor([0, 0, 2, 2, 0, 3, 1, 3]))),
        (("a", "ab", "b"), (torch.tensor([0, 1, 1, 3]), torch.tensor([2, 2, 0, 1]))),
        (("b", "ba", "a"), (torch.tensor([0, 2, 2]), torch.tensor([3, 3, 0]))),
        (("b", "bc", "c"), (torch.tensor([0, 1, 1]), torch.tensor([0, 0, 0]))),
        (("c", "ca", "a"), (torch.tensor([], dtype=torch.int64), torch.tensor([], dtype=torch.int64))),
        (("c", "cc", "c"), (torch.tensor([0]), torch.tensor([0]))),
    ])
    gen = torch.Generator().manual_seed(7)
    g = W.HeteroGraph.from_coo(nn_, edges, feat={t: torch.rand(c, 4, generator=gen) for t, c in nn_.items()},
                               sim={r: torch.rand(u.numel(), generator=gen) for r, (u, v) in edges.items()})
    for t, c in nn_.items():
        g.nodes[t].data["_ID"] = torch.arange(c) + 100
    for r in g.canonical_etypes:
        g._eframes[r]["tag"] = torch.arange(g.num_edges(r)) * 3
    return g


def _assert_same(a, b):
    assert a.ntypes == b.ntypes and a.canonical_etypes == b.canonical_etypes
    assert a.batch_size == b.batch_size
    for t in b.ntypes:
        assert a.num_nodes(t) == b.num_nodes(t), t
        assert torch.equal(a.batch_num_nodes(t), b.batch_num_nodes(t)), t
        assert set(a._nframes[t]) == set(b._nframes[t]), t
        for k, x in b._nframes[t].items():
            y = a._nframes[t][k]
            assert y.dtype == x.dtype and y.shape == x.shape and torch.equal(y, x), (t, k)
    for r in b.canonical_etypes:
        for x, y in zip(a.edges(r), b.edges(r)):
            assert x.dtype == y.dtype and torch.equal(x, y), r
        assert set(a._eframes[r]) == set(b._eframes[r]), r
        for k, x in b._eframes[r].items():
            y = a._eframes[r][k]
            assert y.dtype == x.dtype and y.shape == x.shape and torch.equal(y, x), (r, k)


def test_tables_predict_every_copys_edge_counts():
    g = _hand_graph()
    for t in g.ntypes:
        tb = G.leave_one_out_tables(g, t)
        assert tb.ntype == t and tb.num_nodes == g.num_nodes(t)
        assert tb.num_edges == [g.num_edges(r) for r in g.canonical_etypes]
        for j, (s, _, d) in enumerate(g.canonical_etypes):      # a table exists exactly where the relation touches the type
            assert (tb.out_degree[j] is not None) == (s == t)
            assert (tb.in_degree[j] is not None) == (d == t)
            assert (tb.self_loops[j] is not None) == (s == t and d == t)
        for i in range(g.num_nodes(t)):
            h = W.remove_nodes(g, torch.tensor([i]), t)
            assert tb.surviving_edges(i) == [h.num_edges(r) for r in h.canonical_etypes], (t, i)
    tb = G.leave_one_out_tables(g, "a")
    j = g.canonical_etypes.index(("a", "aa", "a"))
    assert tb.out_degree[j].tolist() == [3, 2, 1, 2, 0] and tb.in_degree[j].tolist() == [3, 1, 2, 2, 0] and tb.self_loops[j].tolist() == [2, 0, 0, 1, 0]
    assert tb.surviving_edges(4) == tb.num_edges                # the isolated node takes no edge with it


def test_tables_of_a_homogeneous_graph():
    g = W.HeteroGraph.homogeneous(6, torch.tensor([0, 1, 1, 5, 5, 2]), torch.tensor([1, 1, 2, 5, 0, 2]))
    tb = G.leave_one_out_tables(g)
    for i in range(6):
        assert tb.surviving_edges(i) == [W.remove_nodes(g, torch.tensor([i])).num_edges()]


def test_argument_errors():
    g = _hand_graph()
    with pytest.raises(ValueError):
        G.leave_one_out_batch(g, [], "a")
    with pytest.raises(ValueError):
        G.leave_one_out_batch(g, [0])                           # multi-type graph: ntype is required
    with pytest.raises(ValueError):
        G.leave_one_out_tables(g)
    with pytest.raises(IndexError):
        G.leave_one_out_batch(g, [0, 5], "a")
    with pytest.raises(IndexError):
        G.leave_one_out_batch(g, [-1], "a")
    with pytest.raises(IndexError):
        G.leave_one_out_batch(g, [1], "c")
    with pytest.raises(ValueError):
        G.leave_one_out_batch(W.batch([g, g]), [0], "a")        # a batched graph raises, as remove_nodes does
    with pytest.raises(ValueError):
        W.remove_nodes(W.batch([g, g]), torch.tensor([0]), "a")


def test_cpu_batch_is_the_composition():
    g = _hand_graph()
    for t, nids in (("a", [0]), ("a", [4, 2, 0, 2]), ("a", range(5)), ("b", (2, 0)), ("c", [0, 0])):
        want = W.batch([W.remove_nodes(g, torch.tensor([i]), t) for i in nids])
        _assert_same(G.leave_one_out_batch(g, nids, t), want)
        _assert_same(G.leave_one_out_batch(g, nids, t, tables=G.leave_one_out_tables(g, t), check=True), want)
    hg = W.HeteroGraph.homogeneous(6, torch.tensor([0, 1, 1, 5, 5, 2]), torch.tensor([1, 1, 2, 5, 0, 2]), feat=torch.rand(6, 3))
    _assert_same(G.leave_one_out_batch(hg, [5, 1]), W.batch([W.remove_nodes(hg, torch.tensor([i])) for i in (5, 1)]))
    assert W.leave_one_out_batch is G.leave_one_out_batch and W.leave_one_out_tables is G.leave_one_out_tables


class _Readout(torch.nn.Module):
    """graph -> logits [batch, 2]: per graph and node type the mean feature and a per-relation mean of sim * feat[src], through one linear map."""

    def __init__(self, ntypes, rels, width):
        super().__init__()
        self.lin = torch.nn.Linear(width * (len(ntypes) + len(rels)), 2)

    def forward(self, g):
        B = g.batch_size
        parts = []
        for t in g.ntypes:
            x = g.nodes[t].data["feat"]
            gid = torch.repeat_interleave(torch.arange(B), g.batch_num_nodes(t))
            s = torch.zeros(B, x.shape[1]).index_add_(0, gid, x)
            parts.append(s / g.batch_num_nodes(t).clamp(min=1).unsqueeze(1))
        for (s_, e, d) in g.canonical_etypes:
            u, v = g.edges((s_, e, d))
            x = g.nodes[s_].data["feat"]
            gid = torch.repeat_interleave(torch.arange(B), g.batch_num_nodes(s_))
            w = g._eframes[(s_, e, d)]["sim"].unsqueeze(1) if "sim" in g._eframes[(s_, e, d)] else 1.0
            parts.append(torch.zeros(B, x.shape[1]).index_add_(0, gid[u], x[u] * w))
        return self.lin(torch.cat(parts, dim=1))


# Tolerance of the two explainer tests: the explainer's forward sees B graphs at once, the loop one; index_add_ sums each graph's rows in the same
# order, so only the [B, K] x [K, 2] linear map may round differently with B.  Losses and normalised masks are <= ~1 in fp32 (ulp 1.2e-7); 1e-6 is
# 8 ulp of that, the bound the GPU test is given for the same comparison.
def test_het_gem_explainer_matches_an_explicit_loop():
    g = _hand_graph()
    gc = collapse_relations(g)
    torch.manual_seed(3)
    m = _Readout(gc.ntypes, gc.canonical_etypes, 4).eval()
    label = torch.tensor([1])
    mask = HetGemExplainer(g, m, label, batch_size=2).explain_node()
    assert list(mask) == gc.ntypes
    with torch.no_grad():
        loss = torch.nn.functional.cross_entropy(m(gc), label)
        for t in gc.ntypes:
            want = torch.stack([loss - torch.nn.functional.cross_entropy(m(W.remove_nodes(gc, torch.tensor([i]), t)), label)
                                for i in range(gc.num_nodes(t))])
            assert mask[t].shape == want.shape and mask[t].dtype == torch.float32 and not mask[t].is_cuda
            assert (mask[t] - want).abs().max().item() < 1e-6, t


def test_gem_explainer_matches_an_explicit_loop():
    gen = torch.Generator().manual_seed(11)
    hg = W.HeteroGraph.homogeneous(13, torch.randint(0, 13, (40,), generator=gen), torch.randint(0, 13, (40,), generator=gen),
                                   feat=torch.rand(13, 4, generator=gen))
    torch.manual_seed(5)
    m = _Readout(hg.ntypes, hg.canonical_etypes, 4).eval()
    label = torch.tensor([1])
    got = GemExplainer(hg, m, label, batch_size=5).explain_node()
    with torch.no_grad():
        pred = m(hg)
        raw = torch.stack([torch.nn.functional.cross_entropy(pred - m(W.remove_nodes(hg, torch.tensor([i]))), label) for i in range(13)]).numpy()
    want = (raw - raw.min()) / (raw.max() - raw.min())
    assert isinstance(got, np.ndarray) and got.shape == (13,)
    assert np.abs(got - want).max() < 1e-6
