"""Shared cases of tests/test_plan_by_relation.py and tests/test_plan_by_relation_gpu.py: small COO graphs at the edges of the derivation of
the per-relation-source plan (graph.plan_by_relation).  Every builder returns a CPU ``HeteroGraph``."""
from collections import OrderedDict

import torch

TILE = 1024                 # WSI_PLAN_REL_TILE: counts per workgroup of the kernel's prefix sum
TABLES = ("rowptr", "src", "colptr", "csc_eid", "csc_dst", "order_dst", "order_src")
ALL18 = [(s, e, d) for s in "012" for e in ("neg", "pos") for d in "012"]


def rand_graph(seed, counts, rels, per_rel):
    """``per_rel`` random edges in every relation of ``rels`` (an int, or one count per relation)."""
    from wsi_hgnn_amd.graph import HeteroGraph
    gen = torch.Generator().manual_seed(seed)
    nn_ = OrderedDict((str(i), c) for i, c in enumerate(counts))
    edges = OrderedDict()
    for k, (s, e, d) in enumerate(rels):
        ne = per_rel if isinstance(per_rel, int) else per_rel[k]
        if nn_[s] == 0 or nn_[d] == 0:
            ne = 0
        edges[(s, e, d)] = (torch.randint(0, max(nn_[s], 1), (ne,), generator=gen), torch.randint(0, max(nn_[d], 1), (ne,), generator=gen))
    return HeteroGraph.from_coo(nn_, edges)


def hub_source(degree):
    """Source 3 of type 0 sends ``degree`` extra edges whose relations ALTERNATE (edge j goes into relation j mod 6 of the six leaving type 0):
    inside one wave's 64 entries every relation occurs, ranks and stride loops go round.  Source 0 of type 1 does the same over its six."""
    from wsi_hgnn_amd.graph import HeteroGraph
    g = rand_graph(50 + degree, (40, 30, 20), ALL18, 25)
    edges = OrderedDict()
    nn_ = OrderedDict((t, g.num_nodes(t)) for t in g.ntypes)
    for r in g.canonical_etypes:
        u, v = g.edges(r)
        for stype, node in (("0", 3), ("1", 0)):
            if r[0] == stype:
                mine = [x for x in g.canonical_etypes if x[0] == stype]
                j = torch.arange(mine.index(r), degree, len(mine))
                u = torch.cat([u, torch.full((j.numel(),), node, dtype=torch.int64)])
                v = torch.cat([v, (j * 7) % nn_[r[2]]])
        edges[r] = (u, v)
    return HeteroGraph.from_coo(nn_, edges)


def batch_of_two():
    from wsi_hgnn_amd import graph as G
    return G.batch([rand_graph(21, (30, 20, 10), ALL18, 40), rand_graph(22, (17, 33, 9), ALL18, 31)])


def rows_total(n0, n1):
    """Two node types, relations 0->0, 0->1, 1->0: NS = 2 n0 + n1."""
    return rand_graph(n0 + n1, (n0, n1), [("0", "a", "0"), ("0", "b", "1"), ("1", "a", "0")], 3000)


def cases():
    some_empty = [0 if k % 3 == 1 else 35 for k in range(18)]
    no_source_2 = [r for r in ALL18 if r[0] != "2"]
    out = [(f"all18-{s}", lambda s=s: rand_graph(s, (23 + 5 * s, 31, 12 + s), ALL18, 30 + 7 * s)) for s in range(4)]
    out += [("some-relations-empty", lambda: rand_graph(7, (25, 18, 30), ALL18, some_empty)),
            ("type-2-never-a-source", lambda: rand_graph(8, (25, 18, 30), no_source_2, 40)),
            ("hub-70", lambda: hub_source(70)), ("hub-300", lambda: hub_source(300)), ("hub-5000", lambda: hub_source(5000)),
            ("batch-of-2", batch_of_two),
            ("no-edges", lambda: rand_graph(9, (5, 4, 3), ALL18, 0)),
            ("rows-tile", lambda: rows_total(400, TILE - 800)), ("rows-tile-minus-1", lambda: rows_total(400, TILE - 801)),
            ("rows-tile-plus-1", lambda: rows_total(400, TILE - 799)), ("rows-2-tiles-plus-1", lambda: rows_total(900, 2 * TILE - 1799))]
    return out


def header(g):
    from wsi_hgnn_amd.graph import PlanHeader
    return PlanHeader(g.ntypes, g.canonical_etypes, [g.num_nodes(t) for t in g.ntypes])


def explicit_padded(ld, slot, idxs, device="cpu"):
    """The padded batch of a slot spelled out as graphs: the slides, empty graphs up to b_cap, the filler; with (nf, ef)."""
    from wsi_hgnn_amd import graph as G
    from wsi_hgnn_amd.graph import HeteroGraph
    lay = slot.layout
    its = [ld.items[i] for i in idxs]
    nf = [lay.n_cap[t] - sum(it.num_nodes[t] for it in its) for t in range(lay.T)]
    ef = [lay.e_cap[t] - sum(it.pieces.ecount[t] for it in its) for t in range(lay.T)]
    real = [HeteroGraph.from_coo(OrderedDict(zip(it.ntypes, it.num_nodes)), OrderedDict((r, (u.cpu(), v.cpu())) for r, (u, v) in it.edges.items()))
            for it in its]
    bare = lambda g: HeteroGraph.from_coo(OrderedDict((t, g.num_nodes(t)) for t in g.ntypes), OrderedDict((r, g.edges(r)) for r in g.canonical_etypes))
    extra = [bare(G.filler_graph(lay.ntypes, lay.rels, [0] * lay.T, [0] * lay.T, 0))] * (lay.b_cap - len(idxs))
    extra.append(bare(G.filler_graph(lay.ntypes, lay.rels, nf, ef, 0)))
    return G.batch(real + extra).to(device), nf, ef
