"""Shared helpers of tests/test_batch_slot_quota.py and tests/test_batch_slot_quota_gpu.py: survivor quotas of augmented batch
slots.  The slides are those of tests/slot_cases.py; at their sizes (40-351 nodes per type) the "bound" quota never binds, so the binding
cases set their limits through a callable, from the survivors the draw contract gives."""
import math
from collections import OrderedDict

import torch

import slot_cases as C
from test_batch_slot_augment import SEED, _slides, aug_loader, draws_of, pipelines, same  # noqa: F401  (re-exported)

LAM = math.log(2.0 ** 32) / 2.0
BATCH = [0, 1]             # the batch the binding cases truncate: the two largest slides that share the big slot


def stored_graph(ld, i):
    from wsi_hgnn_amd.graph import HeteroGraph
    it = ld.items[i]
    return HeteroGraph.from_coo(OrderedDict(zip(it.ntypes, it.num_nodes)), it.edges, feat=dict(zip(it.ntypes, it.feat)), sim=it.sims)


def restated_bound(g, p_node, p_edge):
    """Section 2 of the contract, restated plainly over a HeteroGraph: ``p_node`` / ``p_edge`` are the QUANTISED probabilities, None for an
    absent stage."""
    pn, pe = (p_node or 0.0), (p_edge or 0.0)
    qn = []
    for t in g.ntypes:
        n = g.num_nodes(t)
        qn.append(n if p_node is None else min(n, math.ceil(n * (1.0 - pn) + math.sqrt(LAM * n))))
    qe = []
    for (s, e, d) in g.canonical_etypes:
        u, v = (x.tolist() for x in g.edges((s, e, d)))
        E = len(u)
        inc, loops = {}, 0
        for a, b in zip(u, v):
            if s == d and a == b:
                loops += 1
                inc[("n", a)] = inc.get(("n", a), 0) + 1
            else:
                ka, kb = (("n", a), ("n", b)) if s == d else (("s", a), ("d", b))
                inc[ka] = inc.get(ka, 0) + 1
                inc[kb] = inc.get(kb, 0) + 1
        csq = sum(c * c for c in inc.values())
        mu = (E - loops) * (1.0 - pn) ** 2 * (1.0 - pe) + loops * (1.0 - pn) * (1.0 - pe)
        qe.append(min(E, math.ceil(mu + math.sqrt(LAM * (csq + E)))))
    return qn, qe


def stage_probabilities(pipe):
    """(p_node, p_edge) of a pipeline, quantised as the draw rule quantises them (threshold / 65536); None for an absent stage."""
    from wsi_hgnn_amd import transforms as T
    pn = pe = None
    for t in pipe.transforms:
        if isinstance(t, T.DropNode):
            pn = t.threshold / 65536.0
        if isinstance(t, T.DropEdge):
            pe = t.threshold / 65536.0
    return pn, pe


def drawn_counts(ld, pipe, i, draw, qn=None):
    """(survivors of DropNode's draw per node type, final edges per relation) of slide i: the nodes by the draw contract (AugmentSpec.node_keep),
    the edges by the tensor formulation of the pipeline - with ``qn`` of the pipeline truncated by that node quota alone."""
    from wsi_hgnn_amd import transforms as T
    from wsi_hgnn_amd.data import slot_augment_spec
    it = ld.items[i]
    keep = slot_augment_spec(pipe).node_keep(draw, it.num_nodes, "cpu")
    g = stored_graph(ld, i)
    g = pipe(g, draw=draw, fused=False) if qn is None else T.truncated(pipe, g, draw, qn, None)[0]
    return [int(k.sum()) for k in keep], [int(g.edges(r)[0].numel()) for r in g.canonical_etypes]


def stored_quota(ld, i):
    it = ld.items[i]
    return list(it.num_nodes), [int(it.edges[r][0].numel()) for r in it.rels]


BINDING = ["node_minus_one", "node_half", "edge_minus_one", "edge_zero", "both", "node_zero"]


def binding_quotas(ld, pipe, idxs, draws, case):
    """``{slide: (qn, qe)}`` of a binding case for the batch ``idxs`` under ``draws``, and what the fill must then record:
    ``(quotas, node_excess, edge_excess)`` - the excesses computed here from the draw contract and the node-truncated pipeline, not read from
    the code under test's own bookkeeping."""
    has_dn = stage_probabilities(pipe)[0] is not None
    out, xn, xe = {}, 0, 0
    for b, (i, d) in enumerate(zip(idxs, draws)):
        qn, qe = stored_quota(ld, i)
        n, e = drawn_counts(ld, pipe, i, d)
        j = max(range(len(e)), key=lambda r: e[r])               # the relation with the most survivors
        if case == "node_minus_one" and b == 0:
            qn[0] = max(0, n[0] - 1)
        elif case == "node_half" and b == 1:
            qn[1] = n[1] // 2
        elif case == "edge_minus_one" and b == 0:
            qe[j] = max(0, e[j] - 1)
        elif case == "edge_zero" and b == 0:
            qe[j] = 0
        elif case == "both":
            qn[0] = n[0] // 2
            e2 = drawn_counts(ld, pipe, i, d, qn)[1] if has_dn else e
            j2 = max(range(len(e2)), key=lambda r: e2[r])
            qe[j2] = max(0, e2[j2] - 1)
        elif case == "node_zero":                                # every slide: the type is emptied, the filler takes it whole
            qn[2] = 0
        out[i] = (qn, qe)
        if has_dn:
            xn = max([xn] + [max(0, a - q) for a, q in zip(n, qn)])
        e_after = drawn_counts(ld, pipe, i, d, qn)[1] if has_dn else e
        xe = max([xe] + [max(0, a - q) for a, q in zip(e_after, qe)])
    return out, xn, xe


def quota_fn(ld, table):
    """A callable quota over ``table`` ({slide: (qn, qe)}); other slides get their stored counts (a quota that cannot bind)."""
    return lambda i: table[i] if i in table else stored_quota(ld, i)


def truncated_slide(ld, pipe, i, draw, quota):
    """Slide i through the truncated tensor formulation: (graph, the truncated keep flags per node type)."""
    from wsi_hgnn_amd import transforms as T
    from wsi_hgnn_amd.data import slot_augment_spec
    it = ld.items[i]
    spec = slot_augment_spec(pipe)
    keep = spec.node_keep(draw, it.num_nodes, ld.device)
    if spec.drop_node is not None:
        keep = [k & (torch.cumsum(k.long(), 0) <= int(q)) for k, q in zip(keep, quota[0])]
    return T.truncated(pipe, stored_graph(ld, i), draw, quota[0], quota[1])[0], keep


def expected_tables(ld, slot, pipe, idxs, draws):
    """The contract, spelled out: slot_fill_torch over the TRUNCATED augmented slides stored anew; the two orders by the restriction rule from
    the unaugmented fill's order tables (in a layout of its own: the stored batch need not fit a quota slot) and the truncated keep flags."""
    from wsi_hgnn_amd import graph as G
    from wsi_hgnn_amd.data import StoredGraph
    lay, T = slot.layout, slot.layout.T
    its = [ld.items[i] for i in idxs]
    got = [truncated_slide(ld, pipe, i, d, slot.quota_of(i)) for i, d in zip(idxs, draws)]
    aug = [StoredGraph(g, it.label, ld.device, True) for (g, _), it in zip(got, its)]
    out = G.slot_fill_torch(lay, [a.pieces for a in aug], [a.label for a in aug], [a.feat for a in aug], None, ld.device, allow_empty_type=True)
    sb = out["batch"]
    wide = G.SlotLayout(lay.ntypes, lay.rels, [sum(it.num_nodes[t] for it in its) + 1 for t in range(T)],
                        [sum(it.pieces.ecount[t] for it in its) for t in range(T)], lay.b_cap, lay.in_dim)
    plain = G.slot_fill_torch(wide, [it.pieces for it in its], [it.label for it in its], [it.feat for it in its], None, ld.device)
    pb = plain["batch"]
    to_aug = torch.full((wide.N,), -1, dtype=torch.int64)
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
