"""Shared fixture of tests/test_slot_type_mask.py and tests/test_slot_type_mask_gpu.py: batch slots with a device-side presence
table.  3 node types, 48-d features, slides of 60-250 nodes, B_cap = 2 (synthetic.hetero_graph, 8 in-edges per node).

Slides (node counts per type):
  0: 200 (100, 60, 40)   1: 120 (60, 36, 24)   2: 100, NO node of type 2 (60, 40, 0)   3: 100, exactly THREE nodes of type 2 (57, 40, 3)
  4: 250, hub destinations (125, 75, 50)      5: 60 (30, 18, 12)                      6: 80, NO node of type 2 (48, 32, 0)
Big slot: N_cap = (200, 120, 80), E_cap = 8 N_cap.  Small slot: N_cap = (95, 58, 40).  [0, 4] (225 nodes of type 0) fits neither."""
from collections import OrderedDict

import torch

IN_DIM = 48
ND = {"0": 0, "1": 1, "2": 2}
BIG = ((200, 120, 80), (1600, 960, 640), 2)
SMALL = ((95, 58, 40), (760, 464, 320), 2)
LABELS = [1, 0, 1, 1, 0, 0, 1]
TYPELESS, THREE, HUB, RARE = 2, 3, 4, 2          # the slide without type 2, the slide with three nodes of it, the hub slide; the rare type
NO_FIT = [0, 4]
SEED = 611

# plain fills: (batch, the case it is there for)
PLAIN = [([1, TYPELESS], "the type in one of two slides"), ([TYPELESS, 6], "the type in none"), ([TYPELESS], "one slide plus an empty graph"),
         ([THREE], "three nodes of the type"), ([HUB, 5], "hub slide, every type present"), ([6, THREE], "the type in the second slide only")]

_CACHE = {}


def slides():
    if "slides" not in _CACHE:
        from wsi_hgnn_amd import synthetic
        sizes = [200, 120, 100, 100, 250, 60, 80]
        kw = {TYPELESS: {"fractions": (0.6, 0.4, 0.0)}, 6: {"fractions": (0.6, 0.4, 0.0)}, THREE: {"fractions": (0.57, 0.40, 0.03)},
              HUB: {"dst_mode": "hub"}}
        _CACHE["slides"] = [synthetic.hetero_graph(n, IN_DIM, seed=1200 + i, **kw.get(i, {})) for i, n in enumerate(sizes)]
        assert [g.num_nodes("2") for g in _CACHE["slides"]] == [40, 24, 0, 3, 50, 12, 0]
    return _CACHE["slides"]


def pipeline():
    """DropNode at p = 0.5: one draw in eight empties the three nodes of type 2 of slide THREE."""
    from wsi_hgnn_amd import transforms as T
    return T.Compose([T.DropNode(0.5), T.DropEdge(0.3), T.NodeShuffle(), T.FeatMask(0.3, node_feat_names=["feat"])])


def loader(device, augment=False):
    from wsi_hgnn_amd.data import GraphBatchLoader
    return GraphBatchLoader(slides(), LABELS, 2, device, shuffle=False, resident=True, seed=SEED, transform=pipeline() if augment else None)


def stored_graph(ld, i):
    from wsi_hgnn_amd.graph import HeteroGraph
    it = ld.items[i]
    return HeteroGraph.from_coo(OrderedDict(zip(it.ntypes, it.num_nodes)), it.edges, feat=dict(zip(it.ntypes, it.feat)), sim=it.sims)


def found_draws():
    """(a draw in 0..255 that empties type 2 of slide THREE, one that does not), searched on the CPU with the slot's own draw contract
    (``AugmentSpec.node_keep``).  A condition, not a measurement: at p = 0.5 one draw in eight empties three nodes."""
    if "draws" not in _CACHE:
        from wsi_hgnn_amd.data import slot_augment_spec
        spec = slot_augment_spec(pipeline())
        counts = [g.num_nodes(t) for g in [slides()[THREE]] for t in g.ntypes]
        left = [int(spec.node_keep(d, counts, "cpu")[RARE].sum()) for d in range(256)]
        emptying = next((d for d, k in enumerate(left) if k == 0), None)
        sparing = next((d for d, k in enumerate(left) if k > 0), None)
        assert emptying is not None and sparing is not None, "no emptying / no sparing draw among 0..255"
        _CACHE["draws"] = (emptying, sparing)
    return _CACHE["draws"]


def unpadded_augmented(ld, idxs, draws, quotas=None):
    """The slides ``idxs`` through the tensor formulation of the loader's pipeline under ``draws`` (truncated to ``quotas[b] = (qn, qe)``), as
    single graphs: what the eager loader batches for these draws."""
    from wsi_hgnn_amd import transforms as T
    out = []
    for b, (i, d) in enumerate(zip(idxs, draws)):
        g = stored_graph(ld, i)
        out.append(ld.transform(g, draw=d, fused=False) if quotas is None else T.truncated(ld.transform, g, d, *quotas[b])[0])
    return out


def expected_present(graphs):
    """Presence of every node type over single (unpadded) graphs, from their node counts."""
    return [1.0 if sum(g.num_nodes(t) for g in graphs) > 0 else 0.0 for t in graphs[0].ntypes]


def stored_quota(ld, i):
    it = ld.items[i]
    return list(it.num_nodes), [int(it.edges[r][0].numel()) for r in it.rels]
