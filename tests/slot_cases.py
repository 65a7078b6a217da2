"""Shared fixture of tests/test_batch_slot.py and tests/test_batch_slot_gpu.py: a small data set and the batches that exercise a padded
batch slot's edge cases.  3 node types, 48-d features, slides of 60-420 nodes, B_cap = 2.

Slides (synthetic.hetero_graph: 50/30/20 % node types, 8 in-edges per node; sorted relations: slot 0 of destination type 0 and 1 comes from type
0, of type 2 from type 1):
  0: 400 nodes (200, 120, 80)   1: 300 (150, 90, 60)   2: 200 (100, 60, 40)   3: 120 (60, 36, 24)   4: 60 (30, 18, 12)
  5: 100 nodes, NO node of type 2 (60, 40, 0)          6: 250, hub destinations (125, 75, 50)       7: 420 (210, 126, 84)
Big slot: N_cap = (351, 215, 150), E_cap = (3100, 1680, 1125).  Small slot: N_cap = (95, 58, 40), E_cap = (760, 432, 300)."""
import torch

IN_DIM = 48
ND = {"0": 0, "1": 1, "2": 2}
BIG = ((351, 215, 150), (3100, 1680, 1125), 2)
SMALL = ((95, 58, 40), (760, 432, 300), 2)
LABELS = [1, 0, 1, 1, 0, 0, 1, 0]

# batches of the big slot and the edge case each is there for
CASES = [
    [0, 1],    # nf = (1, 5, 10), ef = (300, 0, 5): (a) ef = 0 beside ef > 0, (b) ONE filler node carries 300 edges, (c) ef < nf: zero-degree filler nodes
    [2],       # (d) one slide, the second graph is empty; a large filler
    [5, 3],    # (e) a slide without any node of type 2
    [4],       # the smallest slide
    [1, 2],    # nf != nf of the source type on every relation
    [6, 4],    # hub slide first
    [3, 5],    # (e) again, the slide without type 2 second
    [2, 6],
]
NO_FIT = [0, 7]            # (f) 410 nodes of type 0 > 351
SMALL_CASES = [[3, 4], [4], [3]]


def slides():
    from wsi_hgnn_amd import synthetic
    sizes = [400, 300, 200, 120, 60, 100, 250, 420]
    gs = []
    for i, n in enumerate(sizes):
        kw = {}
        if i == 5:
            kw["fractions"] = (0.6, 0.4, 0.0)
        if i == 6:
            kw["dst_mode"] = "hub"
        gs.append(synthetic.hetero_graph(n, IN_DIM, seed=900 + i, **kw))
    return gs


def loader(device):
    from wsi_hgnn_amd.data import GraphBatchLoader
    return GraphBatchLoader(slides(), LABELS, 2, device, shuffle=False, resident=True)
