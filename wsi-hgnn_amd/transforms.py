"""Train-time graph augmentation: the ``dgl.transforms`` the reference puts in front of every TRAINING graph (data.py:16-23,116-117)

    Compose([DropNode(p=0.5), DropEdge(p=0.5), NodeShuffle(), FeatMask(p=0.5, node_feat_names=['feat'])])

with the names and constructor arguments of ``dgl.transforms``; ``reference_train_transform()`` returns exactly that pipeline.  Validation and
test graphs are left alone there (``type_ == "train"`` only), so evaluation loaders take no transform.

Every transform is a callable ``(HeteroGraph, draw=None) -> HeteroGraph`` that returns a NEW graph and never writes to its input (DGL clones
first; tensors a transform does not change may be shared with the input), works on SINGLE graphs only (a batch raises ``ValueError``, as
``graph.remove_nodes`` does: augment the slides, then batch them) and runs on a CPU graph as plain tensor operations - the code below - and
on a GPU graph through the HIP kernels of csrc/augment.hip (``ops.augment_graph``).  Semantics follow DGL's documented behaviour; DGL is not
installed where this package is developed, so parity with DGL itself is unpinned, as for the rest of the DGL surface (oracle/dgl_semantics.py).

* ``DropNode``: per node type (``g.ntypes`` order) one Bernoulli(p) draw per node; the drawn nodes and every edge that touches one go, survivors
  keep their relative order (ids shift down), all node and edge fields follow, the schema is kept (a relation may end with 0 edges, a type
  with 0 nodes: SURVEY A.1.5).
* ``DropEdge``: per canonical relation one draw per edge; edge order is otherwise stable, edge fields (``sim``) follow.
* ``NodeShuffle``: per node type a random permutation ``perm``; every node field ``x`` becomes ``x[perm]``.  Edges are untouched, so features
  MOVE to other nodes: not a relabelling, model outputs change.  ``'_pos'`` (this container's own field, ``graph.apply_locality_order``)
  no longer describes the topology afterwards and is dropped from the output.
* ``FeatMask``: for each name in ``node_feat_names`` and each node type that has the field one draw per feature COLUMN (its own per type); the
  drawn columns are 0 for all nodes of the type; ``edge_feat_names`` likewise per relation.  A name no type has is skipped, as DGL skips it.

Draws are counter-based like ``ops.CounterDropout``: every decision is a function of (draw seed, the transform's number in the pipeline,
type / relation index, element index), specified in include/wsi_hgnn.h beside the dropout contract.  The element index counts in the graph the
transform RECEIVES (DropEdge behind DropNode indexes the surviving edges).  ``draw`` is the 32-bit seed; ``draw=None`` takes one from torch's
CPU generator (``torch.manual_seed`` replays a run; no device round trip).  A transform called on its own is number 0 of its pipeline;
``index=k`` places it (so ``Compose([a, b])(g, draw=s)`` equals ``b(a(g, draw=s, index=0), draw=s, index=1)``).  The CPU and the GPU produce the
same graph from the same draw, bit for bit.
"""
from __future__ import annotations

from collections import OrderedDict
from typing import Callable, List, Optional, Sequence

import torch

from . import ops
from .graph import HeteroGraph


def _single(g: HeteroGraph) -> None:
    if g._batch_num_nodes is not None and g.batch_size > 1:
        raise ValueError("graph transforms work on single graphs (augment the slides, then batch them)")


def _seed(draw) -> int:
    return ops.next_dropout_seed() if draw is None else int(draw) & 0xffffffff


def _copy_frames(g: HeteroGraph, out: HeteroGraph, node=lambda t, k, x: x, edge=lambda r, k, x: x) -> HeteroGraph:
    for t in g.ntypes:
        for k, x in g._nframes[t].items():
            y = node(t, k, x)
            if y is not None:
                out._nframes[t][k] = y
    for r in g.canonical_etypes:
        for k, x in g._eframes[r].items():
            out._eframes[r][k] = edge(r, k, x)
    return out


class BaseTransform:
    """Common calling convention; ``kind`` names the transform for the fused device path."""
    kind: str = ""
    p: float = 0.0
    node_feat_names = None
    edge_feat_names = None

    def stage(self, k: int):
        return (self.kind, int(k), float(self.p), self.node_feat_names, self.edge_feat_names)

    def __call__(self, g: HeteroGraph, draw=None, index: int = 0, fused: Optional[bool] = None) -> HeteroGraph:
        _single(g)
        seed = _seed(draw)
        if g.device.type == "cuda" and (fused is None or fused):
            return ops.augment_graph(g, [self.stage(index)], seed)
        return self.apply(g, seed, int(index))

    def apply(self, g: HeteroGraph, seed: int, k: int) -> HeteroGraph:        # the tensor formulation (any device)
        raise NotImplementedError

    def __repr__(self) -> str:
        return f"{type(self).__name__}()"


class DropNode(BaseTransform):
    kind = "drop_node"

    def __init__(self, p: float = 0.5):
        self.p = float(p)
        self.threshold = ops.augment_threshold(p)

    def apply(self, g, seed, k, quota=None, excess=None):
        """``quota[j]`` (``truncated``): of the nodes of type j that the draw keeps only the first ``quota[j]`` in node-id order stay, the others
        go exactly as if drawn; ``excess``: a list that receives, per type, by how many the draw exceeded its quota."""
        dev = g.device
        keep, new_id, counts = {}, {}, OrderedDict()
        for j, t in enumerate(g.ntypes):
            keep[t] = ~ops.augment_drawn(g.num_nodes(t), ops.augment_subseed(seed, k, j), self.threshold, dev)
            if quota is not None:
                if excess is not None:
                    excess.append(max(0, int(keep[t].sum()) - int(quota[j])))
                keep[t] = keep[t] & (torch.cumsum(keep[t], 0) <= int(quota[j]))
            new_id[t] = torch.cumsum(keep[t], 0) - 1
            counts[t] = int(keep[t].sum())
        edges, emask = OrderedDict(), {}
        for (s, e, d) in g.canonical_etypes:
            u, v = g._edges[(s, e, d)]
            m = keep[s][u] & keep[d][v]
            edges[(s, e, d)] = (new_id[s][u[m]], new_id[d][v[m]])
            emask[(s, e, d)] = m
        return _copy_frames(g, HeteroGraph(counts, edges), lambda t, key, x: x[keep[t]], lambda r, key, x: x[emask[r]])

    def __repr__(self):
        return f"DropNode(p={self.p})"


class DropEdge(BaseTransform):
    kind = "drop_edge"

    def __init__(self, p: float = 0.5):
        self.p = float(p)
        self.threshold = ops.augment_threshold(p)

    def apply(self, g, seed, k):
        edges, emask = OrderedDict(), {}
        for j, r in enumerate(g.canonical_etypes):
            u, v = g._edges[r]
            m = ~ops.augment_drawn(u.numel(), ops.augment_subseed(seed, k, j), self.threshold, u.device)
            edges[r] = (u[m], v[m])
            emask[r] = m
        out = HeteroGraph(OrderedDict((t, g.num_nodes(t)) for t in g.ntypes), edges)
        return _copy_frames(g, out, edge=lambda r, key, x: x[emask[r]])

    def __repr__(self):
        return f"DropEdge(p={self.p})"


class NodeShuffle(BaseTransform):
    kind = "node_shuffle"

    def permutation(self, n: int, seed: int, k: int, j: int, device="cpu") -> torch.Tensor:
        """The permutation of node type number ``j``: stable argsort of the 32-bit hash keys (equal keys in index order)."""
        return torch.sort(ops.augment_hash(n, ops.augment_subseed(seed, k, j), device), stable=True).indices

    def apply(self, g, seed, k):
        perm = {t: self.permutation(g.num_nodes(t), seed, k, j, g.device) for j, t in enumerate(g.ntypes)}
        out = HeteroGraph(OrderedDict((t, g.num_nodes(t)) for t in g.ntypes), OrderedDict(g._edges))
        return _copy_frames(g, out, lambda t, key, x: None if key == "_pos" else x[perm[t]])


class FeatMask(BaseTransform):
    kind = "feat_mask"

    def __init__(self, p: float = 0.5, node_feat_names: Optional[Sequence[str]] = None, edge_feat_names: Optional[Sequence[str]] = None):
        self.p = float(p)
        self.threshold = ops.augment_threshold(p)
        self.node_feat_names = None if node_feat_names is None else list(node_feat_names)
        self.edge_feat_names = None if edge_feat_names is None else list(edge_feat_names)

    def apply(self, g, seed, k):
        nn_, en = self.node_feat_names or [], self.edge_feat_names or []
        tix = {t: j for j, t in enumerate(g.ntypes)}
        rix = {r: j for j, r in enumerate(g.canonical_etypes)}
        node = lambda t, key, x: ops.mask_columns(x, ops.augment_subseed(seed, k, 65536 * nn_.index(key) + tix[t]), self.threshold) if key in nn_ else x
        edge = lambda r, key, x: ops.mask_columns(x, ops.augment_subseed(seed, k, 65536 * en.index(key) + 32768 + rix[r]), self.threshold) if key in en else x
        out = HeteroGraph(OrderedDict((t, g.num_nodes(t)) for t in g.ntypes), OrderedDict(g._edges))
        return _copy_frames(g, out, node, edge)

    def __repr__(self):
        return f"FeatMask(p={self.p}, node_feat_names={self.node_feat_names}, edge_feat_names={self.edge_feat_names})"


class Compose:
    """``dgl.transforms.Compose``: the transforms one after another, under ONE draw; member number k uses transform index k.

    On a GPU graph every run of consecutive members that are transforms of this module, with no kind twice, is ONE ``ops.augment_graph`` call:
    any sub-sequence of the four, in the order given, at a launch count that does not depend on the run's length (a kind that occurs again
    starts the next run).  Foreign callables are applied one by one as ``f(g)``.  ``fused=False`` keeps the tensor formulation on the GPU as
    well (tools/augment_bench.py times one against the other)."""

    def __init__(self, transforms: Sequence[Callable], fused: Optional[bool] = None):
        self.transforms: List[Callable] = list(transforms)
        self.fused = fused

    def __call__(self, g: HeteroGraph, draw=None, fused: Optional[bool] = None, quota=None) -> HeteroGraph:
        """``quota=(qn, qe)``: the truncated pipeline (``truncated``; tensor formulation on any device).  ``None``: the pipeline as drawn."""
        if quota is not None:
            return truncated(self, g, draw, quota[0], quota[1])[0]
        seed = _seed(draw)
        fused = self.fused if fused is None else fused
        run: list = []

        def flush(g):
            if run:
                _single(g)
                g = ops.augment_graph(g, [t.stage(k) for k, t in run], seed)
                run.clear()
            return g

        for k, t in enumerate(self.transforms):
            if not isinstance(t, BaseTransform):
                g = t(flush(g))
            elif g.device.type == "cuda" and (fused is None or fused):
                if any(t.kind == u.kind for _, u in run):
                    g = flush(g)
                run.append((k, t))
            else:
                _single(g)
                g = t.apply(g, seed, k)
        return flush(g)

    def __repr__(self):
        return "Compose([" + ", ".join(repr(t) for t in self.transforms) + "])"


def truncated(pipe: Compose, g: HeteroGraph, draw, qn=None, qe=None):
    """The pipeline under survivor QUOTAS (what a ``data.BatchSlot(quota=...)`` holds): ``qn[t]`` per node type and ``qe[j]`` per
    relation, in ``g.ntypes`` / ``g.canonical_etypes`` order, either may be None.

    * The node quota acts inside DropNode: of the nodes of type t it keeps, the first ``qn[t]`` in node-id order stay; the others are removed
      as if drawn, their edges in the same stage.  A DropEdge behind DropNode ranks the edges that remain, a NodeShuffle behind it permutes the
      nodes that remain.  Without a DropNode in the pipeline the node quota is ignored.
    * The edge quota acts behind the last stage: relation j keeps the first ``qe[j]`` of its final edges in input order (which every stage
      preserves); edge fields follow.
    * A quota that is not reached changes nothing: the result is ``pipe(g, draw, fused=False)`` bit for bit.

    Tensor formulation, any device.  Returns ``(graph, node_excess, edge_excess)``: by how many the draw exceeded the quota of every node type
    (survivors of DropNode's draw minus ``qn[t]``; empty without DropNode or ``qn``) and of every relation (final edges of the node-truncated
    pipeline minus ``qe[j]``), zeros where it did not."""
    seed = _seed(draw)
    _single(g)
    xn: List[int] = []
    for k, t in enumerate(pipe.transforms):
        if not isinstance(t, BaseTransform):
            raise ValueError("truncated: every member of the pipeline must be a transform of this module")
        g = t.apply(g, seed, k, quota=qn, excess=xn) if isinstance(t, DropNode) and qn is not None else t.apply(g, seed, k)
    if qe is None:
        return g, xn, []
    lim = {r: max(0, int(qe[j])) for j, r in enumerate(g.canonical_etypes)}
    xe = [max(0, g._edges[r][0].numel() - lim[r]) for r in g.canonical_etypes]
    if any(xe):
        edges = OrderedDict((r, (u[:lim[r]], v[:lim[r]])) for r, (u, v) in g._edges.items())
        g = _copy_frames(g, HeteroGraph(OrderedDict((t, g.num_nodes(t)) for t in g.ntypes), edges), edge=lambda r, key, x: x[:lim[r]])
    return g, xn, xe


def reference_train_transform() -> Compose:
    """The reference's training pipeline (data.py:16-23)."""
    return Compose([DropNode(p=0.5), DropEdge(p=0.5), NodeShuffle(), FeatMask(p=0.5, node_feat_names=["feat"])])
