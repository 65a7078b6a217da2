"""The packed batch of the H2MIL baseline: the three-level trees of all slides one after the other.

The reference handles one ``Data`` object (one slide) per forward.  Here a batch is the concatenation of the slides' nodes - per slide the
root, then its level-1 nodes, then its level-2 nodes, which ``from_slides`` checks - with ``tree`` and the edges renumbered to global rows.
Everything the layers need that depends on the slides' sizes alone (the rows of every level, the parent of every level-2 node as a position
among the level-1 nodes, the per-slide reduction plan) is worked out here, once per batch, from host integers: no layer reads it back.
"""
from __future__ import annotations

from typing import List, Optional, Sequence

import torch

from .. import ops


def _get(slide, name):
    return slide[name] if isinstance(slide, dict) else getattr(slide, name)


class TreeBatch:
    """``x`` [N, F]; ``node_type`` [N] in {0, 1, 2}; ``tree`` [N]: the GLOBAL row of every node's parent (-1 for a root); ``x_y_index`` [N, 2];
    ``edge_index`` [2, E] (source row 0, destination row 1, global rows); ``sizes`` / ``n1`` / ``n2``: nodes, level-1 nodes and level-2 nodes
    of every slide (host integers).  Build one with ``from_slides``; the constructor trusts its arguments."""

    def __init__(self, x, node_type, tree, x_y_index, edge_index, sizes: Sequence[int], n1: Sequence[int], n2: Sequence[int]):
        self.x, self.node_type, self.tree, self.x_y_index, self.edge_index = x, node_type, tree, x_y_index, edge_index
        self.sizes, self.n1, self.n2 = [int(c) for c in sizes], [int(c) for c in n1], [int(c) for c in n2]
        self.starts = [0]
        for c in self.sizes:
            self.starts.append(self.starts[-1] + c)
        dev = node_type.device
        B = len(self.sizes)
        ar = lambda a, b: torch.arange(a, b, dtype=torch.int64)
        cat = lambda parts: (torch.cat(parts) if parts else torch.zeros(0, dtype=torch.int64)).to(dev)
        self.roots = torch.tensor(self.starts[:-1], dtype=torch.int64).to(dev)
        self.idx1 = cat([ar(self.starts[b] + 1, self.starts[b] + 1 + self.n1[b]) for b in range(B)])
        self.idx2 = cat([ar(self.starts[b] + 1 + self.n1[b], self.starts[b + 1]) for b in range(B)])
        rep = lambda counts: torch.repeat_interleave(torch.arange(B, dtype=torch.int64), torch.tensor(counts, dtype=torch.int64)).to(dev)
        self.slide = rep(self.sizes)          # the slide of every node, of every level-1 node, of every level-2 node
        self.slide1 = rep(self.n1)
        self.slide2 = rep(self.n2)
        self.ptr1 = [0]                       # where every slide's level-1 nodes start among all level-1 nodes
        for c in self.n1:
            self.ptr1.append(self.ptr1[-1] + c)
        # the parent of every level-2 node as a position among all level-1 nodes: tree - (the slide's first level-1 row) + ptr1[slide]
        shift = torch.tensor([self.ptr1[b] - (self.starts[b] + 1) for b in range(B)], dtype=torch.int64).to(dev)
        self.parent1 = tree[self.idx2] + shift[self.slide2]
        self._ec = None
        self._rp = None

    @property
    def device(self) -> torch.device:
        return self.node_type.device

    @property
    def num_slides(self) -> int:
        return len(self.sizes)

    @property
    def num_nodes(self) -> int:
        return self.starts[-1]

    @property
    def ec(self) -> "ops.EdgeCSR":
        """The edges grouped by (destination, source type) and by source: what ``ops.ra_attention`` reads."""
        if self._ec is None:
            self._ec = ops.edge_csr_by_source_type(self.edge_index[0], self.edge_index[1], self.node_type, self.num_nodes)
        return self._ec

    @property
    def rp(self) -> "ops.ReducePlan":
        """One segment per slide."""
        if self._rp is None:
            self._rp = ops.ReducePlan.from_ptr(self.starts, self.device)
        return self._rp

    def to(self, device) -> "TreeBatch":
        device = torch.device(device)
        if device.type == self.device.type and (device.index is None or device.index == self.device.index):
            return self
        return TreeBatch(self.x.to(device), self.node_type.to(device), self.tree.to(device), self.x_y_index.to(device), self.edge_index.to(device),
                         self.sizes, self.n1, self.n2)

    def per_slide(self, t: torch.Tensor, local: Optional[str] = None) -> List[torch.Tensor]:
        """A per-node tensor cut into the slides' pieces.  ``local='tree'`` turns global parent rows into rows of the slide (the root keeps
        -1), ``local='rows'`` subtracts the slide's first row from every entry."""
        out = []
        for b in range(self.num_slides):
            p = t[self.starts[b]:self.starts[b + 1]]
            if local == "tree":
                p = torch.where(p >= 0, p - self.starts[b], p)
            elif local == "rows":
                p = p - self.starts[b]
            out.append(p)
        return out

    def edges_per_slide(self) -> List[torch.Tensor]:
        """The edges of every slide with local rows, in the batch's order (an edge belongs to the slide of its source)."""
        s = self.slide[self.edge_index[0]]
        return [self.edge_index[:, s == b] - self.starts[b] for b in range(self.num_slides)]


def from_slides(slides: Sequence, dtype: Optional[torch.dtype] = None) -> TreeBatch:
    """A packed batch from per-slide tensors named as the reference's ``Data`` fields: ``x`` [n, F], ``edge_index_tree_8nb`` [2, e],
    ``node_type`` [n], ``node_tree`` [n] (the LOCAL row of the parent, -1 for the root), ``x_y_index`` [n, 2] - objects with these attributes
    or dicts.  Refused: a slide whose nodes are not ordered root, level 1, level 2 with exactly one root, a level-1 node whose parent is not the
    root, a level-2 node whose parent is not a level-1 node of its slide, an edge that leaves its slide."""
    if not slides:
        raise ValueError("from_slides: no slide")
    xs, types, trees, xys, edges, sizes, n1s, n2s, off = [], [], [], [], [], [], [], [], 0
    for i, s in enumerate(slides):
        x, nt, tr, xy, ei = (_get(s, k) for k in ("x", "node_type", "node_tree", "x_y_index", "edge_index_tree_8nb"))
        n = x.shape[0]
        nt, tr, ei = nt.to(torch.int64).reshape(-1), tr.to(torch.int64).reshape(-1), ei.to(torch.int64)
        if x.dim() != 2 or nt.shape[0] != n or tr.shape[0] != n or tuple(xy.shape) != (n, 2) or ei.dim() != 2 or ei.shape[0] != 2:
            raise ValueError(f"from_slides: slide {i}: x [n, F], node_type [n], node_tree [n], x_y_index [n, 2], edge_index_tree_8nb [2, e]")
        h = nt.cpu()
        c0, c1, c2 = (int((h == k).sum()) for k in range(3))
        if n < 1 or c0 != 1 or c0 + c1 + c2 != n or not bool((h[1:] >= h[:-1]).all()) or int(h[0]) != 0:
            raise ValueError(f"from_slides: slide {i}: the nodes of a slide are ordered root, level 1, level 2, with exactly one root")
        th = tr.cpu()
        if int(th[0]) != -1 or not bool((th[1:1 + c1] == 0).all()) or not bool(((th[1 + c1:] >= 1) & (th[1 + c1:] <= c1)).all()):
            raise ValueError(f"from_slides: slide {i}: node_tree is -1 for the root, 0 for a level-1 node and the row of a level-1 node for a level-2 node")
        if ei.numel() and (int(ei.min()) < 0 or int(ei.max()) >= n):
            raise ValueError(f"from_slides: slide {i}: an edge names a row outside the slide")
        xs.append(x); types.append(nt); xys.append(xy); edges.append(ei + off)
        trees.append(torch.where(tr >= 0, tr + off, tr))
        sizes.append(n); n1s.append(c1); n2s.append(c2)
        off += n
    x = torch.cat(xs, 0)
    xy = torch.cat(xys, 0)
    if dtype is not None:
        x, xy = x.to(dtype), xy.to(dtype)
    return TreeBatch(x, torch.cat(types), torch.cat(trees), xy, torch.cat(edges, 1), sizes, n1s, n2s)


def tables_from_names(names: Sequence[str]):
    """The host-side name parser of one slide (github_pretreat.py:64-76).  ``names``: the patch names of the slide in file order, with or without
    an extension - ``-1`` the thumbnail (the root), ``a-b-c-d-i-j`` a 5x patch, ``x-y`` a 10x patch.  Returns ``(coords1 [n1, 2], cover [n1, 4],
    coords2 [n2, 2], perm [1 + n1 + n2])``, int64: the integer tables ``from_grid`` takes, in the reference's order (the root, the 6-field names
    in file order, the 2-field names in file order), and the permutation to apply to the feature rows (``x[perm]``).  ``ValueError``: no root or
    more than one, a name of any other shape."""
    root, l1, l2 = [], [], []
    for pos, name in enumerate(names):
        stem = str(name).split(".")[0]
        if stem == "-1":
            root.append(pos)
            continue
        fields = stem.split("-")
        try:
            values = [int(v) for v in fields]
            if len(values) not in (2, 6) or any(v < 0 for v in values) or any(not v.isdigit() for v in fields):
                raise ValueError
        except ValueError:
            raise ValueError(f"tables_from_names: {name!r} is neither '-1', a 5x name a-b-c-d-i-j nor a 10x name x-y") from None
        (l1 if len(values) == 6 else l2).append((pos, values))
    if len(root) != 1:
        raise ValueError(f"tables_from_names: a slide has exactly one root '-1', got {len(root)}")
    t = lambda rows, width: torch.tensor(rows, dtype=torch.int64).reshape(-1, width)
    return (t([v[4:] for _, v in l1], 2), t([v[:4] for _, v in l1], 4), t([v for _, v in l2], 2),
            torch.tensor(root + [p for p, _ in l1] + [p for p, _ in l2], dtype=torch.int64))


def from_grid(slides: Sequence, dtype: Optional[torch.dtype] = None, kernels: Optional[bool] = None) -> TreeBatch:
    """A packed batch from patch features and grid tables, the trees built on the device by ``construct.slide_trees`` in one pass for all
    slides.  Every slide (a dict or an object) gives ``x`` [1 + n1 + n2, F] (the root's row, the level-1 rows, the level-2 rows), ``coords1``
    [n1, 2], ``cover`` [n1, 4] and ``coords2`` [n2, 2] as ``tables_from_names`` returns them.  Equal, field by field, to ``from_slides`` of the
    tensors the reference's github_pretreat.py makes for the same slides.  ``x_y_index`` is float64 unless ``dtype`` is given (which also
    converts ``x``)."""
    from ..construct import slide_trees
    if not slides:
        raise ValueError("from_grid: no slide")
    xs, c1, cv, c2 = ([_get(s, k) for s in slides] for k in ("x", "coords1", "cover", "coords2"))
    for i, (x, a, c, b) in enumerate(zip(xs, c1, cv, c2)):
        if x.dim() != 2 or a.dim() != 2 or b.dim() != 2 or c.dim() != 2 or c.shape[0] != a.shape[0] or x.shape[0] != 1 + a.shape[0] + b.shape[0]:
            raise ValueError(f"from_grid: slide {i}: x [1 + n1 + n2, F], coords1 [n1, 2], cover [n1, 4], coords2 [n2, 2]")
    n1, n2 = [a.shape[0] for a in c1], [b.shape[0] for b in c2]
    x = torch.cat(xs, 0)
    dev = x.device
    edge_index, node_type, node_tree, xy = slide_trees(torch.cat(c1, 0).to(dev), torch.cat(cv, 0).to(dev), torch.cat(c2, 0).to(dev), n1, n2, kernels=kernels)
    if dtype is not None:
        x, xy = x.to(dtype), xy.to(dtype)
    return TreeBatch(x, node_type, node_tree, xy, edge_index, [1 + a + b for a, b in zip(n1, n2)], n1, n2)
