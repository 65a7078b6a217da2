"""The packed graph batch of the GTNMIL baseline: the rows of all slides one after the other, the adjacency as a list of entries.

The reference pads every slide to the largest one and carries a dense ``[B, Nmax, Nmax]`` adjacency with a ``[B, Nmax]`` mask
(``helper.preparefeatureLabel``).  Here a batch is ``x`` [N, F], the entries ``(row, col, weight)`` of the block-diagonal adjacency and the
slides' sizes; ``from_dense`` converts the reference's three tensors, a homogeneous ``HeteroGraph`` batch converts through ``as_batch``.
"""
from __future__ import annotations

from typing import Optional, Sequence

import torch

from .. import ops
from ..graph import HeteroGraph


class GraphBatch:
    """``x`` [N, F] fp32; ``row`` / ``col`` int64 [E] (global row numbers; A[row, col] += weight, repeated entries add up); ``weight`` fp32 [E]
    or None (= 1); ``sizes``: rows of every slide, in order.  A slide without rows is refused: the reference's mincut loss of an all-masked
    slide is 0 / 0 and its BatchNorm sees no row of it."""

    def __init__(self, x: torch.Tensor, row: torch.Tensor, col: torch.Tensor, weight: Optional[torch.Tensor], sizes: Sequence[int]):
        sizes = [int(c) for c in sizes]
        if any(c <= 0 for c in sizes):
            raise ValueError("GraphBatch: a graph without rows (the mincut loss and the BatchNorm statistics are undefined for it)")
        if x.dim() != 2 or x.shape[0] != sum(sizes):
            raise ValueError(f"GraphBatch: x is [N, F] with N = {sum(sizes)} rows, got {tuple(x.shape)}")
        if row.shape != col.shape or row.dim() != 1 or (weight is not None and weight.shape != row.shape):
            raise ValueError("GraphBatch: row, col (and weight) are 1-D tensors of one length")
        self.x = x.to(torch.float32)
        self.row, self.col = row.to(torch.int64), col.to(torch.int64)
        self.weight = None if weight is None else weight.detach().to(torch.float32)
        self.sizes = sizes
        self._ec = None
        self._rp = None
        self._seg = None

    @property
    def device(self) -> torch.device:
        return self.x.device

    @property
    def num_graphs(self) -> int:
        return len(self.sizes)

    @property
    def num_rows(self) -> int:
        return self.x.shape[0]

    def to(self, device) -> "GraphBatch":
        device = torch.device(device)
        if device.type == self.x.device.type and (device.index is None or device.index == self.x.device.index):
            return self
        return GraphBatch(self.x.to(device), self.row.to(device), self.col.to(device), None if self.weight is None else self.weight.to(device), self.sizes)

    @property
    def ec(self) -> "ops.EdgeCSR":
        """The adjacency grouped by row (CSR) and by column (CSC), weights attached: what the kernels read."""
        if self._ec is None:
            self._ec = ops.EdgeCSR(self.row, self.col, self.num_rows).with_weights(self.weight)
        return self._ec

    @property
    def rp(self) -> "ops.ReducePlan":
        """One segment per slide."""
        if self._rp is None:
            ptr = [0]
            for c in self.sizes:
                ptr.append(ptr[-1] + c)
            self._rp = ops.ReducePlan.from_ptr(ptr, self.x.device)
        return self._rp

    def segment(self) -> torch.Tensor:
        """[N] int64: the slide of every row (the tensor-operation path)."""
        if self._seg is None:
            self._seg = torch.repeat_interleave(torch.arange(len(self.sizes)), torch.tensor(self.sizes, dtype=torch.int64)).to(self.x.device)
        return self._seg


def from_dense(node_feat: torch.Tensor, adj: torch.Tensor, mask: torch.Tensor) -> GraphBatch:
    """The reference's padded tensors - ``node_feat`` [B, Nmax, F], ``adj`` [B, Nmax, Nmax], ``mask`` [B, Nmax] with the real rows of every slide
    first - as a packed batch: the non-zero entries of each slide's leading block, in row-major order, with their values as weights."""
    if node_feat.dim() != 3 or adj.shape != (node_feat.shape[0], node_feat.shape[1], node_feat.shape[1]) or mask.shape != node_feat.shape[:2]:
        raise ValueError("from_dense: node_feat [B, Nmax, F], adj [B, Nmax, Nmax], mask [B, Nmax]")
    sizes = [int(c) for c in mask.sum(1).round().to(torch.int64).tolist()]
    for b, c in enumerate(sizes):
        if not bool((mask[b, :c] != 0).all()) or bool((mask[b, c:] != 0).any()):
            raise ValueError("from_dense: the real rows of a slide come first (a mask of ones followed by zeros)")
    xs, rows, cols, ws, off = [], [], [], [], 0
    for b, c in enumerate(sizes):
        xs.append(node_feat[b, :c])
        nz = adj[b, :c, :c].nonzero()
        rows.append(nz[:, 0] + off)
        cols.append(nz[:, 1] + off)
        ws.append(adj[b, :c, :c][nz[:, 0], nz[:, 1]])
        off += c
    return GraphBatch(torch.cat(xs, 0), torch.cat(rows), torch.cat(cols), torch.cat(ws).to(torch.float32), sizes)


def as_batch(batch) -> GraphBatch:
    """A ``GraphBatch`` as it is; a homogeneous ``HeteroGraph`` batch with its features in ``ndata['feat']``: an edge u -> v is the entry
    A[v, u] = 1 (the destination aggregates its sources).  The conversion is kept on the graph."""
    if isinstance(batch, GraphBatch) or getattr(batch, "is_slot", False):       # (a gtn.GraphSlot passes through: the model reads its masks)
        return batch
    if isinstance(batch, HeteroGraph):
        if not batch.is_homogeneous:
            raise ValueError("gtn: a homogeneous graph batch (one node type, one relation) or a gtn.GraphBatch")
        feat = batch.ndata["feat"]
        cache = batch.__dict__.setdefault("_gtn_batches", {})
        hit = cache.get(str(feat.device))
        if hit is None:
            u, v = batch.edges()
            hit = cache[str(feat.device)] = GraphBatch(feat, v.to(feat.device), u.to(feat.device), None,
                                                       [int(c) for c in batch.batch_num_nodes().tolist()])
        return hit
    raise TypeError(f"gtn: expected a HeteroGraph batch or a gtn.GraphBatch, got {type(batch).__name__}")


def read_coords(path: str) -> torch.Tensor:
    """The reference's ``c_idx.txt`` (build_graphs.py:72-76: one ``x<TAB>y`` line per patch, in file order) as an int64 [n, 2] tensor."""
    rows = []
    with open(path, "r") as f:
        for number, line in enumerate(f, 1):
            if not line.strip():
                continue
            fields = line.rstrip("\n").split("\t")
            try:
                if len(fields) != 2:
                    raise ValueError
                rows.append((int(fields[0]), int(fields[1])))
            except ValueError:
                raise ValueError(f"read_coords: {path}:{number}: expected two integers separated by a tab, got {line.rstrip()!r}") from None
    return torch.tensor(rows, dtype=torch.int64).reshape(-1, 2)


def from_grid(feats, coords, sizes: Optional[Sequence[int]] = None, kernels: Optional[bool] = None) -> GraphBatch:
    """A packed batch from patch features and grid coordinates, with the reference's adjacency (build_graphs.py:78-96: 1 where two patches of a
    slide are at most one grid step apart in x and in y) built on the device by ``construct.grid_adjacency`` - no dense matrix, no host loop.
    ``feats`` / ``coords``: lists of per-slide [n, F] / [n, 2] tensors, or packed tensors [N, F] / [N, 2] with ``sizes``.  The entries come in the
    order ``from_dense`` gives for the reference's dense matrix; ``weight`` is None (every entry is 1)."""
    from ..construct import grid_adjacency
    if isinstance(feats, torch.Tensor) != isinstance(coords, torch.Tensor):
        raise ValueError("from_grid: feats and coords are both lists of per-slide tensors or both packed tensors")
    if isinstance(feats, torch.Tensor):
        if sizes is None:
            raise ValueError("from_grid: packed tensors need the slides' sizes")
    else:
        if sizes is not None or len(feats) != len(coords) or not len(feats):
            raise ValueError("from_grid: one coordinate tensor per feature tensor, at least one slide, and no sizes with lists")
        if any(f.dim() != 2 or c.dim() != 2 or f.shape[0] != c.shape[0] for f, c in zip(feats, coords)):
            raise ValueError("from_grid: every slide gives feats [n, F] and coords [n, 2] with one n")
        sizes = [f.shape[0] for f in feats]
        feats, coords = torch.cat(list(feats), 0), torch.cat(list(coords), 0)
    if feats.dim() != 2 or feats.shape[0] != coords.shape[0]:
        raise ValueError("from_grid: one coordinate pair per feature row")
    coords = coords.to(feats.device)
    row, col = grid_adjacency(coords, sizes, kernels=kernels)
    return GraphBatch(feats, row, col, None, sizes)
