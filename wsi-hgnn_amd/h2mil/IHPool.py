"""IHPool of the H2MIL baseline (``baselines/H2MIL/code/IHPool.py``) at ``select='inter', dis='ou'``, over the packed batch.

Per slide the reference sorts the level-1 nodes by fitness, takes every step-th as a seed and gives every node to the nearest seed; then, in a
Python loop over the level-1 clusters with several device-to-host copies per pass, does the same for the level-2 nodes whose parents fell into
that cluster; then coarsens the graph through a dense [N, N] adjacency.  Here every slide and every substructure is a SEGMENT of one pass:

  fitness      one matrix-vector product per level
  seeds        two stable sorts (fitness, then segment) put every segment's members in ascending fitness, ties in node order; the seeds are
               the sorted positions 0, step, 2 step, ... of every segment - arithmetic on positions
  assignment   ``ops.ihpool_assign``, one launch per level for all segments of all slides (``kernels=False``: a dense [members, max seeds]
               distance table)
  means        one aggregation over the cluster map (``wsi_spmm_sum``, which has a backward)
  edges        keys cluster[u] * N + cluster[v], sorted, first occurrences kept

The layer reads back ONE small tensor per forward: the pooled size of every slide and the number of coarsened edges, B + 1 integers in one
copy (``kernels=False`` reads one more value, the largest seed count of a level-2 segment).  The pooling is not differentiable in its fitness:
``weight_1`` and ``weight_2`` decide clusters only, gradients flow through the cluster means.
Decisions where the reference leaves the outcome open: equal fitness goes in node order and equal distance to the lowest seed (torch.sort is
unstable); a seed always belongs to its own cluster (the reference mis-indexes when two seeds of a segment coincide exactly); a level-1
cluster without level-2 children contributes no level-2 cluster (the reference raises).
"""
from __future__ import annotations

import math

import torch
import torch.nn as nn

from .. import ops
from ..graph import _count
from .batch import TreeBatch


def level1_step(n: int, ratio) -> int:
    """The reference's stride over the sorted level-1 nodes (IHPool.py:128-134), its float32 rounding included."""
    if n <= 0:
        return 1
    if ratio < 1:
        return int(torch.ceil(torch.tensor(n / (n * ratio))))
    if n < ratio:
        return 1
    return int(torch.ceil(torch.tensor(n / ratio)))


def seed_count(n: int, step: int) -> int:
    return len(range(0, n, step))


def _steps_on_device(nk: torch.Tensor, ratio) -> torch.Tensor:
    """The stride of every level-2 segment from its size (IHPool.py:176-182): the float64 quotient, rounded to float32, then the ceiling - the
    same IEEE operations as the reference's Python arithmetic followed by ``torch.tensor``."""
    if ratio < 1:
        d = nk.to(torch.float64)
        step = torch.ceil((d / (d * ratio)).to(torch.float32)).to(torch.int64)
        return torch.where(nk > 0, step, torch.ones_like(step))
    return (nk - 1).clamp(min=1)


def _sorted_members(f: torch.Tensor, seg: torch.Tensor) -> torch.Tensor:
    """The members grouped by segment, ascending fitness inside a segment, equal fitness in node order."""
    o = torch.sort(f, stable=True).indices
    return o[torch.sort(seg[o], stable=True).indices]


def _assign_dense(xyf, order, seg_sorted, seed_ptr, seeds, seed_seg, valid, kmax: int) -> torch.Tensor:
    """``ops.ihpool_assign`` in tensor operations (any device and dtype) through a dense [members, max seeds] distance table.  ``seeds`` may
    be padded past ``seed_ptr[-1]`` (``valid`` False there): the padding is parked in one extra row that no member looks at."""
    dev = order.device
    if order.shape[0] == 0:
        return torch.zeros(0, dtype=torch.int64, device=dev)
    S, width = seed_ptr.shape[0] - 1, max(int(kmax), 1)
    seg_c = torch.where(valid, seed_seg, torch.full_like(seed_seg, S))
    pos = torch.where(valid, torch.arange(seeds.shape[0], device=dev) - seed_ptr[seg_c], torch.zeros_like(seeds))
    tab = torch.full((S + 1, width), -1, dtype=torch.int64, device=dev)
    tab[seg_c, pos] = torch.where(valid, seeds, torch.full_like(seeds, -1))
    cand = tab[seg_sorted]                                                     # [m, width]
    me = xyf[order]
    sd = xyf[cand.clamp(min=0)]
    d = (sd[..., :2] - me[:, None, :2]).pow(2).sum(-1).sqrt() + (sd[..., 2] - me[:, None, 2]).abs()
    d = torch.where(cand == order[:, None], torch.full_like(d, -1.0), d)
    d = torch.where(cand < 0, torch.full_like(d, math.inf), d)
    col = torch.arange(width, device=dev).expand_as(cand)
    hit = torch.where((d == d.min(1, keepdim=True).values) & (cand >= 0), col, torch.full_like(col, width))
    best = hit.min(1).values                                                   # the LOWEST position among equal distances
    return torch.where(best < width, best, torch.full_like(best, -1))


class IHPool(nn.Module):
    """The reference's constructor arguments and defaults.  ``state_dict`` keeps ``weight_1``, ``weight_2``, ``lin.*`` and ``att.*``; the
    reference's ``gnn_score.*`` entries (torch_geometric's LEConv, which never enters ``forward``) are accepted and dropped on load.
    ``forward(x, batch)`` with ``batch`` a ``TreeBatch`` whose ``x_y_index`` already holds the coordinates the layer is to use; returns
    ``(x_new, batch_new, cluster, fitness)``: ``batch_new`` carries the pooled node types, trees, coordinates and edges, ``cluster`` [N] maps
    old rows to new rows, ``fitness`` [N] is 0 for roots.  ``readbacks`` counts the device-to-host copies made so far."""

    def __init__(self, in_channels: int, ratio=0.1, GNN=None, dropout: float = 0.0, select="inter", dis="ou", kernels=True, **kwargs):
        super().__init__()
        if select != "inter" or dis != "ou":
            raise ValueError("IHPool: select='inter' and dis='ou' (anything else is a NameError in the reference)")
        if GNN is not None:
            raise ValueError("IHPool: the GNN argument builds a layer the reference's forward never calls; it is not built")
        if not ratio > 0:
            raise ValueError(f"IHPool: ratio {ratio!r} must be positive")
        self.in_channels, self.ratio, self.dropout, self.GNN, self.select, self.dis = in_channels, ratio, dropout, GNN, select, dis
        self.kernels = bool(kernels)
        self.lin = nn.Linear(in_channels, in_channels)
        self.att = nn.Linear(2 * in_channels, 1)
        self.weight_1 = nn.Parameter(torch.empty(1, in_channels))
        self.weight_2 = nn.Parameter(torch.empty(1, in_channels))
        self.nonlinearity = torch.tanh
        self.readbacks = 0
        self.reset_parameters()

    def reset_parameters(self):
        self.lin.reset_parameters()
        self.att.reset_parameters()
        bound = 1.0 / math.sqrt(self.in_channels)
        self.weight_1.data.uniform_(-bound, bound)
        self.weight_2.data.uniform_(-bound, bound)

    def _load_from_state_dict(self, state_dict, prefix, *args, **kwargs):
        for k in [k for k in state_dict if k.startswith(prefix + "gnn_score.")]:
            del state_dict[k]
        super()._load_from_state_dict(state_dict, prefix, *args, **kwargs)

    def _assign(self, xyf, order, seg_sorted, seed_ptr, seeds, seed_seg, valid, kmax):
        if self.kernels:
            i32 = lambda t: t.to(torch.int32)
            return ops.ihpool_assign(xyf.to(torch.float32), i32(order), i32(seg_sorted), i32(seed_ptr), i32(seeds)).to(torch.int64)
        if kmax is None:                                                        # (the tensor-operation path sizes its distance table)
            self.readbacks += 1
            kmax = int((seed_ptr[1:] - seed_ptr[:-1]).max()) if seed_ptr.numel() > 1 else 0
        return _assign_dense(xyf, order, seg_sorted, seed_ptr, seeds, seed_seg, valid, kmax)

    def forward(self, x: torch.Tensor, tb: TreeBatch):
        dev, B, N = x.device, tb.num_slides, tb.num_nodes
        if x.dim() != 2 or x.shape[0] != N:
            raise ValueError(f"IHPool: x is [N, C] with the batch's N = {N} rows, got {tuple(x.shape)}")
        i64 = lambda v: torch.tensor(v, dtype=torch.int64).to(dev)
        xy = tb.x_y_index.to(x.dtype)
        with torch.no_grad():
            xd = x.detach()
            w1, w2 = self.weight_1.detach().to(x.dtype), self.weight_2.detach().to(x.dtype)
            f1 = torch.tanh((xd[tb.idx1] * w1).sum(-1) / w1.norm(p=2, dim=-1))
            f2 = torch.tanh((xd[tb.idx2] * w2).sum(-1) / w2.norm(p=2, dim=-1))
            # ---- level 1: one segment per slide; every count is a function of the slides' sizes (host integers)
            steps1 = [level1_step(n, self.ratio) for n in tb.n1]
            K1 = [seed_count(n, s) for n, s in zip(tb.n1, steps1)]
            sp1 = [0]
            for k in K1:
                sp1.append(sp1[-1] + k)
            K1tot = sp1[-1]
            sp1_dev = i64(sp1)
            order1 = _sorted_members(f1, tb.slide1)
            seed_seg1 = i64([b for b in range(B) for _ in range(K1[b])])       # = the slide of every level-1 cluster
            seeds1 = order1[i64([tb.ptr1[b] + j * steps1[b] for b in range(B) for j in range(K1[b])])]
            xyf1 = torch.cat([xy[tb.idx1], f1[:, None]], 1)
            c1 = torch.empty_like(order1)
            c1[order1] = self._assign(xyf1, order1, tb.slide1[order1], sp1_dev, seeds1, seed_seg1, torch.ones_like(seeds1, dtype=torch.bool),
                                      max(K1, default=0))
            c1g = c1 + sp1_dev[tb.slide1]                                       # the level-1 cluster of every level-1 node, among all slides'
            # ---- level 2: one segment per level-1 cluster; sizes, strides and seed counts stay on the device
            M2 = tb.idx2.shape[0]
            seg2 = c1g[tb.parent1]
            nk = _count(seg2, K1tot)
            step2 = _steps_on_device(nk, self.ratio)
            kk = torch.where(nk > 0, (nk + step2 - 1) // step2, torch.zeros_like(nk))
            zero = torch.zeros(1, dtype=torch.int64, device=dev)
            sp2 = torch.cat([zero, torch.cumsum(kk, 0)])
            mem2 = torch.cat([zero, torch.cumsum(nk, 0)])
            order2 = _sorted_members(f2, seg2)
            # a segment has at most as many seeds as members: the seed list is laid out over M2 slots, the unused tail marked invalid, so that
            # its length need not be known here
            slot_i = torch.arange(M2, device=dev)
            seed_seg2 = torch.searchsorted(sp2[1:].contiguous(), slot_i, right=True)            # K1tot for the unused tail
            valid2 = slot_i < sp2[-1]
            sseg = seed_seg2.clamp(max=max(K1tot - 1, 0))
            pos2 = (mem2[sseg] + (slot_i - sp2[sseg]) * step2[sseg]).clamp(min=0, max=max(M2 - 1, 0)) if K1tot else slot_i
            seeds2 = torch.where(valid2, order2[pos2], torch.full_like(pos2, -1))
            xyf2 = torch.cat([xy[tb.idx2], f2[:, None]], 1)
            c2 = torch.empty_like(order2)
            c2[order2] = self._assign(xyf2, order2, seg2[order2], sp2, seeds2, seed_seg2, valid2, None)
            c2g = c2 + sp2[seg2]
            # ---- a provisional numbering that needs no pooled size: slide b's new nodes are numbered from the slide's OLD first row, in the
            # final order (root, level-1 clusters, level-2 clusters); the final numbering is a per-slide shift of it
            starts = i64(tb.starts[:-1])
            base2 = sp2[sp1_dev]                                                # [B + 1]: where every slide's level-2 clusters start
            prov = torch.empty(N, dtype=torch.int64, device=dev)
            prov[tb.roots] = starts
            prov[tb.idx1] = (starts + 1 - sp1_dev[:-1])[tb.slide1] + c1g
            prov[tb.idx2] = (starts + 1 + i64(K1) - base2[:-1])[tb.slide2] + c2g
            # ---- coarsened edges: the distinct pairs over the input edges and one self loop per node (IHPool.py:109,215-220), sorted by
            # (source, destination); the provisional numbering is a monotone image of the final one, so this order is the final order
            keys = torch.sort(torch.cat([prov[tb.edge_index[0]] * N + prov[tb.edge_index[1]], prov * (N + 1)])).values
            first = torch.ones_like(keys, dtype=torch.bool)
            first[1:] = keys[1:] != keys[:-1]
            slot = torch.cumsum(first, 0) - 1
            # ---- THE read-back: the pooled level-2 clusters of every slide and the number of distinct edges, B + 1 integers in one copy
            self.readbacks += 1
            back = torch.cat([base2[1:] - base2[:-1], slot[-1:] + 1]).tolist()
            T2, n_edges = [int(t) for t in back[:B]], int(back[B])
            new_sizes = [1 + K1[b] + T2[b] for b in range(B)]
            new_starts = [0]
            for c in new_sizes:
                new_starts.append(new_starts[-1] + c)
            Nn, T2tot = new_starts[-1], sum(T2)
            roots_new = i64(new_starts[:-1])
            shift = starts - roots_new                                          # provisional row - final row, per slide
            cluster = prov - shift[tb.slide]
            uniq = torch.empty(n_edges, dtype=torch.int64, device=dev).scatter_(0, slot, keys)      # equal keys write equal values
            pu, pv = uniq // N, uniq % N
            edge_new = torch.stack([pu - shift[tb.slide[pu]], pv - shift[tb.slide[pv]]])
            # ---- the pooled batch's discrete fields
            type_new = torch.cat([torch.tensor([0] + [1] * K1[b] + [2] * T2[b], dtype=torch.int64) for b in range(B)]).to(dev)
            idx1_new = torch.cat([torch.arange(new_starts[b] + 1, new_starts[b] + 1 + K1[b]) for b in range(B)]).to(dev)
            idx2_new = torch.cat([torch.arange(new_starts[b] + 1 + K1[b], new_starts[b + 1]) for b in range(B)]).to(dev)
            l1_final = roots_new + 1 - sp1_dev[:-1]                             # final row of level-1 cluster k of slide b: l1_final[b] + k
            parent_seg = seed_seg2[:T2tot]                                      # the level-1 cluster every level-2 cluster hangs under
            tree_new = torch.empty(Nn, dtype=torch.int64, device=dev)
            tree_new[roots_new] = -1
            tree_new[idx1_new] = roots_new[seed_seg1]
            tree_new[idx2_new] = l1_final[seed_seg1[parent_seg]] + parent_seg
            counts = _count(cluster, Nn)
            fitness = torch.zeros(N, dtype=x.dtype, device=dev)
            fitness[tb.idx1] = f1
            fitness[tb.idx2] = f2
        # ---- cluster means: x with a gradient, the coordinates without (the root's are (0, 0), IHPool.py:146)
        x_new = self._cluster_mean(x, cluster, counts, Nn)
        with torch.no_grad():
            xy_new = self._cluster_mean(xy, cluster, counts, Nn).to(xy.dtype)
            xy_new[roots_new] = 0
        return x_new, TreeBatch(x_new, type_new, tree_new, xy_new, edge_new, new_sizes, K1, T2), cluster, fitness

    def _cluster_mean(self, t, cluster, counts, Nn):
        n, D = t.shape
        if self.kernels:
            ec = ops.EdgeCSR(cluster, torch.arange(n, device=t.device), n)
            inv = torch.zeros(n, dtype=torch.float32, device=t.device)
            inv[:Nn] = 1.0 / counts.to(torch.float32)
            ec.in_norm = inv
            return ops.graph_conv_aggregate(t.to(torch.float32).contiguous(), None, ec, False)[:Nn]
        return torch.zeros((Nn, D), dtype=t.dtype, device=t.device).index_add(0, cluster, t) / counts.to(t.dtype)[:, None]

    def __repr__(self):
        return "{}({}, ratio={})".format(self.__class__.__name__, self.in_channels, self.ratio)
