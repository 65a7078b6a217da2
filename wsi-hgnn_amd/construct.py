"""Graph construction edge step on the GPU — the producer of the hot path's input.

Mirrors ``GraphConstructor.construct_graph`` (construct_graph/graph_constructor.py:256-303) from the point where the
per-patch features and node types exist (the CNN encoders / HoVer-Net / openslide tiling upstream are out of scope):

* reference :265-273  ``Hnsw(space='l2').fit(features)`` + one ``knnQuery(features[v], k=radius)`` per patch, first hit (the
  patch itself) dropped: ``a = repeat(range(N), radius-1)``, ``b = neighbours``; edge ``a -> b``;
* reference :276-282  ``scipy.stats.pearsonr(features[a], features[b])[0]`` in a Python loop over all E pairs; edge type
  ``1 if corr > 0 else 0`` (names ``['neg', 'pos']``), ``edata['sim'] = corr``;
* reference :285-301  ``dgl.to_heterogeneous(graph, ['0'..str(T-1)], ['neg', 'pos'])`` and a homogeneous twin.

Here: ``X X^T`` row blocks on the matrix cores (the grouped GEMM of the hot path), a streaming top-(k+pad) shortlist per row
(``wsi_knn_select``) and one gather kernel that computes, for the shortlisted pairs, the EXACT squared distance and the
Pearson correlation and keeps the ``radius-1`` nearest (``wsi_pair_stats``).  HNSW is an approximate index; this is an exact
re-ranking of a shortlist whose membership is reliable down to neighbour gaps of about ``slack``: the shortlist ranks by
``|x_j|^2 - 2 x_i.x_j`` in fp32, whose absolute error ``e`` is a few ulp of ``|x|^2`` (about 4e-4 at F = 1024, ``|x|^2`` = 350),
and ``slack = 8 e``.  Every returned distance lies within ``slack`` above the exact one at the same position, and the list is
the exact one wherever the exact distances of the ``radius-1``-th and the ``(radius+pad)``-th neighbour differ by more than
``slack``; inside a tight cluster far from the origin (near-duplicate patches) the neighbours returned are near but need not
be the nearest.  Ties are broken towards the smaller index.  A constant feature row gives ``corr`` = nan, as
``scipy.stats.pearsonr`` does, and its edges are typed ``neg``.
There is no CPU fallback: the kernels live in libwsi_hgnn.so.
"""
from __future__ import annotations

from collections import OrderedDict
from typing import Optional, Sequence, Tuple

import torch

from . import _native as N
from . import ops
from .graph import HeteroGraph

EDGE_TYPE_NAMES = ["neg", "pos"]          # graph_constructor.py:295: index = (corr > 0)


def knn_pearson(features: torch.Tensor, radius: int, pad: int = 8, block_rows: Optional[int] = None
                ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """For every row of ``features`` [N, F] (fp32, CUDA) its ``radius - 1`` nearest OTHER rows under L2.

    Returns ``(nbr [N, radius-1] int64, corr [N, radius-1] float32, dist2 [N, radius-1] float32)``, neighbours ascending by
    (distance, index).  ``pad`` extra candidates are shortlisted from the GEMM form of the distance and re-ranked exactly
    (the module docstring states how far the shortlist can be trusted).  ``block_rows``: rows of ``X X^T`` per GEMM launch.
    """
    N.require_cuda(features)
    if features.dim() != 2 or features.dtype != torch.float32:
        raise ValueError("features must be a 2-D float32 tensor")
    x = features.contiguous()
    n, F = x.shape
    keep = int(radius) - 1
    if keep < 1:
        raise ValueError("radius must be >= 2 (the first neighbour is the patch itself and is dropped)")
    if n < radius:
        raise ValueError(f"{n} patches cannot have {keep} distinct neighbours each (the reference's np.fromiter fails here too)")
    kc = min(keep + int(pad), n - 1, 32)
    if kc < keep:
        raise ValueError(f"radius - 1 = {keep} exceeds the 32-candidate limit of wsi_knn_select")
    lib = N.load()
    dev = x.device
    st = N.stream()
    sqn = torch.empty(n, dtype=torch.float32, device=dev)
    N.check(lib.wsi_row_sqnorm(N.ptr(x), F, n, F, N.ptr(sqn), st), "wsi_row_sqnorm")
    if block_rows is None:      # <= 1 GiB of dot products in flight
        block_rows = max(128, min(n, (1 << 28) // max(n, 1)))
    cand = torch.empty((n, kc), dtype=torch.int32, device=dev)
    dots = torch.empty((min(block_rows, n), n), dtype=torch.float32, device=dev)
    for r0 in range(0, n, block_rows):
        rows = min(block_rows, n - r0)
        ops._gemm(N.WSI_GEMM_NT, 0, [dict(A=N.ptr(x, r0 * F * 4), lda=F, B=N.ptr(x), ldb=F, C=N.ptr(dots), ldc=n,
                                          M=rows, N=n, K=F)], dev)
        N.check(lib.wsi_knn_select(N.ptr(dots), n, N.ptr(sqn), r0, rows, n, kc, N.ptr(cand, r0 * kc * 4), st), "wsi_knn_select")
    nbr = torch.full((n, keep), -1, dtype=torch.int32, device=dev)
    dist2 = torch.empty((n, keep), dtype=torch.float32, device=dev)
    corr = torch.empty((n, keep), dtype=torch.float32, device=dev)
    N.check(lib.wsi_pair_stats(N.ptr(x), F, n, F, N.ptr(cand), kc, keep, N.ptr(nbr), N.ptr(dist2), N.ptr(corr), st),
            "wsi_pair_stats")
    return nbr.long(), corr, dist2


def to_heterogeneous(num_nodes: int, src: torch.Tensor, dst: torch.Tensor, node_type: torch.Tensor, edge_type: torch.Tensor,
                     ntypes, etypes, feat: Optional[torch.Tensor] = None, sim: Optional[torch.Tensor] = None) -> HeteroGraph:
    """``dgl.to_heterogeneous`` as graph_constructor.py:292-296 uses it: nodes of each type are renumbered in increasing
    homogeneous id (``ndata['_ID']`` keeps the original id), one relation per (source type, edge type, destination type)
    triple that occurs, edges in their original order.  Relations are ordered lexicographically by (source type id, edge
    type id, destination type id) — DGL's own order is not verifiable here (third-party, absent); no model on the path
    depends on it beyond the summation order of the cross-relation mean."""
    dev = src.device
    node_type = node_type.to(dev).long()
    edge_type = edge_type.to(dev).long()
    T = len(ntypes)
    order = torch.argsort(node_type, stable=True)
    counts = torch.bincount(node_type, minlength=T)
    starts = torch.cumsum(counts, 0) - counts
    local = torch.empty(num_nodes, dtype=torch.int64, device=dev)
    local[order] = torch.arange(num_nodes, device=dev) - starts[node_type[order]]
    counts_h = counts.tolist()
    nn_ = OrderedDict((str(t), counts_h[i]) for i, t in enumerate(ntypes))
    st, dt = node_type[src], node_type[dst]
    key = (st * len(etypes) + edge_type) * T + dt
    present = torch.unique(key).tolist()
    edges, sims = OrderedDict(), {}
    for kk in present:
        m = (key == kk).nonzero(as_tuple=True)[0]
        s_id, rest = divmod(kk, len(etypes) * T)
        e_id, d_id = divmod(rest, T)
        r = (str(ntypes[s_id]), str(etypes[e_id]), str(ntypes[d_id]))
        edges[r] = (local[src[m]], local[dst[m]])
        if sim is not None:
            sims[r] = sim[m]
    g = HeteroGraph.from_coo(nn_, edges, sim=sims if sim is not None else None)
    off = 0
    for i, t in enumerate(ntypes):
        ids = order[off:off + counts_h[i]]
        off += counts_h[i]
        g.nodes[str(t)].data["_ID"] = ids
        if feat is not None:
            g.nodes[str(t)].data["feat"] = feat[ids]
    return g


def construct_graph(features: torch.Tensor, node_type, radius: int, n_node_type: int, pad: int = 8):
    """``GraphConstructor.construct_graph`` (graph_constructor.py:256-303) from (features, node types) on:
    returns ``(het_graph, homo_graph, node_type)`` like the reference.  ``features``: [N, F] fp32 on the GPU;
    ``node_type``: N ints in [0, n_node_type)."""
    n = features.shape[0]
    dev = features.device
    nbr, corr, _ = knn_pearson(features, radius, pad)
    keep = nbr.shape[1]
    a = torch.arange(n, device=dev).repeat_interleave(keep, output_size=n * keep)      # :263 np.repeat(range(N), radius-1)
    b = nbr.reshape(-1)
    sim = corr.reshape(-1)
    etype = (sim > 0).long()                                                            # :279  1 if corr > 0 else 0
    nt = torch.as_tensor(node_type, dtype=torch.int64, device=dev)
    het = to_heterogeneous(n, a, b, nt, etype, [str(t) for t in range(n_node_type)], EDGE_TYPE_NAMES, feat=features, sim=sim)
    homo = HeteroGraph.homogeneous(n, a, b, feat=features)
    return het, homo, node_type


# ------------------------------------------------------------------------------------------------
# Slide graphs of the two grid baselines from patch coordinates
# ------------------------------------------------------------------------------------------------
# GTNMIL (baselines/GTNMIL/feature_extractor/build_graphs.py:78-96): the reference fills a dense float64 n x n matrix in an O(n^2) double loop
# over file names - 1 where two patches are at most one grid step apart in x and in y.  H2MIL (baselines/H2MIL/code/github_pretreat.py:94-329):
# the three-level tree (thumbnail root, 5x patches, 10x patches) by dictionary look-ups on name strings.  Both are exact look-ups in small
# integer point sets; here they run for a whole batch at once, either through the kernels of csrc/grid_graph.hip (one hash table over all
# sets, count, prefix sum, write) or through the tensor formulation below (sorted packed keys + torch.searchsorted).  The two give the same
# tensors, element for element, in the order the reference's loops produce.
_KEY_X = 1 << 25                                   # key = (set << 50) | ((x + 1) << 25) | (y + 1): the probes at -1 and 2^24 are representable
_KEY_SET = 1 << 50
_NB8 = ((0, 1), (0, -1), (1, 0), (-1, 0), (1, 1), (-1, 1), (1, -1), (-1, -1))        # github_pretreat.py:147-170, in this order


def _use_kernels(kernels: Optional[bool], *tensors) -> bool:
    if kernels is None:
        return all(t.is_cuda for t in tensors)
    if kernels:
        N.require_cuda(*tensors)
    return bool(kernels)


def _coords(what: str, t: torch.Tensor, cols: int = 2) -> torch.Tensor:
    if t.dim() != 2 or t.shape[1] != cols or t.is_floating_point() or t.dtype == torch.bool:
        raise ValueError(f"{what} is an integer [n, {cols}] tensor, got {tuple(t.shape)} {t.dtype}")
    return t


def _sizes(what: str, sizes: Sequence[int], total: int):
    sizes = [int(c) for c in sizes]
    if not sizes or any(c < 0 for c in sizes) or sum(sizes) != total:
        raise ValueError(f"{what}: the sizes {sizes} do not add up to the {total} rows given")
    return sizes


def _ptr(sizes: Sequence[int]):
    ptr = [0]
    for c in sizes:
        ptr.append(ptr[-1] + c)
    return ptr


def _raise_flags(what: str, word: int) -> None:
    broken = [text for bit, text in ops.GRID_FLAGS if word & bit]
    if broken:
        raise ValueError(f"{what}: " + "; ".join(broken))


def _to_int32(t: torch.Tensor) -> torch.Tensor:
    """int32 for the kernels; a value int32 cannot hold becomes -1, which the range rule refuses like the original."""
    if t.dtype == torch.int32:
        return t.contiguous()
    lim = ops.GRID_COORD_LIMIT
    return torch.where((t >= 0) & (t < lim), t, torch.full_like(t, -1)).to(torch.int32).contiguous()


def _sorted_keys(coords: torch.Tensor, set_of: torch.Tensor):
    """(key per point, keys sorted, the point of every sorted key, flag word tensor) of the tensor formulation."""
    c = coords.to(torch.int64)
    bad = ((c < 0) | (c >= ops.GRID_COORD_LIMIT)).any()
    key = set_of * _KEY_SET + (c[:, 0] + 1) * _KEY_X + (c[:, 1] + 1)
    skey, order = torch.sort(key)
    rep = (skey[1:] == skey[:-1]).any() if key.numel() > 1 else torch.zeros((), dtype=torch.bool, device=key.device)
    return key, skey, order, bad.to(torch.int64) * N.WSI_GRID_BAD_COORD + rep.to(torch.int64) * N.WSI_GRID_REPEATED


def _lookup(skey: torch.Tensor, order: torch.Tensor, query: torch.Tensor) -> torch.Tensor:
    """The point stored under every query key, -1 for a miss."""
    if skey.numel() == 0:
        return torch.full_like(query, -1)
    pos = torch.searchsorted(skey, query).clamp_(max=skey.numel() - 1)
    return torch.where(skey[pos] == query, order[pos], torch.full_like(query, -1))


def _neighbours(key: torch.Tensor, skey: torch.Tensor, order: torch.Tensor) -> torch.Tensor:
    """[n, 8]: the point at each of the 8 offsets of _NB8, -1 where there is none."""
    delta = torch.tensor([dx * _KEY_X + dy for dx, dy in _NB8], dtype=torch.int64, device=key.device)
    return _lookup(skey, order, key[:, None] + delta[None, :])


def grid_adjacency(coords: torch.Tensor, sizes: Sequence[int], kernels: Optional[bool] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """The 8-neighbour grid adjacency of GTNMIL (build_graphs.py:78-96) for a packed batch: ``coords`` [N, 2] integer grid positions, the
    slides one after the other in the caller's node order (the reference: file order), ``sizes`` their row counts.  Returns ``(row, col)``
    int64: for every node i the entries (i, j), j != i of the same slide with |x_i - x_j| <= 1 and |y_i - y_j| <= 1; rows ascend and the
    columns of a row ascend - the order of the dense matrix's ``nonzero()``, so of ``gtn.from_dense`` - with global row numbers.  Every entry
    is 1.  ``ValueError``: a coordinate outside 0 <= c < 2^24, or one repeated within a slide (two files of a folder cannot share a name).
    ``kernels=None``: the HIP kernels for CUDA tensors, the tensor formulation for CPU tensors; ``False`` forces the tensor formulation,
    ``True`` on a CPU tensor raises."""
    coords = _coords("grid_adjacency: coords", coords)
    sizes = _sizes("grid_adjacency", sizes, coords.shape[0])
    dev = coords.device
    if len(sizes) > ops.GRID_MAX_SETS:
        raise ValueError(f"grid_adjacency: at most {ops.GRID_MAX_SETS} slides per call")
    if _use_kernels(kernels, coords):
        index = ops.grid_index(_to_int32(coords), torch.tensor(_ptr(sizes), dtype=torch.int32).to(dev))
        counts, _ = ops.grid_count(index, "adjacency")
        incl = torch.cumsum(counts, 0, dtype=torch.int64)
        row, col = ops.grid_write(index, "adjacency", counts, incl)
        total, f0, f1 = torch.cat([incl[-1:] if incl.numel() else incl.new_zeros(1), index.flags.to(torch.int64)]).tolist()      # the one read-back
        _raise_flags("grid_adjacency", f0 | f1)
        return row[:total], col[:total]
    set_of = torch.repeat_interleave(torch.arange(len(sizes)), torch.tensor(sizes, dtype=torch.int64)).to(dev)
    key, skey, order, flags = _sorted_keys(coords, set_of)
    _raise_flags("grid_adjacency", int(flags))
    hits = _neighbours(key, skey, order)
    big = torch.iinfo(torch.int64).max
    hits = torch.sort(torch.where(hits >= 0, hits, torch.full_like(hits, big)), dim=1).values
    keep = hits != big
    row = torch.arange(coords.shape[0], device=dev)[:, None].expand(-1, 8)
    return row[keep], hits[keep]


def slide_trees(coords1: torch.Tensor, cover: torch.Tensor, coords2: torch.Tensor, n1: Sequence[int], n2: Sequence[int],
                kernels: Optional[bool] = None):
    """The three-level slide trees of H2MIL (github_pretreat.py:94-329) for a whole batch.  ``coords1`` [sum n1, 2]: the fields (i, j) of every 5x
    patch name a-b-c-d-i-j, ``cover`` [sum n1, 4]: its fields (a, b, c, d), ``coords2`` [sum n2, 2]: every 10x patch name x-y; each packed
    slide after slide in the reference's order, ``n1`` / ``n2`` the slides' counts.  A slide's rows are its root, its level-1 nodes, its level-2
    nodes; all rows returned are GLOBAL rows of the batch (what ``h2mil.TreeBatch`` holds).  Returns

    * ``edge_index`` int64 [2, E]: per slide section A (:106-133: per level-1 node r, r -> root, root -> r, then for the children (a,c), (b,c),
      (a,d), (b,d) that exist r -> child, child -> r; a == b or c == d emits a child twice), section B (:142-170: per level-1 node, self ->
      neighbour for the 8 offsets in the reference's order) and section C (:173-202: the same over level-2 nodes);
    * ``node_type`` int64 [N]: 0 / 1 / 2;
    * ``node_tree`` int64 [N] (:228-254): -1 for a root, the root's row for a level-1 node, for a level-2 node the row of the LAST level-1 node in
      order that covers it;
    * ``x_y_index`` float64 [N, 2] (:257-315): (0, 0) for a root, else (x / max_x, y / max_y) over the node's slide and level - one IEEE double
      division per value; a maximum of 0 gives inf / nan as numpy does.

    ``ValueError``: a slide without level-1 or without level-2 nodes (the reference drops it, :278-296), a coordinate outside 0 <= c < 2^24, an
    (i, j) repeated within a level of a slide, a level-2 node that no level-1 node covers.  ``kernels`` as for ``grid_adjacency``."""
    coords1, cover, coords2 = _coords("slide_trees: coords1", coords1), _coords("slide_trees: cover", cover, 4), _coords("slide_trees: coords2", coords2)
    if cover.shape[0] != coords1.shape[0]:
        raise ValueError("slide_trees: one row of cover per row of coords1")
    n1, n2 = _sizes("slide_trees: n1", n1, coords1.shape[0]), _sizes("slide_trees: n2", n2, coords2.shape[0])
    B = len(n1)
    if len(n2) != B:
        raise ValueError("slide_trees: n1 and n2 have one entry per slide")
    if any(c == 0 for c in n1) or any(c == 0 for c in n2):
        raise ValueError("slide_trees: a slide without level-1 nodes or without level-2 nodes (an empty level: the reference drops such a slide)")
    if 2 * B > ops.GRID_MAX_SETS:
        raise ValueError(f"slide_trees: at most {ops.GRID_MAX_SETS // 2} slides per call")
    dev = coords1.device
    N1, N2 = coords1.shape[0], coords2.shape[0]
    ptr1, ptr2 = _ptr(n1), _ptr(n2)
    if _use_kernels(kernels, coords1, cover, coords2):
        pts = torch.cat([_to_int32(coords1), _to_int32(coords2)])
        set_ptr = torch.tensor(ptr1 + [N1 + p for p in ptr2[1:]], dtype=torch.int32).to(dev)
        cov = _to_int32(cover)
        index = ops.grid_index(pts, set_ptr)
        counts, parent = ops.grid_count(index, "tree", N1, cov)
        incl = torch.cumsum(counts, 0, dtype=torch.int64)
        edges, node_type, node_tree, xy = ops.grid_write(index, "tree", counts, incl, N1, cov, parent)
        total, f0, f1 = torch.cat([incl[-1:], index.flags.to(torch.int64)]).tolist()                       # the one read-back
        _raise_flags("slide_trees", f0 | f1)
        return edges[:, :total], node_type, node_tree, xy
    # ---- the tensor formulation
    i64 = lambda v: torch.tensor(v, dtype=torch.int64)
    slide1 = torch.repeat_interleave(torch.arange(B), i64(n1)).to(dev)
    slide2 = torch.repeat_interleave(torch.arange(B), i64(n2)).to(dev)
    key1, skey1, order1, flag1 = _sorted_keys(coords1, slide1)
    key2, skey2, order2, flag2 = _sorted_keys(coords2, slide2)
    _raise_flags("slide_trees", int(flag1 | flag2))
    starts = i64([ptr1[b] + ptr2[b] + b for b in range(B)]).to(dev)             # the root's row
    row1 = torch.arange(N1, device=dev) + (starts + 1 - i64(ptr1[:-1]).to(dev))[slide1]
    row2 = torch.arange(N2, device=dev) + (starts + 1 + i64(n1).to(dev) - i64(ptr2[:-1]).to(dev))[slide2]
    root1 = starts[slide1]
    cv = cover.to(torch.int64)
    cok = (cv >= 0) & (cv < ops.GRID_COORD_LIMIT)
    kid = torch.stack([_lookup(skey2, order2, torch.where(cok[:, ax] & cok[:, ay], slide1 * _KEY_SET + (cv[:, ax] + 1) * _KEY_X + cv[:, ay] + 1,
                                                           torch.full_like(slide1, -1)))
                       for ax, ay in ((0, 2), (1, 2), (0, 3), (1, 3))], 1)                                   # [N1, 4] level-2 points or -1
    has = kid >= 0
    kid_row = row2[kid.clamp(min=0)]
    me4 = row1[:, None].expand(-1, 4)
    # section A as [N1, 10] slots: r -> root, root -> r, then (r -> child, child -> r) x 4
    a_src = torch.cat([row1[:, None], root1[:, None], torch.stack([me4, kid_row], 2).reshape(N1, 8)], 1)
    a_dst = torch.cat([root1[:, None], row1[:, None], torch.stack([kid_row, me4], 2).reshape(N1, 8)], 1)
    a_keep = torch.cat([torch.ones((N1, 2), dtype=torch.bool, device=dev), has.repeat_interleave(2, dim=1)], 1)
    nb1, nb2 = _neighbours(key1, skey1, order1), _neighbours(key2, skey2, order2)
    parts = ((a_src, a_dst, a_keep, slide1 * 3),
             (row1[:, None].expand(-1, 8), row1[nb1.clamp(min=0)], nb1 >= 0, slide1 * 3 + 1),
             (row2[:, None].expand(-1, 8), row2[nb2.clamp(min=0)], nb2 >= 0, slide2 * 3 + 2))
    src = torch.cat([s[k] for s, _, k, _ in parts])
    dst = torch.cat([d[k] for _, d, k, _ in parts])
    group = torch.cat([g[:, None].expand(-1, k.shape[1])[k] for _, _, k, g in parts])
    by_slide = torch.sort(group, stable=True).indices                           # [slide][section], the order within a section kept
    edge_index = torch.stack([src[by_slide], dst[by_slide]])
    parent = torch.full((N2,), -1, dtype=torch.int64, device=dev)
    parent.scatter_reduce_(0, kid[has], me4[has], reduce="amax", include_self=True)                  # the last in order = the largest row
    uncovered = (parent < 0).any().to(torch.int64) * N.WSI_GRID_UNCOVERED
    _raise_flags("slide_trees", int(uncovered))
    N_ = B + N1 + N2
    node_type = torch.zeros(N_, dtype=torch.int64, device=dev)
    node_type[row1], node_type[row2] = 1, 2
    node_tree = torch.full((N_,), -1, dtype=torch.int64, device=dev)
    node_tree[row1], node_tree[row2] = root1, parent
    xy = torch.zeros((N_, 2), dtype=torch.float64, device=dev)
    for coords, slide, rows in ((coords1, slide1, row1), (coords2, slide2, row2)):
        c = coords.to(torch.int64)
        top = torch.full((B, 2), -1, dtype=torch.int64, device=dev).scatter_reduce_(0, slide[:, None].expand(-1, 2), c, reduce="amax")
        xy[rows] = c.to(torch.float64) / top[slide].to(torch.float64)
    return edge_index, node_type, node_tree, xy
