"""Explanations scored against annotations: the part of the reference's ``graph_explain`` mode behind the explainer
(``evaluator/explain_graphs.py::ExplainGraph``), without shapely, sklearn, openslide or cv2.

* ``read_annotations`` / ``AnnotationBatch``: the ASAP (Camelyon16) XML rings of :87-101, packed for several slides.
* ``patch_centres`` / ``tiles_from_names`` / ``patch_order``: the integer arithmetic of :70-79 and :104-109, and heterogeneous masks put
  back into patch order.
* ``patch_labels``: which patch centres lie inside the annotation (:103-117, shapely's ``Polygon.contains``).
* ``score``: the per-slide localisation AUROC and its NaN-skipping mean (:179-184, sklearn's ``roc_curve`` + ``auc``).
* ``heat_image``: the filled heat map (:136-141, ``cv2.rectangle`` over the Wistia colours).
* ``explain_and_score``: the body of ``ExplainGraph.eval`` (:151-184) over a list of slides.

Every function takes ``kernels=None``: the HIP kernels of ``csrc/localization.hip`` for CUDA tensors, the tensor formulation below for CPU
tensors; ``False`` forces the tensor formulation on any device, ``True`` on a CPU tensor raises.  The two give the same bits.  Not built:
polygon outlines (``cv2.polylines``), reading slides or thumbnails, writing image files.
"""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence, Tuple, Union
from xml.dom import minidom

import torch

from . import _native as N
from . import ops

__all__ = ["Annotation", "AnnotationBatch", "LocalizationScore", "WISTIA", "read_annotations", "patch_centres", "tiles_from_names",
           "patch_order", "patch_labels", "score", "heat_image", "explain_and_score"]


def _use_kernels(kernels: Optional[bool], *tensors) -> bool:
    if kernels is None:
        return all(t.is_cuda for t in tensors)
    if kernels:
        N.require_cuda(*tensors)
    return bool(kernels)


# ------------------------------------------------------------------------------------------------
# Annotations and patch centres (host, small)
# ------------------------------------------------------------------------------------------------
class Annotation:
    """The rings of one slide: ``vertices`` fp64 [V, 2] = (X, Y) and ``ring_ptr`` int64 [P + 1]; ring p = the vertices
    [ring_ptr[p], ring_ptr[p + 1]), closed from its last vertex to its first.  A ring with fewer than 3 vertices is kept and contains nothing."""

    def __init__(self, vertices: torch.Tensor, ring_ptr: torch.Tensor):
        self.vertices = torch.as_tensor(vertices, dtype=torch.float64).reshape(-1, 2).cpu()
        self.ring_ptr = torch.as_tensor(ring_ptr, dtype=torch.int64).reshape(-1).cpu()
        ptr = self.ring_ptr.tolist()
        if not ptr or ptr[0] != 0 or ptr[-1] != self.vertices.shape[0] or any(b < a for a, b in zip(ptr, ptr[1:])):
            raise ValueError(f"Annotation: ring_ptr {ptr} does not partition {self.vertices.shape[0]} vertices")

    @classmethod
    def from_rings(cls, rings: Sequence) -> "Annotation":
        """From a list of rings, each a list of (x, y)."""
        flat = [tuple(float(c) for c in v) for r in rings for v in r]
        ptr = [0]
        for r in rings:
            ptr.append(ptr[-1] + len(r))
        return cls(torch.tensor(flat, dtype=torch.float64).reshape(-1, 2), torch.tensor(ptr, dtype=torch.int64))

    @property
    def num_rings(self) -> int:
        return self.ring_ptr.shape[0] - 1


def read_annotations(xml_path) -> Annotation:
    """The rings of an ASAP / Camelyon16 annotation file as explain_graphs.py:87-101 reads them: every ``Coordinates`` element is one ring,
    its vertices the (X, Y) attributes of its children that have attributes, as floats, in document order (text nodes between the children
    are skipped)."""
    rings = []
    for p in minidom.parse(str(xml_path)).getElementsByTagName("Coordinates"):
        rings.append([(float(c.attributes["X"].value), float(c.attributes["Y"].value)) for c in p.childNodes if c.attributes])
    return Annotation.from_rings(rings)


class AnnotationBatch:
    """The annotations of B slides packed: ``vertices`` fp64 [V, 2], ``ring_ptr`` int64 [R + 1], ``slide_ring_ptr`` int64 [B + 1],
    ``ring_box`` fp64 [R, 4] = (min x, min y, max x, max y; an empty ring: +inf, +inf, -inf, -inf), and the chunk table the kernels walk:
    every ring cut into runs of at most ``chunk`` edges - ``chunks`` int32 [K, 4] = (ring, first edge, edges, slide), ``slide_chunk_ptr``
    int32 [B + 1].  Every size is known on the host (``chunks_per_slide``, ``num_rings`` ...), so nothing downstream reads anything back.
    ``.to(device)`` moves the tensors."""

    _TENSORS = ("vertices", "ring_ptr", "slide_ring_ptr", "ring_box", "chunks", "slide_chunk_ptr")

    def __init__(self, annotations: Sequence[Annotation], chunk: int = ops.LOC_CHUNK):
        if not 1 <= int(chunk) <= ops.LOC_CHUNK_MAX:
            raise ValueError(f"AnnotationBatch: chunk {chunk} outside 1 .. {ops.LOC_CHUNK_MAX}")
        self.chunk = int(chunk)
        annotations = list(annotations)
        ring_ptr, slide_ring_ptr, chunks, slide_chunk_ptr, boxes = [0], [0], [], [0], []
        inf = float("inf")
        for s, a in enumerate(annotations):
            ptr = a.ring_ptr.tolist()
            for lo, hi in zip(ptr, ptr[1:]):
                ring = len(ring_ptr) - 1
                ring_ptr.append(ring_ptr[-1] + hi - lo)
                if hi > lo:
                    v = a.vertices[lo:hi]
                    boxes.append(v.min(0).values.tolist() + v.max(0).values.tolist())
                else:
                    boxes.append([inf, inf, -inf, -inf])
                for e0 in range(0, hi - lo, self.chunk):              # a ring of V vertices has V edges (the closing one included)
                    chunks += [ring, e0, min(self.chunk, hi - lo - e0), s]
            slide_ring_ptr.append(len(ring_ptr) - 1)
            slide_chunk_ptr.append(len(chunks) // 4)
        self.vertices = torch.cat([a.vertices for a in annotations]) if annotations else torch.zeros((0, 2), dtype=torch.float64)
        self.ring_ptr = torch.tensor(ring_ptr, dtype=torch.int64)
        self.slide_ring_ptr = torch.tensor(slide_ring_ptr, dtype=torch.int64)
        self.ring_box = torch.tensor(boxes, dtype=torch.float64).reshape(-1, 4)
        self.chunks = torch.tensor(chunks, dtype=torch.int32).reshape(len(chunks) // 4, 4)
        self.slide_chunk_ptr = torch.tensor(slide_chunk_ptr, dtype=torch.int32)
        self.num_slides = len(annotations)
        self.rings_per_slide = [b - a for a, b in zip(slide_ring_ptr, slide_ring_ptr[1:])]
        self.chunks_per_slide = [b - a for a, b in zip(slide_chunk_ptr, slide_chunk_ptr[1:])]
        self._ring_ptr_host, self._slide_ring_ptr_host = ring_ptr, slide_ring_ptr

    @property
    def device(self) -> torch.device:
        return self.vertices.device

    @property
    def num_rings(self) -> int:
        return len(self._ring_ptr_host) - 1

    def to(self, device) -> "AnnotationBatch":
        out = object.__new__(AnnotationBatch)
        out.__dict__.update(self.__dict__)
        for name in self._TENSORS:
            setattr(out, name, getattr(self, name).to(device))
        return out


def tiles_from_names(names: Sequence[str]) -> torch.Tensor:
    """int64 [N, 2] tile indices (x, y) from patch file names ``"{x}_{y}.jpeg"`` (explain_graphs.py:75-76: the last path part without its
    five-character suffix, split at ``_``)."""
    out = []
    for name in names:
        x, y = str(name).replace("\\", "/").rsplit("/", 1)[-1][:-5].split("_")
        out.append((int(x), int(y)))
    return torch.tensor(out, dtype=torch.int64).reshape(-1, 2)


def patch_centres(tile_xy: torch.Tensor, patch_size: int, level: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """``(grid, centres)``, both int64 [N, 2], of the tiles ``tile_xy`` (int64 [N, 2] tile indices), in the reference's integer arithmetic:

    * grid coordinate (explain_graphs.py:70-77): ``c = dz._z_from_t(t) // 2 ** (level - 1)``.  ``dz`` is
      ``DeepZoomGenerator(wsi, patch_size, overlap=0)`` (:174), whose ``_z_from_t(t)`` is ``tile_size * t`` (openslide is not needed to say
      so), hence ``c = (t * patch_size) // 2 ** (level - 1)``.  This is where ``heat_image`` paints the patch.
    * centre in level-0 pixels (:104-109): ``c * 2 ** level + patch_size * 2 // 2`` - the point tested against the annotation."""
    if tile_xy.dim() != 2 or tile_xy.shape[1] != 2 or tile_xy.is_floating_point() or tile_xy.dtype == torch.bool:
        raise ValueError(f"patch_centres: tile_xy is an integer [N, 2] tensor, got {tuple(tile_xy.shape)} {tile_xy.dtype}")
    if int(level) < 1 or int(patch_size) < 1:
        raise ValueError("patch_centres: level >= 1 (the base level is 1) and patch_size >= 1")
    grid = torch.div(tile_xy.to(torch.int64) * int(patch_size), 2 ** (int(level) - 1), rounding_mode="floor")
    return grid, grid * 2 ** int(level) + int(patch_size) * 2 // 2


def patch_order(graph, node_mask):
    """A per-node-type mask dict (``HetGemExplainer.explain_node()``) scattered back to patch order through ``nodes[t].data['_ID']``
    (``construct.to_heterogeneous`` keeps it): ``out[_ID[t][i]] = node_mask[t][i]``.  A flat mask passes through unchanged."""
    if not isinstance(node_mask, dict):
        return node_mask
    parts = {t: torch.as_tensor(m) for t, m in node_mask.items()}
    total = sum(int(m.shape[0]) for m in parts.values())
    first = next(iter(parts.values()))
    out = torch.zeros((total,) + tuple(first.shape[1:]), dtype=first.dtype, device=first.device)
    for t, m in parts.items():
        if "_ID" not in graph.nodes[t].data:
            raise ValueError(f"patch_order: node type {t!r} has no '_ID' field to put its mask back into patch order")
        ids = graph.nodes[t].data["_ID"].to(device=m.device, dtype=torch.int64)
        if ids.shape[0] != m.shape[0]:
            raise ValueError(f"patch_order: {m.shape[0]} mask values for the {ids.shape[0]} nodes of type {t!r}")
        out[ids] = m
    return out


# ------------------------------------------------------------------------------------------------
# Patch labels
# ------------------------------------------------------------------------------------------------
def _sizes(what: str, sizes: Sequence[int], total: int) -> List[int]:
    sizes = [int(c) for c in sizes]
    if any(c < 0 for c in sizes) or sum(sizes) != total:
        raise ValueError(f"{what}: the sizes {sizes} do not add up to the {total} rows given")
    return sizes


def _labels_tensor(centres: torch.Tensor, sizes: List[int], ann: AnnotationBatch, block: int = 1 << 22) -> torch.Tensor:
    """The tensor formulation: per slide, blocks of (centres x edges) comparisons summed per ring."""
    dev = centres.device
    out = torch.zeros(centres.shape[0], dtype=torch.int32, device=dev)
    ring_ptr, slide_ring = ann._ring_ptr_host, ann._slide_ring_ptr_host
    row = 0
    for s, n in enumerate(sizes):
        r0, r1 = slide_ring[s], slide_ring[s + 1]
        v0, v1 = ring_ptr[r0], ring_ptr[r1]
        if n and v1 > v0:
            lens = [ring_ptr[r + 1] - ring_ptr[r] for r in range(r0, r1)]
            nxt, ring_of = [], []                                   # the vertex an edge ends on, the slide-local ring of an edge
            for j, ln in enumerate(lens):
                base = ring_ptr[r0 + j] - v0
                nxt += [base + (i + 1) % ln for i in range(ln)]
                ring_of += [j] * ln
            a = ann.vertices[v0:v1]
            b = a[torch.tensor(nxt, dtype=torch.int64).to(dev)]
            ring_of = torch.tensor(ring_of, dtype=torch.int64).to(dev)
            x, y = centres[row:row + n, 0:1], centres[row:row + n, 1:2]
            cross = torch.zeros((n, r1 - r0), dtype=torch.int32, device=dev)
            edge = torch.zeros((n, r1 - r0), dtype=torch.int32, device=dev)
            step = max(1, block // n)
            for e in range(0, v1 - v0, step):
                x0, y0, x1, y1 = a[e:e + step, 0], a[e:e + step, 1], b[e:e + step, 0], b[e:e + step, 1]
                o = (x1 - x0) * (y - y0) - (x - x0) * (y1 - y0)
                hit = ((y0 > y) != (y1 > y)) & ((o > 0) == (y1 > y0))
                on = (o == 0) & (x >= torch.minimum(x0, x1)) & (x <= torch.maximum(x0, x1)) & (y >= torch.minimum(y0, y1)) & (y <= torch.maximum(y0, y1))
                cross.index_add_(1, ring_of[e:e + step], hit.to(torch.int32))
                edge.index_add_(1, ring_of[e:e + step], on.to(torch.int32))
            box = ann.ring_box[r0:r1]
            inbox = (x >= box[:, 0]) & (y >= box[:, 1]) & (x <= box[:, 2]) & (y <= box[:, 3])
            out[row:row + n] = (((cross & 1) == 1) & (edge == 0) & inbox).any(1).to(torch.int32)
        row += n
    return out


def patch_labels(centres: torch.Tensor, sizes: Sequence[int], annotations: Union[AnnotationBatch, Sequence[Annotation]],
                 kernels: Optional[bool] = None, max_scratch_words: int = ops.LOC_MAX_SCRATCH_WORDS) -> torch.Tensor:
    """int32 [N]: the ground-truth label of every patch of a packed batch (explain_graphs.py:103-117).  ``centres`` [N, 2] = (x, y), the
    slides one after the other with ``sizes`` rows each; ``annotations`` an ``AnnotationBatch`` of as many slides (on the centres' device),
    or the list of ``Annotation`` to pack.

    The rule: a patch is labelled 1 iff its centre lies STRICTLY inside at least one ring of its own slide.  Inside a ring is the even-odd
    (crossing-number) rule; a point on a ring's boundary - an edge or a vertex - is not inside that ring (shapely's ``contains``).  Rings are
    independent: Camelyon's exclusion groups are ignored, as the reference ignores them, and a ring nested in a ring still labels 1.  A
    self-intersecting ring follows even-odd (shapely leaves that case undefined).  A ring with fewer than 3 vertices contains nothing.

    All arithmetic is fp64 without a division.  For an edge (x0, y0) -> (x1, y1) and a centre (x, y):
    ``o = (x1 - x0) * (y - y0) - (x - x0) * (y1 - y0)``; the edge is crossed iff ``(y0 > y) != (y1 > y)`` and ``(o > 0) == (y1 > y0)``; the
    centre is on the edge iff ``o == 0`` inside the edge's closed bounding box.  A centre outside a ring's closed bounding box is outside the
    ring.  For coordinates on a quarter-integer lattice below 2^20 every difference and product is exact, so the kernels, the tensor
    formulation and a Python loop agree bit for bit; for general XML decimals the result can differ from another fp64 evaluation only for
    centres within rounding of an edge.

    A slide without rings labels everything 0; a slide without centres costs nothing.  ``ValueError`` when the kernels' (chunk, centre)
    scratch would exceed ``max_scratch_words`` (1 GiB by default): label fewer slides per call.  No read-back."""
    if centres.dim() != 2 or centres.shape[1] != 2 or centres.dtype == torch.bool:
        raise ValueError(f"patch_labels: centres is an [N, 2] tensor, got {tuple(centres.shape)} {centres.dtype}")
    sizes = _sizes("patch_labels", sizes, centres.shape[0])
    ann = annotations if isinstance(annotations, AnnotationBatch) else AnnotationBatch(annotations).to(centres.device)
    if ann.num_slides != len(sizes):
        raise ValueError(f"patch_labels: {len(sizes)} slides of centres against {ann.num_slides} annotations")
    if ann.device != centres.device:
        raise ValueError(f"patch_labels: the centres are on {centres.device}, the annotations on {ann.device} (AnnotationBatch.to)")
    centres = centres.to(torch.float64)
    if _use_kernels(kernels, centres):
        return ops.loc_labels(centres, sizes, ann.vertices, ann.ring_ptr, ann.ring_box, ann.chunks, ann.slide_chunk_ptr, ann.chunks_per_slide,
                              ann.chunk, max_scratch_words)
    return _labels_tensor(centres, sizes, ann)


# ------------------------------------------------------------------------------------------------
# The localisation AUROC
# ------------------------------------------------------------------------------------------------
class LocalizationScore:
    """Per slide (and score column): ``auc`` fp64 = (2 gt + eq) / (2 P N), ``pos`` = P, ``neg`` = N, ``gt`` / ``eq`` = the (positive,
    negative) pairs with s_pos > / == s_neg (int64), ``flags`` int32 (``WSI_LOC_NONFINITE``: a score of the slide is not finite; its auc
    is NaN), all [B] for [N] scores and [B, C] for [N, C]; ``mean`` = the NaN-skipping mean of ``auc`` over the slides (explain_graphs.py:184;
    a scalar, or [C]), NaN if every slide is NaN.  Everything stays on the device it was computed on; ``.cpu()`` is the one read-back."""

    _FIELDS = ("auc", "pos", "neg", "gt", "eq", "flags", "mean")

    def __init__(self, auc, pos, neg, gt, eq, flags, mean):
        self.auc, self.pos, self.neg, self.gt, self.eq, self.flags, self.mean = auc, pos, neg, gt, eq, flags, mean

    def cpu(self) -> "LocalizationScore":
        if not self.auc.is_cuda:
            return self
        words = torch.cat([self.auc.reshape(-1).view(torch.int64), self.mean.reshape(-1).view(torch.int64), self.pos.reshape(-1), self.neg.reshape(-1),
                           self.gt.reshape(-1), self.eq.reshape(-1), self.flags.reshape(-1).to(torch.int64)]).cpu()       # ONE copy
        n, m, at, out = self.auc.numel(), self.mean.numel(), 0, {}
        for name, count in (("auc", n), ("mean", m), ("pos", n), ("neg", n), ("gt", n), ("eq", n), ("flags", n)):
            out[name] = words[at:at + count]
            at += count
        shape = self.auc.shape
        return LocalizationScore(out["auc"].view(torch.float64).reshape(shape), out["pos"].reshape(shape), out["neg"].reshape(shape),
                                 out["gt"].reshape(shape), out["eq"].reshape(shape), out["flags"].to(torch.int32).reshape(shape),
                                 out["mean"].view(torch.float64).reshape(self.mean.shape))

    def __repr__(self) -> str:
        return f"LocalizationScore(slides={self.auc.shape[0]}, device={self.auc.device})"


def _block_sum(a: torch.Tensor) -> torch.Tensor:
    """Sum over dim 0 of n <= 128 rows in the order of numpy's pairwise summation: eight running sums, then the rest."""
    n = a.shape[0]
    if n < 8:
        res = torch.zeros_like(a[0]) if n else torch.zeros(a.shape[1:], dtype=a.dtype, device=a.device)
        for i in range(n):
            res = res + a[i]
        return res
    r = a[0:8].clone()
    i = 8
    while i < n - n % 8:
        r = r + a[i:i + 8]
        i += 8
    res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]))
    for j in range(i, n):
        res = res + a[j]
    return res


def _pairwise_sum(a: torch.Tensor) -> torch.Tensor:
    n = a.shape[0]
    if n <= 128:
        return _block_sum(a)
    n2 = n // 2
    n2 -= n2 % 8
    return _pairwise_sum(a[:n2]) + _pairwise_sum(a[n2:])


def _nan_mean(auc: torch.Tensor) -> torch.Tensor:
    """numpy.nanmean over dim 0 of every column, to the last bit: NaN -> 0, numpy's pairwise order, one division by the count."""
    ok = auc == auc
    total = _pairwise_sum(torch.where(ok, auc, torch.zeros_like(auc)))
    cnt = ok.sum(0)
    return torch.where(cnt > 0, total / cnt.to(torch.float64), torch.full_like(total, float("nan")))


def _score_tensor(scores: torch.Tensor, labels: torch.Tensor, sizes: List[int], block: int = 1 << 22):
    dev, C = scores.device, scores.shape[1]
    counts = torch.zeros((len(sizes), C, 4), dtype=torch.int64, device=dev)
    flags = torch.zeros((len(sizes), C), dtype=torch.int32, device=dev)
    row = 0
    for s, n in enumerate(sizes):
        if n:
            sc, lab = scores[row:row + n], labels[row:row + n]
            pos, neg = lab != 0, lab == 0
            counts[s, :, 0], counts[s, :, 1] = pos.sum(), neg.sum()
            flags[s] = (~torch.isfinite(sc)).any(0).to(torch.int32) * N.WSI_LOC_NONFINITE
            step = max(1, block // n)
            for c in range(C):
                col = sc[:, c]
                for i in range(0, n, step):
                    a, m = col[i:i + step, None], (pos[i:i + step, None] & neg[None, :])
                    counts[s, c, 2] += ((a > col[None, :]) & m).sum()
                    counts[s, c, 3] += ((a == col[None, :]) & m).sum()
        row += n
    P, Nn, gt, eq = counts.unbind(-1)
    auc = (2 * gt + eq).to(torch.float64) / (2 * P * Nn).to(torch.float64)
    auc = torch.where((P > 0) & (Nn > 0) & (flags == 0), auc, torch.full_like(auc, float("nan")))
    return auc, counts, flags, _nan_mean(auc)


def score(node_scores: torch.Tensor, labels: torch.Tensor, sizes: Sequence[int], kernels: Optional[bool] = None) -> LocalizationScore:
    """The localisation AUROC of every slide of a packed batch (explain_graphs.py:179-184).  ``node_scores`` fp32 [N] or [N, C] (one AUC per
    column: GraphCAM's ``node_heat`` has a column per class), ``labels`` int32 [N] (``patch_labels``), ``sizes`` the slides' row counts.

    Per slide and column the exact Mann-Whitney statistic by pair counting: P / N positives / negatives, gt / eq the (positive, negative)
    pairs with s_pos > s_neg / s_pos == s_neg, all int64, and ``auc = (2 gt + eq) / (2 P N)`` as one fp64 division - the trapezoid under
    sklearn's ``roc_curve`` points is this tie-aware statistic, up to the rounding of its float sums (about n 2^-53).  P == 0 or N == 0 gives
    NaN, as ``roc_curve`` + ``auc`` do for a one-class slide.  A score that is not finite (``GemExplainer`` returns 0 / 0 for a constant
    mask) flags its slide, whose AUC is NaN; the other slides are untouched.  ``mean`` is ``numpy.nanmean`` over the slides.  No read-back:
    ``LocalizationScore.cpu()`` is the one."""
    if node_scores.dim() not in (1, 2) or node_scores.dtype != torch.float32:
        raise ValueError(f"score: node_scores is an fp32 [N] or [N, C] tensor, got {tuple(node_scores.shape)} {node_scores.dtype}")
    if labels.dtype != torch.int32 or labels.shape != node_scores.shape[:1]:
        raise ValueError(f"score: labels is an int32 [{node_scores.shape[0]}] tensor, got {tuple(labels.shape)} {labels.dtype}")
    if labels.device != node_scores.device:
        raise ValueError("score: node_scores and labels are on different devices")
    sizes = _sizes("score", sizes, node_scores.shape[0])
    flat = node_scores.dim() == 1
    sc = node_scores.reshape(node_scores.shape[0], -1)
    if sc.shape[1] < 1 or sc.shape[1] > N.WSI_LOC_MAX_COLUMNS:
        raise ValueError(f"score: 1 .. {N.WSI_LOC_MAX_COLUMNS} score columns")
    if _use_kernels(kernels, sc, labels):
        auc, counts, flags, mean = ops.loc_score(sc, labels, sizes)
    else:
        auc, counts, flags, mean = _score_tensor(sc, labels, sizes)
    pick = (lambda t: t[:, 0]) if flat else (lambda t: t)
    P, Nn, gt, eq = (pick(t) for t in counts.unbind(-1))
    return LocalizationScore(pick(auc), P, Nn, gt, eq, pick(flags), mean[0] if flat else mean)


# ------------------------------------------------------------------------------------------------
# The heat map
# ------------------------------------------------------------------------------------------------
def _wistia() -> torch.Tensor:
    """matplotlib's 'Wistia' as a uint8 [256, 3] table: five stops at 0, 1/4, 1/2, 3/4, 1, linearly interpolated at i / 255 the way
    ``LinearSegmentedColormap`` fills its 256-entry table, then rint(255 * value)."""
    stops = ((228, 255, 122), (255, 232, 26), (255, 189, 0), (255, 160, 0), (252, 127, 0))
    x = [255 * k / 4 for k in range(5)]
    rows = []
    for i in range(256):
        if i == 0 or i == 255:
            rows.append(stops[0] if i == 0 else stops[4])
            continue
        k = next(j for j in range(1, 5) if x[j] >= i)                # numpy.searchsorted(x, i), side='left'
        d = (i - x[k - 1]) / (x[k] - x[k - 1])
        rows.append(tuple(int(round(255 * (d * (stops[k][c] / 255 - stops[k - 1][c] / 255) + stops[k - 1][c] / 255))) for c in range(3)))
    return torch.tensor(rows, dtype=torch.uint8)


WISTIA = _wistia()


def _owner_tensor(grid_xy: torch.Tensor, patch: int, height: int, width: int) -> torch.Tensor:
    dev, n, side = grid_xy.device, grid_xy.shape[0], patch + 1
    owner = torch.full((height * width,), -1, dtype=torch.int64, device=dev)
    if n and height and width:
        off = torch.arange(side * side, device=dev)
        x = grid_xy[:, 0:1].to(torch.int64) + off % side
        y = grid_xy[:, 1:2].to(torch.int64) + off // side
        ok = (x >= 0) & (x < width) & (y >= 0) & (y < height)
        who = torch.arange(n, device=dev)[:, None].expand(-1, side * side)
        owner.scatter_reduce_(0, (y * width + x)[ok], who[ok], "amax", include_self=True)
    return owner.reshape(height, width).to(torch.int32)


def heat_image(grid_xy: torch.Tensor, values: torch.Tensor, height: int, width: int, patch: int, lut: torch.Tensor = WISTIA,
               base: Optional[torch.Tensor] = None, kernels: Optional[bool] = None) -> torch.Tensor:
    """uint8 [height, width, 3]: the fill of explain_graphs.py:136-141 without openslide or cv2.  Patch i at ``grid_xy[i]`` = (x, y)
    (``patch_centres``' grid coordinate) covers the pixels x .. x + patch, y .. y + patch INCLUSIVE - (patch + 1)^2 pixels, what
    ``cv2.rectangle(..., FILLED)`` paints between those corners - clipped to the image; where patches overlap the highest index wins
    (later draws overwrite).  Colour: ``lut[index(v)]``, ``index(v) = min(int(v * 256), 255)`` for v clamped to [0, 1] (``Normalize(0, 1)``
    and the colormap's own clipping); a NaN value paints black.  Pixels no patch covers keep ``base`` (uint8 [height, width, 3]) or are
    white.  ``lut`` uint8 [256, 3] (default: matplotlib's Wistia)."""
    if grid_xy.dim() != 2 or grid_xy.shape[1] != 2 or grid_xy.is_floating_point() or grid_xy.dtype == torch.bool:
        raise ValueError(f"heat_image: grid_xy is an integer [n, 2] tensor, got {tuple(grid_xy.shape)} {grid_xy.dtype}")
    if values.shape != grid_xy.shape[:1] or not values.is_floating_point() or values.device != grid_xy.device:
        raise ValueError(f"heat_image: values is a floating [{grid_xy.shape[0]}] tensor on the device of grid_xy")
    height, width, patch = int(height), int(width), int(patch)
    if height < 0 or width < 0 or height * width >= 1 << 31 or not 0 <= patch <= N.WSI_LOC_MAX_PATCH:
        raise ValueError(f"heat_image: an image below 2^31 pixels and 0 <= patch <= {N.WSI_LOC_MAX_PATCH}")
    if lut.shape != (256, 3) or lut.dtype != torch.uint8:
        raise ValueError("heat_image: lut is a uint8 [256, 3] table")
    dev = grid_xy.device
    if base is not None and (base.shape != (height, width, 3) or base.dtype != torch.uint8):
        raise ValueError(f"heat_image: base is a uint8 [{height}, {width}, 3] image")
    if _use_kernels(kernels, grid_xy, values):
        lim = 1 << 30
        owner = ops.loc_owner(grid_xy.clamp(-lim, lim).to(torch.int32), patch, height, width)
    else:
        owner = _owner_tensor(grid_xy, patch, height, width)
    v = values.clamp(0, 1)
    index = torch.where(values != values, torch.full_like(v, 256), (v * 256).clamp(max=255)).to(torch.int64)
    table = torch.cat([lut, torch.zeros((1, 3), dtype=torch.uint8)]).to(dev)
    colours = torch.cat([table[index], torch.full((1, 3), 255, dtype=torch.uint8, device=dev)])       # the last row: no owner, no base
    image = colours[torch.where(owner >= 0, owner, torch.full_like(owner, colours.shape[0] - 1)).to(torch.int64)]
    if base is not None:
        image = torch.where((owner >= 0)[..., None], image, base.to(dev))
    return image


# ------------------------------------------------------------------------------------------------
# The loop
# ------------------------------------------------------------------------------------------------
def explain_and_score(model, slides, explainer="GemExplainer", num_hops: Optional[int] = None, scores: Optional[Sequence] = None,
                      kernels: Optional[bool] = None):
    """The body of ``ExplainGraph.eval`` (explain_graphs.py:151-184) over ``slides``, an iterable of ``(graph, label, centres, annotation)``:
    ``centres`` [n, 2] the level-0 patch centres in patch order (``patch_centres``), ``annotation`` the slide's ``Annotation``.

    The explainer is picked as :160-168 does: ``"GNNExplainer"`` (``num_hops`` defaults to ``model.n_layers - 1``, :45), or ``"GemExplainer"``
    - ``GemExplainer`` for a homogeneous graph, ``HetGemExplainer`` otherwise, whose per-type masks go back to patch order (``patch_order``).
    ``explainer`` may also be a class with ``GemExplainer``'s constructor and ``explain_node()``.  ``scores``: one precomputed per-patch score
    tensor ([n] or [n, C]; or a per-type dict) per slide INSTEAD of running an explainer - GraphCAM's ``node_heat``, say; ``model`` may then
    be None, and ``graph`` too unless a score is a dict.

    The masks are collected in patch order, all slides are labelled in ONE ``patch_labels`` call and scored in ONE ``score`` call on the
    device of the centres.  Returns ``(LocalizationScore on the host, [mask per slide])``: its ``.cpu()`` is the only read-back after the
    explainers have run."""
    from . import explainers as E
    slides = list(slides)
    if scores is not None and len(scores) != len(slides):
        raise ValueError(f"explain_and_score: {len(scores)} precomputed scores for {len(slides)} slides")
    masks = []
    for i, (graph, label, centres, annotation) in enumerate(slides):
        if scores is not None:
            mask = scores[i]
        elif explainer == "GNNExplainer":                                                               # :160-162
            hops = int(num_hops) if num_hops is not None else model.n_layers - 1
            _, mask = E.GNNExplainer(graph, model, num_hops=hops).explain_node(node_idx=None)
        elif explainer == "GemExplainer":                                                               # :163-168
            mask = (E.GemExplainer if graph.is_homogeneous else E.HetGemExplainer)(graph, model, label).explain_node()
        elif isinstance(explainer, str):
            raise NotImplementedError("This Explainer is not implemented")                              # :170
        else:
            mask = explainer(graph, model, label).explain_node()
        mask = patch_order(graph, mask)
        mask = torch.as_tensor(mask).to(device=centres.device, dtype=torch.float32)
        if mask.shape[0] != centres.shape[0]:
            raise ValueError(f"explain_and_score: slide {i} has {centres.shape[0]} centres and {mask.shape[0]} scores")
        masks.append(mask)
    if not slides:
        raise ValueError("explain_and_score: no slides")
    sizes = [m.shape[0] for m in masks]
    centres = torch.cat([c for _, _, c, _ in slides])
    ann = AnnotationBatch([a for _, _, _, a in slides]).to(centres.device)
    labels = patch_labels(centres, sizes, ann, kernels=kernels)
    return score(torch.cat(masks), labels, sizes, kernels=kernels).cpu(), masks
