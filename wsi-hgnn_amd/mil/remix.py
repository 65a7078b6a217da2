"""ReMix (``baselines/ReMix_DSMIL_ABMIL``: reduce.py, tools/clustering.py, train_remix_k-fold.py) on the device.

Every training bag is reduced once to K prototypes by a k-means over its L2-normalised rows (``reduce_bags``: the Lloyd iterations are
``ops.bag_kmeans_step``, all bags in one launch, nothing read back), a bank of "semantic shift" vectors is drawn per prototype from the
cluster's covariance, and every training step mixes the reduced bag with a same-class partner's prototypes (``draw_mix`` consumes the
reference's random draws in its order on the host; ``mix`` writes every row of every mixed bag of the step in two launches).

Every operation has a tensor formulation that runs on any device (``kmeans_step_tensor``, ``nearest_tensor``, ``mix_rows_tensor``, and
``reduce_bags`` / ``mix`` with ``kernels=False``): the CPU tests use it and the GPU tests compare the kernels against it.

Two rules differ from faiss, whose generator cannot be replayed: the initial centroids are the K normalised rows that come first in the
stable order of ``ops.augment_hash(n, ops.augment_subseed(seed, 0, bag))``, and an empty cluster is split off the cluster with the largest
current count (lowest index on a tie) instead of a drawn one.  Not built: PCA, PIC, the k-fold scripts
(evaluation and ``multi_label_roc``: ``mil.metrics``)."""
from __future__ import annotations

import os
from typing import List, NamedTuple, Optional, Sequence

import numpy as np
import torch

from .. import _native as N
from .. import ops
from ..graph import host_to_device
from .bags import bag_plan

NORM_EPS = 1e-10            # tools/clustering.py:44
SPLIT_EPS = 1.0 / 1024.0
MODES = ("replace", "append", "interpolate", "cov", "joint")
KEEP, APPEND, INTERPOLATE, COV = 0, 1, 2, 3          # WSI_REMIX_* of include/wsi_hgnn.h (restated: this module also runs without the library)


class ReducedBags(NamedTuple):
    prototypes: torch.Tensor            # [S, K, D]: the mean of the RAW rows per label (reduce.py:22-23)
    shifts: Optional[torch.Tensor]      # [S, K, V, D] or None
    labels: torch.Tensor                # [N] int32
    counts: torch.Tensor                # [S, K] int32
    ok: torch.Tensor                    # [S] bool, on the device: the bag has at least K rows (and, with shifts, every cluster at least 2)
    objective: torch.Tensor             # [niter + 1, S]: the k-means objective of every assignment (the last row: the final one)
    centroids: torch.Tensor             # [S, K, D]: the final centroids (of the normalised rows) the labels are the assignment to


def _sizes(bags) -> List[int]:
    if isinstance(bags, ops.ReducePlan):
        if bags.first_row != 0:
            raise ValueError("remix: the bag plan must start at row 0")
        return [b - a for a, b in bags.ranges]
    if isinstance(bags, torch.Tensor):
        if bags.is_cuda:
            raise ValueError("remix: the bags' row counts are host values (a list, a CPU tensor or a bag plan): a device tensor would be read back")
        bags = bags.tolist()
    return [int(c) for c in bags]


def _offsets(sizes: Sequence[int]) -> List[int]:
    o = [0]
    for n in sizes:
        o.append(o[-1] + n)
    return o


def normalize_rows(x: torch.Tensor) -> torch.Tensor:
    """x / (|x|_2 + 1e-10) per row (tools/clustering.py:42-44); a zero row stays zero."""
    return x / (torch.linalg.vector_norm(x, dim=1, keepdim=True) + NORM_EPS)


# ------------------------------------------------------------------------------------------------ k-means
def initial_rows(sizes: Sequence[int], K: int, seed: int, device="cpu", kernels: Optional[bool] = None) -> torch.Tensor:
    """[S, K] int64: the rows (numbered over the whole table) whose normalised copies are the initial centroids of every bag - the K rows
    that come first in the stable order of ``ops.augment_hash(n, ops.augment_subseed(seed, 0, bag))``; a bag with fewer than K rows gets
    row 0 K times (its centroids are zeroed by the caller).  On the GPU: one key launch and one sort for all bags, no read-back."""
    dev = torch.device(device)
    subs = [ops.augment_subseed(seed, 0, s) for s in range(len(sizes))]
    off = _offsets(sizes)
    if kernels is None:
        kernels = dev.type == "cuda"
    if kernels:
        order, _ = ops.segment_hash_order(list(sizes), subs, dev)
        if off[-1] == 0:
            return torch.zeros((len(sizes), K), dtype=torch.int64, device=dev)
        pos = host_to_device([[off[s] + j if n >= K else -1 for j in range(K)] for s, n in enumerate(sizes)], torch.int64, dev).view(-1)
        return (order[pos.clamp(min=0)] * (pos >= 0)).view(len(sizes), K)
    rows = []
    for s, n in enumerate(sizes):
        if n < K:
            rows.append(torch.zeros(K, dtype=torch.int64, device=dev))
        else:
            rows.append(torch.sort(ops.augment_hash(n, subs[s], dev), stable=True).indices[:K] + off[s])
    return torch.stack(rows) if rows else torch.zeros((0, K), dtype=torch.int64, device=dev)


def split_empty_clusters(cen: torch.Tensor, cnt: torch.Tensor):
    """The split rule of ``wsi_bag_kmeans_step`` on one bag's means [K, D] and counts [K], as tensor operations without a read-back."""
    K, D = cen.shape
    e = torch.where(torch.arange(D, device=cen.device) % 2 == 0, SPLIT_EPS, -SPLIT_EPS).to(cen.dtype)
    cen, cnt = cen.clone(), cnt.clone()
    for k in range(K):
        empty = cnt[k] == 0
        d = torch.argmax(cnt).view(1)                          # the first maximum
        most, cd = cnt[d], cen[d]                              # [1], [1, D]
        half = most // 2
        new_k = torch.where(empty, cd[0] * (1 + e), cen[k])
        cnt_k = torch.where(empty, half[0], cnt[k])
        cen = cen.index_copy(0, d, torch.where(empty, cd * (1 - e), cd))
        cnt = cnt.index_copy(0, d, torch.where(empty, most - half, most))
        cen[k], cnt[k] = new_k, cnt_k
    return cen, cnt


def kmeans_step_tensor(x: torch.Tensor, bags, centroids: torch.Tensor, normalize: bool = True, update: bool = True):
    """``ops.bag_kmeans_step`` as tensor operations in x's dtype on x's device (bag by bag; nothing is read back)."""
    sizes = _sizes(bags)
    S, K, D = centroids.shape
    off = _offsets(sizes)
    dev = x.device
    labels = torch.zeros(x.shape[0], dtype=torch.int32, device=dev)
    counts = torch.zeros((S, K), dtype=torch.int32, device=dev)
    objective = torch.zeros(S, dtype=x.dtype, device=dev)
    new = torch.zeros_like(centroids) if update else None
    ks = torch.arange(K, device=dev)
    for s, n in enumerate(sizes):
        if n < K:
            continue
        xs = x[off[s]:off[s + 1]]
        xn = normalize_rows(xs) if normalize else xs
        d2 = torch.stack([((xn - centroids[s, k]) ** 2).sum(1) for k in range(K)], 1)           # [n, K]
        lab = torch.argmin(d2, 1)                                                                # (the first minimum)
        best = d2.gather(1, lab.view(-1, 1))
        labels[off[s]:off[s + 1]] = lab.to(torch.int32)
        objective[s] = best.sum()
        onehot = (lab.view(-1, 1) == ks).to(x.dtype)
        cnt = onehot.sum(0).to(torch.int32)
        if update:
            mean = (onehot.t() @ xn) / cnt.clamp(min=1).view(-1, 1).to(x.dtype)
            new[s], cnt = split_empty_clusters(mean, cnt)
        counts[s] = cnt
    return labels, counts, objective, new


def shift_bank(x: torch.Tensor, bags, labels: torch.Tensor, counts: torch.Tensor, prototypes: torch.Tensor, z: torch.Tensor,
               kernels: Optional[bool] = None) -> torch.Tensor:
    """[S, K, V, D]: shift[s, k, v] = (n_k - 1)^(-1/2) * sum over the rows r of cluster (s, k) of z[r, v] * (x[r] - prototype[s, k]) - with
    z iid standard normal a draw from N(0, np.cov(cluster rows)) (reduce.py:26-34) without the D x D covariance; 0 where n_k < 2.
    The cluster's rows are selected by zeroing z outside it, so every product runs over the bag's whole (host-known) row range: the
    grouped weight-gradient GEMM in exact fp32 on the GPU (one group per bag, one call per cluster index), ``matmul`` otherwise."""
    sizes = _sizes(bags)
    S, K, D = prototypes.shape
    V = z.shape[1]
    off = _offsets(sizes)
    dev = x.device
    if kernels is None:
        kernels = dev.type == "cuda"
    if kernels and isinstance(bags, ops.ReducePlan):
        seg = bags.row_segment().to(torch.int64)
    else:
        seg = torch.repeat_interleave(torch.arange(S), torch.tensor(sizes, dtype=torch.int64)).to(dev)         # (expanded on the host)
    cluster = seg * K + labels.to(torch.int64)
    xc = (x - prototypes.reshape(S * K, D)[cluster]).contiguous()
    nk = counts.reshape(-1)[cluster].to(x.dtype)
    zs = (z * torch.where(nk >= 2, (nk - 1).clamp(min=1).rsqrt(), torch.zeros_like(nk)).view(-1, 1)).contiguous()
    out = torch.zeros((S, K, V, D), dtype=x.dtype, device=dev)
    for k in range(K):
        a = (zs * (labels == k).view(-1, 1)).contiguous()
        if kernels:
            ops.gemm_tn_fp32([dict(A=N.ptr(a, off[s] * V * 4), lda=V, B=N.ptr(xc, off[s] * D * 4), ldb=D, C=N.ptr(out, (s * K + k) * V * D * 4),
                                   ldc=D, M=V, N=D, K=n) for s, n in enumerate(sizes) if n >= 2], dev)
        else:
            for s, n in enumerate(sizes):
                if n >= 2:
                    out[s, k] = a[off[s]:off[s + 1]].t() @ xc[off[s]:off[s + 1]]
    return out


def reduce_bags(x: torch.Tensor, bags, num_prototypes: int = 8, niter: int = 20, seed: int = 66, num_shift_vectors: int = 200,
                z: Optional[torch.Tensor] = None, kernels: Optional[bool] = None, initial: Optional[torch.Tensor] = None) -> ReducedBags:
    """reduce.py:14-38 for a batch of bags: x [N, D] fp32, the bags one after the other (``bags``: their row counts or their ``bag_plan``).
    ``niter`` Lloyd iterations from the hashed initial rows (``initial``: [S, K] rows of the table to start from instead), then one
    assignment; prototypes = the means of the RAW rows per label; shifts from ``z`` [N, V] (None: ``torch.randn`` on x's device seeded
    by ``seed``), None when ``num_shift_vectors`` is 0.  ``kernels``: None = the HIP kernels on the GPU, the tensor formulation elsewhere.
    Nothing is read back: ``ok`` stays on the device."""
    K, V = int(num_prototypes), int(num_shift_vectors)
    if x.dim() != 2:
        raise ValueError("reduce_bags: x is [rows, D]")
    dev = x.device
    if kernels is None:
        kernels = dev.type == "cuda"
    if kernels:
        x = x.to(torch.float32).contiguous()
    sizes = _sizes(bags)
    if sum(sizes) != x.shape[0]:
        raise ValueError(f"reduce_bags: the bags hold {sum(sizes)} rows, the table has {x.shape[0]}")
    if not 1 <= K <= ops.KMEANS_MAX_K:
        raise ValueError(f"reduce_bags: 1 <= num_prototypes <= {ops.KMEANS_MAX_K}")
    S, D = len(sizes), x.shape[1]
    plan = (bags if isinstance(bags, ops.ReducePlan) else bag_plan(sizes, dev)) if kernels else sizes
    enough = host_to_device([1.0 if n >= K else 0.0 for n in sizes] or [0.0], torch.float32, dev)[:S]
    rows = initial_rows(sizes, K, seed, dev, kernels) if initial is None else initial.to(dev)
    if x.shape[0]:
        cen = (normalize_rows(x[rows.reshape(-1)]).view(S, K, D) * enough.view(-1, 1, 1).to(x.dtype)).contiguous()
    else:
        cen = torch.zeros((S, K, D), dtype=x.dtype, device=dev)
    step = ops.bag_kmeans_step if kernels else kmeans_step_tensor
    objs = []
    for _ in range(niter):
        _, _, obj, cen = step(x, plan, cen, True, True)
        objs.append(obj)
    labels, counts, obj, _ = step(x, plan, cen, True, False)
    objs.append(obj)
    onehot = (labels.view(-1, 1) == torch.arange(K, device=dev, dtype=torch.int32)).to(x.dtype)
    if kernels:
        sums = ops.segment_weighted_sums(x, onehot, plan)
    else:
        off = _offsets(sizes)
        sums = torch.stack([onehot[off[s]:off[s + 1]].t() @ x[off[s]:off[s + 1]] for s in range(S)]) if S else x.new_zeros((0, K, D))
    prototypes = sums / counts.clamp(min=1).to(x.dtype).unsqueeze(-1) * enough.view(-1, 1, 1).to(x.dtype)       # (a bag with fewer than K rows: 0)
    ok = enough > 0
    shifts = None
    if V:
        if z is None:
            z = torch.randn((x.shape[0], V), generator=torch.Generator(device=dev).manual_seed(int(seed)), device=dev, dtype=torch.float32)
        if z.shape != (x.shape[0], V):
            raise ValueError(f"reduce_bags: z is [{x.shape[0]}, {V}]")
        shifts = shift_bank(x, plan, labels, counts, prototypes, z.to(dev, x.dtype), kernels)
        ok = ok & (counts.min(1).values >= 2)
    return ReducedBags(prototypes, shifts, labels, counts, ok, torch.stack(objs), cen)


# ------------------------------------------------------------------------------------------------ mixing
class MixDraw(NamedTuple):
    idx: int                    # the bag that is trained on
    partner: int                # the same-class bag it is mixed with (idx itself with mode None)
    lam: float                  # the strength (a double, as np.random.uniform returns it)
    perm: np.ndarray            # the row shuffle of get_bag_feats_v2
    replaced: np.ndarray        # [K] bool: position i was overwritten
    appended: list              # (op, position, replaced at that moment, shift index) in generation order
    num_rows: int
    desc: np.ndarray            # [num_rows, 8] int32 rows of wsi_remix_rows, `slot` relative to this bag (``mix`` adds b * K)


def draw_rows(rng, K: int, mode: str, rate: float, V: int = 200):
    """The per-row draws of ``mix_aug`` (train_remix_k-fold.py:76-106) in its order: (replaced [K], appended list)."""
    if mode not in MODES:
        raise ValueError(f"remix: mode is one of {MODES} (or None)")
    replaced = np.zeros(K, dtype=bool)
    appended = []
    for i in range(K):
        if mode != "joint":
            if rng.rand() <= rate:
                if mode == "replace":
                    replaced[i] = True
                elif mode == "append":
                    appended.append((APPEND, i, False, 0))
                elif mode == "interpolate":
                    appended.append((INTERPOLATE, i, False, 0))
                else:
                    appended.append((COV, i, False, int(rng.choice(V, 1)[0])))
            continue
        if rng.rand() <= rate:
            replaced[i] = True
        if rng.rand() <= rate:
            appended.append((APPEND, i, bool(replaced[i]), 0))
        if rng.rand() <= rate:
            appended.append((INTERPOLATE, i, bool(replaced[i]), 0))
        if rng.rand() <= rate:
            appended.append((COV, i, bool(replaced[i]), int(rng.choice(V, 1)[0])))
    return replaced, appended


def _f32_bits(v: float) -> int:
    return int(np.float32(v).view(np.int32))


def draw_mix(rng, labels, idx: int, K: int, mode: Optional[str], rate: float, V: int = 200) -> MixDraw:
    """One training bag's draws in the reference's order - ``permutation(K)`` (get_bag_feats_v2, line 36), ``choice`` over the same-class
    bags (lines 113-114), ``uniform(0, 1)`` (line 116), then ``draw_rows`` - and what follows from them on the host: the decisions, the
    number of output rows and the row descriptor table.  ``rng``: a ``np.random.RandomState`` or the ``np.random`` module; ``labels``: the
    bank's labels (host).  ``mode=None``: the shuffle alone."""
    perm = np.asarray(rng.permutation(K))
    if mode is None:
        partner, lam, replaced, appended = int(idx), 0.0, np.zeros(K, dtype=bool), []
    else:
        labels = np.asarray(labels)
        same = np.argwhere(labels == labels[idx]).reshape(-1)
        partner = int(rng.choice(same))
        lam = float(rng.uniform(0, 1))
        replaced, appended = draw_rows(rng, K, mode, rate, V)
    lam_bits, oml_bits = _f32_bits(lam), _f32_bits(1.0 - lam)           # (1 - strength) is taken in double, then meets float32 rows
    rows = [(KEEP, int(perm[i]), idx * K + int(perm[i]), partner, int(replaced[i]), 0, lam_bits, oml_bits) for i in range(K)]
    rows += [(op, int(perm[i]), idx * K + int(perm[i]), partner, int(rep), v, lam_bits, oml_bits) for op, i, rep, v in appended]
    return MixDraw(int(idx), partner, lam, perm, replaced, appended, len(rows), np.asarray(rows, dtype=np.int32).reshape(-1, 8))


def nearest_tensor(protos: torch.Tensor, src: torch.Tensor, tgt: torch.Tensor) -> torch.Tensor:
    """``ops.remix_nearest`` as tensor operations: [B, K] int32."""
    a, b = protos[src.to(torch.int64)], protos[tgt.to(torch.int64)]                   # [B, K, D]
    d2 = ((a.unsqueeze(2) - b.unsqueeze(1)) ** 2).sum(-1)                                # [B, K, K]
    return torch.argmin(d2, 2).to(torch.int32)


def mix_rows_tensor(protos: torch.Tensor, shifts: Optional[torch.Tensor], nearest: torch.Tensor, desc: torch.Tensor) -> torch.Tensor:
    """``ops.remix_rows`` as tensor operations in the prototypes' dtype (float32: the kernel's arithmetic, product by product)."""
    S, K, D = protos.shape
    d = desc.to(torch.int64)
    op, slot, src_row, partner, replaced, v = (d[:, i] for i in range(6))
    lam = desc[:, 6].contiguous().view(torch.float32).to(protos.dtype).view(-1, 1)
    oml = desc[:, 7].contiguous().view(torch.float32).to(protos.dtype).view(-1, 1)
    c = nearest.reshape(-1).to(torch.int64)[slot]
    tgt = protos[partner, c]
    cur = torch.where(replaced.view(-1, 1) != 0, tgt, protos.reshape(S * K, D)[src_row])
    out = torch.where(op.view(-1, 1) == APPEND, tgt, cur)
    out = torch.where(op.view(-1, 1) == INTERPOLATE, oml * cur + lam * tgt, out)
    if shifts is not None:
        out = torch.where(op.view(-1, 1) == COV, cur + lam * shifts[partner, c, v.clamp(max=shifts.shape[2] - 1)], out)
    return out


class PrototypeBank:
    """The reduced training set: ``prototypes`` [S, K, D], ``shifts`` [S, K, V, D] or None (both on one device), ``labels`` [S] (host)."""

    def __init__(self, prototypes: torch.Tensor, shifts: Optional[torch.Tensor], labels):
        self.prototypes, self.shifts, self.labels = prototypes, shifts, np.asarray(labels)
        if self.labels.shape[0] != prototypes.shape[0] or (shifts is not None and shifts.shape[:2] != prototypes.shape[:2]):
            raise ValueError("PrototypeBank: prototypes, shifts and labels disagree on the number of bags")

    @classmethod
    def from_reduced(cls, reduced: ReducedBags, labels) -> "PrototypeBank":
        """Keeps the bags whose ``ok`` is set, as reduce.py's try / except does (lines 41-42): the one read-back of the reduction."""
        keep = torch.nonzero(reduced.ok.cpu()).view(-1)
        on = keep.to(reduced.prototypes.device)
        return cls(reduced.prototypes[on], None if reduced.shifts is None else reduced.shifts[on], np.asarray(labels)[keep.numpy()])

    @staticmethod
    def paths(directory: str, K: int):
        return (os.path.join(directory, f"train_bag_feats_proto_{K}_base.npy"), os.path.join(directory, f"train_bag_feats_shift_{K}_base.npy"),
                os.path.join(directory, "train_bag_labels_base.npy"))

    def save(self, directory: str, K: int) -> None:
        """reduce.py:46-58's files: ``train_bag_feats_proto_{K}_base.npy`` [S, K, D], ``train_bag_feats_shift_{K}_base.npy`` [S, K, V, D],
        ``train_bag_labels_base.npy``."""
        if K != self.prototypes.shape[1]:
            raise ValueError(f"PrototypeBank.save: the bank has {self.prototypes.shape[1]} prototypes per bag, not {K}")
        os.makedirs(directory, exist_ok=True)
        proto, shift, lab = self.paths(directory, K)
        np.save(proto, self.prototypes.detach().cpu().numpy())
        if self.shifts is not None:
            np.save(shift, self.shifts.detach().cpu().numpy())
        np.save(lab, self.labels)

    @classmethod
    def load(cls, directory: str, K: int, device="cpu") -> "PrototypeBank":
        proto, shift, lab = cls.paths(directory, K)
        f32 = lambda p: torch.from_numpy(np.ascontiguousarray(np.load(p), dtype=np.float32)).to(device)
        return cls(f32(proto), f32(shift) if os.path.exists(shift) else None, np.load(lab))


def mix(bank: PrototypeBank, draws: Sequence[MixDraw], kernels: Optional[bool] = None):
    """(rows [sum of the bags' rows, D], the row count of every mixed bag): the mixed bags of one step, one after the other.  Two launches on
    the GPU (``ops.remix_nearest``, ``ops.remix_rows``) whatever the number of bags; the sizes come from the draws, not from the device."""
    protos = bank.prototypes
    dev, K = protos.device, protos.shape[1]
    if kernels is None:
        kernels = dev.type == "cuda"
    desc = np.concatenate([d.desc + np.asarray([0, b * K, 0, 0, 0, 0, 0, 0], dtype=np.int32) for b, d in enumerate(draws)]) if draws \
        else np.zeros((0, 8), dtype=np.int32)
    if bank.shifts is None and bool((desc[:, 0] == COV).any()):
        raise ValueError("remix: a 'cov' row needs the shift bank")
    words = host_to_device(torch.from_numpy(np.concatenate([np.asarray([d.idx for d in draws] + [d.partner for d in draws], dtype=np.int32), desc.reshape(-1)])),
                           torch.int32, dev)
    B = len(draws)
    src, tgt, desc_t = words[:B], words[B:2 * B], words[2 * B:].view(-1, 8)
    if kernels:
        rows = ops.remix_rows(protos, bank.shifts, ops.remix_nearest(protos, src, tgt), desc_t)
    else:
        rows = mix_rows_tensor(protos, bank.shifts, nearest_tensor(protos, src, tgt), desc_t)
    return rows, [d.num_rows for d in draws]


def train_one_step(milnet, optimizer, bank: PrototypeBank, idxs: Sequence[int], mode: Optional[str], rate: float, rng) -> torch.Tensor:
    """The body of train_remix_k-fold.py's ``train`` loop (lines 128-153) for the reduced bags ``idxs`` at once: draw, mix on the device, build
    the bag plan from the drawn sizes and run ``mil.train_one_step``.  ``mode=None`` trains on the (shuffled) reduced bags as they are."""
    from . import train_one_step as step
    K = bank.prototypes.shape[1]
    V = bank.shifts.shape[2] if bank.shifts is not None else 200
    draws = [draw_mix(rng, bank.labels, int(i), K, mode, rate, V) for i in idxs]
    rows, sizes = mix(bank, draws)
    return step(milnet, optimizer, rows, bag_plan(sizes, rows.device), bank.labels[np.asarray(list(idxs), dtype=np.int64)])
