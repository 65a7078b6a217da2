"""ReMix restated in plain float64 numpy, one bag and one row at a time so that it is obviously the arithmetic of the reference
(baselines/ReMix_DSMIL_ABMIL: tools/clustering.py:42-44, reduce.py:14-38, train_remix_k-fold.py:71-107) and of the k-means contract in
include/wsi_hgnn.h (wsi_bag_kmeans_step), plus the shape tables the ReMix tests share."""
import numpy as np
from scipy.spatial.distance import cdist

from mil_cases import Ratios, offsets, rel_err  # noqa: F401  (re-exported: the ReMix tests report in the MIL tests' norm)

# K = 8: two bags with fewer rows than clusters (one empty), a bag of exactly K rows, the chunk boundary (default chunk 128) from both sides,
# combines of 3 and 9 chunks
KERNEL_SIZES = (0, 5, 8, 9, 127, 128, 129, 293, 1061)
KERNEL_KS = (1, 2, 8, 16)
KERNEL_DS = (1, 3, 4, 50, 512, 1024)
SPLIT_EPS = 1.0 / 1024.0
BAND = 1e-5                     # rows whose best and second-best squared distance are closer than this may take either label in float32

KEEP, APPEND, INTERPOLATE, COV = 0, 1, 2, 3


def normalize64(x):
    x = np.asarray(x, dtype=np.float64)
    return x / (np.linalg.norm(x, axis=1)[:, None] + 1e-10)


def split64(mean, cnt):
    """The empty-cluster walk: k upwards, donor = largest current count (lowest index on a tie)."""
    mean, cnt = mean.copy(), cnt.copy()
    K, D = mean.shape
    sign = np.where(np.arange(D) % 2 == 0, 1.0, -1.0)
    for k in range(K):
        if cnt[k] != 0:
            continue
        donor = int(np.argmax(cnt))
        cd = mean[donor].copy()
        mean[k] = cd * (1 + SPLIT_EPS * sign)
        mean[donor] = cd * (1 - SPLIT_EPS * sign)
        cnt[k] = cnt[donor] // 2
        cnt[donor] -= cnt[k]
    return mean, cnt


def step64(x, sizes, cen, normalize=True, update=True, labels=None):
    """One Lloyd iteration over the bags: (labels [N], counts [S, K], objective [S], new centroids [S, K, D] or None, gap [N]) with
    gap = second-best minus best squared distance (inf at K = 1).  ``labels``: take these instead of the argmin (the means of a kernel's
    own labels)."""
    x = np.asarray(x, dtype=np.float64)
    cen = np.asarray(cen, dtype=np.float64)
    S, K, D = cen.shape
    o = offsets(sizes)
    lab = np.zeros(x.shape[0], dtype=np.int64)
    gap = np.full(x.shape[0], np.inf)
    counts = np.zeros((S, K), dtype=np.int64)
    obj = np.zeros(S)
    new = np.zeros_like(cen) if update else None
    for s, n in enumerate(sizes):
        if n < K:
            continue
        xs = x[o[s]:o[s + 1]]
        xn = normalize64(xs) if normalize else xs
        d2 = np.stack([((xn - cen[s, k]) ** 2).sum(1) for k in range(K)], 1)
        ls = np.argmin(d2, 1) if labels is None else np.asarray(labels[o[s]:o[s + 1]], dtype=np.int64)
        lab[o[s]:o[s + 1]] = ls
        obj[s] = d2[np.arange(n), ls].sum()
        if K > 1:
            part = np.partition(d2, 1, axis=1)
            gap[o[s]:o[s + 1]] = part[:, 1] - part[:, 0]
        cnt = np.bincount(ls, minlength=K)
        if update:
            mean = np.zeros((K, D))
            for k in range(K):
                if cnt[k]:
                    mean[k] = xn[ls == k].mean(0)
            new[s], cnt = split64(mean, cnt)
        counts[s] = cnt
    return lab, counts, obj, new, gap


def reduce64(x, sizes, init_rows, K, niter=20):
    """reduce.py:14-23 from given initial rows [S, K] (rows of the whole table): (labels, counts, prototypes, objectives [niter + 1, S],
    final centroids, gap of the final assignment)."""
    x = np.asarray(x, dtype=np.float64)
    S, D = len(sizes), x.shape[1]
    cen = np.zeros((S, K, D))
    for s, n in enumerate(sizes):
        if n >= K:
            cen[s] = normalize64(x[np.asarray(init_rows[s])])
    objs = []
    for _ in range(niter):
        _, _, obj, cen, _ = step64(x, sizes, cen)
        objs.append(obj)
    lab, counts, obj, _, gap = step64(x, sizes, cen, update=False)
    objs.append(obj)
    o = offsets(sizes)
    protos = np.zeros((S, K, D))
    for s in range(S):
        for k in range(K):
            if counts[s, k]:
                protos[s, k] = x[o[s]:o[s + 1]][lab[o[s]:o[s + 1]] == k].mean(0)
    return lab, counts, protos, np.stack(objs), cen, gap


def shift64(x, sizes, labels, K, z):
    """[S, K, V, D]: (n_k - 1)^(-1/2) * sum_r z[r, v] * (x[r] - mean of the cluster's rows); 0 where n_k < 2."""
    x, z = np.asarray(x, dtype=np.float64), np.asarray(z, dtype=np.float64)
    o = offsets(sizes)
    out = np.zeros((len(sizes), K, z.shape[1], x.shape[1]))
    for s in range(len(sizes)):
        xs, zs, ls = x[o[s]:o[s + 1]], z[o[s]:o[s + 1]], np.asarray(labels[o[s]:o[s + 1]])
        for k in range(K):
            m = ls == k
            if m.sum() >= 2:
                out[s, k] = zs[m].T @ (xs[m] - xs[m].mean(0)) / np.sqrt(m.sum() - 1)
    return out


def mix_aug_rows(src, tgt, shift, lam, replaced, appended):
    """mix_aug (train_remix_k-fold.py:71-107) with its draws already made: ``src`` = the shuffled source rows, ``replaced`` [K] and
    ``appended`` = (op, position, replaced at that moment, shift index) in generation order, as ``remix.draw_rows`` returns them.
    numpy arithmetic in the reference's expression order and dtypes."""
    closest = np.argmin(cdist(src, tgt), axis=1)
    rows = [r for r in src]
    for i in range(len(src)):
        if replaced[i]:
            rows[i] = tgt[closest[i]]
    out = list(rows)
    for op, i, rep, v in appended:
        cur = tgt[closest[i]] if rep else src[i]
        if op == APPEND:
            out.append(tgt[closest[i]])
        elif op == INTERPOLATE:
            out.append((1 - lam) * cur + lam * tgt[closest[i]])
        else:
            out.append((cur[np.newaxis, :] + lam * shift[closest[i]][[v]]).flatten())
    return np.array(out)


def gaussian_rows(sizes, D, seed):
    return np.random.RandomState(seed).standard_normal((sum(sizes), D)).astype(np.float32)


def blob_rows(sizes, D, K, seed, centre_sd=3.0, noise=0.5):
    """Every bag: K separated blobs - centres N(0, centre_sd^2), noise N(0, noise^2) - in shuffled row order."""
    rs = np.random.RandomState(seed)
    out = []
    for n in sizes:
        centres = rs.standard_normal((K, D)) * centre_sd
        which = rs.permutation(n) % K
        out.append(centres[which] + rs.standard_normal((n, D)) * noise)
    return np.concatenate(out).astype(np.float32) if out else np.zeros((0, D), dtype=np.float32)


def integer_rows(sizes, D, seed, lo=-3, hi=4):
    return np.random.RandomState(seed).randint(lo, hi, size=(sum(sizes), D)).astype(np.float32)
