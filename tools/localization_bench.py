#!/usr/bin/env python
"""Scoring explanations against annotations on one GPU (``localization.patch_labels`` / ``score`` / ``heat_image``), ms per call, medians of
interleaved windows.

Workload: 8 slides x 10 000 patch centres (a 100 x 100 patch grid, centres 512 apart); per slide a synthetic annotation of about 200
star-shaped rings with about 10^5 vertices in total, three of them with 12 000 vertices, all on the quarter-integer lattice (so the legs must
agree bit for bit).  Scores quantised to 64 levels.  Legs:
``kernels``      the HIP kernels of csrc/localization.hip,
``tensor_ops``   the tensor formulation (``kernels=False``) on the same GPU, on the same device tensors,
``cpu``          ``matplotlib.path.Path.contains_points`` per ring (labels, ONE slide, host clock, scaled by the slide count in the ratio) and
                 sklearn's ``roc_curve`` + ``auc`` per slide (score, all slides), where those libraries are present.
``heat_image`` is timed at 2 000 x 2 000 pixels (10 000 patches of 20 x 20).  Prints one JSON line (and writes it to --out when given).

    python tools/localization_bench.py --repeats 5 --inner 2 [--out profiles/r28_localization.json]
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np
import torch

import __graft_entry__
from mil_bench import _interleaved

SLIDES, SIDE, STEP = 8, 100, 512


def star(rng, cx, cy, radius, k):
    """A star-shaped ring of k vertices around (cx, cy) on the quarter-integer lattice."""
    ang = np.sort(rng.rand(k)) * 2 * np.pi
    r = radius * (0.6 + 0.4 * rng.rand(k))
    return np.round(np.stack([cx + r * np.cos(ang), cy + r * np.sin(ang)], 1) * 4) / 4


def annotation(seed: int):
    rng = np.random.RandomState(seed)
    extent = SIDE * STEP
    rings = [star(rng, *(rng.rand(2) * extent), 8000 + 7000 * rng.rand(), 12000) for _ in range(3)]
    rings += [star(rng, *(rng.rand(2) * extent), 500 + 2500 * rng.rand(), int(rng.randint(200, 460))) for _ in range(196)]
    return rings


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--inner", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    __graft_entry__.build()
    from wsi_hgnn_amd import localization as L, ops

    dev = torch.device("cuda:0")
    n = SIDE * SIDE
    tiles = torch.stack([torch.arange(n) % SIDE, torch.arange(n) // SIDE], 1)
    _, centres1 = L.patch_centres(tiles, STEP // 2, 1)
    rings = [annotation(611 + s) for s in range(SLIDES)]
    anns = [L.Annotation.from_rings([r.tolist() for r in rs]) for rs in rings]
    batch = L.AnnotationBatch(anns).to(dev)
    centres = centres1.repeat(SLIDES, 1).to(dev)
    sizes = [n] * SLIDES
    res = {"workload": "explanations scored against annotations: patch labels, per-slide AUROC, heat map", "slides": SLIDES, "centres_per_slide": n,
           "rings_per_slide": batch.rings_per_slide[0], "vertices": int(batch.vertices.shape[0]), "chunks_per_slide": batch.chunks_per_slide,
           "chunk_edges": batch.chunk, "repeats": args.repeats, "inner": args.inner,
           "unit": "ms per call, median of interleaved windows (cpu: one run, host clock)"}

    def measure(call, row, equal):
        a, b = call(None), call(False)
        row["kernels_equal_tensor_ops"] = bool(equal(a, b))
        med, spread = _interleaved({"kernels_ms": lambda: call(None), "tensor_ops_ms": lambda: call(False)}, args.repeats, args.inner, warmup=1)
        row.update(med)
        row["min_max"] = spread
        row["tensor_ops_over_kernels"] = round(med["tensor_ops_ms"] / med["kernels_ms"], 3)
        ops.enable_kernel_timing(True)
        for _ in range(3):
            call(None)
        torch.cuda.synchronize()
        row["kernel_ms_per_3_calls"] = ops.kernel_timing_summary()
        ops.enable_kernel_timing(False)
        return a

    row = {}
    labels = measure(lambda k: L.patch_labels(centres, sizes, batch, kernels=k), row, torch.equal)
    row["positives"] = int(labels.sum())
    try:
        from matplotlib.path import Path
        pts = centres1.numpy().astype(np.float64)
        t0 = time.perf_counter()
        inside = np.zeros(n, dtype=bool)
        for r in rings[0]:
            inside |= Path(np.concatenate([r, r[:1]]), closed=True).contains_points(pts)
        row["cpu_matplotlib_one_slide_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
        row["cpu_matplotlib_differs_at"] = int((inside.astype(np.int32) != labels[:n].cpu().numpy()).sum())      # boundary points only, if any
        row["cpu_all_slides_over_kernels"] = round(SLIDES * row["cpu_matplotlib_one_slide_ms"] / row["kernels_ms"], 1)
    except ImportError:
        row["cpu_matplotlib_one_slide_ms"] = "not measured: matplotlib is absent"
    res["patch_labels"] = row

    gen = torch.Generator().manual_seed(611)
    scores = (torch.floor((torch.rand(n * SLIDES, generator=gen) * 0.7 + labels.cpu() * 0.2) * 64) / 64).to(dev)
    same = lambda a, b: all(torch.equal(getattr(a, f).nan_to_num(-1.0) if getattr(a, f).is_floating_point() else getattr(a, f),
                                        getattr(b, f).nan_to_num(-1.0) if getattr(b, f).is_floating_point() else getattr(b, f)) for f in L.LocalizationScore._FIELDS)
    row = {}
    got = measure(lambda k: L.score(scores, labels, sizes, kernels=k), row, same).cpu()
    row["auc"] = [round(v, 6) for v in got.auc.tolist()]
    try:
        from sklearn.metrics import auc, roc_curve
        y, s = labels.cpu().numpy(), scores.cpu().numpy()
        t0 = time.perf_counter()
        ref = [auc(*roc_curve(y[i * n:(i + 1) * n], s[i * n:(i + 1) * n])[:2]) for i in range(SLIDES)]
        row["cpu_sklearn_ms"] = round((time.perf_counter() - t0) * 1e3, 2)
        row["cpu_sklearn_max_abs_diff"] = float(np.nanmax(np.abs(np.array(ref) - got.auc.numpy())))
        row["cpu_over_kernels"] = round(row["cpu_sklearn_ms"] / row["kernels_ms"], 2)
    except ImportError:
        row["cpu_sklearn_ms"] = "not measured: scikit-learn is absent"
    res["score"] = row

    grid = (tiles * 20).to(dev)
    values = scores[:n]
    row = {"pixels": [2000, 2000], "patch": 19}
    measure(lambda k: L.heat_image(grid, values, 2000, 2000, 19, kernels=k), row, torch.equal)
    res["heat_image"] = row

    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
