#!/usr/bin/env python
"""Slide graphs from patch grids on one GPU (``construct.grid_adjacency`` / ``construct.slide_trees``), ms per call, medians of interleaved
windows; every call ends in its read-back of the item total, so a window is whole calls.

GTNMIL: 8 slides of 2 000 and of 10 000 patches - a filled disc on the grid, nodes in shuffled order.  H2MIL: 8 slides of 901 and of 4 501 nodes
(the sizes of profiles/r19_h2mil.json: a root, a disc of level-1 cells, four level-2 cells under each).  Three legs:
``kernels``      the HIP kernels (wsi_grid_index / _count / _write) with the prefix sum between them,
``tensor_ops``   the tensor formulation (sorted keys + searchsorted) on the same GPU, on the same device tensors,
``cpu_loops``    the reference's rule as Python loops on the CPU - the O(n^2) double loop of build_graphs.py:78-96 over integer pairs, the
                 dictionary look-ups of github_pretreat.py:94-329 over integer tuples - timed once with the host clock, at the small size only
                 (the double loop is quadratic).  The reference's own scripts also parse every file name inside those loops; that is left out,
                 so this leg flatters the reference.
The outputs of the first two legs are compared (they must be equal).  Prints one JSON line (and writes it to --out when given).

    python tools/grid_graph_bench.py --repeats 7 --inner 5 [--out profiles/r20_grid_graph.json]
"""
import argparse
import json
import math
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch

import __graft_entry__
from mil_bench import _interleaved

SLIDES = 8
NB8 = ((0, 1), (0, -1), (1, 0), (-1, 0), (1, 1), (-1, 1), (1, -1), (-1, -1))


def disc(n: int, seed: int):
    """The ``n`` grid cells nearest to a centre, shifted to start at 0, in shuffled order: int64 [n, 2]."""
    r = int(math.ceil(math.sqrt(n / math.pi))) + 2
    cells = sorted((x * x + y * y, x, y) for x in range(-r, r + 1) for y in range(-r, r + 1))[:n]
    pts = torch.tensor([(x, y) for _, x, y in cells], dtype=torch.int64)
    pts = pts - pts.min(0).values
    return pts[torch.randperm(n, generator=torch.Generator().manual_seed(seed))]


def tree_tables(n1: int, seed: int):
    """(coords1 [n1, 2], cover [n1, 4], coords2 [4 n1, 2]): a disc of level-1 cells, cell (i, j) covering the level-2 cells (2i, 2i+1) x (2j, 2j+1)."""
    c1 = disc(n1, seed)
    cover = torch.stack([2 * c1[:, 0], 2 * c1[:, 0] + 1, 2 * c1[:, 1], 2 * c1[:, 1] + 1], 1)
    c2 = torch.stack([cover[:, [0, 2]], cover[:, [1, 2]], cover[:, [0, 3]], cover[:, [1, 3]]], 1).reshape(-1, 2)
    return c1, cover, c2[torch.randperm(c2.shape[0], generator=torch.Generator().manual_seed(seed + 1000))]


def adjacency_double_loop(points):
    """build_graphs.py:78-96 over integer pairs: the entries of the dense matrix (its nonzero() follows in one numpy call, not timed apart)."""
    total = len(points)
    hits = []
    for i in range(total - 1):
        x_i, y_i = points[i]
        for j in range(i + 1, total):
            x_j, y_j = points[j]
            if abs(x_i - x_j) <= 1 and abs(y_i - y_j) <= 1:
                hits.append((i, j))
    return hits


def tree_dictionary_loops(coords1, cover, coords2):
    """github_pretreat.py:94-254 over integer tuples: the edges and the parent table of one slide."""
    n1 = len(coords1)
    at1 = {p: 1 + r for r, p in enumerate(coords1)}
    at2 = {p: 1 + n1 + r for r, p in enumerate(coords2)}
    start, end, tree = [], [], [-1] + [0] * n1 + [-2] * len(coords2)
    for r, (a, b, c, d) in enumerate(cover):
        start += [1 + r, 0]
        end += [0, 1 + r]
        for child in ((a, c), (b, c), (a, d), (b, d)):
            if child in at2:
                start += [1 + r, at2[child]]
                end += [at2[child], 1 + r]
                tree[at2[child]] = 1 + r
    for points, at in ((coords1, at1), (coords2, at2)):
        for x, y in points:
            for dx, dy in NB8:
                if (x + dx, y + dy) in at:
                    start.append(at[(x, y)])
                    end.append(at[(x + dx, y + dy)])
    return start, end, tree


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--inner", type=int, default=5)
    ap.add_argument("--gtn-sizes", type=int, nargs=2, default=(2000, 10000), help="patches per slide of the small and the large GTNMIL batch")
    ap.add_argument("--tree-sizes", type=int, nargs=2, default=(180, 900), help="level-1 nodes per slide of the small and the large H2MIL batch")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("grid_graph_bench.py measures on the GPU; none is visible")
    __graft_entry__.build()
    from wsi_hgnn_amd import construct, ops

    dev = torch.device("cuda:0")
    res = {"workload": "slide graphs from patch grids: GTNMIL grid adjacency and H2MIL slide trees", "slides": SLIDES, "repeats": args.repeats,
           "inner": args.inner, "unit": "ms per call, median of interleaved windows (cpu_loops: one run, host clock)", "gtn": {}, "h2mil": {}}

    def measure(call, row):
        legs = {"kernels_ms": lambda: call(True), "tensor_ops_ms": lambda: call(False)}
        a, b = call(True), call(False)
        row["kernels_equal_tensor_ops"] = bool(all(torch.equal(p, q) or (p.is_floating_point() and torch.equal(p.nan_to_num(-1.0), q.nan_to_num(-1.0)))
                                                   for p, q in zip(a, b)))
        med, spread = _interleaved(legs, args.repeats, args.inner)
        row.update(med)
        row["min_max"] = spread
        row["tensor_ops_over_kernels"] = round(med["tensor_ops_ms"] / med["kernels_ms"], 3)
        ops.enable_kernel_timing(True)
        for _ in range(3):
            call(True)
        torch.cuda.synchronize()
        row["kernel_ms_per_3_calls"] = ops.kernel_timing_summary()
        ops.enable_kernel_timing(False)
        return a

    for name, n in zip(("small", "large"), args.gtn_sizes):
        slides = [disc(n, 611 + i) for i in range(SLIDES)]
        coords, sizes = torch.cat(slides).to(dev), [n] * SLIDES
        row = {"patches_per_slide": n, "nodes": n * SLIDES}
        out = measure(lambda k: construct.grid_adjacency(coords, sizes, kernels=k), row)
        row["entries"] = int(out[0].numel())
        row["dense_adjacency_bytes_avoided"] = 8 * n * n * SLIDES                       # the reference's float64 n x n matrix per slide
        if name == "small":
            lists = [[tuple(p) for p in s.tolist()] for s in slides]
            t0 = time.perf_counter()
            hits = [adjacency_double_loop(pts) for pts in lists]
            row["cpu_loops_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
            row["cpu_loops_equal"] = 2 * sum(len(h) for h in hits) == row["entries"]
            row["cpu_loops_over_kernels"] = round(row["cpu_loops_ms"] / row["kernels_ms"], 1)
        else:
            row["cpu_loops_ms"] = "not measured: the double loop is quadratic"
        res["gtn"][name] = row

    for name, n1 in zip(("small", "large"), args.tree_sizes):
        tables = [tree_tables(n1, 611 + i) for i in range(SLIDES)]
        c1, cv, c2 = (torch.cat([t[k] for t in tables]).to(dev) for k in range(3))
        n1s, n2s = [n1] * SLIDES, [4 * n1] * SLIDES
        row = {"nodes_per_slide": 1 + 5 * n1, "nodes": SLIDES * (1 + 5 * n1)}
        out = measure(lambda k: construct.slide_trees(c1, cv, c2, n1s, n2s, kernels=k), row)
        row["edges"] = int(out[0].shape[1])
        if name == "small":
            lists = [tuple([tuple(p) for p in t[k].tolist()] for k in range(3)) for t in tables]
            t0 = time.perf_counter()
            loops = [tree_dictionary_loops(*l) for l in lists]
            row["cpu_loops_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
            row["cpu_loops_equal"] = sum(len(l[0]) for l in loops) == row["edges"]
            row["cpu_loops_over_kernels"] = round(row["cpu_loops_ms"] / row["kernels_ms"], 1)
        else:
            row["cpu_loops_ms"] = "not measured: the small size only, as for GTNMIL"
        res["h2mil"][name] = row

    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
