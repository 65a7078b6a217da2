#!/usr/bin/env python
"""ReMix timing on one GPU: ``mil.remix.reduce_bags`` over 1 and 8 bags of 10 000 x 1024 rows at K = 8 (20 Lloyd iterations and the final
assignment; with and without the 200 shift vectors per prototype), the k-means step kernel alone per iteration (HIP events) with the bytes its
algorithm has to move - the rows once, N * D * 4 - over the time against the project's measured streaming rate, for several
chunk sizes of the bag plan, and the same reduction written in plain PyTorch on the same GPU (``cdist``, ``argmin``, ``index_add_`` per bag,
the same number of iterations).  Then one mixed training step (``remix.train_one_step``, mode 'joint') of DSMIL and ABMIL at 8 and 64 reduced
bags per step.  The legs of a comparison are interleaved and the medians of the repeats reported.  Prints one JSON line (and writes it to
--out when given).

    python tools/remix_bench.py --repeats 5 --inner 3 [--out profiles/r16_remix.json]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np
import torch

import __graft_entry__
from mil_bench import STREAM_GBS, _interleaved

FEATS, CLASSES, ROWS, K, NITER, SHIFTS = 1024, 2, 10000, 8, 20, 200


def torch_reduce(x, sizes, init, niter):
    """The reduction in plain PyTorch, bag by bag: normalise, niter x (cdist, argmin, index_add_, divide), a final assignment, raw means."""
    protos, off = [], 0
    for s, n in enumerate(sizes):
        xs = x[off:off + n]
        xn = xs / (torch.linalg.vector_norm(xs, dim=1, keepdim=True) + 1e-10)
        cen = xn[init[s] - off]
        for it in range(niter + 1):
            lab = torch.cdist(xn, cen).argmin(1)
            if it == niter:
                break
            cnt = torch.zeros(K, device=x.device).index_add_(0, lab, torch.ones(n, device=x.device))
            cen = torch.zeros_like(cen).index_add_(0, lab, xn) / cnt.clamp(min=1).view(-1, 1)
        cnt = torch.zeros(K, device=x.device).index_add_(0, lab, torch.ones(n, device=x.device))
        protos.append(torch.zeros_like(cen).index_add_(0, lab, xs) / cnt.clamp(min=1).view(-1, 1))
        off += n
    return torch.stack(protos)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--inner", type=int, default=3)
    ap.add_argument("--rows", type=int, default=ROWS)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("remix_bench.py measures on the GPU; none is visible")
    __graft_entry__.build()
    from wsi_hgnn_amd import mil, ops
    from wsi_hgnn_amd.mil import abmil, dsmil, remix

    dev = torch.device("cuda:0")
    torch.manual_seed(611)
    res = {"workload": "ReMix reduction and mixed train step", "feats": FEATS, "rows_per_bag": args.rows, "K": K, "niter": NITER,
           "shift_vectors": SHIFTS, "repeats": args.repeats, "inner": args.inner, "stream_GBs": STREAM_GBS, "step_kernel": {}, "reduce": {},
           "train": {}}

    for B in (1, 8):
        sizes = [args.rows] * B
        n = B * args.rows
        x = torch.randn(n, FEATS, device=dev)
        init = remix.initial_rows(sizes, K, 66, dev)
        cen = remix.normalize_rows(x[init.view(-1)]).view(B, K, FEATS).contiguous()
        # ---- the step kernel alone, per iteration
        legs = {}
        for chunk in (128, 64, 32):
            rp = mil.bag_plan(sizes, dev, chunk=chunk)
            legs[f"update_chunk{chunk}"] = lambda rp=rp: ops.bag_kmeans_step(x, rp, cen, True, True)
            legs[f"assign_chunk{chunk}"] = lambda rp=rp: ops.bag_kmeans_step(x, rp, cen, True, False)
        med, spread = _interleaved(legs, args.repeats, max(args.inner, 20))
        row = {"bytes_rows": n * FEATS * 4, "workgroups_chunk128": ((args.rows + 127) // 128) * B}
        for k, ms in med.items():
            gbs = n * FEATS * 4 / ms / 1e6
            row[k] = {"ms": ms, "GBs": round(gbs, 1), "share_of_stream": round(gbs / STREAM_GBS, 3), "min_max_ms": spread[k]}
        res["step_kernel"][f"B{B}"] = row
        # ---- the whole reduction against plain PyTorch
        plan = mil.bag_plan(sizes, dev)
        plan.row_segment()
        legs = {"hip_reduce_no_shifts_ms": lambda: remix.reduce_bags(x, plan, K, NITER, 66, 0),
                "hip_reduce_with_shifts_ms": lambda: remix.reduce_bags(x, plan, K, NITER, 66, SHIFTS),
                "torch_reduce_no_shifts_ms": lambda: torch_reduce(x, sizes, init, NITER)}
        med, spread = _interleaved(legs, args.repeats, args.inner, warmup=2)
        med["torch_over_hip"] = round(med["torch_reduce_no_shifts_ms"] / med["hip_reduce_no_shifts_ms"], 3)
        med["min_max"] = spread
        a = remix.reduce_bags(x, plan, K, NITER, 66, 0)
        b = torch_reduce(x, sizes, init, NITER)
        med["labels_differ_from_torch"] = "not compared (two float32 orders of the distance sums)"
        med["prototype_max_abs_diff_from_torch"] = float((a.prototypes - b).abs().max())
        res["reduce"][f"B{B}"] = med
        del x, cen, a, b
        torch.cuda.empty_cache()

    # ---- one mixed training step over reduced bags
    bank_bags = 256
    g = torch.Generator(device=dev).manual_seed(612)
    bank = remix.PrototypeBank(torch.randn(bank_bags, K, FEATS, device=dev, generator=g),
                               torch.randn(bank_bags, K, SHIFTS, FEATS, device=dev, generator=g) * 0.1, np.arange(bank_bags) % 2)
    for name in ("dsmil", "abmil"):
        m = (dsmil.MILNet(dsmil.FCLayer(FEATS, CLASSES), dsmil.BClassifier(FEATS, CLASSES)) if name == "dsmil"
             else abmil.BClassifier(FEATS, CLASSES)).to(dev)
        opt = torch.optim.Adam(m.parameters(), lr=1e-4, betas=(0.5, 0.9), weight_decay=1e-4)
        rng = np.random.RandomState(613)
        legs = {}
        for per_step in (8, 64):
            idxs = list(range(per_step))
            legs[f"mixed_step_{per_step}_bags_ms"] = lambda idxs=idxs: remix.train_one_step(m, opt, bank, idxs, "joint", 0.5, rng)
            legs[f"plain_step_{per_step}_bags_ms"] = lambda idxs=idxs: remix.train_one_step(m, opt, bank, idxs, None, 0.5, rng)
        med, spread = _interleaved(legs, args.repeats, max(args.inner, 10))
        med["min_max"] = spread
        res["train"][name] = med

    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
