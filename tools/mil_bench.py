#!/usr/bin/env python
"""MIL baselines timing on one GPU: one training step of DSMIL and of ABMIL (feats 1024, 2 classes, bags of 10 000 rows, batches of 1 / 2 / 8
bags, fp32 GEMMs, torch Adam) through the package - all bags of the batch in one step - against the reference's loop restated in plain
PyTorch on the same GPU: one bag per step, so B forward / backward / optimizer steps for the same B bags (model/abmil.py, model/dsmil.py,
train_tcga_k-fold.py:60-84).  The two legs are interleaved and the medians of the repeats reported.  Then the two pooling kernels alone
(HIP events), with the bytes their algorithm has to move over the time against the project's measured streaming rate, for
several chunk sizes of the bag plan.  Prints one JSON line (and writes it to --out when given).

    python tools/mil_bench.py --repeats 7 --inner 5 [--out profiles/r15_mil.json]
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn.functional as F

import __graft_entry__

STREAM_GBS = 6300.0                  # the streaming ceiling this project measured on one MI355X
FEATS, CLASSES, ROWS = 1024, 2, 10000


def _window(fn, inner):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(inner):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / inner


def _interleaved(legs, repeats, inner, warmup=3):
    """{name: median ms per call} of the legs, one window of each per repeat in turn."""
    for fn in legs.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    samples = {k: [] for k in legs}
    for _ in range(repeats):
        for k, fn in legs.items():
            samples[k].append(_window(fn, inner))
    return {k: round(statistics.median(v), 4) for k, v in samples.items()}, {k: [round(min(v), 4), round(max(v), 4)] for k, v in samples.items()}


def torch_abmil(p, x):
    a = F.linear(torch.relu(F.linear(x, p["attention.0.weight"], p["attention.0.bias"])), p["attention.2.weight"], p["attention.2.bias"])
    a = F.softmax(a.t(), dim=1)
    return F.linear(a @ x, p["classifier.0.weight"], p["classifier.0.bias"]).view(1, -1)


def torch_dsmil(p, x):
    c = F.linear(x, p["i_classifier.fc.0.weight"], p["i_classifier.fc.0.bias"])
    V = F.linear(x, p["b_classifier.v.1.weight"], p["b_classifier.v.1.bias"])
    Q = F.linear(x, p["b_classifier.q.weight"], p["b_classifier.q.bias"])
    _, m_idx = torch.sort(c, 0, descending=True)
    q_max = F.linear(torch.index_select(x, 0, m_idx[0, :]), p["b_classifier.q.weight"], p["b_classifier.q.bias"])
    A = F.softmax((Q @ q_max.t()) / torch.sqrt(torch.tensor(Q.shape[1], dtype=torch.float32, device=x.device)), 0)
    B = (A.t() @ V).unsqueeze(0)
    return c, F.conv1d(B, p["b_classifier.fcc.weight"], p["b_classifier.fcc.bias"]).view(1, -1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--inner", type=int, default=5)
    ap.add_argument("--rows", type=int, default=ROWS)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mil_bench.py measures on the GPU; none is visible")
    __graft_entry__.build()
    from wsi_hgnn_amd import _native as N, mil, ops
    from wsi_hgnn_amd.mil import abmil, dsmil

    dev = torch.device("cuda:0")
    torch.manual_seed(611)
    res = {"workload": "MIL train step", "feats": FEATS, "classes": CLASSES, "rows_per_bag": args.rows, "gemm": ops.gemm_precision(),
           "repeats": args.repeats, "inner": args.inner, "stream_GBs": STREAM_GBS, "steps": {}, "kernels": {}}
    bce = torch.nn.BCEWithLogitsLoss()

    for B in (1, 2, 8):
        x = torch.randn(B * args.rows, FEATS, device=dev)
        labels = [i % 2 for i in range(B)]
        targets = mil.bag_targets(labels, CLASSES, dev)
        bags = mil.bag_plan([args.rows] * B, dev)
        bags.row_segment()
        for name in ("dsmil", "abmil"):
            m = (dsmil.MILNet(dsmil.FCLayer(FEATS, CLASSES), dsmil.BClassifier(FEATS, CLASSES)) if name == "dsmil"
                 else abmil.BClassifier_(FEATS, CLASSES)).to(dev)
            opt = torch.optim.Adam(m.parameters(), lr=1e-4, betas=(0.5, 0.9), weight_decay=1e-4)
            params = {k: p.detach().clone().requires_grad_(True) for k, p in m.named_parameters()}
            topt = torch.optim.Adam(list(params.values()), lr=1e-4, betas=(0.5, 0.9), weight_decay=1e-4)

            def hip_step():
                mil.train_one_step(m, opt, x, bags, labels)

            def torch_steps():                                   # the reference's loop: one bag, one optimizer step at a time
                for b in range(B):
                    topt.zero_grad()
                    xb = x[b * args.rows:(b + 1) * args.rows]
                    if name == "dsmil":
                        ins, pred = torch_dsmil(params, xb)
                        loss = 0.5 * bce(pred, targets[b:b + 1]) + 0.5 * bce(ins.max(0)[0].view(1, -1), targets[b:b + 1])
                    else:
                        loss = bce(torch_abmil(params, xb), targets[b:b + 1])
                    loss.backward()
                    topt.step()
            med, spread = _interleaved({"hip_batch_step_ms": hip_step, "torch_bag_loop_ms": torch_steps}, args.repeats, args.inner)
            med["torch_over_hip"] = round(med["torch_bag_loop_ms"] / med["hip_batch_step_ms"], 3)
            med["min_max"] = spread
            res["steps"][f"{name}_B{B}"] = med
            del m, opt, params, topt
        del x
        torch.cuda.empty_cache()

    # the pooling kernels alone: DSMIL's shape (C = 2) and ABMIL's (C = 1), D = 1024
    lib = N.load()
    for B in (1, 8):
        n = B * args.rows
        values = torch.randn(n, FEATS, device=dev)
        for C in (1, 2):
            scores = torch.randn(n, C, device=dev)
            g_out = torch.randn(B, C, FEATS, device=dev)
            out, lse, stats = torch.empty(B, C, FEATS, device=dev), torch.empty(B, C, device=dev), torch.empty(B, C, 2, device=dev)
            g_s, g_v, delta = torch.empty(n, C, device=dev), torch.empty(n, FEATS, device=dev), torch.empty(B * C, device=dev)
            legs = {}
            for chunk in (128, 64, 32):
                rp = mil.bag_plan([args.rows] * B, dev, chunk=chunk)
                partial = torch.empty(rp.num_chunks * C * (FEATS + 2), device=dev)

                def fwd(rp=rp, partial=partial):
                    N.check(lib.wsi_bag_softmax_pool_fwd(N.ptr(scores), C, C, 1.0, N.ptr(values), FEATS, FEATS, N.ptr(rp.chunk_row), rp.num_chunks,
                                                         N.ptr(rp.seg_chunk), rp.num_segs, N.ptr(partial), N.ptr(out), N.ptr(lse), N.ptr(stats),
                                                         N.stream()), "fwd")

                def bwd(rp=rp):
                    N.check(lib.wsi_bag_softmax_pool_bwd(N.ptr(g_out), N.ptr(out), N.ptr(scores), C, C, 1.0, N.ptr(stats), N.ptr(values), FEATS,
                                                         FEATS, N.ptr(rp.chunk_row), N.ptr(rp.chunk_seg), rp.num_chunks, rp.num_segs, N.ptr(delta),
                                                         N.ptr(g_s), C, N.ptr(g_v), FEATS, N.stream()), "bwd")
                legs[f"fwd_chunk{chunk}"], legs[f"bwd_chunk{chunk}"] = fwd, bwd
            med, spread = _interleaved(legs, args.repeats, max(args.inner, 20))
            b_fwd = n * (FEATS + C) * 4 + B * C * FEATS * 4                      # values and scores in, out written
            b_bwd = 2 * n * FEATS * 4 + 2 * n * C * 4                            # values in, g_values out, scores in, g_scores out
            row = {"workgroups_fwd_chunk128": ((args.rows + 127) // 128) * B * (FEATS // 256), "bytes_fwd": b_fwd, "bytes_bwd": b_bwd}
            for k, ms in med.items():
                gbs = (b_fwd if k.startswith("fwd") else b_bwd) / ms / 1e6
                row[k] = {"ms": ms, "GBs": round(gbs, 1), "share_of_stream": round(gbs / STREAM_GBS, 3), "min_max_ms": spread[k]}
            res["kernels"][f"B{B}_C{C}"] = row
        del values
        torch.cuda.empty_cache()

    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
