#!/usr/bin/env python
"""GIN timing on one GPU.  Prints one JSON line (and writes it to --out when given).

(a) the aggregation kernels alone on a batch of 8 x 10 000 nodes with 8 in-edges per node (synthetic.homogeneous_graph without self loops),
    D = 512 and 1024, mean and max, forward and backward, against the same result composed from the kernels the tree had before -
    ``wsi_spmm_sum`` (mean: the degree as its output scale) / ``wsi_csr_gather_max_*`` - plus the tensor operations for the (1 + eps) x self
    term; bytes gathered per unit time (one row per edge) against the 8.0 TB/s that tools/ubench/gather_rate.hip established;
(b) one training step of the reference's GIN_COAD config (1024 -> 512, num_layers 2, 2-layer MLPs, mean neighbours, 'att' readout, Adam
    lr 5e-4 weight decay 1e-4, 'auto' GEMMs): native, the aggregation through ``ops.gin_aggregate_reference`` on the same GPU
    (``kernels=False``), and projection-first off.

Every figure is the median of --repeats timings of --steps calls each (HIP events around the batch of calls), after --warmup calls; the
legs that are compared are timed in alternating rounds of one process; the smallest and largest repeat are kept next to the median.

    python tools/gin_bench.py --steps 10 --warmup 3 --repeats 5 [--out profiles/r29_gin.json]
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

GATHER_CEILING_GBS = 8000.0          # tools/ubench/gather_rate.hip: random whole-row gathers beyond L2, chip-wide


def _time(fns, steps, warmup, repeats):
    """{name: timing} of the callables in ``fns``, timed in alternating rounds: every round times ``steps`` calls of each, in turn."""
    for fn in fns.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in fns}
    for _ in range(repeats):
        for k, fn in fns.items():
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(steps):
                fn()
            t1.record()
            torch.cuda.synchronize()
            ms[k].append(t0.elapsed_time(t1) / steps)
    return {k: {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)} for k, v in ms.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--graphs", type=int, default=8)
    ap.add_argument("--nodes", type=int, default=10000)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("gin_bench.py measures on the GPU; none is visible")
    __graft_entry__.build()
    import wsi_hgnn_amd as W
    from wsi_hgnn_amd import _native as N, ops, synthetic
    from wsi_hgnn_amd.models import from_config
    from wsi_hgnn_amd.models.GCN import homo_plan

    dev = torch.device("cuda:0")
    ops.set_gemm_precision("auto")
    torch.manual_seed(611)
    T = lambda fns: _time(fns, args.steps, args.warmup, args.repeats)
    res = {"workload": "GIN aggregation kernels and GIN_COAD train step", "graphs": args.graphs, "steps": args.steps, "warmup": args.warmup,
           "repeats": args.repeats, "gather_ceiling_GBs": GATHER_CEILING_GBS, "kernels": [], "train_step": {}}

    # ---------------------------------------------------------------- (a) the aggregation alone
    Gk = W.batch([synthetic.homogeneous_graph(args.nodes, 4, seed=611 + i, self_loops=False) for i in range(args.graphs)]).to(dev)
    hp = homo_plan(Gk)
    n, E = hp.num_nodes, hp.num_edges
    res["nodes"], res["edges"] = n, E
    lib = N.load()
    eps = torch.full((1,), 0.3, device=dev)
    inv_deg = (1.0 / (hp.rowptr[1:n + 1] - hp.rowptr[:n]).clamp(min=1).float()).contiguous()
    for D in (512, 1024):
        x, g = torch.randn(n, D, device=dev), torch.randn(n, D, device=dev)
        out, gx = torch.empty(n, D, device=dev), torch.empty(n, D, device=dev)
        arg = torch.empty(n, D, dtype=torch.int32, device=dev)
        for mode in ("mean", "max"):
            code = ops.GIN_MODES[mode]

            def fwd():
                N.check(lib.wsi_gin_aggregate_fwd(N.ptr(x), D, n, D, N.ptr(hp.rowptr), N.ptr(hp.src), None, N.ptr(eps), code, None, N.ptr(out), D,
                                                  N.ptr(arg) if mode == "max" else None, N.stream()), "fwd")

            def bwd():
                N.check(lib.wsi_gin_aggregate_bwd(N.ptr(g), D, n, D, N.ptr(hp.rowptr), N.ptr(hp.colptr), N.ptr(hp.csc_eid), N.ptr(hp.csc_dst), None,
                                                  N.ptr(eps), code, N.ptr(arg) if mode == "max" else None, N.ptr(gx), D, N.stream()), "bwd")

            def old_fwd():
                if mode == "mean":
                    N.check(lib.wsi_spmm_sum(N.ptr(x), D, n, D, N.ptr(hp.rowptr), N.ptr(hp.src), None, None, N.ptr(inv_deg), None, 0, None, 0,
                                             N.ptr(out), D, N.stream()), "spmm")
                else:
                    N.check(lib.wsi_csr_gather_max_fwd(N.ptr(x), D, n, D, N.ptr(hp.rowptr), N.ptr(hp.src), N.ptr(out), D, N.ptr(arg), N.stream()), "max")
                return torch.addcmul(out, x, 1 + eps)

            def old_bwd():
                if mode == "mean":
                    N.check(lib.wsi_spmm_sum(N.ptr(g), D, n, D, N.ptr(hp.colptr), N.ptr(hp.csc_dst), None, N.ptr(inv_deg), None, None, 0, None, 0,
                                             N.ptr(gx), D, N.stream()), "spmm")
                else:
                    N.check(lib.wsi_csr_gather_max_bwd(N.ptr(g), D, N.ptr(arg), n, D, N.ptr(hp.colptr), N.ptr(hp.csc_eid), N.ptr(hp.csc_dst),
                                                       N.ptr(gx), D, N.stream()), "max")
                return torch.addcmul(gx, g, 1 + eps)

            fwd()
            mine = out.clone()
            theirs = old_fwd()
            agree = float((mine - theirs).abs().max() / theirs.abs().max())
            row = D * 4
            rec = {"D": D, "mode": mode, "fwd_agrees_rel": agree}
            times = T({"fwd": fwd, "composite_fwd": old_fwd, "bwd": bwd, "composite_bwd": old_bwd})
            for name, t in times.items():
                gathered = E * row * (2 if (name.endswith("bwd") and mode == "max") else 1)       # one row per edge (bwd under max: g and arg)
                rec[name] = dict(t, gathered_GBs=round(gathered / t["median_ms"] / 1e6, 1),
                                 share_of_ceiling=round(gathered / t["median_ms"] / 1e6 / GATHER_CEILING_GBS, 3))
            res["kernels"].append(rec)
        del x, g, out, gx, arg
        torch.cuda.empty_cache()

    # ---------------------------------------------------------------- (b) one training step of GIN_COAD
    cfg = {"name": "GIN", "num_layers": 2, "num_mlp_layers": 2, "in_dim": 1024, "hidden_dim": 512, "out_dim": 2, "feat_drop": 0.2,
           "graph_pooling_type": "att", "neighbor_pooling_type": "mean"}
    G = W.batch([synthetic.homogeneous_graph(args.nodes, 1024, seed=611 + i, self_loops=False) for i in range(args.graphs)]).to(dev)
    y = (torch.arange(args.graphs) % 2).to(dev)
    native = ops.gin_aggregate
    legs = {"native": (True, native), "project_first_off": (False, native),
            "aggregation_in_tensor_ops": (True, lambda *a, **k: native(*a, **dict(k, kernels=False)))}
    steps = {}
    for name, (first, agg) in legs.items():
        torch.manual_seed(611)
        m = from_config(cfg).to(dev).train()
        live = [p for k, p in m.named_parameters() if k not in set(m.dead_parameter_names())]
        opt = torch.optim.Adam(live, lr=5e-4, weight_decay=1e-4)

        def step(m=m, opt=opt, first=first, agg=agg):
            ops.set_gin_project_first(first)
            ops.gin_aggregate = agg
            try:
                opt.zero_grad(set_to_none=True)
                F.cross_entropy(m(G), y).backward()
                opt.step()
            finally:
                ops.gin_aggregate = native
                ops.set_gin_project_first(True)
        steps[name] = step
    res["train_step"] = T(steps)
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
