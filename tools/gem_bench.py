#!/usr/bin/env python
"""Leave-one-node-out batches of the GEM explainers: the host composition against the device builder, in ONE run on one GPU.

Workload of tools/gem_stress.py: HEATNet4 (in 1024, hidden 512, 4 heads), one synthetic 10k-node slide on the collapsed schema, 16 altered graphs
per forward, the first 640 nodes of type '0' (40 batches).  Two builders of the same batch:

  * host   : graph.batch([graph.remove_nodes(g, [i], t) for i in ...])          (what explainers/gem.py did)
  * device : graph.leave_one_out_batch(g, ..., t, tables=...)                    (csrc/loo.hip; tables built once, timed apart)

Per batch and builder, each span between two device synchronisations (host clock): the build alone, ``plan()`` alone, the forward alone; the two
builders alternate batch by batch.  The two forwards of every batch are compared bit for bit.  Then the whole slice end to end, three alternating
rounds: the previous explainer loop (host builder, one read-back per batch) against ``HetGemExplainer`` as it is now (device builder, tables
included, one read-back after the loop); their masks are compared.

Prints one JSON line (and writes it to --out when given).

    python tools/gem_bench.py [--out profiles/r11_gem_loo.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import __graft_entry__


def _span(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, (time.perf_counter() - t0) * 1e3


def _stats(xs):
    return {"median_ms": round(statistics.median(xs), 3), "min_ms": round(min(xs), 3), "max_ms": round(max(xs), 3), "sum_ms": round(sum(xs), 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=10000)
    ap.add_argument("--limit", type=int, default=640)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--in-dim", type=int, default=1024)
    ap.add_argument("--hidden", type=int, default=512)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("gem_bench.py measures on the GPU; none is visible")
    __graft_entry__.build()
    from wsi_hgnn_amd import graph as G, models, synthetic
    from wsi_hgnn_amd.explainers import HetGemExplainer

    dev = torch.device("cuda:0")
    nd = {"0": 0, "1": 1, "2": 2}
    torch.manual_seed(611)
    m = models.HEATNet4(args.in_dim, args.hidden, 2, 2, 4, nd, 0.0, "mean").to(dev).eval()
    g = synthetic.hetero_graph(args.nodes, args.in_dim, seed=611).to(dev)
    label = torch.tensor([1], device=dev)
    ex = HetGemExplainer(g, m, label, batch_size=args.batch)
    gc, t, bs = ex.graph, "0", args.batch
    limit = min(args.limit, gc.num_nodes(t))
    starts = list(range(0, limit, bs))
    res = {"workload": f"HEATNet4 leave-one-node-out forwards on a {args.nodes}-node slide, {bs} altered graphs per forward, first {limit} nodes of type '{t}'",
           "nodes": args.nodes, "edges": gc.num_edges(), "in_dim": args.in_dim, "hidden": args.hidden, "batch": bs, "batches": len(starts), "gemm": "fp32"}

    _, cold = _span(lambda: G.leave_one_out_tables(gc, t))            # the process's first index_add_ launches: code-object loads included
    tables, warm = _span(lambda: G.leave_one_out_tables(gc, t))
    res["tables_once_ms"] = {"first_call": round(cold, 3), "warm": round(warm, 3)}
    builders = {"host": lambda a, b: G.batch([G.remove_nodes(gc, torch.tensor([i]), t) for i in range(a, b)]),
                "device": lambda a, b: G.leave_one_out_batch(gc, range(a, b), t, tables=tables)}
    spans = {k: {"build": [], "plan": [], "forward": []} for k in builders}
    same = True
    with torch.no_grad():
        for k, f in builders.items():           # warm-up: code objects, allocator, GEMM choices for this batch shape
            for a in starts[:2]:
                m(f(a, min(a + bs, limit)))
        for a in starts:
            outs = {}
            for k, f in builders.items():
                bg, dt = _span(lambda: f(a, min(a + bs, limit)))
                spans[k]["build"].append(dt)
                _, dt = _span(bg.plan)
                spans[k]["plan"].append(dt)
                outs[k], dt = _span(lambda: m(bg))
                spans[k]["forward"].append(dt)
            same = same and torch.equal(outs["host"], outs["device"])
    res["forwards_equal_bitwise"] = bool(same)
    res["per_batch"] = {k: {part: _stats(v) for part, v in d.items()} for k, d in spans.items()}
    res["build_host_over_device"] = round(statistics.median(spans["host"]["build"]) / statistics.median(spans["device"]["build"]), 2)

    # ---- the slice end to end: the previous loop against the explainer as it is
    def previous_loop():
        mask = torch.zeros(limit)
        with torch.no_grad():
            loss = ex.loss_fcn(m(gc), label)
            lf = torch.nn.CrossEntropyLoss(reduction="none")
            for a in starts:
                b = min(a + bs, limit)
                bg = G.batch([G.remove_nodes(gc, torch.tensor([i]), t) for i in range(a, b)])
                mask[a:b] = (loss - lf(m(bg), label.expand(b - a))).cpu()
        return mask

    e2e = {"host": [], "device": []}
    masks = {}
    for _ in range(args.rounds):
        masks["host"], dt = _span(previous_loop)
        e2e["host"].append(dt)
        out, dt = _span(lambda: ex._explain([t], limit))
        masks["device"] = out[t]
        e2e["device"].append(dt)
    res["slice_end_to_end_ms"] = {k: {"median": round(statistics.median(v), 1), "min": round(min(v), 1), "all": [round(x, 1) for x in v]} for k, v in e2e.items()}
    res["slice_host_over_device"] = round(statistics.median(e2e["host"]) / statistics.median(e2e["device"]), 2)
    res["masks_max_abs_diff"] = float((masks["host"] - masks["device"]).abs().max())
    res["full_slide_estimate_s"] = {k: round(statistics.median(v) * args.nodes / limit / 1e3, 1) for k, v in e2e.items()}
    res["build_below_host"] = bool(statistics.median(spans["device"]["build"]) < statistics.median(spans["host"]["build"]))
    res["end_to_end_below_host"] = bool(statistics.median(e2e["device"]) < statistics.median(e2e["host"]))
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
