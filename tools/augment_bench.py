#!/usr/bin/env python
"""Train-time graph augmentation timing (transforms.reference_train_transform(): DropNode 0.5, DropEdge 0.5, NodeShuffle, FeatMask 0.5 on 'feat';
DESIGN 3.12) on one GPU, 'auto' GEMMs:

  * one synthetic.hetero_graph(10000, 1024) slide (10k nodes, 80k edges, 41 MB of features), and the bench batch of 8 such slides:
    the fused device path (ops.augment_graph: csrc/augment.hip) against the SAME pipeline in its tensor formulation on the same GPU
    (transforms.py's CPU code run on device tensors, Compose(fused=False)), alternating, with the two results compared bit for bit first;
  * the gather kernel alone (wsi_gather_rows_masked) on the surviving rows of the slide's largest node type and on all 80k rows of a batch-sized
    table, against its byte model rows * F * 4 read + rows * F * 4 written + rows * 8 of indices, and against torch's x[row_of] * keep;
  * the plan build that follows (graph.batch + HeteroGraph.plan) for the augmented and the unaugmented batch of 8;
  * the HEATNet4 training step (hidden 512, 4 heads, dropout 0.2, Adam, cross entropy) on the augmented against the unaugmented batch.

Prints one JSON line (and writes it to --out when given).

    python tools/augment_bench.py --steps 20 --warmup 5 [--out profiles/r09_augment.json]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import __graft_entry__


def _time(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(steps):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / steps


def _alternate(fns, steps, warmup, rounds=3):
    """Each variant ``rounds`` times, interleaved in one process; returns {name: (median, min)} in ms."""
    got = {k: [] for k in fns}
    for r in range(rounds):
        for k, f in fns.items():
            got[k].append(_time(f, steps, warmup if r == 0 else 1))
    return {k: (sorted(v)[len(v) // 2], min(v)) for k, v in got.items()}


def _same(a, b):
    ok = [a.num_nodes(t) for t in a.ntypes] == [b.num_nodes(t) for t in b.ntypes]
    for r in a.canonical_etypes:
        ok = ok and all(torch.equal(x, y) for x, y in zip(a.edges(r), b.edges(r))) and torch.equal(a.edata["sim"][r], b.edata["sim"][r])
    return ok and all(torch.equal(a.nodes[t].data["feat"], b.nodes[t].data["feat"]) for t in a.ntypes)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--nodes", type=int, default=10000)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("augment_bench.py measures on the GPU; none is visible")
    __graft_entry__.build()
    import wsi_hgnn_amd as W
    from wsi_hgnn_amd import models, ops, synthetic, trainer, transforms as TR

    dev = torch.device("cuda:0")
    ops.set_gemm_precision("auto")
    slides = [synthetic.hetero_graph(args.nodes, 1024, seed=611 + i).to(dev) for i in range(args.batch)]
    fused, eager = TR.reference_train_transform(), TR.reference_train_transform()
    eager.fused = False
    res = {"workload": "reference_train_transform()", "nodes": args.nodes, "edges": slides[0].num_edges(), "in_dim": 1024, "batch": args.batch,
           "gemm": "auto", "steps": args.steps, "warmup": args.warmup}
    seeds = list(range(1000, 1000 + args.batch))
    a, b = fused(slides[0], draw=seeds[0]), eager(slides[0], draw=seeds[0])
    res["fused_equals_eager_bitwise"] = bool(_same(a, b))
    res["augmented_slide"] = {"nodes": a.num_nodes(), "edges": a.num_edges()}

    # ---- the pipeline: one slide, and the batch of 8 slides one after another (what the loader does per batch)
    one = _alternate({"fused": lambda: fused(slides[0], draw=seeds[0]), "eager": lambda: eager(slides[0], draw=seeds[0])}, args.steps, args.warmup)
    many = _alternate({"fused": lambda: [fused(g, draw=s) for g, s in zip(slides, seeds)],
                       "eager": lambda: [eager(g, draw=s) for g, s in zip(slides, seeds)]}, max(args.steps // 4, 3), 2)
    res["slide_ms"] = {k: {"median": round(v[0], 4), "min": round(v[1], 4)} for k, v in one.items()}
    res["batch_ms"] = {k: {"median": round(v[0], 4), "min": round(v[1], 4)} for k, v in many.items()}
    res["slide_eager_over_fused"] = round(one["eager"][0] / one["fused"][0], 2)
    res["batch_eager_over_fused"] = round(many["eager"][0] / many["fused"][0], 2)
    ops.enable_kernel_timing(True)
    for _ in range(args.steps):
        fused(slides[0], draw=seeds[0])
    fam = ops.kernel_timing_summary()
    ops.enable_kernel_timing(False)
    res["slide_fused_parts_ms"] = {k: round(v["ms"] / args.steps, 4) for k, v in fam.items() if k.startswith("augment")}   # augment_index holds the read-back

    # ---- the gather kernel against its byte model and against the tensor formulation
    gk = {}
    for name, rows_src, rows in (("slide_type0", slides[0].num_nodes("0"), a.num_nodes("0")), ("batch_table", args.nodes * args.batch, args.nodes * args.batch // 2)):
        x = torch.rand(rows_src, 1024, device=dev)
        row_of = torch.randperm(rows_src, device=dev)[:rows]
        sub, thr = ops.augment_subseed(7, 3, 0), 32768
        keep = (~ops.augment_drawn(1024, sub, thr, dev)).to(torch.float32)
        assert torch.equal(ops.gather_rows_masked(x, row_of, sub, thr), x[row_of] * keep)
        t = _alternate({"hip": lambda: ops.gather_rows_masked(x, row_of, sub, thr), "torch": lambda: x[row_of] * keep}, args.steps, args.warmup)
        model_bytes = rows * 1024 * 4 * 2 + rows * 8
        gk[name] = {"rows": rows, "table_rows": rows_src, "model_MB": round(model_bytes / 1e6, 2),
                    "hip_ms": round(t["hip"][0], 4), "hip_min_ms": round(t["hip"][1], 4), "torch_ms": round(t["torch"][0], 4),
                    "hip_GBs": round(model_bytes / t["hip"][0] / 1e6, 1), "share_of_6.3TBs": round(model_bytes / t["hip"][0] / 1e6 / 6300, 3),
                    "torch_over_hip": round(t["torch"][0] / t["hip"][0], 2)}
        del x, row_of
    res["gather_kernel"] = gk

    # ---- the plan build that follows, and the training step
    aug = [fused(g, draw=s) for g, s in zip(slides, seeds)]

    def build(gs):
        G = W.batch(gs)
        G.plan()
        return G
    pb = _alternate({"augmented": lambda: build(aug), "unaugmented": lambda: build(slides)}, max(args.steps // 2, 3), 2)
    res["batch_and_plan_ms"] = {k: round(v[0], 3) for k, v in pb.items()}
    nd = {"0": 0, "1": 1, "2": 2}
    torch.manual_seed(611)
    gnn = models.HEATNet4(1024, 512, 2, 2, 4, nd, 0.2, "mean").to(dev)
    opt = torch.optim.Adam(gnn.parameters(), lr=1e-5, weight_decay=5e-3)
    loss_fn = torch.nn.CrossEntropyLoss()
    y = torch.tensor([i % 2 for i in range(args.batch)], device=dev)
    Ga, Gu = build(aug), build(slides)
    st = _alternate({"augmented": lambda: trainer.train_one_step(gnn, opt, loss_fn, Ga, y, dev, sync=False),
                     "unaugmented": lambda: trainer.train_one_step(gnn, opt, loss_fn, Gu, y, dev, sync=False)}, args.steps, args.warmup)
    res["train_step_ms"] = {k: {"median": round(v[0], 3), "min": round(v[1], 3)} for k, v in st.items()}
    res["augmented_batch"] = {"nodes": Ga.num_nodes(), "edges": Ga.num_edges()}
    res["per_step_total_ms"] = {"augmented": round(many["fused"][0] + pb["augmented"][0] + st["augmented"][0], 3),
                                "unaugmented_general_route": round(pb["unaugmented"][0] + st["unaugmented"][0], 3)}
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
