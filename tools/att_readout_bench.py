#!/usr/bin/env python
"""The attention readout ('att') as one pass, and what it opens in captured slots -> profiles/r27_att_readout.json.  One run, one GPU:

  readout   pooling.GlobalAttentionPooling over 8 segments of 10 000 rows at D = 1024 and D = 512, fused (ops.attention_readout:
            wsi_attn_readout_fwd / _bwd) against composite (a one-column GEMM, three segmented reductions, an exp and x * (ex / den)), forward
            alone and forward + backward with a gradient for x; the two legs alternate window by window (device events), medians reported.
  kernels   the fused forward and the fused backward (with and without g_x) alone between events, and the bytes their algorithm has to move
            (x once; g_x once) over that time as a share of the streaming rate the project's other tools report.
  steps     a training step of GCN ('att') over 64 homogeneous synthetic slides of 6k-12k nodes, one and two slides per step, three legs over
            the same batches alternating round by round (tools/slot_bench.py's rounds): eager on the loader's batch (composite readout), ONE
            captured slot, THREE captured slots by size class; then HEATNet4 ('att', hidden = in_dim) the same three ways.
A GPU is required: nothing is estimated.

    python tools/att_readout_bench.py [--rounds 5] [--out profiles/r27_att_readout.json]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch  # noqa: E402

import slot_bench as SB  # noqa: E402

STREAM_GBS = 6300.0                  # the streaming ceiling this project measured on one MI355X (tools/mil_bench.py reports against it)
SEGS, ROWS = 8, 10000


def _window(fn, inner):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(inner):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / inner


def _interleaved(legs, repeats, inner, warmup=3):
    """{name: median / fastest / slowest ms per call}, one window of every leg per repeat in turn."""
    for fn in legs.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    samples = {k: [] for k in legs}
    for _ in range(repeats):
        for k, fn in legs.items():
            samples[k].append(_window(fn, inner))
    return {k: SB._stats(v) for k, v in samples.items()}


def readout_legs(args, dev):
    from wsi_hgnn_amd import ops
    from wsi_hgnn_amd.pooling import GlobalAttentionPooling

    class Batch:                                  # what the readouts ask of a batched graph of one node type
        ntypes = ["n"]

        def batch_num_nodes(self, ntype=None):
            return torch.full((SEGS,), ROWS, dtype=torch.int64)

    out = []
    for D in (1024, 512):
        torch.manual_seed(D)
        pool = GlobalAttentionPooling(torch.nn.Linear(D, 1)).to(dev)
        x = torch.randn(SEGS * ROWS, D, device=dev, requires_grad=True)
        g_out = torch.randn(SEGS, D, device=dev)
        graph = Batch()
        rp = ops.ReducePlan.from_ptr([i * ROWS for i in range(SEGS + 1)], dev)

        def run(fused, backward):
            ops.set_fused_attention_readout(fused)
            y = pool(graph, x)
            if backward:
                x.grad = None
                pool.zero_grad(set_to_none=True)
                y.backward(g_out)
            return y

        try:
            a, b = run(True, False).detach(), run(False, False).detach()
            entry = {"D": D, "segments": SEGS, "rows_per_segment": ROWS, "x_MB": round(SEGS * ROWS * D * 4 / 1e6, 1),
                     "max_abs_difference_of_the_two_forms": float((a - b).abs().max()), "largest_entry": float(b.abs().max())}
            entry["forward"] = _interleaved({"fused": lambda: run(True, False), "composite": lambda: run(False, False)}, args.repeats, args.inner)
            entry["forward_backward"] = _interleaved({"fused": lambda: run(True, True), "composite": lambda: run(False, True)}, args.repeats, args.inner)
        finally:
            ops.set_fused_attention_readout(False)
        # the kernels alone, and their share of the streaming rate
        w, bias = pool.gate_nn.weight.detach().reshape(-1).contiguous(), pool.gate_nn.bias.detach()
        xd = x.detach()
        y, gate, stats = ops._attn_readout_forward(xd, w, bias, rp)
        legs = {"forward": (lambda: ops._attn_readout_forward(xd, w, bias, rp), 1),
                "backward": (lambda: ops._attn_readout_backward(g_out, y, gate, stats, xd, w, rp, True), 2),
                "backward_without_g_x": (lambda: ops._attn_readout_backward(g_out, y, gate, stats, xd, w, rp, False), 1)}
        entry["kernels"] = {}
        for name, (fn, passes) in legs.items():
            ms = _interleaved({name: fn}, args.repeats, 4 * args.inner)[name]
            byts = passes * SEGS * ROWS * D * 4
            gbs = byts / (ms["median_ms"] * 1e-3) / 1e9
            entry["kernels"][name] = {**ms, "bytes_the_algorithm_moves": byts, "GB_per_s": round(gbs, 1),
                                      "share_of_streaming_rate": round(gbs / STREAM_GBS, 3)}
        entry["kernels"]["note"] = ("between events, launches back to back, allocation of the outputs included: an upper bound of the kernels' own "
                                    "time; bytes = x once (forward, backward without g_x) or x and g_x once each; at these sizes x fits the 256 MB "
                                    "last-level cache, so a share above 1 would be a cache rate, not an HBM rate")
        out.append(entry)
    return out


def step_legs(args, dev, name):
    from wsi_hgnn_amd import graph as G_, models, ops, synthetic, optim as O
    from wsi_hgnn_amd.data import BatchSlot, GraphBatchLoader
    from wsi_hgnn_amd.trainer import CapturedSlotStep
    lf = torch.nn.CrossEntropyLoss()
    in_dim = args.in_dim if name == "GCN" else args.hidden                 # HEATNet4 applies the first gate to its hidden states: hidden = in_dim
    gen = torch.Generator().manual_seed(611)
    sizes = torch.randint(args.min_nodes, args.max_nodes + 1, (args.slides,), generator=gen).tolist()
    graphs = [synthetic.hetero_graph(n, in_dim, seed=3000 + i) for i, n in enumerate(sizes)]
    if name == "GCN":
        graphs = [G_.to_homogeneous(g, add_self_loop=True) for g in graphs]
    labels = torch.randint(0, 2, (args.slides,), generator=gen).tolist()

    def make():
        torch.manual_seed(611)
        if name == "GCN":
            m = models.GCN(in_dim, args.hidden, 2, 2, torch.nn.functional.relu, args.dropout, "att")
        else:
            m = models.HEATNet4(in_dim, args.hidden, 2, 2, 4, SB.ND, args.dropout, "att")
        m = m.to(dev).train()
        return m, O.Adam(m.parameters(), lr=1e-5, weight_decay=5e-3, capturable=True)

    res = {"workload": (f"{name}({in_dim}, {args.hidden}, 2 layers, 'att'), dropout {args.dropout}, train mode, {args.slides} synthetic slides of "
                        f"{args.min_nodes}-{args.max_nodes} nodes" + (" as graph.to_homogeneous output with self-loops" if name == "GCN" else "") +
                        ", resident; every leg a model and a wsi_hgnn_amd.optim.Adam(capturable=True) of its own; eager = the loader's batch, "
                        "composite readout; slots = fused readout from the slot's tables"), "configs": []}
    for bs in (1, 2):
        loader = GraphBatchLoader(graphs, labels, bs, dev, shuffle=False, resident=True)
        order = torch.randperm(args.slides, generator=gen).tolist()
        batches = [order[i:i + bs] for i in range(0, len(order), bs)]
        m0, o0 = make()
        eager = SB._AllEager(m0, o0, lf, loader)
        m1, o1 = make()
        one = CapturedSlotStep(m1, o1, lf, BatchSlot(loader), warmup=2)
        m3, o3 = make()
        three = CapturedSlotStep(m3, o3, lf, [BatchSlot(loader, c) for c in SB._class_capacities(loader, bs, 3)], warmup=2)
        legs = {"eager": lambda: [eager.step(i) for i in batches], "one_slot": lambda: [one.step(i) for i in batches],
                "three_slots": lambda: [three.step(i) for i in batches]}
        times = SB._rounds(legs, batches, args.rounds)
        res["configs"].append({"batch_size": bs, "steps_per_round": len(batches), "legs": {k: SB._stats(v) for k, v in times.items()},
                               "one_slot": {"replays": one.replays, "eager_steps": one.eager_steps},
                               "three_slots": {"replays": three.replays, "eager_steps": three.eager_steps,
                                               "node_capacities": [s.layout.N for s in three.slots]}})
        del eager, one, three, loader
        torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--inner", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--slides", type=int, default=64)
    ap.add_argument("--min-nodes", type=int, default=6000)
    ap.add_argument("--max-nodes", type=int, default=12000)
    ap.add_argument("--in-dim", type=int, default=1024)
    ap.add_argument("--hidden", type=int, default=512)
    ap.add_argument("--dropout", type=float, default=0.2)
    ap.add_argument("--gemm", default="fp32")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r27_att_readout.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("att_readout_bench.py measures on the GPU; none is visible")
    import __graft_entry__
    __graft_entry__.build()
    from wsi_hgnn_amd import ops
    dev = torch.device("cuda:0")
    ops.set_gemm_precision(args.gemm)
    result = {"device": torch.cuda.get_device_name(0), "gemm": args.gemm, "repeats": args.repeats, "inner": args.inner, "rounds": args.rounds,
              "streaming_rate_GB_per_s": STREAM_GBS, "timing": "readout and kernels: device events, ms per call; steps: wall ms per step over a round "
              "of all batches between two device synchronisations"}
    result["readout"] = readout_legs(args, dev)
    result["gcn_att_step"] = step_legs(args, dev, "GCN")
    result["heatnet4_att_step"] = step_legs(args, dev, "HEATNet4")
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
