#!/usr/bin/env python
"""GIN in captured batch slots, and BatchNorm + ReLU over live rows in one pass -> profiles/r30_gin_slot.json.  One run, one GPU:

  pair      one BatchNorm + ReLU pair (ops.masked_batch_norm(relu=True), train mode, all rows live) at 80 000 x 512 and 80 000 x 64, fused
            (wsi_masked_bn_relu_fwd / _bwd) against composite (wsi_masked_bn_fwd, then F.relu), forward alone and forward + backward; the
            two legs alternate window by window (device events), medians reported, with the bytes the algorithm must move over that time
            as a share of the streaming rate the project's other tools report.
  steps     a training step of GIN_COAD (1024 -> 512, 2 layers, 2-layer MLPs, mean neighbours, 'att') over 64 resident synthetic
            homogeneous slides of 6k-12k nodes, one and two slides per step, legs over the same batches alternating round by round
            (tools/slot_bench.py's rounds): eager on the loader's batch, ONE captured slot, THREE captured slots by size class - each with
            the fusion on and off (a capture freezes the switch, so every slot leg has captures of its own).
  coad      the GIN_COAD step of tools/gin_bench.py (8 x 10 000 nodes, torch.optim.Adam, eager) with the fusion on and off.
A GPU is required: nothing is estimated.

    python tools/gin_slot_bench.py [--rounds 5] [--out profiles/r30_gin_slot.json]
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
from att_readout_bench import STREAM_GBS, _interleaved  # noqa: E402

PAIR_ROWS = 80000


def pair_legs(args, dev):
    from wsi_hgnn_amd import ops
    out = []
    for C in (512, 64):
        torch.manual_seed(C)
        x = torch.randn(PAIR_ROWS, C, device=dev, requires_grad=True)
        g = torch.randn(PAIR_ROWS, C, device=dev)
        gamma, beta = (1 + 0.1 * torch.randn(C, device=dev)).requires_grad_(True), (0.1 * torch.randn(C, device=dev)).requires_grad_(True)
        rm, rv = torch.zeros(C, device=dev), torch.ones(C, device=dev)
        live, n = torch.ones(PAIR_ROWS, device=dev), torch.full((1,), float(PAIR_ROWS), device=dev)

        def run(fused, backward):
            ops.set_fused_bn_relu(fused)
            y = ops.masked_batch_norm(x, live, n, gamma, beta, rm, rv, True, 0.1, 1e-5, relu=True)
            if backward:
                x.grad = gamma.grad = beta.grad = None
                y.backward(g)
            return y

        try:
            a, b = run(True, False).detach(), run(False, False).detach()
            table = PAIR_ROWS * C * 4
            entry = {"rows": PAIR_ROWS, "C": C, "table_MB": round(table / 1e6, 1), "the_two_forms_are_bit_equal": bool(torch.equal(a, b))}
            # what the algorithm must move: forward x twice (statistics, normalise) and out once; backward g and x twice each (sums, dx) and dx once
            moved = {"forward": 3 * table, "forward_backward": 8 * table}
            for name, back in (("forward", False), ("forward_backward", True)):
                t = _interleaved({"fused": lambda: run(True, back), "composite": lambda: run(False, back)}, args.repeats, args.inner)
                for leg in t.values():
                    gbs = moved[name] / (leg["median_ms"] * 1e-3) / 1e9
                    leg.update(GB_per_s_of_the_fused_algorithm=round(gbs, 1), share_of_streaming_rate=round(gbs / STREAM_GBS, 3))
                t["bytes_the_fused_algorithm_moves"] = moved[name]
                entry[name] = t
        finally:
            ops.set_fused_bn_relu(True)
        entry["note"] = ("between events, launches back to back, allocation of the outputs included; the composite moves 2 tables more forward "
                         "(F.relu reads y, writes out) and 3 more backward (ReLU's backward reads g and out, writes g'); tables of this size fit "
                         "the 256 MB last-level cache, so a share above 1 would be a cache rate, not an HBM rate")
        out.append(entry)
    return out


def step_legs(args, dev):
    from wsi_hgnn_amd import models, ops, synthetic, optim as O
    from wsi_hgnn_amd.data import BatchSlot, GraphBatchLoader
    from wsi_hgnn_amd.trainer import CapturedSlotStep
    lf = torch.nn.CrossEntropyLoss()
    gen = torch.Generator().manual_seed(611)
    sizes = torch.randint(args.min_nodes, args.max_nodes + 1, (args.slides,), generator=gen).tolist()
    graphs = [synthetic.homogeneous_graph(n, args.in_dim, seed=3000 + i) for i, n in enumerate(sizes)]
    labels = torch.randint(0, 2, (args.slides,), generator=gen).tolist()

    def make():
        torch.manual_seed(611)
        m = models.GIN(args.in_dim, args.hidden, 2, 2, 2, args.dropout, "att", "mean").to(dev).train()
        return m, O.Adam(m.parameters(), lr=1e-5, weight_decay=5e-3, capturable=True)

    def switched(fused, fn):
        def run():
            ops.set_fused_bn_relu(fused)
            try:
                return fn()
            finally:
                ops.set_fused_bn_relu(True)
        return run

    res = {"workload": (f"GIN({args.in_dim}, {args.hidden}, 2 layers, 2-layer MLPs, mean, 'att'), dropout {args.dropout}, train mode, {args.slides} "
                        f"synthetic homogeneous slides of {args.min_nodes}-{args.max_nodes} nodes with self-loops, resident; every leg a model and a "
                        "wsi_hgnn_amd.optim.Adam(capturable=True) of its own; eager = the loader's batch; *_composite = ops.set_fused_bn_relu(False), "
                        "which is what the parent commit's eager step computes"), "configs": []}
    for bs in (1, 2):
        loader = GraphBatchLoader(graphs, labels, bs, dev, shuffle=False, resident=True)
        order = torch.randperm(args.slides, generator=gen).tolist()
        batches = [order[i:i + bs] for i in range(0, len(order), bs)]
        legs, steppers = {}, {}
        for fused in (True, False):
            tag = "" if fused else "_composite"
            m0, o0 = make()
            eager = SB._AllEager(m0, o0, lf, loader)
            m1, o1 = make()
            one = switched(fused, lambda: CapturedSlotStep(m1, o1, lf, BatchSlot(loader), warmup=2))()
            m3, o3 = make()
            three = switched(fused, lambda: CapturedSlotStep(m3, o3, lf, [BatchSlot(loader, c) for c in SB._class_capacities(loader, bs, 3)],
                                                             warmup=2))()
            for name, s in (("eager", eager), ("one_slot", one), ("three_slots", three)):
                steppers[name + tag] = s
                legs[name + tag] = switched(fused, lambda s=s: [s.step(i) for i in batches])
        times = SB._rounds(legs, batches, args.rounds)
        res["configs"].append({"batch_size": bs, "steps_per_round": len(batches), "legs": {k: SB._stats(v) for k, v in times.items()},
                               "replays": {k: s.replays for k, s in steppers.items() if k.find("slot") >= 0},
                               "eager_steps": {k: s.eager_steps for k, s in steppers.items() if k.find("slot") >= 0},
                               "three_slots_node_capacities": [s.layout.N for s in steppers["three_slots"].slots]})
        del legs, steppers, loader
        torch.cuda.empty_cache()
    return res


def coad_step(args, dev):
    """tools/gin_bench.py's (b): one eager GIN_COAD step over 8 x 10 000 nodes, with the fusion on and off."""
    import torch.nn.functional as F
    import wsi_hgnn_amd as W
    from wsi_hgnn_amd import ops, synthetic
    from wsi_hgnn_amd.models import from_config
    cfg = {"name": "GIN", "num_layers": 2, "num_mlp_layers": 2, "in_dim": 1024, "hidden_dim": 512, "out_dim": 2, "feat_drop": 0.2,
           "graph_pooling_type": "att", "neighbor_pooling_type": "mean"}
    G = W.batch([synthetic.homogeneous_graph(10000, 1024, seed=611 + i, self_loops=False) for i in range(8)]).to(dev)
    y = (torch.arange(8) % 2).to(dev)
    steps = {}
    for name, fused in (("fused", True), ("composite", False)):
        torch.manual_seed(611)
        m = from_config(cfg).to(dev).train()
        live = [p for k, p in m.named_parameters() if k not in set(m.dead_parameter_names())]
        opt = torch.optim.Adam(live, lr=5e-4, weight_decay=1e-4)

        def step(m=m, opt=opt, fused=fused):
            ops.set_fused_bn_relu(fused)
            try:
                opt.zero_grad(set_to_none=True)
                F.cross_entropy(m(G), y).backward()
                opt.step()
            finally:
                ops.set_fused_bn_relu(True)
        steps[name] = step
    return {"workload": "GIN_COAD, 8 graphs of 10 000 nodes, torch.optim.Adam, eager, gemm auto", "legs": _interleaved(steps, args.repeats, args.inner)}


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r30_gin_slot.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("gin_slot_bench.py measures on the GPU; none is visible")
    import __graft_entry__
    __graft_entry__.build()
    from wsi_hgnn_amd import ops
    dev = torch.device("cuda:0")
    result = {"device": torch.cuda.get_device_name(0), "gemm": args.gemm, "repeats": args.repeats, "inner": args.inner, "rounds": args.rounds,
              "runs": 1, "streaming_rate_GB_per_s": STREAM_GBS,
              "timing": "pair and coad: device events, ms per call; steps: wall ms per step over a round of all batches between two device synchronisations"}
    ops.set_gemm_precision(args.gemm)
    result["bn_relu_pair"] = pair_legs(args, dev)
    result["gin_coad_slot_step"] = step_legs(args, dev)
    ops.set_gemm_precision("auto")
    result["gin_coad_step"] = coad_step(args, dev)
    ops.set_gemm_precision(args.gemm)
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
