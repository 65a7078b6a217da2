#!/usr/bin/env python
"""What an evaluation pass costs eagerly and replayed (trainer.CapturedSlotEval + metrics.EpochMetrics) -> profiles/r14_captured_eval.json.

The reference evaluates the test and the validation set after every epoch, one slide at a time (trainer/train_gnn.py:110-115).  The data set and
the model are tools/slot_bench.py's: HEATNet4 at the benchmark's model size over 64 resident synthetic slides of 6k-12k nodes; batch_size 1 and 2;
three legs over the SAME model, in one process, alternating round by round:
  (i)   eager: ``io.evaluate`` - the forward launch by launch, every batch's logits kept, the metrics on the host - the yardstick;
  (ii)  ``CapturedSlotEval`` over ONE slot sized for the largest batch;
  (iii) ``CapturedSlotEval`` over THREE slots by size class.
A round is one whole pass (fills, replays, finalize, the one read-back) behind a device synchronise; reported: median / fastest / slowest round in
wall ms per pass and per batch.  Separately: the device time of ``update`` and of ``finalize`` at n = 64 and n = 4096 rows (C = 4; by events over
back-to-back calls queued behind a few ms of unrelated work), and what a ``CapturedSlotStep`` replay costs with and without ``metrics=``.
A GPU is required: nothing is estimated."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch  # noqa: E402

ND = {"0": 0, "1": 1, "2": 2}


def _stats(v):
    return {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)}


def _alternate(legs, rounds, per):
    for fn in legs.values():                                 # one untimed pass each: caches, allocator pools
        fn()
    times = {k: [] for k in legs}
    for _ in range(rounds):
        for k, fn in legs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            times[k].append((time.perf_counter() - t0) / per * 1e3)
    return times


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--slides", type=int, default=64)
    ap.add_argument("--min-nodes", type=int, default=6000)
    ap.add_argument("--max-nodes", type=int, default=12000)
    ap.add_argument("--in-dim", type=int, default=1024)
    ap.add_argument("--hidden", type=int, default=512)
    ap.add_argument("--rounds", type=int, default=11)
    ap.add_argument("--gemm", default="auto", choices=["fp32", "bf16x6", "fp16x3", "auto"])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r14_captured_eval.json"))
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("tools/eval_bench.py measures on the GPU; none is visible (nothing is estimated on the CPU)")
    import __graft_entry__
    __graft_entry__.build()
    from slot_bench import _class_capacities
    from wsi_hgnn_amd import _native as N, io, models, ops, synthetic, optim as O
    from wsi_hgnn_amd.data import BatchSlot, GraphBatchLoader
    from wsi_hgnn_amd.metrics import EpochMetrics
    from wsi_hgnn_amd.trainer import CapturedSlotEval, CapturedSlotStep
    dev = torch.device("cuda:0")
    ops.set_gemm_precision(args.gemm)
    gen = torch.Generator().manual_seed(611)
    sizes = torch.randint(args.min_nodes, args.max_nodes + 1, (args.slides,), generator=gen).tolist()
    graphs = [synthetic.hetero_graph(n, args.in_dim, seed=3000 + i) for i, n in enumerate(sizes)]
    labels = torch.randint(0, 2, (args.slides,), generator=gen).tolist()
    result = {"workload": f"HEATNet4({args.in_dim}, {args.hidden}, 2 layers, 4 heads), {args.slides} synthetic slides of {args.min_nodes}-{args.max_nodes} nodes "
                          f"(mean {sum(sizes) / len(sizes):.0f}), resident, gemm={args.gemm}, eval mode, no_grad",
              "device": torch.cuda.get_device_name(0), "rounds": args.rounds, "evaluation": [], "kernels": [], "training_step": None}
    torch.manual_seed(611)
    model = models.HEATNet4(args.in_dim, args.hidden, 2, 2, 4, ND, 0.2, "mean").to(dev).eval()

    # ---- an evaluation pass
    for bs in (1, 2):
        loader = GraphBatchLoader(graphs, labels, bs, dev, shuffle=False, resident=True)
        one = CapturedSlotEval(model, [BatchSlot(loader)], warmup=2)
        three = CapturedSlotEval(model, [BatchSlot(loader, c) for c in _class_capacities(loader, bs, 3)], warmup=2)
        out = {}
        legs = {"eager": lambda: out.__setitem__("eager", io.evaluate(model, loader)),
                "one_slot": lambda: out.__setitem__("one_slot", one.evaluate()),
                "three_slots": lambda: out.__setitem__("three_slots", three.evaluate())}
        nb = len(one.batches())
        times = _alternate(legs, args.rounds, 1)
        entry = {"batch_size": bs, "batches_per_pass": nb, "legs_ms_per_pass": {k: _stats(v) for k, v in times.items()},
                 "legs_ms_per_batch": {k: round(statistics.median(v) / nb, 4) for k, v in times.items()},
                 "results": {k: {m_: (None if v != v else round(v, 6)) for m_, v in r.items()} for k, r in out.items()},
                 "slot_rows": {"one_slot": [s.layout.N for s in one.slots], "three_slots": [s.layout.N for s in three.slots]},
                 "eager_fallbacks_per_pass": {"one_slot": one.eager_runs // (args.rounds + 1), "three_slots": three.eager_runs // (args.rounds + 1)}}
        e_ms = entry["legs_ms_per_pass"]["eager"]["median_ms"]
        entry["speedup_one_slot"] = round(e_ms / entry["legs_ms_per_pass"]["one_slot"]["median_ms"], 3)
        entry["speedup_three_slots"] = round(e_ms / entry["legs_ms_per_pass"]["three_slots"]["median_ms"], 3)
        result["evaluation"].append(entry)
        print(json.dumps(entry), flush=True)
        del one, three
        torch.cuda.empty_cache()

    # ---- the two entry points alone: device time by events, queued behind unrelated work
    busy = torch.randn(4096, 4096, device=dev)
    busy_out = torch.empty_like(busy)

    def device_us(fn, calls=50, repeats=5):
        best = []
        for _ in range(repeats):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            for _ in range(3):
                torch.mm(busy, busy, out=busy_out)
            a.record()
            for _ in range(calls):
                fn()
            b.record()
            torch.cuda.synchronize()
            best.append(a.elapsed_time(b) / calls * 1e3)
        return round(statistics.median(best), 3)

    C = 4
    for n in (64, 4096):
        em = EpochMetrics(C, n + 2 * 50 * 5 + 16, dev)
        x = torch.randn(n, C, generator=torch.Generator().manual_seed(n)).to(dev)
        y = torch.randint(0, C, (n,), generator=torch.Generator().manual_seed(n + 1)).to(dev)
        em.update(x, y)
        x2, y2 = x[:2].contiguous(), y[:2].contiguous()
        em.result_block()
        fin = lambda: N.load().wsi_metrics_finalize(N.ptr(em.state), N.ptr(em.probs), N.ptr(em.row_labels), C, em.capacity, N.ptr(em._partials),
                                                    N.ptr(em.result), N.stream())
        f_us = device_us(fin)                                # (before the timed updates move n)
        u_us = device_us(lambda: em.update(x2, y2))
        entry = {"n": n, "classes": C, "capacity": em.capacity, "finalize_device_us": f_us, "update_2_rows_device_us": u_us}
        result["kernels"].append(entry)
        print(json.dumps(entry), flush=True)

    # ---- a captured training step with and without metrics=
    lf = torch.nn.CrossEntropyLoss()
    loader = GraphBatchLoader(graphs, labels, 1, dev, shuffle=False, resident=True)
    order = torch.randperm(args.slides, generator=gen).tolist()
    batches = [[i] for i in order]

    def make():
        torch.manual_seed(611)
        m = models.HEATNet4(args.in_dim, args.hidden, 2, 2, 4, ND, 0.0, "mean").to(dev).train()
        return m, O.Adam(m.parameters(), lr=1e-5, weight_decay=5e-3, capturable=True)

    m0, o0 = make()
    plain = CapturedSlotStep(m0, o0, lf, [BatchSlot(loader)], warmup=2)
    m1, o1 = make()
    tm = EpochMetrics(2, args.slides, dev)
    with_m = CapturedSlotStep(m1, o1, lf, [BatchSlot(loader)], warmup=2, metrics=tm)

    def metered():
        tm.reset()
        for idxs in batches:
            with_m.step(idxs)

    times = _alternate({"plain": lambda: [plain.step(idxs) for idxs in batches], "with_metrics": metered}, args.rounds, len(batches))
    result["training_step"] = {"batch_size": 1, "feat_drop": 0.0, "steps_per_round": len(batches), "ms_per_step": {k: _stats(v) for k, v in times.items()},
                               "epoch_training_metrics": {k: (None if v != v else round(v, 6)) for k, v in tm.compute().items()}}
    print(json.dumps(result["training_step"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
