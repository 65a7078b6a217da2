#!/usr/bin/env python
"""What HGT gains from a per-relation-source plan DERIVED on the device and from captured batch slots (graph.plan_by_relation,
data.BatchSlot(per_relation_src=True) + trainer.CapturedSlotStep) -> profiles/r24_hgt_slot.json.

The reference's regime (configs/COAD/HGT_Kimia_v2.yml): one new slide per step, HGT 1024 -> 200, 4 heads, 2 layers, use_norm, train mode with the
layer's dropout 0.2.  A resident data set of 64 synthetic slides of 6k-12k nodes, batch_size 1 and 2, four legs over the SAME sequence of
batches, in one process, alternating round by round:
  (1) eager, the loader's batch with HGT's plan REBUILT from the batch's COO (graph._build_plan: what every step paid before the derivation);
  (2) eager, the loader's batch with the plan derived from the assembled plan;
  (3) CapturedSlotStep over ONE slot sized for the largest batch;
  (4) CapturedSlotStep over THREE slots by size class.
Every leg has a model and an optimizer of its own (same initial values, wsi_hgnn_amd.optim.Adam(capturable=True)).  A round is one pass over the
batches behind a device synchronise and ends in one.  The eager legs are host-bound, so beside median / fastest / slowest round in wall ms per
step the RATIO of leg 1 to every other leg is reported per round (median and spread).  Also: the plan build of leg 1 and the derivation alone
(wall ms with the device idle; the derivation's device time by events behind a few ms of unrelated work), the derivation's share of a slot's
``load``, the filler's share of the slot's rows, and the one-slot leg with the per-relation source order sorted by out-degree against the rows'
own order (the attention backward walks it).  A GPU is required: nothing is estimated."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from slot_bench import _class_capacities, _stats  # noqa: E402

ND = {"0": 0, "1": 1, "2": 2}


def _ratio(num, den):
    r = [a / b for a, b in zip(num, den)]
    return {"median": round(statistics.median(r), 3), "min": round(min(r), 3), "max": round(max(r), 3)}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--slides", type=int, default=64)
    ap.add_argument("--min-nodes", type=int, default=6000)
    ap.add_argument("--max-nodes", type=int, default=12000)
    ap.add_argument("--in-dim", type=int, default=1024)
    ap.add_argument("--hidden", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--gemm", default="auto", choices=["fp32", "bf16x6", "fp16x3", "auto"])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r24_hgt_slot.json"))
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("tools/hgt_slot_bench.py measures on the GPU; none is visible (nothing is estimated on the CPU)")
    import __graft_entry__
    __graft_entry__.build()
    from wsi_hgnn_amd import graph as G, models, ops, synthetic, optim as O
    from wsi_hgnn_amd.data import BatchSlot, GraphBatchLoader
    from wsi_hgnn_amd.trainer import CapturedSlotStep, apply_loss
    dev = torch.device("cuda:0")
    ops.set_gemm_precision(args.gemm)
    gen = torch.Generator().manual_seed(611)
    sizes = torch.randint(args.min_nodes, args.max_nodes + 1, (args.slides,), generator=gen).tolist()
    graphs = [synthetic.hetero_graph(n, args.in_dim, seed=3000 + i) for i, n in enumerate(sizes)]
    labels = torch.randint(0, 2, (args.slides,), generator=gen).tolist()
    lf = torch.nn.CrossEntropyLoss()
    busy = torch.randn(4096, 4096, device=dev)
    busy_out = torch.empty_like(busy)
    ed = {r: i for i, r in enumerate(graphs[0].canonical_etypes)}
    result = {"workload": f"HGT({args.in_dim} -> {args.hidden}, 2 layers, 4 heads, use_norm, layer dropout 0.2, train mode), {args.slides} synthetic slides of "
                          f"{args.min_nodes}-{args.max_nodes} nodes (mean {sum(sizes) / len(sizes):.0f}), 3 node types, {len(ed)} relations, resident, "
                          f"gemm={args.gemm}, wsi_hgnn_amd.optim.Adam(capturable=True)",
              "device": torch.cuda.get_device_name(0), "rounds": args.rounds, "configs": []}

    def make():
        torch.manual_seed(611)
        m = models.HGT(ND, ed, args.in_dim, args.hidden, 2, 2, 4, use_norm=True, graph_pooling_type="mean").to(dev).train()
        return m, O.Adam(m.parameters(), lr=1e-5, weight_decay=5e-3, capturable=True)

    for bs in (1, 2):
        loader = GraphBatchLoader(graphs, labels, bs, dev, shuffle=False, resident=True)
        order = torch.randperm(args.slides, generator=gen).tolist()
        batches = [order[i:i + bs] for i in range(0, len(order), bs)]

        def eager_round(model, opt, derive):
            G.DERIVE_REL_PLAN = derive
            try:
                for idxs in batches:
                    batch, y = loader._assemble(idxs, 0)[:2]
                    opt.zero_grad(set_to_none=True)
                    loss = apply_loss(lf, model(batch), y)
                    loss.backward()
                    opt.step()
            finally:
                G.DERIVE_REL_PLAN = True

        m_r, o_r = make()
        m_d, o_d = make()
        m1, o1 = make()
        one = CapturedSlotStep(m1, o1, lf, [BatchSlot(loader, per_relation_src=True)], warmup=2)
        m3, o3 = make()
        three = CapturedSlotStep(m3, o3, lf, [BatchSlot(loader, c, per_relation_src=True) for c in _class_capacities(loader, bs, 3)], warmup=2)
        legs = {"eager_rebuilt_plan": lambda: eager_round(m_r, o_r, False), "eager_derived_plan": lambda: eager_round(m_d, o_d, True),
                "one_slot": lambda: [one.step(idxs) for idxs in batches], "three_slots": lambda: [three.step(idxs) for idxs in batches]}
        for fn in legs.values():                             # one untimed pass each: caches, allocator pools
            fn()
        times = {k: [] for k in legs}
        for _ in range(args.rounds):
            for k, fn in legs.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                times[k].append((time.perf_counter() - t0) / len(batches) * 1e3)
        entry = {"batch_size": bs, "steps_per_round": len(batches), "legs": {k: _stats(v) for k, v in times.items()},
                 "ratio_of_eager_rebuilt_to": {k: _ratio(times["eager_rebuilt_plan"], v) for k, v in times.items() if k != "eager_rebuilt_plan"},
                 "ratio_of_eager_derived_to": {k: _ratio(times["eager_derived_plan"], times[k]) for k in ("one_slot", "three_slots")}}
        # the plan alone: rebuilt from the COO against derived, on the loader's batches
        build_wall, derive_wall, derive_dev = [], [], []
        for idxs in batches:
            for derive, wall in ((False, build_wall), (True, derive_wall)):
                G.DERIVE_REL_PLAN = derive
                batch = loader._assemble(idxs, 0)[0]
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                batch.plan(per_relation_src=True)
                torch.cuda.synchronize()
                wall.append((time.perf_counter() - t0) * 1e3)
            G.DERIVE_REL_PLAN = True
            batch = loader._assemble(idxs, 0)[0]
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            for _ in range(3):
                torch.mm(busy, busy, out=busy_out)
            a.record()
            batch.plan(per_relation_src=True)
            b.record()
            torch.cuda.synchronize()
            derive_dev.append(a.elapsed_time(b))
        entry["plan"] = {"rebuilt_from_coo_wall_ms": _stats(build_wall), "derived_wall_ms": _stats(derive_wall), "derived_device_ms": _stats(derive_dev)}
        # the slot's load with and without the derivation, the derivation alone on the slot, and what the filler takes
        for name, step in (("one_slot", one), ("three_slots", three)):
            with_d, without, dev_d, rows, routed = [], [], [], [], [0] * len(step.slots)
            for idxs in batches:
                i = step.slot_for(idxs)
                if i is None:
                    continue
                slot = step.slots[i]
                routed[i] += 1
                for keep, wall in ((slot.rel, with_d), (None, without)):
                    saved, slot.rel = slot.rel, keep
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    slot.load(idxs)
                    torch.cuda.synchronize()
                    wall.append((time.perf_counter() - t0) * 1e3)
                    slot.rel = saved
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                for _ in range(3):
                    torch.mm(busy, busy, out=busy_out)
                a.record()
                slot._derive()
                b.record()
                torch.cuda.synchronize()
                dev_d.append(a.elapsed_time(b))
                rows.append(slot.padded_share()[0])
            entry[name] = {"load_wall_ms": _stats(with_d), "load_without_derivation_wall_ms": _stats(without), "derivation_device_ms": _stats(dev_d),
                           "padded_row_share": round(sum(rows) / len(rows), 4), "batches_per_slot": routed,
                           "slot_rows": [s.layout.N for s in step.slots], "slot_source_rows": [s.layout.hd.rel_rows_total for s in step.slots],
                           "eager_fallbacks_per_round": len(batches) - sum(routed)}
        # the source order of the attention backward: sorted by out-degree (finish_plan's rule) against the rows' own order, one slot, same capture
        slot = one.slots[0]
        order_times = {"sorted": [], "identity": []}
        for _ in range(args.rounds):
            for k in order_times:
                slot.rel_sorted = k == "sorted"
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for idxs in batches:
                    one.step(idxs)
                torch.cuda.synchronize()
                order_times[k].append((time.perf_counter() - t0) / len(batches) * 1e3)
        slot.rel_sorted = False
        entry["one_slot_source_order"] = {k: _stats(v) for k, v in order_times.items()}
        entry["one_slot_source_order"]["ratio_sorted_to_identity"] = _ratio(order_times["sorted"], order_times["identity"])
        result["configs"].append(entry)
        print(json.dumps(entry), flush=True)
        del one, three, m1, m3, m_r, m_d
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
