#!/usr/bin/env python
"""What replaying ONE captured step over new slides costs (data.BatchSlot + trainer.CapturedSlotStep) -> profiles/r12_slot_step.json.

The reference's regime: one or two new slides per step (trainer/train_gnn.py:48-79).  HEATNet4 at the benchmark's model size over a resident data
set of 64 synthetic slides of 6k-12k nodes, batch_size 1 and 2, feat_drop 0 and 0.2 (train mode), three legs over the SAME sequence of batches, in
one process, alternating round by round:
  (i)   eager: the loader's assembled batch (graph.assemble_plan), forward, loss, backward, optimizer step - the yardstick;
  (ii)  CapturedSlotStep over ONE slot sized for the largest batch;
  (iii) CapturedSlotStep over THREE slots by size class.
Every leg has a model and an optimizer of its own (same initial values, wsi_hgnn_amd.optim.Adam(capturable=True)).  A round is one pass over the
batches behind a device synchronise and ends in one; reported: median / fastest / slowest round in wall ms per step, the fill alone (wall ms per
``slot.load`` with the device idle - host arithmetic, upload and kernel - and the device time of upload + kernel by events, queued behind a few ms
of unrelated work), the share of the slot's rows and edges the filler takes, and which
slot the batches went to.  A GPU is required: nothing is estimated.

``--augment`` (profiles/r13_slot_augment.json is its record before the quota legs): the same data set, rounds and alternation with the reference's training pipeline
(``transforms.reference_train_transform()``) on the loader.  The yardstick leg is then the only way to train augmented without slots -
``GraphBatchLoader(transform=...)``'s batch (fused device augmentation, one read-back per slide, ``graph.batch``, ``plan()``) stepped eagerly - and
the slots draw the augmentation on the device in front of every replay; also reported: the kernel launches of one fill (torch.profiler) and the
filler's share from ``BatchSlot.counts()``, read outside the timed windows.

``--augment`` also runs the QUOTA legs -> profiles/r25_slot_quota.json by default: ``BatchSlot(quota="bound")`` sized for the draw
instead of for the stored slides, one slot and three slots by size class, in the same alternating rounds as the stored-capacity legs (which are
the ``quota=None`` code path, unchanged); reported beside them, with the overflow count over the whole run (expected 0).

``--type-mask`` -> profiles/r26_slot_type_mask.json: slots with a device-side presence table (``BatchSlot(type_mask=True)``).
COST: on the slides, model and pipeline of the quota legs above (three quota slots by size class, augmented), ms per replayed step with and
without ``type_mask`` in the same alternating rounds, and beside the difference the device time of the launches the table adds (the presence
kernel behind the fill, the heads' multiply forward and backward), each timed back to back between events.  REACH: a six-type synthetic cohort
with one rare type - a quarter of the slides hold none of it, half of them fewer than 32 nodes; the generator's parameters are in the JSON -
plain and under ``--augment --quota``-style slots: the share of an epoch's steps that is replayed and the ms per step over the epoch, default
slots against ``type_mask`` slots, again alternating round by round."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

ND = {"0": 0, "1": 1, "2": 2}


def _stats(v):
    return {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)}


def _class_capacities(loader, batch_size, classes):
    """Capacities of `classes` slots by slide size: slot k holds any `batch_size` slides out of the smallest (k + 1) / classes of the data set."""
    its = sorted(loader.items, key=lambda it: sum(it.num_nodes))
    T = len(its[0].num_nodes)
    caps = []
    for k in range(classes):
        part = its[:max(batch_size, (len(its) * (k + 1) + classes - 1) // classes)]
        top = lambda xs: sum(sorted(xs, reverse=True)[:batch_size])
        caps.append(([top([it.num_nodes[t] for it in part]) + 1 for t in range(T)], [top([it.pieces.ecount[t] for it in part]) for t in range(T)], batch_size))
    return caps


def _quota_class_capacities(loader, batch_size, classes):
    """``_class_capacities`` from the slides' "bound" quotas (data.slot_quota_bound) instead of their stored counts."""
    from wsi_hgnn_amd.data import slot_augment_spec, slot_quota_bound
    spec = slot_augment_spec(loader.transform)
    its = sorted(loader.items, key=lambda it: sum(it.num_nodes))
    T = len(its[0].num_nodes)
    tix = {t: i for i, t in enumerate(its[0].ntypes)}
    dst = [tix[r[2]] for r in its[0].rels]
    q = {id(it): slot_quota_bound(it, spec) for it in its}
    by_dst = lambda it, t: sum(x for x, d in zip(q[id(it)][1], dst) if d == t)
    caps = []
    for k in range(classes):
        part = its[:max(batch_size, (len(its) * (k + 1) + classes - 1) // classes)]
        top = lambda xs: sum(sorted(xs, reverse=True)[:batch_size])
        caps.append(([top([q[id(it)][0][t] for it in part]) + 1 for t in range(T)], [top([by_dst(it, t) for it in part]) for t in range(T)], batch_size))
    return caps


def _usable(slots):
    """The slots at least one slide of the data set fits alone (a default augmented slot over small slides may take none)."""
    return [s for s in slots if any(s.fits([j]) for j in sorted(s.members))]


class _AllEager:
    """What a leg whose slots take no slide of the data set amounts to: every batch through the loader's ordinary route, stepped eagerly."""

    def __init__(self, gnn, optimizer, loss_fcn, loader):
        self.gnn, self.optimizer, self.loss_fcn, self.loader = gnn, optimizer, loss_fcn, loader
        self.slots, self.replays, self.eager_steps = [], 0, 0

    def overflows(self):
        return 0

    def step(self, idxs):
        from wsi_hgnn_amd.trainer import apply_loss
        G, y = self.loader._augmented(idxs) if self.loader.transform is not None else self.loader._assemble(idxs, 0)[:2]
        self.optimizer.zero_grad(set_to_none=True)
        loss = apply_loss(self.loss_fcn, self.gnn(G), y)
        loss.backward()
        self.optimizer.step()
        self.eager_steps += 1
        return loss


def _rounds(legs, batches, rounds):
    """One untimed pass of every leg, then ``rounds`` alternating timed passes: wall ms per step, per leg."""
    for fn in legs.values():
        fn()
    times = {k: [] for k in legs}
    for _ in range(rounds):
        for k, fn in legs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            times[k].append((time.perf_counter() - t0) / len(batches) * 1e3)
    return times


def _back_to_back_ms(fn, n=200):
    """Device ms per call of ``fn`` queued ``n`` times back to back between two events, behind unrelated work (an upper bound of the kernels'
    own time: it includes the gaps between launches)."""
    dev = torch.device("cuda:0")
    busy = torch.randn(2048, 2048, device=dev)
    for _ in range(10):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    for _ in range(4):
        torch.mm(busy, busy)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / n


RARE = {"types": 6, "common_fractions": [0.35, 0.25, 0.17, 0.13, 0.10], "p_none": 0.25, "p_few": 0.5, "few_nodes": [1, 31], "many_nodes": [32, 200],
        "relations": "per node type t: (t, pos, t) and ((t + 1) mod 6, neg, t); 4 edges per destination node and relation", "seed": 611}


def _rare_cohort(synthetic, slides, min_nodes, max_nodes, in_dim):
    """Six node types, the last one rare: per slide none of it (p_none), 1-31 nodes (p_few) or 32-200."""
    gen = torch.Generator().manual_seed(RARE["seed"])
    T = RARE["types"]
    rels = sorted([(str(t), "pos", str(t)) for t in range(T)] + [(str((t + 1) % T), "neg", str(t)) for t in range(T)])
    graphs, rare = [], []
    for i in range(slides):
        n = int(torch.randint(min_nodes, max_nodes + 1, (1,), generator=gen))
        u = float(torch.rand(1, generator=gen))
        lo, hi = RARE["few_nodes"] if u < RARE["p_none"] + RARE["p_few"] else RARE["many_nodes"]
        k = 0 if u < RARE["p_none"] else int(torch.randint(lo, hi + 1, (1,), generator=gen))
        fr = [f * (1.0 - k / n) for f in RARE["common_fractions"]] + [k / n]
        g = synthetic.hetero_graph(n, in_dim, seed=5000 + i, fractions=fr, relations=rels)
        assert g.num_nodes(str(T - 1)) == k
        graphs.append(g)
        rare.append(k)
    labels = torch.randint(0, 2, (slides,), generator=gen).tolist()
    return graphs, labels, rare


def type_mask_main(args):
    """``--type-mask``: the cost and the reach of slots with a presence table -> profiles/r26_slot_type_mask.json."""
    import __graft_entry__
    __graft_entry__.build()
    from wsi_hgnn_amd import graph as G_, models, ops, synthetic, transforms, optim as O
    from wsi_hgnn_amd.data import BatchSlot, GraphBatchLoader
    from wsi_hgnn_amd.trainer import CapturedSlotStep
    dev = torch.device("cuda:0")
    ops.set_gemm_precision(args.gemm)
    lf = torch.nn.CrossEntropyLoss()
    result = {"device": torch.cuda.get_device_name(0), "rounds": args.rounds, "gemm": args.gemm,
              "optimizer": "wsi_hgnn_amd.optim.Adam(capturable=True), gated by node type under type_mask", "cost": {}, "reach": {}}

    def make(in_dim, hidden, nd, drop):
        torch.manual_seed(611)
        m = models.HEATNet4(in_dim, hidden, 2, 2, 4, nd, drop, "mean").to(dev).train()
        return m, O.Adam(m.parameters(), lr=1e-5, weight_decay=5e-3, capturable=True)

    # ---- cost: the quota legs of --augment, with and without the table
    gen = torch.Generator().manual_seed(611)
    sizes = torch.randint(args.min_nodes, args.max_nodes + 1, (args.slides,), generator=gen).tolist()
    graphs = [synthetic.hetero_graph(n, args.in_dim, seed=3000 + i) for i, n in enumerate(sizes)]
    labels = torch.randint(0, 2, (args.slides,), generator=gen).tolist()
    result["cost"]["workload"] = (f"HEATNet4({args.in_dim}, {args.hidden}, 2 layers, 4 heads), {args.slides} synthetic slides of {args.min_nodes}-"
                                  f"{args.max_nodes} nodes, resident, train mode, transform = reference_train_transform(), three quota=\"bound\" "
                                  "slots by size class; legs differ in type_mask only")
    result["cost"]["configs"] = []
    for bs in (1, 2):
        loader = GraphBatchLoader(graphs, labels, bs, dev, shuffle=False, resident=True, transform=transforms.reference_train_transform())
        order = torch.randperm(args.slides, generator=gen).tolist()
        batches = [order[i:i + bs] for i in range(0, len(order), bs)]
        caps = _quota_class_capacities(loader, bs, 3)
        for drop in (0.0, 0.2):
            steps = {}
            for name, tm in (("default", False), ("type_mask", True)):
                m, o = make(args.in_dim, args.hidden, ND, drop)
                steps[name] = CapturedSlotStep(m, o, lf, [BatchSlot(loader, c, quota="bound", type_mask=tm) for c in caps], warmup=2)
            times = _rounds({k: (lambda st=st: [st.step(idxs) for idxs in batches]) for k, st in steps.items()}, batches, args.rounds)
            entry = {"batch_size": bs, "feat_drop": drop, "steps_per_round": len(batches), "legs": {k: _stats(v) for k, v in times.items()}}
            for k, st in steps.items():
                entry[k] = {"replays": st.replays, "eager_steps": st.eager_steps, "overflows": st.overflows()}
            slot = steps["type_mask"].slots[-1]
            B, T, W = slot.layout.graphs, slot.layout.T, 256
            x, mask = torch.randn(B, T * W, device=dev), slot.type_present
            added = {"presence_kernel_ms": _back_to_back_ms(lambda: G_.derive_type_present(slot.layout, slot.bufs, slot.type_present)),
                     "head_multiply_ms": _back_to_back_ms(lambda: (x.view(B, T, W) * mask.view(1, T, 1)))}
            added["per_step_ms"] = added["presence_kernel_ms"] + 2 * added["head_multiply_ms"]          # the multiply runs forward and backward
            entry["added_launches"] = {k: round(v, 5) for k, v in added.items()}
            entry["added_launches"]["launches_per_step"] = 3
            entry["difference_ms"] = round(entry["legs"]["type_mask"]["median_ms"] - entry["legs"]["default"]["median_ms"], 4)
            result["cost"]["configs"].append(entry)
            print(json.dumps(entry), flush=True)
            del steps, m, o, slot
            torch.cuda.empty_cache()
    del graphs, loader
    torch.cuda.empty_cache()

    # ---- reach: a six-type cohort with one rare type
    r = args.reach
    graphs, labels, rare = _rare_cohort(synthetic, r["slides"], r["min_nodes"], r["max_nodes"], r["in_dim"])
    nd = {str(t): t for t in range(RARE["types"])}
    result["reach"]["generator"] = dict(RARE, **r)
    result["reach"]["rare_nodes_per_slide"] = rare
    result["reach"]["slides_without_the_type"] = sum(1 for k in rare if k == 0)
    result["reach"]["slides_with_fewer_than_32"] = sum(1 for k in rare if 0 < k < 32)
    result["reach"]["workload"] = (f"HEATNet4({r['in_dim']}, {r['hidden']}, 2 layers, 4 heads, feat_drop 0.2), {r['slides']} slides of {r['min_nodes']}-"
                                   f"{r['max_nodes']} nodes, resident, train mode, one epoch = every slide once; three slots by size class")
    result["reach"]["configs"] = []
    for augment in (False, True):
        for bs in (1, 2):
            loader = GraphBatchLoader(graphs, labels, bs, dev, shuffle=False, resident=True,
                                      transform=transforms.reference_train_transform() if augment else None)
            order = torch.randperm(r["slides"], generator=gen).tolist()
            batches = [order[i:i + bs] for i in range(0, len(order), bs)]
            caps = _quota_class_capacities(loader, bs, 3) if augment else _class_capacities(loader, bs, 3)
            steps = {}
            for name, tm in (("default", False), ("type_mask", True)):
                m, o = make(r["in_dim"], r["hidden"], nd, 0.2)
                slots = _usable([BatchSlot(loader, c, quota="bound" if augment else None, type_mask=tm) for c in caps])
                steps[name] = CapturedSlotStep(m, o, lf, slots, warmup=2) if slots else _AllEager(m, o, lf, loader)
            base = {k: (st.replays, st.eager_steps) for k, st in steps.items()}
            times = _rounds({k: (lambda st=st: [st.step(idxs) for idxs in batches]) for k, st in steps.items()}, batches, args.rounds)
            entry = {"augment_and_quota": augment, "batch_size": bs, "steps_per_epoch": len(batches), "legs": {k: _stats(v) for k, v in times.items()}}
            for k, st in steps.items():
                rep_, eag = st.replays - base[k][0], st.eager_steps - base[k][1]
                entry[k] = {"slots": len(st.slots), "replayed_share": round(rep_ / max(rep_ + eag, 1), 4), "replayed": rep_, "eager": eag,
                            "overflows": st.overflows()}
            entry["speedup_type_mask"] = round(entry["legs"]["default"]["median_ms"] / entry["legs"]["type_mask"]["median_ms"], 3)
            result["reach"]["configs"].append(entry)
            print(json.dumps(entry), flush=True)
            del steps, m, o, loader
            torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--slides", type=int, default=64)
    ap.add_argument("--min-nodes", type=int, default=6000)
    ap.add_argument("--max-nodes", type=int, default=12000)
    ap.add_argument("--in-dim", type=int, default=1024)
    ap.add_argument("--hidden", type=int, default=512)
    ap.add_argument("--rounds", type=int, default=11)
    ap.add_argument("--gemm", default="auto", choices=["fp32", "bf16x6", "fp16x3", "auto"])
    ap.add_argument("--augment", action="store_true", help="the reference's train-time augmentation on the loader: eager augmented batches against augmented slots")
    ap.add_argument("--type-mask", action="store_true", help="slots with a device-side presence table (DESIGN 3.29): their cost per replayed step "
                                                             "on the quota legs' workload, and their reach on a six-type cohort with one rare type")
    ap.add_argument("--reach-slides", type=int, default=64)
    ap.add_argument("--reach-min-nodes", type=int, default=2000)
    ap.add_argument("--reach-max-nodes", type=int, default=4000)
    ap.add_argument("--reach-in-dim", type=int, default=256)
    ap.add_argument("--reach-hidden", type=int, default=256)
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    if args.out is None:
        args.out = os.path.join(ROOT, "profiles", "r26_slot_type_mask.json" if args.type_mask else "r25_slot_quota.json" if args.augment else "r12_slot_step.json")
    if not torch.cuda.is_available():
        raise SystemExit("tools/slot_bench.py measures on the GPU; none is visible (nothing is estimated on the CPU)")
    if args.type_mask:
        args.reach = {"slides": args.reach_slides, "min_nodes": args.reach_min_nodes, "max_nodes": args.reach_max_nodes, "in_dim": args.reach_in_dim,
                      "hidden": args.reach_hidden}
        return type_mask_main(args)
    import __graft_entry__
    __graft_entry__.build()
    from wsi_hgnn_amd import models, ops, synthetic, transforms, optim as O
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
    result = {"workload": f"HEATNet4({args.in_dim}, {args.hidden}, 2 layers, 4 heads), {args.slides} synthetic slides of {args.min_nodes}-{args.max_nodes} nodes "
                          f"(mean {sum(sizes) / len(sizes):.0f}), resident, gemm={args.gemm}, wsi_hgnn_amd.optim.Adam(capturable=True), train mode",
              "device": torch.cuda.get_device_name(0), "rounds": args.rounds, "configs": []}
    if args.augment:
        result["workload"] += ", transform = Compose([DropNode(0.5), DropEdge(0.5), NodeShuffle(), FeatMask(0.5, ['feat'])]) drawn anew every step"

    def make(drop):
        torch.manual_seed(611)
        m = models.HEATNet4(args.in_dim, args.hidden, 2, 2, 4, ND, drop, "mean").to(dev).train()
        return m, O.Adam(m.parameters(), lr=1e-5, weight_decay=5e-3, capturable=True)

    for bs in (1, 2):
        loader = GraphBatchLoader(graphs, labels, bs, dev, shuffle=False, resident=True,
                                  transform=transforms.reference_train_transform() if args.augment else None)
        order = torch.randperm(args.slides, generator=gen).tolist()
        batches = [order[i:i + bs] for i in range(0, len(order), bs)]
        for drop in (0.0, 0.2):
            m_e, o_e = make(drop)

            def eager_round():
                for idxs in batches:
                    G, y = loader._augmented(idxs) if args.augment else loader._assemble(idxs, 0)[:2]
                    o_e.zero_grad(set_to_none=True)
                    loss = apply_loss(lf, m_e(G), y)
                    loss.backward()
                    o_e.step()

            m1, o1 = make(drop)
            one = CapturedSlotStep(m1, o1, lf, [BatchSlot(loader)], warmup=2)
            m3, o3 = make(drop)
            three = CapturedSlotStep(m3, o3, lf, [BatchSlot(loader, c) for c in _class_capacities(loader, bs, 3)], warmup=2)
            legs = {"eager": eager_round,
                    "one_slot": lambda: [one.step(idxs) for idxs in batches],
                    "three_slots": lambda: [three.step(idxs) for idxs in batches]}
            steppers = [("one_slot", one), ("three_slots", three)]
            if args.augment:                                 # the quota legs: slots sized for the draw
                mq1, oq1 = make(drop)
                q_one = CapturedSlotStep(mq1, oq1, lf, [BatchSlot(loader, quota="bound")], warmup=2)
                mq3, oq3 = make(drop)
                q_three = CapturedSlotStep(mq3, oq3, lf, [BatchSlot(loader, c, quota="bound") for c in _quota_class_capacities(loader, bs, 3)], warmup=2)
                legs["quota_one_slot"] = lambda: [q_one.step(idxs) for idxs in batches]
                legs["quota_three_slots"] = lambda: [q_three.step(idxs) for idxs in batches]
                steppers += [("quota_one_slot", q_one), ("quota_three_slots", q_three)]
            for fn in legs.values():                         # one untimed pass each: caches, allocator pools
                fn()
            times = {k: [] for k in legs}
            for _ in range(args.rounds):
                for k, fn in legs.items():
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    fn()
                    torch.cuda.synchronize()
                    times[k].append((time.perf_counter() - t0) / len(batches) * 1e3)
            entry = {"batch_size": bs, "feat_drop": drop, "steps_per_round": len(batches), "legs": {k: _stats(v) for k, v in times.items()}}
            # the fill alone, and what the filler takes
            for name, step in steppers:
                wall, devt, rows, edges, routed = [], [], [], [], [0] * len(step.slots)
                for idxs in batches:
                    i = step.slot_for(idxs)
                    if i is None:
                        continue
                    slot = step.slots[i]
                    routed[i] += 1
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    slot.load(idxs)
                    torch.cuda.synchronize()
                    wall.append((time.perf_counter() - t0) * 1e3)
                    # device time: behind a few ms of unrelated work, so that the upload and the kernel are queued before the GPU reaches them
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    for _ in range(3):
                        torch.mm(busy, busy, out=busy_out)
                    a.record()
                    slot.load(idxs)
                    b.record()
                    torch.cuda.synchronize()
                    devt.append(a.elapsed_time(b))
                    r, e = slot.padded_share()
                    rows.append(r)
                    edges.append(e)
                entry[name] = {"fill_wall_ms": _stats(wall), "fill_device_ms": _stats(devt), "padded_row_share": round(sum(rows) / len(rows), 4),
                               "padded_edge_share": round(sum(edges) / len(edges), 4), "batches_per_slot": routed,
                               "slot_rows": [s.layout.N for s in step.slots], "eager_fallbacks_per_round": len(batches) - sum(routed)}
                if args.augment:                             # kernel launches of ONE fill (the sort's and the column statistics' included)
                    try:
                        from torch.profiler import ProfilerActivity, profile
                        idxs = next(b_ for b_ in batches if step.slot_for(b_) is not None)
                        torch.cuda.synchronize()
                        with profile(activities=[ProfilerActivity.CUDA]) as prof:
                            step.slots[step.slot_for(idxs)].load(idxs)
                            torch.cuda.synchronize()
                        entry[name]["launches_per_fill"] = sum(ev.count for ev in prof.key_averages() if "memcpy" not in ev.key.lower() and "memset" not in ev.key.lower())
                    except Exception as exc:                 # (no tracer in this build: the count is then documented arithmetic only)
                        entry[name]["launches_per_fill"] = None
                        entry[name]["launches_note"] = f"torch.profiler unavailable: {type(exc).__name__}"
            e_ms = entry["legs"]["eager"]["median_ms"]
            entry["speedup_one_slot"] = round(e_ms / entry["legs"]["one_slot"]["median_ms"], 3)
            entry["speedup_three_slots"] = round(e_ms / entry["legs"]["three_slots"]["median_ms"], 3)
            if args.augment:
                for name, step in steppers[2:]:
                    entry[name]["overflows"] = step.overflows()
                    entry[name]["replays"], entry[name]["eager_steps"] = step.replays, step.eager_steps
                    entry["speedup_" + name] = round(e_ms / entry["legs"][name]["median_ms"], 3)
                entry["quota_over_stored_one_slot"] = round(entry["legs"]["one_slot"]["median_ms"] / entry["legs"]["quota_one_slot"]["median_ms"], 3)
                entry["quota_over_stored_three_slots"] = round(entry["legs"]["three_slots"]["median_ms"] / entry["legs"]["quota_three_slots"]["median_ms"], 3)
                del q_one, q_three, mq1, mq3
            result["configs"].append(entry)
            print(json.dumps(entry), flush=True)
            del one, three, m1, m3, m_e
            torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
