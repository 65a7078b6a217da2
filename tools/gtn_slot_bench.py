#!/usr/bin/env python
"""The GTNMIL training step of the reference's regime on one GPU: 64 slides of 1 000 - 2 000 nodes with 8 neighbours each, feats
1024, the reference's model size (embed 64, 100 clusters, depth 3, 8 heads), batches of 6 slides (the reference's default batch size,
``drop_last``: 10 batches an epoch), a NEW batch every step, fp32 GEMMs, Adam:

    package eager        gtn.train_one_step on the packed batch of the step's slides, the batch (concatenation, ops.EdgeCSR, plan) built per step
    eager, prebuilt      the same over batches built before the clock starts (what a resident epoch of fixed batches would pay)
    one slot             gtn.CapturedGraphStep over one GraphSlot of 6 cells x 2 000 rows
    three slots          the same over three slots of 1 800 / 1 900 / 2 000 rows per cell
    dense, plain PyTorch the reference's padded form restated in torch - dense [6, Nmax, Nmax] adjacency, mask, (A x + x) W, s^T A s - over padded
                         tensors built before the clock starts, torch.optim.Adam

interleaved, medians and min / max over the repeats; then the slot fill alone (``GraphSlot.load``): device time by events around 64 loads and
host time to issue them; and - in a child process of its own under ``rocprofv3 --kernel-trace --stats`` - the kernels of the replayed one-slot
step (fill included), summed per step: what the GPU itself needs for a step.  Nothing here has a target; what comes out is written down.
Prints one JSON line and writes it to --out.

    python tools/gtn_slot_bench.py --repeats 7 --inner 50 --out profiles/r22_gtn_slot.json
"""
import argparse
import csv
import glob
import json
import os
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np
import torch
import torch.nn.functional as F

import __graft_entry__
import mil_bench as MB

FEATS, CLASSES, SLIDES, NEIGHBOURS, BATCH = 1024, 2, 64, 8, 6
NODES_LO, NODES_HI = 1000, 2000
TRACE_STEPS, TRACE_WARMUP = 200, 2
CELL_ROWS = (1800, 1900, 2000)             # the LARGEST of a batch's six slides decides its slot: at 1 000 - 2 000 nodes most batches hold one above 1 800


def make_slides(dev):
    rng = np.random.RandomState(22)
    sizes = [int(n) for n in rng.randint(NODES_LO, NODES_HI + 1, SLIDES)]
    gen = torch.Generator().manual_seed(22)
    slides = []
    for n in sizes:
        row = torch.arange(n).repeat_interleave(NEIGHBOURS)
        col = torch.randint(0, n, (n * NEIGHBOURS,), generator=gen)
        slides.append((torch.randn(n, FEATS, generator=gen).to(dev), row.to(dev), col.to(dev), None))
    order = rng.permutation(SLIDES)
    batches = [[int(i) for i in order[k:k + BATCH]] for k in range(0, SLIDES - BATCH + 1, BATCH)]          # drop_last
    return slides, sizes, batches


class _Cycle:
    """Calls ``fn(i)`` with i running over the batches."""

    def __init__(self, fn, count):
        self.fn, self.count, self.i = fn, count, 0

    def __call__(self):
        self.fn(self.i)
        self.i = (self.i + 1) % self.count


def dense_step(model, x, adj, mask, live_idx, labels):
    """The reference's forward over padded tensors in plain PyTorch with the weights of ``model`` (``gtn_bench.dense_step`` with a mask: the
    BatchNorm sees the real rows only, gathered by an index built beforehand)."""
    c = model.conv1
    m = mask.unsqueeze(-1)
    X = x * m
    y = (adj @ X + X) @ c.weight + c.bias
    y = F.normalize(y, p=2, dim=2)
    flat = y.reshape(-1, y.shape[2])
    y = torch.zeros_like(flat).index_copy(0, live_idx, c.bn_layer(flat.index_select(0, live_idx))).reshape(y.shape)
    s = torch.softmax(F.linear(y, model.pool1.weight, model.pool1.bias), -1) * m
    y = y * m
    out = s.transpose(1, 2) @ y
    num = torch.einsum("bii->b", s.transpose(1, 2) @ adj @ s)
    den = torch.einsum("bii->b", s.transpose(1, 2) @ (adj.sum(-1).unsqueeze(-1) * s))
    mc = torch.mean(-(num / den))
    ss = s.transpose(1, 2) @ s
    eye = torch.eye(s.shape[-1], device=s.device)
    ortho = torch.mean(torch.norm(ss / torch.norm(ss, dim=(-1, -2), keepdim=True) - eye / torch.norm(eye), dim=(-1, -2)))
    tokens = torch.cat([model.cls_token.repeat(out.shape[0], 1, 1), out], 1)
    return F.cross_entropy(model.transformer(tokens), labels) + mc + ortho


def replay_loop(dev):
    """What the traced child runs: ``TRACE_WARMUP`` eager steps, the capture, ``TRACE_STEPS`` loads and replays of the one-slot step."""
    from wsi_hgnn_amd import gtn, optim
    torch.manual_seed(611)
    slides, _, batches = make_slides(dev)
    ss = gtn.SlideSet(slides, device=dev)
    labels = [i % CLASSES for i in range(SLIDES)]
    m = gtn.Classifier(CLASSES).to(dev)
    slot = gtn.GraphSlot(FEATS, BATCH, CELL_ROWS[-1], BATCH * max(ss.entries), device=dev)
    cap = gtn.CapturedGraphStep(m, optim.Adam(m.parameters(), lr=1e-4, capturable=True), slot, warmup=TRACE_WARMUP,
                                warmup_batches=[(ss, batches[0], [labels[i] for i in batches[0]])])
    for k in range(TRACE_STEPS):
        b = batches[k % len(batches)]
        cap.step(ss, b, [labels[i] for i in b])
    torch.cuda.synchronize()
    return cap.replays


def traced_kernels(res):
    """The replay loop in a child under rocprofv3 (a run of its own): the summed kernel time per step and the kernels that take most of it."""
    exe = shutil.which("rocprofv3")
    if exe is None:
        res["replayed_step_kernels"] = "not measured: rocprofv3 not found"
        return
    tmp = tempfile.mkdtemp(prefix="gtn_slot_trace_")
    try:
        cmd = [exe, "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "-o", "replay", "--", sys.executable, os.path.abspath(__file__), "--trace-only"]
        run = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
        found = glob.glob(os.path.join(tmp, "**", "*kernel_stats.csv"), recursive=True)
        if run.returncode != 0 or not found:
            res["replayed_step_kernels"] = f"not measured: rocprofv3 ended with {run.returncode}, {len(found)} stats files"
            return
        rows = []
        for r in csv.DictReader(open(found[0])):
            try:
                rows.append((r["Name"], int(r["Calls"]), float(r["AverageNs"])))
            except (KeyError, ValueError):
                res["replayed_step_kernels"] = f"not measured: unexpected columns {sorted(r)}"
                return
        steps = TRACE_STEPS + TRACE_WARMUP                    # (the warm-up steps run the same kernels eagerly; the capture itself runs none)
        total = sum(c * a for _, c, a in rows)
        top = sorted(rows, key=lambda t: -t[1] * t[2])[:8]
        res["replayed_step_kernels"] = {"steps": steps, "kernel_ms_per_step": round(total / steps / 1e6, 4),
                                        "launches_per_step": round(sum(c for _, c, _ in rows) / steps, 1),
                                        "top": [{"name": n.split("(")[0][:80], "calls_per_step": round(c / steps, 2), "avg_us": round(a / 1e3, 2),
                                                 "ms_per_step": round(c * a / steps / 1e6, 4)} for n, c, a in top]}
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--inner", type=int, default=50)
    ap.add_argument("--out", default=None)
    ap.add_argument("--trace-only", action="store_true", help="only the one-slot replay loop (what the traced child runs)")
    ap.add_argument("--no-trace", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("gtn_slot_bench.py measures on the GPU; none is visible")
    __graft_entry__.build()
    from wsi_hgnn_amd import gtn, ops, optim

    dev = torch.device("cuda:0")
    if args.trace_only:
        print(json.dumps({"replays": replay_loop(dev)}))
        return
    torch.manual_seed(611)
    slides, sizes, batches = make_slides(dev)
    ss = gtn.SlideSet(slides, device=dev)
    labels = [i % CLASSES for i in range(SLIDES)]
    nb = len(batches)
    res = {"workload": "GTNMIL train step over new batches: packed eager, captured graph slots, dense plain PyTorch", "feats": FEATS,
           "classes": CLASSES, "slides": SLIDES, "neighbours": NEIGHBOURS, "batch": BATCH, "batches_per_epoch": nb, "gemm": ops.gemm_precision(),
           "nodes": {"min": min(sizes), "median": int(statistics.median(sizes)), "max": max(sizes)}, "cell_rows": list(CELL_ROWS),
           "repeats": args.repeats, "inner": args.inner}
    base = gtn.Classifier(CLASSES).to(dev)

    def model(**kw):
        m = gtn.Classifier(CLASSES, **kw).to(dev)
        m.load_state_dict(base.state_dict())
        return m

    adam = lambda m, **kw: optim.Adam(m.parameters(), lr=1e-4, **kw)
    lab_dev = [torch.tensor([labels[i] for i in b], device=dev) for b in batches]
    legs, keep = {}, []

    m_e, m_p = model(), model()
    o_e, o_p = adam(m_e), adam(m_p)
    legs["package_eager"] = _Cycle(lambda k: gtn.train_one_step(m_e, ss.batch(batches[k]), lab_dev[k], o_e), nb)
    prebuilt = [ss.batch(b) for b in batches]
    for b in prebuilt:
        b.ec, b.rp
    legs["eager_prebuilt"] = _Cycle(lambda k: gtn.train_one_step(m_p, prebuilt[k], lab_dev[k], o_p), nb)

    entry_cap = BATCH * max(ss.entries)
    for leg, rows in (("one_slot", CELL_ROWS[-1:]), ("three_slots", CELL_ROWS)):
        ms = model()
        slots = [gtn.GraphSlot(FEATS, BATCH, r, entry_cap, device=dev) for r in rows]
        warm = []
        for s in slots:                                       # a batch of the epoch that fits this slot (the largest takes any)
            k = next((k for k, b in enumerate(batches) if s.fits([ss.sizes[i] for i in b], [ss.entries[i] for i in b])), None)
            b = batches[k] if k is not None else sorted(range(SLIDES), key=lambda i: ss.sizes[i])[:BATCH]
            warm.append((ss, b, [labels[i] for i in b]))
        cap = gtn.CapturedGraphStep(ms, adam(ms, capturable=True), slots, warmup=2, warmup_batches=warm)
        keep.append(cap)
        legs[leg] = _Cycle(lambda k, cap=cap: cap.step(ss, batches[k], [labels[i] for i in batches[k]]), nb)

    m_d = model(kernels=False)
    o_d = torch.optim.Adam(m_d.parameters(), lr=1e-4)
    dense = []
    for b in batches:
        nmax = max(ss.sizes[i] for i in b)
        x = torch.zeros(BATCH, nmax, FEATS, device=dev)
        adj = torch.zeros(BATCH, nmax, nmax, device=dev)
        mask = torch.zeros(BATCH, nmax, device=dev)
        for g, i in enumerate(b):
            n = ss.sizes[i]
            x[g, :n], mask[g, :n] = ss.x[i], 1.0
            r, c, _ = ss.entries_coo[i]
            adj[g].index_put_((r, c), torch.ones(r.shape[0], device=dev), accumulate=True)
        dense.append((x, adj, mask, mask.flatten().nonzero().flatten()))

    def dense_leg(k):
        m_d.train()
        o_d.zero_grad()
        dense_step(m_d, *dense[k], lab_dev[k]).backward()
        o_d.step()
    legs["dense_plain_pytorch"] = _Cycle(dense_leg, nb)
    res["dense_adjacency_MB_per_batch"] = round(max(d[1].numel() for d in dense) * 4 / 1e6, 1)

    with torch.no_grad():                                     # the three forms compute one objective (same weights, before any step)
        probe, k0 = model(), 0
        probe.train()
        slot = gtn.GraphSlot(FEATS, BATCH, CELL_ROWS[-1], entry_cap, device=dev).load(ss, batches[k0], [labels[i] for i in batches[k0]])
        res["loss_packed_slot_dense"] = [float(probe(prebuilt[k0], lab_dev[k0])[2]), float(probe(slot, None)[2]),
                                         float(dense_step(model(kernels=False).train(), *dense[k0], lab_dev[k0]))]
        del probe, slot

    med, spread = MB._interleaved(legs, args.repeats, args.inner)
    res["steps_ms"] = {k: {"ms": med[k], "min_max_ms": spread[k]} for k in legs}
    res["eager_steps_in_captured_legs"] = {leg: c.eager_steps for leg, c in zip(("one_slot", "three_slots"), keep)}
    res["slot_of_each_batch"] = [keep[1].slot_for([ss.sizes[i] for i in b], [ss.entries[i] for i in b]) for b in batches]
    for other in ("one_slot", "three_slots", "dense_plain_pytorch", "eager_prebuilt"):
        res[other + "_over_package_eager"] = round(med[other] / med["package_eager"], 3)

    # the fill alone, into the largest slot: device time (events around 64 loads) and the host's time to issue them
    slot = gtn.GraphSlot(FEATS, BATCH, CELL_ROWS[-1], entry_cap, device=dev)
    cyc = _Cycle(lambda k: slot.load(ss, batches[k], [labels[i] for i in batches[k]]), nb)
    for _ in range(8):
        cyc()
    dev_ms = [MB._window(cyc, 64) for _ in range(5)]
    host_ms = []
    for _ in range(5):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(64):
            cyc()
        host_ms.append((time.perf_counter() - t0) * 1e3 / 64)
        torch.cuda.synchronize()
    res["fill"] = {"device_ms_per_load": round(statistics.median(dev_ms), 4), "device_min_max_ms": [round(min(dev_ms), 4), round(max(dev_ms), 4)],
                   "host_ms_per_load": round(statistics.median(host_ms), 4), "host_min_max_ms": [round(min(host_ms), 4), round(max(host_ms), 4)],
                   "slot_x_MB": round(BATCH * CELL_ROWS[-1] * FEATS * 4 / 1e6, 1),
                   "note": "device time is the span of back-to-back loads on one stream: it is the larger of the host's issue time and the kernels' time"}
    if not args.no_trace:
        del legs, keep, dense, prebuilt, slot
        torch.cuda.empty_cache()
        traced_kernels(res)
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
