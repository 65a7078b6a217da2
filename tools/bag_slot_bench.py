#!/usr/bin/env python
"""The one-bag-per-step regime of the MIL baselines on one GPU: DSMIL and ABMIL (feats 1024, 2 classes, fp32 GEMMs, the
project's capturable Adam) stepped over 64 bags of 6 000 - 12 000 rows, one bag per step, at dropout_patch 0 and 0.25:

    package eager   mil.train_one_step on the bag (after mil.dropout_patches when the rate is not 0)
    one slot        mil.CapturedBagStep over one BagSlot that holds the largest bag
    three slots     the same over three slots by size
    plain PyTorch   the reference's loop restated in torch (the legs of tools/mil_bench.py), torch.optim.Adam; its dropout is two device permutations

interleaved, medians and min / max over the repeats.  Then one ReMix mixed step per reduced bag (K = 8, 'joint', rate 0.5), eager
(remix.train_one_step) against captured; the slot fill alone (device events around ``BagSlot.load``); and - in a child process of its own under
``rocprofv3 --kernel-trace --stats`` - the selection and row kernels of the fill, with the bytes the row kernel moves over its kernel time
against the project's measured streaming rate.  Prints one JSON line and writes it to --out.

    python tools/bag_slot_bench.py --repeats 7 --inner 16 --out profiles/r21_bag_slot.json
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

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np
import torch

import __graft_entry__
import mil_bench as MB

FEATS, CLASSES, BAGS, ROWS_LO, ROWS_HI = 1024, 2, 64, 6000, 12000
RATES = (0.0, 0.25)
SLOT_CAPS = (8001, 10001, 12001)


def _sizes():
    return [int(n) for n in np.random.RandomState(21).randint(ROWS_LO, ROWS_HI + 1, BAGS)]


def _interleaved(legs, repeats, inner):
    med, spread = MB._interleaved(legs, repeats, inner)
    return {k: {"ms": med[k], "min_max_ms": spread[k]} for k in legs}


def _adam(params):
    from wsi_hgnn_amd import optim
    return optim.Adam(params, lr=2e-4, betas=(0.5, 0.9), weight_decay=5e-3, capturable=True)


def _model(name, dev):
    from wsi_hgnn_amd.mil import abmil, dsmil
    torch.manual_seed(611)
    return (dsmil.MILNet(dsmil.FCLayer(FEATS, CLASSES), dsmil.BClassifier(FEATS, CLASSES)) if name == "dsmil"
            else abmil.BClassifier_(FEATS, CLASSES)).to(dev)


class _Cycle:
    """Calls ``fn(i)`` with i running over the bags."""

    def __init__(self, fn, count):
        self.fn, self.count, self.i = fn, count, 0

    def __call__(self):
        self.fn(self.i)
        self.i = (self.i + 1) % self.count


def steps(res, args, dev):
    from wsi_hgnn_amd import mil
    sizes = _sizes()
    bags = [torch.randn(n, FEATS, device=dev) for n in sizes]
    labels = [i % 2 for i in range(BAGS)]
    targets = mil.bag_targets(labels, CLASSES, dev)
    bce = torch.nn.BCEWithLogitsLoss()
    big = max(range(BAGS), key=lambda i: sizes[i])
    res["bag_rows"] = {"min": min(sizes), "median": int(statistics.median(sizes)), "max": max(sizes)}
    for name in ("dsmil", "abmil"):
        for p in RATES:
            legs, keep = {}, []
            m = _model(name, dev)
            opt = _adam(m.parameters())

            def eager(i, m=m, opt=opt):
                x, plan = mil.dropout_patches(bags[i], [sizes[i]], p, seed=i)
                mil.train_one_step(m, opt, x, plan, [labels[i]])
            legs["package_eager"] = _Cycle(eager, BAGS)
            for leg, caps in (("one_slot", SLOT_CAPS[-1:]), ("three_slots", SLOT_CAPS)):
                ms = _model(name, dev)
                slots = [mil.BagSlot(FEATS, cap, 1, CLASSES, dev, dropout_patch=p, seed=7) for cap in caps]
                warm = [([bags[next(i for i in range(BAGS) if s.fits([sizes[i]]) and (i == big or s is not slots[-1]))]], [1]) for s in slots]
                cap = mil.CapturedBagStep(ms, _adam(ms.parameters()), slots, warmup=2, warmup_batches=warm)
                keep.append(cap)
                legs[leg] = _Cycle(lambda i, cap=cap: cap.step([bags[i]], [labels[i]]), BAGS)
            params = {k: q.detach().clone().requires_grad_(True) for k, q in m.named_parameters()}
            topt = torch.optim.Adam(list(params.values()), lr=2e-4, betas=(0.5, 0.9), weight_decay=5e-3)

            def plain(i, params=params, topt=topt):
                topt.zero_grad()
                x = bags[i]
                if p > 0:                                        # dropout_patches as device permutations (the reference draws on the host)
                    k, mm = mil.patch_counts(sizes[i], p)
                    kept = x.index_select(0, torch.randperm(sizes[i], device=dev)[:k])
                    x = torch.cat([kept, kept.index_select(0, torch.randperm(k, device=dev)[:mm])])
                if name == "dsmil":
                    ins, pred = MB.torch_dsmil(params, x)
                    loss = 0.5 * bce(pred, targets[i:i + 1]) + 0.5 * bce(ins.max(0)[0].view(1, -1), targets[i:i + 1])
                else:
                    loss = bce(MB.torch_abmil(params, x), targets[i:i + 1])
                loss.backward()
                topt.step()
            legs["plain_pytorch"] = _Cycle(plain, BAGS)
            row = _interleaved(legs, args.repeats, args.inner)
            row["captured_over_plain"] = round(row["three_slots"]["ms"] / row["plain_pytorch"]["ms"], 3)
            row["eager_steps"] = {leg: c.eager_steps for leg, c in zip(("one_slot", "three_slots"), keep)}
            res["steps"][f"{name}_p{p}"] = row
            del legs, keep, m, opt, params, topt
            torch.cuda.empty_cache()
    return bags, sizes


def remix_steps(res, args, dev):
    from wsi_hgnn_amd import mil
    from wsi_hgnn_amd.mil import remix
    S, K, V = 64, 8, 16
    g = torch.Generator().manual_seed(5)
    bank = remix.PrototypeBank(torch.randn(S, K, FEATS, generator=g).to(dev), (0.1 * torch.randn(S, K, V, FEATS, generator=g)).to(dev),
                               [i % 2 for i in range(S)])
    for name in ("dsmil", "abmil"):
        m, ms = _model(name, dev), _model(name, dev)
        opt = _adam(m.parameters())
        rng_a, rng_b = np.random.RandomState(1), np.random.RandomState(1)
        slot = mil.BagSlot(FEATS, 4 * K + 1, 1, CLASSES, dev)
        slot.load([bank.prototypes[0]], [int(bank.labels[0])])
        cap = mil.CapturedBagStep(ms, _adam(ms.parameters()), slot, warmup=2)

        def eager(i):
            remix.train_one_step(m, opt, bank, [i], "joint", 0.5, rng_a)

        def captured(i):
            d = remix.draw_mix(rng_b, bank.labels, i, K, "joint", 0.5, V)
            rows, _ = remix.mix(bank, [d])
            cap.step([rows], [int(bank.labels[i])])
        row = _interleaved({"eager": _Cycle(eager, S), "captured": _Cycle(captured, S)}, args.repeats, args.inner)
        row["captured_over_eager"] = round(row["captured"]["ms"] / row["eager"]["ms"], 3)
        res["remix"][name] = row


def fill_loop(dev, loads):
    """The fill alone: ``loads`` loads of the 64 bags into one slot per rate.  Returns {rate: ms per load} by device events."""
    from wsi_hgnn_amd import mil
    sizes = _sizes()
    bags = [torch.randn(n, FEATS, device=dev) for n in sizes]
    out = {}
    for p in RATES:
        slot = mil.BagSlot(FEATS, SLOT_CAPS[-1], 1, CLASSES, dev, dropout_patch=p, seed=7)
        cyc = _Cycle(lambda i: slot.load([bags[i]], [i % 2]), BAGS)
        for _ in range(8):
            cyc()
        samples = [MB._window(cyc, loads) for _ in range(5)]
        out[f"p{p}"] = {"ms": round(statistics.median(samples), 4), "min_max_ms": [round(min(samples), 4), round(max(samples), 4)]}
    return out, sizes


def traced_kernels(res, sizes):
    """The fill loop again in a child under rocprofv3 (a run of its own): per-kernel time of the selection and the row kernel."""
    exe = shutil.which("rocprofv3")
    if exe is None:
        res["fill"]["kernels"] = "not measured: rocprofv3 not found"
        return
    tmp = tempfile.mkdtemp(prefix="bag_slot_trace_")
    try:
        cmd = [exe, "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "-o", "fill", "--", sys.executable, os.path.abspath(__file__), "--fill-only"]
        run = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
        found = glob.glob(os.path.join(tmp, "**", "*kernel_stats.csv"), recursive=True)
        if run.returncode != 0 or not found:
            res["fill"]["kernels"] = f"not measured: rocprofv3 ended with {run.returncode}, {len(found)} stats files"
            return
        rows = {}
        for r in csv.DictReader(open(found[0])):
            nm = r.get("Name", "")
            for key in ("bag_dropout_select_kernel", "bag_slot_rows_kernel"):
                if key in nm:
                    try:
                        rows[key] = {"calls": int(r["Calls"]), "avg_us": round(float(r["AverageNs"]) / 1e3, 2),
                                     "min_us": round(float(r["MinNs"]) / 1e3, 2), "max_us": round(float(r["MaxNs"]) / 1e3, 2)}
                    except (KeyError, ValueError):
                        res["fill"]["kernels"] = f"not measured: unexpected columns {sorted(r)}"
                        return
        # the row kernel rewrites the WHOLE slot (12 001 rows) and reads the bag's kept rows: bytes per call at the median bag, averaged over both rates
        med = statistics.median(sizes)
        moved = SLOT_CAPS[-1] * FEATS * 4 + med * FEATS * 4
        if "bag_slot_rows_kernel" in rows:
            gbs = moved / (rows["bag_slot_rows_kernel"]["avg_us"] * 1e-6) / 1e9
            rows["bag_slot_rows_kernel"].update(bytes_per_call=int(moved), GBs=round(gbs, 1), share_of_stream=round(gbs / MB.STREAM_GBS, 3))
        res["fill"]["kernels"] = rows
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--inner", type=int, default=16)
    ap.add_argument("--out", default=None)
    ap.add_argument("--fill-only", action="store_true", help="only the slot-fill loop (what the traced child runs)")
    ap.add_argument("--no-trace", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bag_slot_bench.py measures on the GPU; none is visible")
    __graft_entry__.build()
    from wsi_hgnn_amd import ops
    dev = torch.device("cuda:0")
    if args.fill_only:
        print(json.dumps(fill_loop(dev, 64)[0]))
        return
    res = {"workload": "MIL one-bag train step in captured bag slots", "feats": FEATS, "classes": CLASSES, "bags": BAGS, "gemm": ops.gemm_precision(),
           "repeats": args.repeats, "inner": args.inner, "stream_GBs": MB.STREAM_GBS, "slot_caps": list(SLOT_CAPS), "steps": {}, "remix": {}, "fill": {}}
    steps(res, args, dev)
    torch.cuda.empty_cache()
    remix_steps(res, args, dev)
    torch.cuda.empty_cache()
    res["fill"]["load_ms"], sizes = fill_loop(dev, 64)
    if not args.no_trace:
        traced_kernels(res, sizes)
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
