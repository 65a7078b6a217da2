#!/usr/bin/env python
"""What the learning rate as a device word costs and what it buys -> profiles/r31_lr_word.json.

1. ``launch``: the optimizer launch over HEATNet4's parameter set (the shapes of tools/optim_bench.py), all four rules with device counts,
   called at the C ABI over one descriptor table: ``wsi_optim_step`` of this library, ``wsi_optim_step_lr`` with a word, and - with
   ``--parent-lib PATH`` - ``wsi_optim_step`` of a library built from the parent commit, TWICE per round.  Device events around windows of
   ``--inner`` back-to-back calls, every leg warmed, the legs alternating window by window, medians over ``--repeats`` windows.  The
   difference of the parent's two series is the spread of the method; ``no_word_within_spread`` says whether this library's launch without a
   word is at most that much slower than the parent's.  Without ``--parent-lib`` those legs say "not measured".
2. ``epoch``: an epoch of 64 one-item steps over three slots by size - GTNMIL on the slides of tools/gtn_slot_bench.py, DSMIL on the bags of
   tools/bag_slot_bench.py - with ``CosineAnnealingLR(opt, epochs, 5e-6)`` stepped once per epoch: a float rate with ``recapture()`` after
   every scheduler step against a word.  Host wall time of the whole epoch, scheduler step (and recapture) included, between two device
   synchronises, the two legs alternating; and the time of one ``recapture()`` alone.

A GPU is required; nothing is estimated.

    python tools/lr_word_bench.py --parent-lib /path/to/parent/libwsi_hgnn.so
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import torch  # noqa: E402

ND = {"0": 0, "1": 1, "2": 2}
EPOCHS = 8          # T_max of the schedule; every timed epoch ends in one scheduler step (past T_max the cosine comes back up: the rate stays in range)


def _window(fn, inner):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(inner):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / inner


def _stats(v):
    return {"median_ms": round(statistics.median(v), 5), "min_ms": round(min(v), 5), "max_ms": round(max(v), 5)}


def launch(args, dev):
    from wsi_hgnn_amd import _native as N, models
    lib = N.load()
    parent = None
    if args.parent_lib:
        parent = ctypes.CDLL(os.path.abspath(args.parent_lib))
        parent.wsi_optim_step.restype, parent.wsi_optim_step.argtypes = N.EXPORTS["wsi_optim_step"]
    torch.manual_seed(611)
    shapes = [tuple(p.shape) for p in models.HEATNet4(args.in_dim, args.hidden, 2, 2, 4, ND, 0.0, "mean").parameters()]
    gen = torch.Generator().manual_seed(1)
    out = {"tensors": len(shapes), "elements": sum(int(torch.Size(s).numel()) for s in shapes), "rules": {}}
    rules = (("sgd", N.WSI_OPTIM_SGD), ("adagrad", N.WSI_OPTIM_ADAGRAD), ("adadelta", N.WSI_OPTIM_ADADELTA), ("adam", N.WSI_OPTIM_ADAM))
    for name, rule in rules:
        keep = []
        arr = (N.OptimTensor * len(shapes))()
        tickets = torch.zeros(len(shapes), dtype=torch.int32, device=dev)
        for k, (a, s) in enumerate(zip(arr, shapes)):
            p, g = torch.randn(s, generator=gen).to(dev), (torch.randn(s, generator=gen) * 1e-2).to(dev)
            s0, s1, step = torch.zeros_like(p), torch.zeros_like(p), torch.zeros((), device=dev)
            keep += [p, g, s0, s1, step]
            a.p, a.g, a.s0, a.s1, a.step, a.ticket, a.n, a.flags = (p.data_ptr(), g.data_ptr(), s0.data_ptr(), s1.data_ptr(), step.data_ptr(),
                                                                     tickets.data_ptr() + 4 * k, p.numel(), 0)
        h = N.OptimHyper(lr=1e-5, weight_decay=5e-3, momentum=0.0, dampening=0.0, nesterov=0.0, lr_decay=5e-3, eps=1e-8, rho=0.9, beta1=0.9,
                         beta2=0.999, host_step=0.0)
        word = torch.full((), 1e-5, dtype=torch.float64, device=dev)
        arr_p, h_p, st = ctypes.cast(arr, ctypes.c_void_p), ctypes.addressof(h), N.stream()

        def call(fn, *extra):
            def go():
                if fn(rule, arr_p, len(shapes), h_p, *extra, st) != 0:
                    raise RuntimeError(f"{name}: the launch failed: {lib.wsi_last_error().decode()}")
            return go

        legs = {"no_word": call(lib.wsi_optim_step), "word": call(lib.wsi_optim_step_lr, None, None, 0, word.data_ptr())}
        if parent is not None:                                    # two series of the same library: their difference is the method's spread
            legs = {"parent_a": call(parent.wsi_optim_step), "no_word": legs["no_word"], "parent_b": call(parent.wsi_optim_step), "word": legs["word"]}
        for fn in legs.values():
            for _ in range(20):
                fn()
        torch.cuda.synchronize()
        samples = {k: [] for k in legs}
        for _ in range(args.repeats):
            for k, fn in legs.items():
                samples[k].append(_window(fn, args.inner))
        row = {k: _stats(v) for k, v in samples.items()}
        row["word_minus_no_word_ms"] = round(row["word"]["median_ms"] - row["no_word"]["median_ms"], 5)
        if parent is not None:
            a, b = row["parent_a"]["median_ms"], row["parent_b"]["median_ms"]
            row["spread_ms"] = round(abs(a - b), 5)
            row["no_word_minus_parent_ms"] = round(row["no_word"]["median_ms"] - min(a, b), 5)
            row["no_word_within_spread"] = bool(row["no_word_minus_parent_ms"] <= row["spread_ms"])       # (parent: the faster of its two series)
        else:
            row["parent"] = "not measured: no --parent-lib"
        out["rules"][name] = row
        print(name, json.dumps(row), file=sys.stderr)
        del keep
        torch.cuda.empty_cache()
    return out


def _epoch_legs(make, steps, dev, repeats):
    """``make(word: bool)`` -> (captured class, optimizer); ``steps(cap)`` runs the 64 one-item steps.  ms per epoch of both legs, alternating."""
    legs = {}
    for name, use_word in (("float_recapture", False), ("word", True)):
        cap, opt = make(use_word)
        sched = torch.optim.lr_scheduler.CosineAnnealingLR(opt, EPOCHS, 5e-6)
        legs[name] = (cap, sched)

    def epoch(name):
        cap, sched = legs[name]
        steps(cap)
        sched.step()
        if name == "float_recapture":
            cap.recapture()

    for name in legs:
        epoch(name)                                               # warm-up epoch
    torch.cuda.synchronize()
    samples = {k: [] for k in legs}
    for _ in range(repeats):
        for name in legs:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            epoch(name)
            torch.cuda.synchronize()
            samples[name].append((time.perf_counter() - t0) * 1e3)
    rec = []
    cap = legs["float_recapture"][0]
    for _ in range(max(5, repeats)):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        cap.recapture()
        torch.cuda.synchronize()
        rec.append((time.perf_counter() - t0) * 1e3)
    out = {k: _stats(v) for k, v in samples.items()}
    out["one_recapture"] = _stats(rec)
    out["eager_steps"] = {k: legs[k][0].eager_steps for k in legs}
    out["graphs_recorded_per_recapture"] = len(cap.graphs)
    return out


def epochs(args, dev):
    import bag_slot_bench as BB
    import gtn_slot_bench as GB
    from wsi_hgnn_amd import gtn, mil, optim
    out = {}
    # GTNMIL, one slide per step
    slides, sizes, _ = GB.make_slides(dev)
    ss = gtn.SlideSet(slides, device=dev)
    labels = [i % GB.CLASSES for i in range(GB.SLIDES)]
    rows = (1350, 1700, 2000)
    torch.manual_seed(611)
    base = gtn.Classifier(GB.CLASSES).to(dev)

    def make_gtn(use_word):
        m = gtn.Classifier(GB.CLASSES).to(dev)
        m.load_state_dict(base.state_dict())
        opt = optim.Adam(m.parameters(), lr=optim.lr_word(1e-4, dev) if use_word else 1e-4, capturable=True)
        slots = [gtn.GraphSlot(GB.FEATS, 1, r, max(ss.entries), device=dev) for r in rows]
        warm = [(ss, [next(i for i in range(GB.SLIDES) if s.fits([ss.sizes[i]], [ss.entries[i]]))], [1]) for s in slots]
        return gtn.CapturedGraphStep(m, opt, slots, warmup=2, warmup_batches=warm), opt

    def gtn_steps(cap):
        for i in range(GB.SLIDES):
            cap.step(ss, [i], [labels[i]])

    out["gtnmil"] = dict(_epoch_legs(make_gtn, gtn_steps, dev, args.epoch_repeats), cell_rows=list(rows), steps_per_epoch=GB.SLIDES,
                         nodes={"min": min(sizes), "max": max(sizes)})
    print("gtnmil", json.dumps(out["gtnmil"]), file=sys.stderr)
    del slides, ss
    torch.cuda.empty_cache()
    # DSMIL, one bag per step
    bsizes = BB._sizes()
    bags = [torch.randn(n, BB.FEATS, device=dev) for n in bsizes]
    big = max(range(BB.BAGS), key=lambda i: bsizes[i])

    def make_dsmil(use_word):
        m = BB._model("dsmil", dev)
        opt = optim.Adam(m.parameters(), lr=optim.lr_word(2e-4, dev) if use_word else 2e-4, betas=(0.5, 0.9), weight_decay=5e-3, capturable=True)
        slots = [mil.BagSlot(BB.FEATS, cap, 1, BB.CLASSES, dev, dropout_patch=0.0, seed=7) for cap in BB.SLOT_CAPS]
        warm = [([bags[next(i for i in range(BB.BAGS) if s.fits([bsizes[i]]) and (i == big or s is not slots[-1]))]], [1]) for s in slots]
        return mil.CapturedBagStep(m, opt, slots, warmup=2, warmup_batches=warm), opt

    def dsmil_steps(cap):
        for i in range(BB.BAGS):
            cap.step([bags[i]], [i % 2])

    out["dsmil"] = dict(_epoch_legs(make_dsmil, dsmil_steps, dev, args.epoch_repeats), slot_caps=list(BB.SLOT_CAPS), steps_per_epoch=BB.BAGS,
                        bag_rows={"min": min(bsizes), "max": max(bsizes)})
    print("dsmil", json.dumps(out["dsmil"]), file=sys.stderr)
    return out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--in-dim", type=int, default=1024)
    ap.add_argument("--hidden", type=int, default=512)
    ap.add_argument("--repeats", type=int, default=9, help="windows per leg of the launch measurement")
    ap.add_argument("--inner", type=int, default=200, help="launches per window")
    ap.add_argument("--epoch-repeats", type=int, default=5)
    ap.add_argument("--parent-lib", default=None, help="libwsi_hgnn.so built from the parent commit: the reference leg of the launch measurement")
    ap.add_argument("--skip-epochs", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r31_lr_word.json"))
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("tools/lr_word_bench.py measures on the GPU; none is visible (nothing is estimated on the CPU)")
    import __graft_entry__
    __graft_entry__.build()
    dev = torch.device("cuda:0")
    out = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__,
           "method": {"launch": f"device events around {args.inner} back-to-back launches, {args.repeats} windows per leg, legs alternating; median (min, max)",
                      "epoch": f"host wall time of 64 one-item steps + scheduler step (+ recapture), between two device synchronises, "
                               f"{args.epoch_repeats} epochs per leg, legs alternating; median (min, max)"},
           "launch": launch(args, dev)}
    if args.skip_epochs:
        out["epoch"] = "not measured: --skip-epochs"
    else:
        try:
            out["epoch"] = epochs(args, dev)
        except (RuntimeError, ValueError, StopIteration) as exc:   # (a Python error, reported as such; the launch figures above stand)
            out["epoch"] = f"not measured: {type(exc).__name__}: {exc}"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
