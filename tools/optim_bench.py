#!/usr/bin/env python
"""What the one-launch optimizers cost (wsi_hgnn_amd.optim: SGD, Adagrad, Adadelta, Adam; csrc/optim.hip) -> profiles/r10_optim.json.

1. ``rules``: one optimizer step over HEATNet4's parameter set (fixed gradients), ours against torch.optim's fastest implementation of the same rule
   (``fused=True`` where torch has one, else ``foreach=True``).  Host wall time around blocks of steps that end in a device synchronise, the two
   sides alternating block by block in one process; median, fastest and slowest block.  ``bytes_per_step`` is what the rule must move, from the
   shapes (csrc/optim.hip's per-element counts); ``gb_per_s`` divides it by the WALL time of a step, launch overhead included - it is not a
   kernel's bandwidth.
2. ``captured_step``: the reference's slide-by-slide regime - HEATNet4, ONE 10k-node graph per step, the whole step replayed from one hipGraph
   (trainer.CapturedStep) - with optim.Adam(capturable=True) against torch.optim.Adam(capturable=True) (and torch's fused capturable form),
   replays alternating block by block.

A GPU is required: there is no CPU path and nothing is estimated."""
import argparse
import gc
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

ND = {"0": 0, "1": 1, "2": 2}
BYTES = {"sgd": 12, "sgd_momentum": 20, "adagrad": 20, "adadelta": 28, "adam": 28, "adam_capturable": 28}


def _blocks(fns, blocks, steps):
    """Wall ms per call of each fn: `blocks` rounds, in each round every fn runs `steps` times behind a synchronise and ends in one."""
    out = [[] for _ in fns]
    for _ in range(blocks):
        for k, fn in enumerate(fns):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                fn()
            torch.cuda.synchronize()
            out[k].append((time.perf_counter() - t0) / steps * 1e3)
    return [{"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)} for v in out]


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--in-dim", type=int, default=1024)
    ap.add_argument("--hidden", type=int, default=512)
    ap.add_argument("--nodes", type=int, default=10000)
    ap.add_argument("--blocks", type=int, default=9)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r10_optim.json"))
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("tools/optim_bench.py measures on the GPU; none is visible (nothing is estimated on the CPU)")
    import __graft_entry__
    __graft_entry__.build()
    import wsi_hgnn_amd as W
    from wsi_hgnn_amd import models, synthetic, optim as O
    from wsi_hgnn_amd.trainer import CapturedStep
    dev = torch.device("cuda:0")

    def model():
        torch.manual_seed(611)
        return models.HEATNet4(args.in_dim, args.hidden, 2, 2, 4, ND, 0.0, "mean").to(dev)

    # ---- 1. the step of each rule over the model's parameters
    shapes = [tuple(p.shape) for p in model().parameters()]
    elements = sum(int(torch.Size(s).numel()) for s in shapes)
    gen = torch.Generator(device="cpu").manual_seed(1)
    grads = [(torch.randn(s, generator=gen) * 1e-2).to(dev) for s in shapes]

    def stepper(cls, **kw):
        ps = [torch.nn.Parameter(torch.randn(s, generator=gen).to(dev)) for s in shapes]
        for p, g in zip(ps, grads):
            p.grad = g
        return cls(ps, **kw).step

    cases = [
        ("sgd", O.SGD, dict(lr=1e-5, weight_decay=5e-3), torch.optim.SGD, dict(fused=True)),
        ("sgd_momentum", O.SGD, dict(lr=1e-5, weight_decay=5e-3, momentum=0.9), torch.optim.SGD, dict(fused=True)),
        ("adagrad", O.Adagrad, dict(lr=1e-5, weight_decay=5e-3, lr_decay=5e-3), torch.optim.Adagrad, dict(foreach=True)),       # (torch's fused Adagrad is CPU-only)
        ("adadelta", O.Adadelta, dict(lr=1e-5, weight_decay=5e-3), torch.optim.Adadelta, dict(foreach=True)),
        ("adam", O.Adam, dict(lr=1e-5, weight_decay=5e-3), torch.optim.Adam, dict(fused=True)),
        ("adam_capturable", O.Adam, dict(lr=1e-5, weight_decay=5e-3, capturable=True), torch.optim.Adam, dict(fused=True, capturable=True)),
    ]
    rules = {}
    for name, ours, kw, theirs, how in cases:
        fns = [stepper(ours, **kw), stepper(theirs, **kw, **{k: v for k, v in how.items() if k not in kw})]
        for fn in fns:
            for _ in range(10):
                fn()
        torch.cuda.synchronize()
        gc.collect()
        mine, ref = _blocks(fns, args.blocks, args.steps)
        nbytes = BYTES[name] * elements
        for r in (mine, ref):
            r["gb_per_s_wall"] = round(nbytes / (r["median_ms"] * 1e-3) / 1e9, 1)
        rules[name] = {"ours": mine, "torch": dict(ref, implementation=", ".join(f"{k}={v}" for k, v in how.items())),
                       "bytes_per_step": nbytes, "torch_over_ours": round(ref["median_ms"] / mine["median_ms"], 3)}
        print(name, json.dumps(rules[name]), file=sys.stderr)

    # ---- 2. the one-slide captured step
    G = W.batch([synthetic.hetero_graph(args.nodes, args.in_dim, seed=100, dst_mode="hub")]).to(dev)
    y = torch.tensor([1], device=dev)
    lf = torch.nn.CrossEntropyLoss()
    makers = [("ours", lambda ps: O.Adam(ps, lr=1e-5, weight_decay=5e-3, capturable=True)),
              ("torch", lambda ps: torch.optim.Adam(ps, lr=1e-5, weight_decay=5e-3, capturable=True)),
              ("torch_fused", lambda ps: torch.optim.Adam(ps, lr=1e-5, weight_decay=5e-3, capturable=True, fused=True))]
    steps, losses = [], {}
    for name, mk in makers:
        m = model()
        steps.append(CapturedStep(m, mk(m.parameters()), lf, G, y, warmup=3))
    for (name, _), s in zip(makers, steps):
        losses[name] = [s().item() for _ in range(5)]
    res = _blocks(steps, args.blocks, args.steps)
    captured = {"workload": f"HEATNet4 hidden {args.hidden}, ONE {args.nodes}-node graph per step, fwd + CE + bwd + Adam replayed from one hipGraph",
                "nodes": G.num_nodes(), "edges": G.num_edges(),
                "ours_capturable_adam": res[0], "torch_adam_capturable": res[1], "torch_adam_capturable_fused": res[2],
                "saved_ms_vs_torch_capturable": round(res[1]["median_ms"] - res[0]["median_ms"], 4),
                "saved_ms_vs_torch_fused_capturable": round(res[2]["median_ms"] - res[0]["median_ms"], 4),
                "first_losses": losses}
    out = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "parameters": {"tensors": len(shapes), "elements": elements},
           "method": f"host wall time, {args.blocks} alternating blocks of {args.steps} calls, each block between two device synchronises; median (min, max)",
           "rules": rules, "captured_step": captured}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
