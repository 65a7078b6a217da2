#!/usr/bin/env python
"""H2MIL timing on one GPU (``wsi_hgnn_amd.h2mil``), ms per call, medians of interleaved windows.

Leg 1, one training step - zero_grad, forward, backward and the reference's ``Adam(lr=5e-5, weight_decay=5e-4)`` - over a batch of 8 synthetic
slides at two sizes: three levels, 8 same-level neighbours plus parent / child edges, feature width 1024, pool ratios 0.1 and 4;
``kernels=True`` against ``kernels=False`` (the same model through tensor operations) on the same weights.
Leg 2, ``ops.ra_attention`` forward + backward alone against its tensor-operation form (``h2mil.ra_attention_tensor``) on the larger batch's
graph at the model's width.
The reference itself cannot be timed: it needs torch_geometric, torch_scatter and torch_sparse, which are not installed; nothing is estimated.
``--from-grid`` draws the slides as patch grids and builds the batch with ``h2mil.from_grid`` instead (1 + 5 n1 nodes per slide; the committed
profile used the default).  Prints one JSON line (and writes it to --out when given).

    python tools/h2mil_bench.py --repeats 7 --inner 3 [--out profiles/r19_h2mil.json]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch

import __graft_entry__
from mil_bench import _interleaved

FEATS, HIDDEN, CLASSES, SLIDES, NEIGHBOURS, CHILDREN = 1024, 256, 2, 8, 8, 8
RATIOS = (0.1, 4)


def synthetic_slide(n1: int, seed: int):
    """One root, ``n1`` level-1 nodes, CHILDREN level-2 nodes each; NEIGHBOURS random same-level in-neighbours per node and parent / child
    edges both ways; the reference's ``Data`` field names."""
    g = torch.Generator().manual_seed(seed)
    n2 = n1 * CHILDREN
    n = 1 + n1 + n2
    nt = torch.cat([torch.zeros(1, dtype=torch.int64), torch.ones(n1, dtype=torch.int64), torch.full((n2,), 2, dtype=torch.int64)])
    tree = torch.cat([torch.tensor([-1]), torch.zeros(n1, dtype=torch.int64), 1 + torch.arange(n1).repeat_interleave(CHILDREN)])
    src, dst = [], []
    for lo, m in ((1, n1), (1 + n1, n2)):
        d = lo + torch.arange(m).repeat_interleave(NEIGHBOURS)
        s = lo + torch.randint(0, m, (m * NEIGHBOURS,), generator=g)
        keep = s != d
        src.append(s[keep]); dst.append(d[keep])
    kids = torch.arange(1, n)
    src += [tree[1:], kids]; dst += [kids, tree[1:]]
    return {"x": torch.randn(n, FEATS, generator=g), "edge_index_tree_8nb": torch.stack([torch.cat(src), torch.cat(dst)]), "node_type": nt,
            "node_tree": tree, "x_y_index": torch.rand(n, 2, generator=g)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--inner", type=int, default=3)
    ap.add_argument("--small", type=int, default=100, help="level-1 nodes per slide of the smaller batch")
    ap.add_argument("--large", type=int, default=500, help="level-1 nodes per slide of the larger batch")
    ap.add_argument("--from-grid", action="store_true", help="draw the slides as patch grids (a disc of level-1 cells, four level-2 cells under each: "
                    "1 + 5 n1 nodes per slide) and build the batch with h2mil.from_grid (the reference's tree, made on the device)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("h2mil_bench.py measures on the GPU; none is visible")
    __graft_entry__.build()
    from wsi_hgnn_amd import h2mil, ops, optim

    dev = torch.device("cuda:0")
    torch.manual_seed(611)
    res = {"workload": "H2MIL training step and RAConv attention", "feats": FEATS, "out_classes": HIDDEN, "slides": SLIDES, "neighbours": NEIGHBOURS,
           "children": CHILDREN, "pool_ratios": list(RATIOS), "optimizer": "Adam(lr=5e-5, weight_decay=5e-4)", "repeats": args.repeats,
           "inner": args.inner, "inputs": "h2mil.from_grid over patch grids" if args.from_grid else "synthetic_slide", "reference": "not measured: torch_geometric, torch_scatter and torch_sparse are not installed", "steps": {}}
    labels = (torch.arange(SLIDES, device=dev) % CLASSES).to(torch.int64)

    def stepper(model, batch):
        opt = optim.Adam(model.parameters(), lr=5e-5, weight_decay=5e-4)
        return lambda: h2mil.train_one_step(model, batch, labels, opt)

    batch = None
    for name, n1 in (("small", args.small), ("large", args.large)):
        if args.from_grid:
            from grid_graph_bench import tree_tables
            tables = [tree_tables(n1, 611 + i) for i in range(SLIDES)]
            batch = h2mil.from_grid([{"x": torch.randn(1 + 5 * n1, FEATS, device=dev), "coords1": t[0].to(dev), "cover": t[1].to(dev), "coords2": t[2].to(dev)}
                                     for t in tables], dtype=torch.float32)
        else:
            batch = h2mil.from_slides([synthetic_slide(n1, 611 + i) for i in range(SLIDES)]).to(dev)
        batch.ec, batch.rp                                          # (the plans are built once per batch, outside the timed step)
        native = h2mil.H2MIL(FEATS, 0, HIDDEN, CLASSES, pool1_ratio=RATIOS[0], pool2_ratio=RATIOS[1], kernels=True).to(dev)
        tensors = h2mil.H2MIL(FEATS, 0, HIDDEN, CLASSES, pool1_ratio=RATIOS[0], pool2_ratio=RATIOS[1], kernels=False).to(dev)
        tensors.load_state_dict(native.state_dict())
        row = {"nodes_per_slide": batch.sizes[0], "nodes": batch.num_nodes, "edges": int(batch.edge_index.shape[1])}
        with torch.no_grad():
            native.eval(); tensors.eval()
            a, b = native(batch), tensors(batch)
            row["max_abs_probability_diff"] = float((a[0] - b[0]).abs().max())
            row["same_clusters"] = bool(all(torch.equal(p, q) for l in (0, 1) for p, q in zip(a[1][l], b[1][l])))
            row["pooled_nodes"] = [int(sum(t.shape[0] for t in a[2][l])) for l in (0, 1)]
        legs = {"kernels_ms": stepper(native, batch), "tensor_ops_ms": stepper(tensors, batch)}
        med, spread = _interleaved(legs, args.repeats, args.inner)
        row.update(med)
        row["min_max"] = spread
        row["tensor_ops_over_kernels"] = round(med["tensor_ops_ms"] / med["kernels_ms"], 3)
        ops.enable_kernel_timing(True)
        for _ in range(3):
            legs["kernels_ms"]()
        torch.cuda.synchronize()
        row["kernel_ms_per_3_steps"] = ops.kernel_timing_summary()
        ops.enable_kernel_timing(False)
        res["steps"][name] = row
        del native, tensors, legs

    # ---- the attention alone, forward + backward, on the larger batch's graph
    n, ec, nt = batch.num_nodes, batch.ec, batch.node_type
    src, dst = batch.edge_index[0], batch.edge_index[1]
    ft = torch.randn(n, HIDDEN, device=dev, requires_grad=True)
    sc = torch.randn(n, 4, device=dev, requires_grad=True)
    bias = torch.randn(HIDDEN, device=dev, requires_grad=True)
    g_out = torch.randn(n, HIDDEN, device=dev)

    def run(fn):
        def leg():
            ft.grad = sc.grad = bias.grad = None
            fn().backward(g_out)
        return leg

    legs = {"kernel_ms": run(lambda: ops.ra_attention(ft, sc, bias, ec, nt)), "tensor_ops_ms": run(lambda: h2mil.ra_attention_tensor(ft, sc, bias, src, dst, nt))}
    med, spread = _interleaved(legs, args.repeats, max(args.inner, 20))
    med["min_max"] = spread
    med["shape"] = {"nodes": n, "edges": int(src.numel()), "C": HIDDEN}
    med["tensor_ops_over_kernel"] = round(med["tensor_ops_ms"] / med["kernel_ms"], 3)
    with torch.no_grad():
        med["max_abs_diff"] = float((ops.ra_attention(ft, sc, bias, ec, nt) - h2mil.ra_attention_tensor(ft, sc, bias, src, dst, nt)).abs().max())
    # the bytes the two kernels must move at least: every edge gathers one C-wide row each way, every node writes one
    E = int(src.numel())
    med["min_bytes_fwd_bwd"] = 4 * HIDDEN * (2 * E + 3 * n)
    med["achieved_GBps"] = round(med["min_bytes_fwd_bwd"] / (med["kernel_ms"] * 1e-3) / 1e9, 1)
    res["attention"] = med

    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
