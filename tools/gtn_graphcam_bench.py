#!/usr/bin/env python
"""GraphCAM timing on one GPU (``wsi_hgnn_amd.gtn.graphcam``), ms per call, medians of interleaved repeats.

8 slides x 2 000 nodes with 8 neighbours each, 3 classes, the reference's model size (64 wide, 100 clusters, 3 blocks of 8 heads).  Three legs
compute the same maps:
  native_ms          ``class_maps(kernels=True)``: all slides and classes in one pass over the relevance kernels;
  tensor_ops_ms      ``class_maps(kernels=False)``: the same closed forms in tensor operations, the whole batch in one pass;
  per_slide_class_ms the tensor-operation form one slide and one class at a time - the reference's regime (its own code additionally re-runs
                     every layer under autograd and writes files in between).
Also the relevance chain alone (``token_maps`` on fixed tokens, native against tensor operations) and the kernel time of one native call.
Prints one JSON line (and writes it to --out when given).

    python tools/gtn_graphcam_bench.py --repeats 7 --inner 5 [--out profiles/r18_graphcam.json]
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

FEATS, CLASSES, SLIDES, NEIGHBOURS = 1024, 3, 8, 8


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--inner", type=int, default=5)
    ap.add_argument("--nodes", type=int, default=2000)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("gtn_graphcam_bench.py measures on the GPU; none is visible")
    __graft_entry__.build()
    import wsi_hgnn_amd as W
    from wsi_hgnn_amd import gtn, ops, synthetic
    from wsi_hgnn_amd.gtn import graphcam

    dev = torch.device("cuda:0")
    torch.manual_seed(611)
    graphs = [synthetic.homogeneous_graph(args.nodes, FEATS, NEIGHBOURS, seed=611 + i) for i in range(SLIDES)]
    batch = gtn.as_batch(W.batch(graphs).to(dev))
    singles = [gtn.as_batch(W.batch([g]).to(dev)) for g in graphs]
    for b in [batch] + singles:
        b.ec, b.rp, b.segment()                                     # (the plans are built once per batch, outside the timed calls)
    model = gtn.Classifier(CLASSES).to(dev).eval()
    with torch.no_grad():                                           # (away from the initial state: a zero class token is a zero row of relevance)
        model.cls_token.normal_(0, 0.5)
        for p in model.conv1.bn_layer.parameters():
            p.add_(0.1 * torch.randn_like(p))

    def per_slide_class():
        out = []
        for b in singles:
            for c in range(CLASSES):
                out.append(graphcam.class_maps(model, b, classes=[c], kernels=False).node_heat)
        return out

    legs = {"native_ms": lambda: graphcam.class_maps(model, batch, kernels=True),
            "tensor_ops_ms": lambda: graphcam.class_maps(model, batch, kernels=False),
            "per_slide_class_ms": per_slide_class}
    res = {"workload": "GraphCAM of GTNMIL: class_maps over a batch", "feats": FEATS, "slides": SLIDES, "nodes_per_slide": args.nodes,
           "classes": CLASSES, "neighbours": NEIGHBOURS, "repeats": args.repeats, "inner": args.inner}
    a, b = legs["native_ms"](), legs["tensor_ops_ms"]()
    c = torch.stack(per_slide_class(), 0).view(SLIDES, CLASSES, args.nodes)
    scale = float(b.cluster_cam.abs().max())
    res["native_vs_tensor_ops_cluster_cam"] = float((a.cluster_cam - b.cluster_cam).abs().max()) / scale
    res["per_slide_class_vs_batched_node_heat"] = float((c.permute(0, 2, 1).reshape(-1, CLASSES) - b.node_heat).abs().max())
    med, spread = _interleaved(legs, args.repeats, args.inner)
    res.update(med)
    res["min_max"] = spread
    res["tensor_ops_over_native"] = round(med["tensor_ops_ms"] / med["native_ms"], 3)
    res["per_slide_class_over_native"] = round(med["per_slide_class_ms"] / med["native_ms"], 3)

    # ---- the relevance chain alone (forward_saving, C autograd calls, the rules, the rollout row) on fixed tokens
    tokens = a.tokens
    chain = {"native_ms": lambda: graphcam.token_maps(model.transformer, tokens, kernels=True),
             "tensor_ops_ms": lambda: graphcam.token_maps(model.transformer, tokens, kernels=False)}
    med, spread = _interleaved(chain, args.repeats, max(args.inner, 20))
    med["min_max"] = spread
    med["tensor_ops_over_native"] = round(med["tensor_ops_ms"] / med["native_ms"], 3)
    res["relevance_chain"] = med

    ops.enable_kernel_timing(True)
    for _ in range(3):
        legs["native_ms"]()
    torch.cuda.synchronize()
    res["native_kernel_ms_per_3_calls"] = ops.kernel_timing_summary()
    ops.enable_kernel_timing(False)

    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
