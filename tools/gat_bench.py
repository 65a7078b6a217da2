#!/usr/bin/env python
"""GAT_Kimia_v2-shaped timing: GAT(2, 1024, 512, 2, heads [4, 4, 1], mean readout) on a batch of 8 x synthetic.homogeneous_graph(10000)
(80k nodes, ~720k edges), one GPU, fwd + CE + bwd + Adam under 'auto' GEMMs, in eval mode and in training mode with feat_drop /
attn_drop 0.2; the same step restated in plain PyTorch (index_add_ / scatter_reduce edge softmax, torch GEMMs, torch Adam) on the same
GPU as a point of comparison; HIP-event times of the edge kernels at the hidden layers' shape with their achieved GB/s against the
~8 TB/s beyond-L2 gather ceiling.  Prints one JSON line (and writes it to --out when given).

    python tools/gat_bench.py --steps 20 --warmup 5 [--out profiles/r07_gat_step.json]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn.functional as F

import __graft_entry__

GATHER_CEILING_GBS = 8000.0          # random whole-row gathers beyond L2, chip-wide


def _time(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(steps):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / steps


def torch_gat_forward(params, n_layers, heads, hidden, x, src, dst, gid, counts, B, slope, training, fdrop, adrop):
    """models/GAT.py in plain PyTorch (the restatement a DGL-less port would write): mean readout of every layer input, GATConv by
    index_add_ / scatter_reduce, leaky_relu(0.01) activation; the last layer skipped (its output is discarded)."""
    h = x
    outs = []
    n = x.shape[0]
    for i in range(n_layers + 1):
        p = torch.zeros(B, h.shape[1], device=h.device).index_add_(0, gid, h) / counts[:, None]
        outs.append(F.linear(p, params[f"linears_prediction.{i}.weight"], params[f"linears_prediction.{i}.bias"]))
        if i == n_layers:
            break
        H = heads[i]
        hin = F.dropout(h, fdrop, training)
        ft = F.linear(hin, params[f"layers.{i}.fc.weight"]).view(n, H, hidden)
        el = (ft * params[f"layers.{i}.attn_l"]).sum(-1)
        er = (ft * params[f"layers.{i}.attn_r"]).sum(-1)
        s = F.leaky_relu(el[src] + er[dst], slope)
        m = torch.full((n, H), -float("inf"), device=h.device).scatter_reduce(0, dst[:, None].expand(-1, H), s, "amax", include_self=True)
        ex = torch.exp(s - m[dst])
        den = torch.zeros(n, H, device=h.device).index_add_(0, dst, ex)
        a = F.dropout(ex / den[dst], adrop, training)
        rst = torch.zeros(n, H, hidden, device=h.device).index_add_(0, dst, a[:, :, None] * ft[src])
        h = F.leaky_relu(rst.reshape(n, H * hidden) + params[f"layers.{i}.bias"], 0.01)
    return torch.stack(outs).mean(0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--graphs", type=int, default=8)
    ap.add_argument("--nodes", type=int, default=10000)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("gat_bench.py measures on the GPU; none is visible")
    __graft_entry__.build()
    import wsi_hgnn_amd as W
    from wsi_hgnn_amd import _native as N, models, ops, synthetic
    from wsi_hgnn_amd.models.GAT import gat_plan
    from wsi_hgnn_amd.optim import Adam

    dev = torch.device("cuda:0")
    ops.set_gemm_precision("auto")
    torch.manual_seed(611)
    G = W.batch([synthetic.homogeneous_graph(args.nodes, 1024, seed=611 + i) for i in range(args.graphs)]).to(dev)
    y = (torch.arange(args.graphs) % 2).to(dev)
    plan = gat_plan(G)
    n, E = plan.num_nodes, plan.num_edges
    heads, hidden = [4, 4, 1], 512
    res = {"workload": "GAT_Kimia_v2 train step", "graphs": args.graphs, "nodes": n, "edges": E, "gemm": "auto",
           "steps": args.steps, "warmup": args.warmup}

    for mode, drop in (("eval", 0.0), ("train_drop0.2", 0.2)):
        m = models.GAT(2, 1024, hidden, 2, heads, F.leaky_relu, drop, drop, 0.2, False, "mean").to(dev)
        m.train(mode != "eval")
        live = [p for k, p in m.named_parameters() if k not in set(m.dead_parameter_names())]       # (the dead layer gets no gradient)
        opt = Adam(live, lr=1e-5)

        def step():
            opt.zero_grad(set_to_none=True)
            F.cross_entropy(m(G), y).backward()
            opt.step()
        res[f"hip_step_ms_{mode}"] = round(_time(step, args.steps, args.warmup), 3)

        dead = set(m.dead_parameter_names())
        params = {k: p.detach().clone().requires_grad_(True) for k, p in m.named_parameters() if k not in dead}
        topt = torch.optim.Adam(list(params.values()), lr=1e-5)
        src, dst = plan.src.long(), torch.repeat_interleave(torch.arange(n, device=dev), (plan.rowptr[1:] - plan.rowptr[:-1]).long())
        bnn = G.batch_num_nodes(G.ntypes[0]).to(dev)
        gid = torch.repeat_interleave(torch.arange(args.graphs, device=dev), bnn)
        x = G.ndata["feat"].float()

        def tstep():
            topt.zero_grad(set_to_none=True)
            out = torch_gat_forward(params, 2, heads, hidden, x, src, dst, gid, bnn.float(), args.graphs, 0.2, mode != "eval", drop, drop)
            F.cross_entropy(out, y).backward()
            topt.step()
        res[f"torch_step_ms_{mode}"] = round(_time(tstep, args.steps, args.warmup), 3)
        del m, opt, params, topt
        torch.cuda.empty_cache()

    # edge kernels alone at the hidden layers' shape (H = 4, D = 512), eval (no dropout), fused leaky_relu
    H, D = 4, hidden
    Fw = H * D
    lib = N.load()
    ft = torch.randn(n, Fw, device=dev)
    al = torch.randn(H * D, device=dev) * 0.05
    ar = torch.randn(H * D, device=dev) * 0.05
    bias = torch.zeros(Fw, device=dev)
    eler = torch.empty(n, 2 * H, device=dev)
    out = torch.empty(n, Fw, device=dev)
    lse = torch.empty(n, 2 * H, device=dev)
    g_out = torch.randn(n, Fw, device=dev)
    ws_bytes = lib.wsi_gat_attn_bwd_workspace_bytes(n, E, H, D, 2)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    g_ft = torch.empty(n, Fw, device=dev)
    g_al, g_ar, g_b = (torch.empty(Fw, device=dev) for _ in range(3))

    def scores():
        N.check(lib.wsi_gat_scores(N.ptr(ft), Fw, n, H, D, N.ptr(al), N.ptr(ar), N.ptr(eler), N.stream()), "scores")

    def fwd():
        N.check(lib.wsi_gat_attn_fwd(N.ptr(ft), Fw, N.ptr(eler), n, H, D, N.ptr(plan.rowptr), N.ptr(plan.src), N.ptr(plan.order_dst), 0.2,
                                     0, None, 0, 1.0, N.ptr(bias), 2, 0.01, N.ptr(out), Fw, N.ptr(lse), N.stream()), "fwd")

    def bwd():
        N.check(lib.wsi_gat_attn_bwd(N.ptr(ft), Fw, N.ptr(eler), N.ptr(lse), N.ptr(out), Fw, N.ptr(g_out), Fw, n, E, H, D,
                                     N.ptr(plan.rowptr), N.ptr(plan.src), N.ptr(plan.colptr), N.ptr(plan.csc_eid), N.ptr(plan.csc_dst),
                                     N.ptr(plan.order_src), N.ptr(al), N.ptr(ar), 0.2, 0, None, 0, 1.0, 2, 0.01, N.ptr(ws), ws_bytes,
                                     N.ptr(g_ft), Fw, N.ptr(g_al), N.ptr(g_ar), N.ptr(g_b), N.stream()), "bwd")
    row = Fw * 4
    t_sc = _time(scores, args.steps, args.warmup)
    t_fw = _time(fwd, args.steps, args.warmup)
    t_bw = _time(bwd, args.steps, args.warmup)
    # byte models (lower bounds: every gathered or streamed row counted once)
    b_sc = n * row
    b_fw = E * row + n * row                               # one ft[src] row per edge + the out row
    b_bw = E * row + 5 * n * row + n * row                 # pass A: one g_rst row per edge; prep g_out/out/g_rst; A ft + g_ft; C ft + g_ft r/w
    res["edge_kernels"] = {
        "shape": {"H": H, "D": D, "nodes": n, "edges": E},
        "scores_ms": round(t_sc, 4), "scores_GBs": round(b_sc / t_sc / 1e6, 1),
        "fwd_ms": round(t_fw, 4), "fwd_GBs": round(b_fw / t_fw / 1e6, 1),
        "bwd_ms": round(t_bw, 4), "bwd_GBs": round(b_bw / t_bw / 1e6, 1),
        "gather_ceiling_GBs": GATHER_CEILING_GBS,
        "fwd_share_of_ceiling": round(b_fw / t_fw / 1e6 / GATHER_CEILING_GBS, 3),
        "bwd_share_of_ceiling": round(b_bw / t_bw / 1e6 / GATHER_CEILING_GBS, 3),
    }
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
