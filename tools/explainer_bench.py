#!/usr/bin/env python
"""GNNExplainer timing: ONE explainer epoch (masked forward, the regularised loss, backward to the two masks, torch Adam on the masks;
explainers/gnn_explainer.py) on a single synthetic.homogeneous_graph(10000) slide (10k nodes, ~90k edges), one GPU, 'auto' GEMMs, through
  * GCN(1024, 512, 2, n_layers=3, relu, mean readout)            - wsi_spmm_sum with edge_w + wsi_sddmm_dot
  * GAT(2, 1024, 512, 2, heads [4, 4, 1], mean readout)          - wsi_gat_attn_fwd_scaled / wsi_gat_attn_bwd_scaled (GAT_Kimia_v2 widths)
against the same epoch restated in plain PyTorch (index_add_ / scatter_reduce, torch GEMMs) on the same GPU, and HIP-event times of
the scaled and unscaled edge kernels side by side (GAT at H = 4, D = 512; GraphConv at D = 512).  Prints one JSON line (and writes it
to --out when given).  --unscaled-check FILE embeds a JSON file (tools/gat_bench.py results of this commit and of its parent, taken in
the same session) under "unscaled_gat_check".

    python tools/explainer_bench.py --steps 20 --warmup 5 [--out profiles/r08_gnn_explainer.json]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn.functional as F

import __graft_entry__


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


def torch_gcn_forward(params, n_layers, x, scale, src, dst, in_norm, out_norm):
    """models/GCN.py (mean readout, eval) in plain PyTorch with the explainer's message mask."""
    h, outs, n = x, [], x.shape[0]

    def agg(z):
        return torch.zeros(n, z.shape[1], device=z.device).index_add_(0, dst, z[src] * (out_norm[src] * scale)[:, None]) * in_norm[:, None]
    for i in range(n_layers):
        outs.append(F.linear(h.mean(0, keepdim=True), params[f"linears_prediction.{i}.weight"], params[f"linears_prediction.{i}.bias"]))
        w, b = params[f"layers.{i}.weight"], params[f"layers.{i}.bias"]
        h = F.relu(agg(h @ w) + b) if w.shape[0] > w.shape[1] else F.relu(agg(h) @ w + b)
    outs.append(F.linear(h.mean(0, keepdim=True), params["classify.weight"], params["classify.bias"]))
    return torch.stack(outs).mean(0)


def torch_gat_forward(params, n_layers, heads, hidden, x, scale, src, dst, slope):
    """models/GAT.py (mean readout, eval) in plain PyTorch with the explainer's message mask (after the edge softmax)."""
    h, outs, n = x, [], x.shape[0]
    for i in range(n_layers + 1):
        outs.append(F.linear(h.mean(0, keepdim=True), params[f"linears_prediction.{i}.weight"], params[f"linears_prediction.{i}.bias"]))
        if i == n_layers:
            break
        H = heads[i]
        ft = F.linear(h, params[f"layers.{i}.fc.weight"]).view(n, H, hidden)
        el = (ft * params[f"layers.{i}.attn_l"]).sum(-1)
        er = (ft * params[f"layers.{i}.attn_r"]).sum(-1)
        s = F.leaky_relu(el[src] + er[dst], slope)
        m = torch.full((n, H), -float("inf"), device=h.device).scatter_reduce(0, dst[:, None].expand(-1, H), s, "amax", include_self=True)
        ex = torch.exp(s - m[dst])
        den = torch.zeros(n, H, device=h.device).index_add_(0, dst, ex)
        a = ex / den[dst] * scale[:, None]
        rst = torch.zeros(n, H, hidden, device=h.device).index_add_(0, dst, a[:, :, None] * ft[src])
        h = F.leaky_relu(rst.reshape(n, H * hidden) + params[f"layers.{i}.bias"], 0.01)
    return torch.stack(outs).mean(0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--nodes", type=int, default=10000)
    ap.add_argument("--out", default=None)
    ap.add_argument("--unscaled-check", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("explainer_bench.py measures on the GPU; none is visible")
    __graft_entry__.build()
    from wsi_hgnn_amd import _native as N, graph as G, models, ops, synthetic
    from wsi_hgnn_amd.explainers import GNNExplainer, ExplainerTags
    from wsi_hgnn_amd.explainers.gnn_explainer import mask_loss
    from wsi_hgnn_amd.models.GAT import gat_plan
    from wsi_hgnn_amd.models.GCN import homo_plan

    dev = torch.device("cuda:0")
    ops.set_gemm_precision("auto")
    g = synthetic.homogeneous_graph(args.nodes, 1024, seed=611).to(dev)
    plan, hp = gat_plan(g), homo_plan(g)
    n, E = plan.num_nodes, plan.num_edges
    src = plan.src.long()
    dst = torch.repeat_interleave(torch.arange(n, device=dev), (plan.rowptr[1:] - plan.rowptr[:-1]).long())
    perm = g._csr_perm()
    feat = g.ndata["feat"].float()
    res = {"workload": "GNNExplainer epoch, one slide", "nodes": n, "edges": E, "gemm": "auto", "steps": args.steps, "warmup": args.warmup}

    for kind in ("gcn", "gat"):
        torch.manual_seed(611)
        if kind == "gcn":
            m = models.GCN(1024, 512, 2, 3, F.relu, 0.0, "mean").to(dev).eval()
        else:
            m = models.GAT(2, 1024, 512, 2, [4, 4, 1], F.leaky_relu, 0.2, 0.2, 0.2, False, "mean").to(dev).eval()
        ex = GNNExplainer(g, m, num_hops=3 if kind == "gcn" else 2)
        with torch.no_grad():
            pred = m(g).argmax(dim=-1)
        sub = ex._create_subgraph(None)
        ex.__set_masks__(sub)
        edge_mask = sub.edata[ExplainerTags.EDGE_MASK]
        opt = torch.optim.Adam([ex.node_mask, edge_mask], lr=ex.lr)
        for p in m.parameters():
            p.requires_grad_(False)

        def epoch():                                            # the body of GNNExplainer.explain_node's loop
            h = ex.__apply_feature_mask__(feat, ex.node_mask)
            with G.message_scale(sub, edge_mask.sigmoid()):
                logits = m(sub, h)
            loss = ex.__loss__(sub, None, logits, pred)
            opt.zero_grad()
            loss.backward()
            opt.step()
        res[f"hip_epoch_ms_{kind}"] = round(_time(epoch, args.steps, args.warmup), 3)

        params = {k: p.detach() for k, p in m.named_parameters()}
        tnode = ex.node_mask.detach().clone().requires_grad_(True)
        tedge = edge_mask.detach().clone().requires_grad_(True)
        topt = torch.optim.Adam([tnode, tedge], lr=ex.lr)

        def tepoch():
            h = feat * tnode.sigmoid()[:, None]
            s = tedge.sigmoid()[perm]
            if kind == "gcn":
                logits = torch_gcn_forward(params, 3, h, s, src, dst, hp.in_norm, hp.out_norm)
            else:
                logits = torch_gat_forward(params, 2, [4, 4, 1], 512, h, s, src, dst, 0.2)
            loss = mask_loss(-logits.view(-1)[pred], tedge.sigmoid(), tnode.sigmoid(), ex.params)
            topt.zero_grad()
            loss.backward()
            topt.step()
        res[f"torch_epoch_ms_{kind}"] = round(_time(tepoch, args.steps, args.warmup), 3)
        res[f"speedup_{kind}"] = round(res[f"torch_epoch_ms_{kind}"] / res[f"hip_epoch_ms_{kind}"], 2)
        del m, ex, opt, topt, params
        torch.cuda.empty_cache()

    # ---- edge kernels alone, scaled next to unscaled
    lib = N.load()
    H, D = 4, 512
    Fw = H * D
    row = Fw * 4
    ft = torch.randn(n, Fw, device=dev)
    al, ar = torch.randn(Fw, device=dev) * 0.05, torch.randn(Fw, device=dev) * 0.05
    bias = torch.zeros(Fw, device=dev)
    eler, lse = torch.empty(n, 2 * H, device=dev), torch.empty(n, 2 * H, device=dev)
    out, g_out, g_ft = torch.empty(n, Fw, device=dev), torch.randn(n, Fw, device=dev), torch.empty(n, Fw, device=dev)
    ws_bytes = lib.wsi_gat_attn_bwd_workspace_bytes(n, E, H, D, 2)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    g_al, g_ar, g_b = (torch.empty(Fw, device=dev) for _ in range(3))
    scale, g_scale = torch.rand(E, device=dev), torch.empty(E, device=dev)
    N.check(lib.wsi_gat_scores(N.ptr(ft), Fw, n, H, D, N.ptr(al), N.ptr(ar), N.ptr(eler), N.stream()), "scores")
    topo = (N.ptr(plan.rowptr), N.ptr(plan.src))
    csc = (N.ptr(plan.colptr), N.ptr(plan.csc_eid), N.ptr(plan.csc_dst), N.ptr(plan.order_src))

    def fwd():
        N.check(lib.wsi_gat_attn_fwd(N.ptr(ft), Fw, N.ptr(eler), n, H, D, *topo, N.ptr(plan.order_dst), 0.2, 0, None, 0, 1.0, N.ptr(bias), 2, 0.01,
                                     N.ptr(out), Fw, N.ptr(lse), N.stream()), "fwd")

    def fwd_s():
        N.check(lib.wsi_gat_attn_fwd_scaled(N.ptr(ft), Fw, N.ptr(eler), n, H, D, *topo, N.ptr(plan.order_dst), 0.2, 0, None, 0, 1.0, N.ptr(bias), 2, 0.01,
                                            N.ptr(scale), N.ptr(out), Fw, N.ptr(lse), N.stream()), "fwd_scaled")

    def bwd():
        N.check(lib.wsi_gat_attn_bwd(N.ptr(ft), Fw, N.ptr(eler), N.ptr(lse), N.ptr(out), Fw, N.ptr(g_out), Fw, n, E, H, D, *topo, *csc, N.ptr(al), N.ptr(ar),
                                     0.2, 0, None, 0, 1.0, 2, 0.01, N.ptr(ws), ws_bytes, N.ptr(g_ft), Fw, N.ptr(g_al), N.ptr(g_ar), N.ptr(g_b), N.stream()), "bwd")

    def bwd_s():
        N.check(lib.wsi_gat_attn_bwd_scaled(N.ptr(ft), Fw, N.ptr(eler), N.ptr(lse), N.ptr(out), Fw, N.ptr(g_out), Fw, n, E, H, D, *topo, *csc, N.ptr(al),
                                            N.ptr(ar), 0.2, 0, None, 0, 1.0, 2, 0.01, N.ptr(scale), N.ptr(ws), ws_bytes, N.ptr(g_ft), Fw, N.ptr(g_al),
                                            N.ptr(g_ar), N.ptr(g_b), N.ptr(g_scale), N.stream()), "bwd_scaled")
    t = {k: _time(f, args.steps, args.warmup) for k, f in (("fwd", fwd), ("fwd_scaled", fwd_s), ("bwd", bwd), ("bwd_scaled", bwd_s))}
    b_fw, b_bw = E * row + n * row, E * row + 6 * n * row           # the byte models of tools/gat_bench.py; the scale adds 4-12 B per edge
    res["gat_edge_kernels"] = {"shape": {"H": H, "D": D, "nodes": n, "edges": E},
                               **{f"{k}_ms": round(v, 4) for k, v in t.items()},
                               "fwd_GBs": round(b_fw / t["fwd"] / 1e6, 1), "fwd_scaled_GBs": round((b_fw + 4 * E) / t["fwd_scaled"] / 1e6, 1),
                               "bwd_GBs": round(b_bw / t["bwd"] / 1e6, 1), "bwd_scaled_GBs": round((b_bw + 12 * E) / t["bwd_scaled"] / 1e6, 1)}

    Dg = 512
    z, gy, y, gz = (torch.randn(n, Dg, device=dev) for _ in range(4))
    s_csc = scale[plan.csc_eid.long()]

    def spmm(w):
        return lambda: N.check(lib.wsi_spmm_sum(N.ptr(z), Dg, n, Dg, *topo, N.ptr(w), N.ptr(hp.out_norm), N.ptr(hp.in_norm), None, 1, None, 0,
                                                N.ptr(y), Dg, N.stream()), "spmm")

    def spmm_bwd(w):
        return lambda: N.check(lib.wsi_spmm_sum(N.ptr(gy), Dg, n, Dg, N.ptr(hp.colptr), N.ptr(hp.csc_dst), N.ptr(w), N.ptr(hp.in_norm), N.ptr(hp.out_norm),
                                                None, 0, N.ptr(y), Dg, N.ptr(gz), Dg, N.stream()), "spmm_bwd")

    def sddmm():
        N.check(lib.wsi_sddmm_dot(N.ptr(gy), Dg, N.ptr(z), Dg, n, Dg, *topo, N.ptr(hp.out_norm), N.ptr(hp.in_norm), N.ptr(y), Dg, N.ptr(g_scale),
                                  N.stream()), "sddmm")
    t = {k: _time(f, args.steps, args.warmup) for k, f in (("spmm_fwd", spmm(None)), ("spmm_fwd_scaled", spmm(scale)), ("spmm_bwd", spmm_bwd(None)),
                                                            ("spmm_bwd_scaled", spmm_bwd(s_csc)), ("sddmm_dot", sddmm))}
    rg = Dg * 4
    res["graphconv_edge_kernels"] = {"shape": {"D": Dg, "nodes": n, "edges": E}, **{f"{k}_ms": round(v, 4) for k, v in t.items()},
                                     "sddmm_dot_GBs": round((E * rg + 2 * n * rg + 4 * E) / t["sddmm_dot"] / 1e6, 1)}   # x[u] per edge + g[w], relu_ref[w] per node + g_w
    if args.unscaled_check:
        res["unscaled_gat_check"] = json.load(open(args.unscaled_check))
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
