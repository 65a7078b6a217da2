"""Relation-attention backward of the bench batch (8 x 10k nodes, D = 512, H = 4, full depth): the dst-major form (pass 1 + two-row pass 3,
measurement build: WSI_ATTN_BWD=dst) against the source-major form (pass A + pass C) with U = 2 / 4 / 8 CSC entries in flight per wave in each of
A and C (WSI_ATTN_SRC_U = "<U_A><U_C>").  Median time of the whole wsi_heat_attn_bwd call, and whether its outputs equal the dst-major ones bit
for bit.  `--dst-mode hub` for the hub-destination batch.  GPU."""
import json, os, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from wsi_hgnn_amd import _native as N
N.use_measurement_library()
from wsi_hgnn_amd import ops, synthetic
lib = N.load()
dev = torch.device("cuda:0")
dst_mode = sys.argv[sys.argv.index("--dst-mode") + 1] if "--dst-mode" in sys.argv else "uniform"
g, _ = synthetic.hetero_batch(8, 10000, in_dim=8, dst_mode=dst_mode)
g = g.to(dev)
plan = g.plan()
sim = g.cat_edata_csr("sim")
D, H = 512, 4
n, E, S = plan.num_nodes, plan.num_edges, plan.num_segs
torch.manual_seed(3)
kqv = torch.randn(n, 3 * D, device=dev) * 0.5
ew, eb = torch.tensor([0.7], device=dev), torch.tensor([0.3], device=dev)
t = torch.empty(n, D, device=dev); score = torch.empty(E, H, device=dev); lse = torch.zeros(S, H, device=dev)
graph = (N.ptr(plan.node_seg), N.ptr(plan.rowptr), N.ptr(plan.src), N.ptr(sim))
N.check(lib.wsi_heat_attn_fwd(N.ptr(kqv, D * 4), 3 * D, N.ptr(kqv), 3 * D, N.ptr(kqv, 8 * D), 3 * D, n, D, H, *graph, N.ptr(plan.order_dst),
                              plan.num_heavy, ops._attn_flags(plan), N.ptr(ew), N.ptr(eb), N.ptr(t), D, N.ptr(score), N.ptr(lse), None,
                              N.context(), N.stream()), "fwd")
g_t = torch.randn(n, D, device=dev)
a = torch.empty_like(score)
scratch = torch.empty(3, E, H, device=dev)
red_ws = torch.empty(1024, device=dev)
gkqv = torch.empty(n, 3 * D, device=dev)
g_e = torch.empty(2, device=dev)
absmax = torch.empty(2 * n, dtype=torch.int32, device=dev)


def bwd():
    N.check(lib.wsi_heat_attn_bwd(
        N.ptr(kqv, D * 4), 3 * D, N.ptr(kqv), 3 * D, N.ptr(kqv, 8 * D), 3 * D, n, plan.num_src_rows, E, D, H, *graph,
        N.ptr(plan.colptr), N.ptr(plan.csc_eid), N.ptr(plan.csc_dst), N.ptr(plan.inv_rd), N.ptr(plan.order_dst), plan.num_heavy,
        N.ptr(plan.order_src), ops._attn_flags(plan), N.ptr(ew), N.ptr(eb), N.ptr(g_t), D, None, N.ptr(score), N.ptr(a), N.ptr(lse),
        N.ptr(scratch[0]), N.ptr(scratch[1]), N.ptr(scratch[2]), N.ptr(red_ws), N.ptr(gkqv, D * 4), 3 * D, N.ptr(gkqv), 3 * D,
        N.ptr(gkqv, 8 * D), 3 * D, N.ptr(g_e), N.ptr(absmax), None, N.context(), N.stream()), "bwd")


def outputs():
    return [x.clone() for x in (gkqv, a, scratch, g_e, absmax)]


out, ref = {"dst_mode": dst_mode, "E": E, "N": n}, None
for cfg in ("dst", "src:22", "src:44", "src:88", "src:24", "src:42", "src:48", "src:84", "dst", "src:default"):
    os.environ.pop("WSI_ATTN_SRC_U", None)
    os.environ["WSI_ATTN_BWD"] = "dst" if cfg == "dst" else "src"
    if cfg.startswith("src:") and cfg != "src:default":
        os.environ["WSI_ATTN_SRC_U"] = cfg[4:]
    for _ in range(3):
        bwd()
    torch.cuda.synchronize()
    ts = []
    for _ in range(30):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); bwd(); e1.record(); e1.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e3)
    o = outputs()
    if ref is None:
        ref = o
    same = all(torch.equal(x, y) for x, y in zip(o, ref))
    out.setdefault(cfg, []).append({"us": round(statistics.median(ts), 1), "bit_equal_to_dst": same})
    print(f"{cfg}: {statistics.median(ts):.1f} us, bit-equal to dst: {same}", flush=True)
if "--out" in sys.argv:
    json.dump(out, open(sys.argv[sys.argv.index("--out") + 1], "w"), indent=1)
