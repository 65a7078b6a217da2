"""Source-major relation-attention backward (pass A, pass 2, pass C) against the dst-major one it replaced (passes 1, 2, 3).

Bit for bit: a child process bound to the measurement library runs wsi_heat_attn_bwd on the same inputs under WSI_ATTN_BWD=dst (dst-major
pass 1 + two-row pass 3) and under the default (source-major), and compares every output with torch.equal.  Against float64: the product
library's backward on graphs with isolated nodes, empty relation segments and sources without out-edges."""
import json
import os
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

pytestmark = pytest.mark.gpu

GRAPHS = ("uniform", "hub", "hub-coop", "sparse", "noedges")
CASES = [(D, H, kind) for D in (128, 256, 512) for H in (1, 4, 8) for kind in GRAPHS]
VARIANTS = [(gt_row, in_place) for gt_row in (False, True) for in_place in (False, True)]
OUTPUTS = ("g_q", "g_k", "g_v", "a", "ga", "gsc", "gea", "g_e", "absmax")


def _graph(kind, seed):
    """'sparse': one in-edge per destination slot on average, and a fourth node type that no relation reaches - isolated nodes (no
    segment at all), present-but-empty relation segments and sources without out-edges.  'noedges': every relation slot present, no edge at all
    (E = 0: every row of g_q / g_k / g_v and of the absmax table must still be written, as zeros)."""
    from wsi_hgnn_amd import synthetic, batch as gbatch
    if kind == "noedges":
        gs = [synthetic.hetero_graph(200, 8, seed=seed + i, edges_per_dst=0) for i in range(2)]
    elif kind == "sparse":
        gs = [synthetic.hetero_graph(300, 8, seed=seed + i, dst_mode="uniform", fractions=(0.4, 0.3, 0.2, 0.1), edges_per_dst=1)
              for i in range(2)]
    else:
        gs = [synthetic.hetero_graph(400, 8, seed=seed + i, dst_mode="uniform" if kind == "uniform" else "hub") for i in range(2)]
    return gbatch(gs)


def _key(D, H, kind, gt_row, in_place):
    return f"{D}-{H}-{kind}-{'gtrow' if gt_row else 'full'}-{'inplace' if in_place else 'score'}"


def _child(out_path):
    """Runs in a fresh process: measurement library, both backward forms per case, mismatching output names to JSON."""
    from wsi_hgnn_amd import _native as N
    N.use_measurement_library()
    lib = N.load()
    from wsi_hgnn_amd import ops, graph as graph_mod
    dev = torch.device("cuda:0")
    default_heavy = graph_mod.HEAVY_DEGREE
    results = {}
    for D, H, kind in CASES:
        graph_mod.HEAVY_DEGREE = 8 if kind == "hub-coop" else default_heavy
        g = _graph(kind, seed=31).to(dev)
        plan = g.plan()
        if kind == "hub-coop":
            assert plan.num_heavy > 0 and plan.heavy_degree == 8
        sim = g.cat_edata_csr("sim")
        n, E = plan.num_nodes, plan.num_edges
        assert (E == 0) == (kind == "noedges")
        Ea = max(E, 1)                                  # (per-edge buffers of one row when there is no edge, as ops.py sizes them)
        torch.manual_seed(D + H)
        kqv = torch.randn(n, 3 * D, device=dev) * 0.5
        ew, eb = torch.tensor([0.7], device=dev), torch.tensor([0.3], device=dev)
        graph_args = (N.ptr(plan.node_seg), N.ptr(plan.rowptr), N.ptr(plan.src), N.ptr(sim), N.ptr(plan.order_dst), plan.num_heavy,
                      ops._attn_flags(plan), N.ptr(ew), N.ptr(eb))
        t = torch.empty(n, D, device=dev)
        score = torch.zeros(Ea, H, device=dev)
        lse = torch.zeros(plan.num_segs, H, device=dev)
        N.check(lib.wsi_heat_attn_fwd(N.ptr(kqv, D * 4), 3 * D, N.ptr(kqv), 3 * D, N.ptr(kqv, 8 * D), 3 * D, n, D, H, *graph_args,
                                      N.ptr(t), D, N.ptr(score), N.ptr(lse), None, N.context(), N.stream()), "fwd")
        g_full = torch.randn(n, D, device=dev)
        g_few = torch.randn(5, D, device=dev)
        row_of = torch.randint(0, 5, (n,), device=dev, dtype=torch.int32)
        for gt_row, in_place in VARIANTS:
            outs = {}
            for form in ("dst", "src"):
                if form == "dst":
                    os.environ["WSI_ATTN_BWD"] = "dst"
                else:
                    os.environ.pop("WSI_ATTN_BWD", None)
                a = score.clone() if in_place else torch.full_like(score, -3.0)
                scratch = torch.full((3, Ea, H), -5.0, device=dev)
                red_ws = torch.empty(1024, device=dev)
                gkqv = torch.full((n, 3 * D), -7.0, device=dev)
                g_e = torch.empty(2, device=dev)
                absmax = torch.full((2 * n,), -1, dtype=torch.int32, device=dev)
                g_t = g_few if gt_row else g_full
                N.check(lib.wsi_heat_attn_bwd(
                    N.ptr(kqv, D * 4), 3 * D, N.ptr(kqv), 3 * D, N.ptr(kqv, 8 * D), 3 * D, n, plan.num_src_rows, E, D, H,
                    N.ptr(plan.node_seg), N.ptr(plan.rowptr), N.ptr(plan.src), N.ptr(sim), N.ptr(plan.colptr), N.ptr(plan.csc_eid),
                    N.ptr(plan.csc_dst), N.ptr(plan.inv_rd), N.ptr(plan.order_dst), plan.num_heavy, N.ptr(plan.order_src),
                    ops._attn_flags(plan), N.ptr(ew), N.ptr(eb),
                    N.ptr(g_t), D, N.ptr(row_of) if gt_row else None, None if in_place else N.ptr(score), N.ptr(a), N.ptr(lse),
                    N.ptr(scratch[0]), N.ptr(scratch[1]), N.ptr(scratch[2]), N.ptr(red_ws),
                    N.ptr(gkqv, D * 4), 3 * D, N.ptr(gkqv), 3 * D, N.ptr(gkqv, 8 * D), 3 * D,
                    N.ptr(g_e), N.ptr(absmax), None, N.context(), N.stream()), f"bwd ({form})")
                torch.cuda.synchronize()
                outs[form] = dict(g_q=gkqv[:, D:2 * D], g_k=gkqv[:, :D], g_v=gkqv[:, 2 * D:], a=a, ga=scratch[0], gsc=scratch[1],
                                  gea=scratch[2], g_e=g_e, absmax=absmax)
            os.environ.pop("WSI_ATTN_BWD", None)
            bad = [k for k in OUTPUTS if not torch.equal(outs["dst"][k], outs["src"][k])]
            if E == 0:                                  # no edge: the gradients and the absmax table are zeros in every row, in both forms
                for form in ("dst", "src"):
                    o = outs[form]
                    if not (torch.all(o["g_q"] == 0) and torch.all(o["g_k"] == 0) and torch.all(o["g_v"] == 0) and torch.all(o["absmax"] == 0)):
                        bad.append(f"nonzero_without_edges_{form}")
            results[_key(D, H, kind, gt_row, in_place)] = bad
    graph_mod.HEAVY_DEGREE = default_heavy
    with open(out_path, "w") as f:
        json.dump(results, f)


@pytest.fixture(scope="module")
def bit_results(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("srcmajor") / "results.json")
    env = {k: v for k, v in os.environ.items() if not k.startswith("WSI_")}
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", out], cwd=ROOT, env=env, capture_output=True, text=True,
                       timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    with open(out) as f:
        return json.load(f)


@pytest.mark.parametrize("D,H,kind", CASES)
def test_source_major_backward_bit_identical(D, H, kind, bit_results):
    for gt_row, in_place in VARIANTS:
        key = _key(D, H, kind, gt_row, in_place)
        assert key in bit_results, key
        assert bit_results[key] == [], (key, bit_results[key])


@pytest.mark.parametrize("D,H", [(128, 1), (128, 8), (256, 4), (512, 1), (512, 4), (512, 8)])
def test_source_major_backward_against_float64_sparse_graph(D, H):
    from wsi_hgnn_amd import ops
    from oracle import kernel_ref
    dev = torch.device("cuda:0")
    g = _graph("sparse", seed=17).to(dev)
    plan = g.plan()
    sim = g.cat_edata_csr("sim")
    torch.manual_seed(3)
    kqv = (torch.randn(plan.num_nodes, 3 * D, device=dev) * 0.5).requires_grad_()
    ew = torch.tensor([[0.7]], device=dev, requires_grad=True)
    eb = torch.tensor([0.3], device=dev, requires_grad=True)
    t = ops.heat_attention(kqv, ew, eb, plan, sim, D, H)
    gt = torch.randn_like(t)
    t.backward(gt)
    pc = kernel_ref.plan_to_cpu(plan)
    kd = kqv.detach().double().cpu().requires_grad_()
    ewd = ew.detach().double().cpu().requires_grad_()
    ebd = eb.detach().double().cpu().requires_grad_()
    ref = kernel_ref.heat_attention_ref(kd, ewd, ebd, pc, sim.double().cpu(), D, H)
    ref.backward(gt.double().cpu())
    rel = lambda x, y: ((x.detach().double().cpu() - y).abs().max() / y.abs().max().clamp(min=1e-30)).item()
    assert rel(t, ref) < 1e-5
    assert rel(kqv.grad[:, D:2 * D], kd.grad[:, D:2 * D]) < 1e-4, "g_q"
    assert rel(kqv.grad[:, :D], kd.grad[:, :D]) < 1e-4, "g_k"
    assert rel(kqv.grad[:, 2 * D:], kd.grad[:, 2 * D:]) < 1e-4, "g_v"
    assert abs(ew.grad.item() - ewd.grad.item()) < 1e-4 * max(1.0, abs(ewd.grad.item()))
    assert abs(eb.grad.item() - ebd.grad.item()) < 1e-4 * max(1.0, abs(ebd.grad.item()))


if __name__ == "__main__" and len(sys.argv) == 3 and sys.argv[1] == "--child":
    _child(sys.argv[2])
