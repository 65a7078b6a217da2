"""Relation attention (csrc/heat_attn.hip) through the C ABI at scores where the softmax maximum matters, against float64
(tests/attn_peak_cases.py: graph, exact-score inputs, patterns, restatement, bounds; tests/test_attn_peak_cases.py holds those without a GPU and
shows that a wrong maximum breaks these bounds here and none of them at the score scale of the other tests).

  a. wsi_heat_attn_fwd at the ten (D, H) of attn_peak_cases.CONFIGS, plain plan and hub plan (the generic kernels once): score EQUAL to the
     float64 scores where d_k is a power of 4, lse and t within bound, nothing non-finite, every row of t written;
  b. wsi_heat_attn_scores_fwd == the full forward's score and lse, bit for bit;
  c. wsi_heat_attn_bwd without a pool descriptor, score passed separately and in place: a, g_q, g_k, g_v, g_e within bound, sum a = 1;
  d. identical calls on the hub plan give identical bits;
  e. HGT's layout (ops.relation_attention on a per_relation_src plan, e_weight = 0) and ops.heat_attention through autograd, at (256, 4).
Every output buffer starts as NaN.  The largest error / bound per tensor and configuration is printed when the module ends."""
import functools

import pytest
import torch

import attn_peak_cases as C

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAN = float("nan")
PLANS = [(D, H, hub) for D, H in C.SPECIALISED for hub in (False, True)] + [(D, H, False) for D, H in C.GENERIC]
RESULTS = {}


def _group(D, H, hub):
    return "generic" if (D, H) in C.GENERIC else ("hub" if hub else "plain")


def _hold(rs, group, D, H, limit=1.0):
    slot = RESULTS.setdefault((group, D, H), {})
    for name, r in rs.items():
        print(f"{group} D={D} H={H} {name}: error / bound {r:.3e}")
        slot[name] = max(slot.get(name, 0.0), r)
    bad = {k: v for k, v in rs.items() if not v <= limit}
    assert not bad, f"{group} D={D} H={H}: error / bound above {limit}: {bad}"


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    print()
    for (group, D, H), slot in RESULTS.items():
        print(f"largest error / bound, {group} D={D} H={H}: " + "  ".join(f"{k} {v:.3f}" for k, v in sorted(slot.items())))


class _Graph:
    pass


@functools.lru_cache(maxsize=None)
def on_device(hub):
    """The case's graph on the GPU with plans of its own (hub: built under graph.HEAVY_DEGREE = 8), checked against the CPU plans."""
    from wsi_hgnn_amd.graph import _build_plan
    c = C.graph_case()
    d = _Graph()
    d.g = c.g.to(DEV)
    if hub:
        with C.heavy_degree(C.HUB_DEGREE):
            d.plan, d.rel_plan = _build_plan(d.g), _build_plan(d.g, per_relation_src=True)
    else:
        d.plan, d.rel_plan = _build_plan(d.g), _build_plan(d.g, per_relation_src=True)
    want = c.hub_plan if hub else c.plan
    for name in ("src", "rowptr", "node_seg", "colptr", "csc_eid", "csc_dst"):
        assert torch.equal(getattr(d.plan, name).cpu(), getattr(want, name)), name
    for name in ("src", "rowptr", "node_seg"):
        assert torch.equal(getattr(d.rel_plan, name).cpu(), getattr(c.rel_plan, name)), name
    assert d.plan.num_src_rows == d.plan.num_nodes == c.n and d.plan.heavy_degree == want.heavy_degree and d.plan.num_segs == c.S
    assert (d.plan.num_heavy > 0) == hub and (d.rel_plan.num_heavy > 0) == hub and d.rel_plan.num_src_rows == c.rel_plan.num_src_rows
    assert torch.equal(C.hub_mask(d.plan), c.hub if hub else torch.zeros(c.n, dtype=torch.bool))
    return d


def _graph_args(d, sim):
    from wsi_hgnn_amd import ops, _native as N
    p = d.plan
    return (N.ptr(p.node_seg), N.ptr(p.rowptr), N.ptr(p.src), N.ptr(sim), N.ptr(p.order_dst), p.num_heavy, ops._attn_flags(p))


@functools.lru_cache(maxsize=4)
def device_inputs(D, H):
    x = C.inputs(D, H)
    s = {k: x[k].to(DEV).contiguous() for k in ("sim", "ew", "eb", "gt")}
    s["kqv"] = torch.cat([x["k"], x["q"], x["v"]], dim=1).to(DEV).contiguous()
    return s


def run_fwd(D, H, hub):
    from wsi_hgnn_amd import _native as N
    c, d, s = C.graph_case(), on_device(hub), device_inputs(D, H)
    t, score, lse = torch.full((c.n, D), NAN, device=DEV), torch.full((c.E, H), NAN, device=DEV), torch.full((c.S, H), NAN, device=DEV)
    N.check(N.load().wsi_heat_attn_fwd(N.ptr(s["kqv"], D * 4), 3 * D, N.ptr(s["kqv"]), 3 * D, N.ptr(s["kqv"], 8 * D), 3 * D, c.n, D, H,
                                       *_graph_args(d, s["sim"]), N.ptr(s["ew"]), N.ptr(s["eb"]), N.ptr(t), D, N.ptr(score), N.ptr(lse), None,
                                       N.context(), N.stream()), "fwd")
    torch.cuda.synchronize()
    return {"t": t, "score": score, "lse": lse}


def run_bwd(D, H, hub, fwd, in_place):
    """One wsi_heat_attn_bwd call without a pool descriptor on the forward's saved score and lse; every output starts as NaN."""
    from wsi_hgnn_amd import ops, _native as N
    c, d, s = C.graph_case(), on_device(hub), device_inputs(D, H)
    p, n, E = d.plan, c.n, c.E
    a = fwd["score"].clone() if in_place else torch.full((E, H), NAN, device=DEV)
    score = fwd["score"].clone()
    scratch, red_ws = torch.full((3, E, H), NAN, device=DEV), torch.empty(1024, device=DEV)
    g, g_e = torch.full((n, 3 * D), NAN, device=DEV), torch.full((2,), NAN, device=DEV)
    N.check(N.load().wsi_heat_attn_bwd(
        N.ptr(s["kqv"], D * 4), 3 * D, N.ptr(s["kqv"]), 3 * D, N.ptr(s["kqv"], 8 * D), 3 * D, n, p.num_src_rows, E, D, H,
        N.ptr(p.node_seg), N.ptr(p.rowptr), N.ptr(p.src), N.ptr(s["sim"]), N.ptr(p.colptr), N.ptr(p.csc_eid), N.ptr(p.csc_dst),
        N.ptr(p.inv_rd), N.ptr(p.order_dst), p.num_heavy, N.ptr(p.order_src), ops._attn_flags(p), N.ptr(s["ew"]), N.ptr(s["eb"]),
        N.ptr(s["gt"]), D, None, None if in_place else N.ptr(score), N.ptr(a), N.ptr(fwd["lse"]),
        N.ptr(scratch[0]), N.ptr(scratch[1]), N.ptr(scratch[2]), N.ptr(red_ws),
        N.ptr(g, D * 4), 3 * D, N.ptr(g), 3 * D, N.ptr(g, 8 * D), 3 * D, N.ptr(g_e), None, None, N.context(), N.stream()), "bwd")
    torch.cuda.synchronize()
    assert torch.equal(score, fwd["score"]), "the saved logits are read only"
    return {"a": a, "g_k": g[:, :D], "g_q": g[:, D:2 * D], "g_v": g[:, 2 * D:], "g_e": g_e, "g": g}


def _live():
    return C.graph_case().seg_len > 0


# ------------------------------------------------------------------------------------------ a. forward
@pytest.mark.parametrize("D,H,hub", PLANS)
def test_forward_against_float64(D, H, hub):
    c, ref, out = C.graph_case(), C.evaluate(D, H), run_fwd(D, H, hub)
    if C.exact(D, H):
        assert torch.equal(out["score"].double().cpu(), ref["score"]), "exactly representable scores come out exact"
    else:
        assert float((out["score"].double().cpu() - ref["score"]).abs().max()) <= 2.0 ** -22 * float(ref["score"].abs().max())
    live = _live()
    assert bool(torch.isfinite(out["score"]).all()) and bool(torch.isfinite(out["t"]).all()) and bool(torch.isfinite(out["lse"].cpu()[live]).all())
    indeg = torch.bincount(c.dst, minlength=c.n)
    assert bool((indeg == 0).any()) and bool((out["t"].cpu()[indeg == 0] == 0).all()), "rows without in-edges are written, as zeros"
    _hold(C.ratios({"t": out["t"], "lse": out["lse"]}, ref, D, H, hub), _group(D, H, hub), D, H)


# ------------------------------------------------------------------------------------------ b. scores forward == full forward
@pytest.mark.parametrize("hub", [False, True])
@pytest.mark.parametrize("D,H", C.SPECIALISED)
def test_scores_fwd_equals_the_full_forward_bit_for_bit(D, H, hub):
    from wsi_hgnn_amd import _native as N
    c, d, s, full = C.graph_case(), on_device(hub), device_inputs(D, H), run_fwd(D, H, hub)
    score, lse = torch.full((c.E, H), NAN, device=DEV), torch.full((c.S, H), NAN, device=DEV)
    N.check(N.load().wsi_heat_attn_scores_fwd(N.ptr(s["kqv"], D * 4), 3 * D, N.ptr(s["kqv"]), 3 * D, c.n, D, H, *_graph_args(d, s["sim"]),
                                              N.ptr(s["ew"]), N.ptr(s["eb"]), N.ptr(score), N.ptr(lse), N.context(), N.stream()), "scores")
    torch.cuda.synchronize()
    live = _live().to(DEV)
    assert torch.equal(score.view(torch.int32), full["score"].view(torch.int32))
    assert torch.equal(lse[live].view(torch.int32), full["lse"][live].view(torch.int32)) and bool(torch.isfinite(lse[live]).all())
    assert bool(torch.isnan(lse[~live]).all()) and bool(torch.isnan(full["lse"][~live]).all()), "an empty segment has no lse: its row is left alone"


# ------------------------------------------------------------------------------------------ c. backward
@pytest.mark.parametrize("in_place", [False, True])
@pytest.mark.parametrize("D,H,hub", PLANS)
def test_backward_against_float64(D, H, hub, in_place):
    c, ref = C.graph_case(), C.evaluate(D, H)
    out = run_bwd(D, H, hub, run_fwd(D, H, hub), in_place)
    assert bool(torch.isfinite(out["g"]).all()) and bool(torch.isfinite(out["a"]).all()) and bool(torch.isfinite(out["g_e"]).all())
    rs = C.ratios({k: out[k] for k in ("a", "g_q", "g_k", "g_v", "g_e")}, ref, D, H, hub)
    rs["sum a"] = C.sum_a_ratio(out["a"], ref)
    plain = C.ratios({"g_e": out["g_e"]}, ref, D, H, hub, g_e_term=False)["g_e"]
    print(f"{_group(D, H, hub)} D={D} H={H} g_e under the plain 1e-4 max(1, |ref|), without the derived lse term: error / bound {plain:.3e}")
    _hold(rs, _group(D, H, hub), D, H)
    indeg, outdeg = torch.bincount(c.dst, minlength=c.n), torch.bincount(c.src, minlength=c.n)
    assert bool((out["g_q"].cpu()[indeg == 0] == 0).all()) and bool((out["g_k"].cpu()[outdeg == 0] == 0).all()) and bool((out["g_v"].cpu()[outdeg == 0] == 0).all())


# ------------------------------------------------------------------------------------------ d. repeatability
@pytest.mark.parametrize("D,H", C.SPECIALISED)
def test_identical_calls_on_the_hub_plan_give_identical_bits(D, H):
    f1, f2 = run_fwd(D, H, True), run_fwd(D, H, True)
    live = _live().to(DEV)
    assert torch.equal(f1["t"].view(torch.int32), f2["t"].view(torch.int32)) and torch.equal(f1["score"].view(torch.int32), f2["score"].view(torch.int32))
    assert torch.equal(f1["lse"][live].view(torch.int32), f2["lse"][live].view(torch.int32))
    b1, b2 = run_bwd(D, H, True, f1, False), run_bwd(D, H, True, f2, False)
    for k in ("a", "g", "g_e"):
        assert torch.equal(b1[k].view(torch.int32), b2[k].view(torch.int32)), k


# ------------------------------------------------------------------------------------------ e. the two product entry points
def test_hgt_layout_through_relation_attention():
    """q by destination, K|V rows per (relation, source node), e_weight = 0 so ea = e_bias: peak and plateau_hi on the hub plan."""
    from wsi_hgnn_amd import ops
    D, H = C.HGT_DH
    c, d, x, ref = C.graph_case(), on_device(True), C.inputs(D, H, "hgt"), C.evaluate(D, H, "hgt")
    q = x["q"].to(DEV).requires_grad_()
    kv = torch.cat([x["k"], x["v"]], dim=1).to(DEV).requires_grad_()
    ew, eb = x["ew"].view(1, 1).to(DEV).requires_grad_(), x["eb"].to(DEV).requires_grad_()
    t = ops.relation_attention(q, kv, ew, eb, d.rel_plan, x["sim"].to(DEV), D, H)
    t.backward(x["gt"].to(DEV))
    torch.cuda.synchronize()
    got = {"t": t, "g_q": q.grad, "g_k": kv.grad[:, :D], "g_v": kv.grad[:, D:], "g_e": torch.stack([ew.grad.reshape(()), eb.grad.reshape(())])}
    assert all(bool(torch.isfinite(v).all()) for v in got.values())
    _hold(C.ratios(got, ref, D, H, True, "hgt"), "hgt layout, hub", D, H)


def test_heat_attention_through_autograd():
    from wsi_hgnn_amd import ops
    D, H = 256, 4
    c, d, x, ref = C.graph_case(), on_device(True), C.inputs(D, H), C.evaluate(D, H)
    kqv = torch.cat([x["k"], x["q"], x["v"]], dim=1).to(DEV).requires_grad_()
    ew, eb = x["ew"].view(1, 1).to(DEV).requires_grad_(), x["eb"].to(DEV).requires_grad_()
    t = ops.heat_attention(kqv, ew, eb, d.plan, x["sim"].to(DEV), D, H)
    t.backward(x["gt"].to(DEV))
    torch.cuda.synchronize()
    got = {"t": t, "g_k": kqv.grad[:, :D], "g_q": kqv.grad[:, D:2 * D], "g_v": kqv.grad[:, 2 * D:],
           "g_e": torch.stack([ew.grad.reshape(()), eb.grad.reshape(())])}
    assert all(bool(torch.isfinite(v).all()) for v in got.values())
    _hold(C.ratios(got, ref, D, H, True), "ops.heat_attention, hub", D, H)
