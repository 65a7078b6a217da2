"""Every (D, H) instantiation of the pooled ("value collapse") attention backward and the entry points around it, directly through the C ABI
against float64 (tests/pooled_cases.py: graphs, inputs, restatement, bounds; tests/test_pooled_cases.py holds those without a GPU).

  a. all 15 (D, H) x {gtab, gather_h, with_v} x {no hub split, hub split at 8 in-edges} on the T = 3 graph: heat_attn_bwd_p1_kernel<.., COOP, POOL>
     (heads_reduce<LPH> at H = 1 .. 16), heat_attn_bwd_p1_flat_kernel, heat_attn_bwd_p3_kernel<.., POOL> with ctab_ready 0 and 1,
     heat_pool_gtab_kernel, heat_pool_coeff_kernel.  Where wsi_heat_pool_gtab's limits exclude the shape the refusal is asserted and the case
     runs as gather_h (ops.py's fallback);
  b. T in {1, 2, 4, 5, 8} node types x B in {1, 3} slides at (128, 4), (256, 8), (512, 2); T = 9 refused by all three entry points;
  c. wsi_heat_pool_gtab alone: J = T H in {1, 5, 12, 14, 16, 24, 28, 32} (JP = 3, 6, 8; partly filled j-groups; whole groups past J), segments
     of 1, 2, 127, 128, 129, 255 and 0 rows, ldh = D and D + 4 with NaN in the padding, misaligned arguments refused;
  d. wsi_heat_pool_coeff at every H and T in {1, 3, 8};
  e. wsi_heat_attn_scores_fwd == wsi_heat_attn_fwd's score and lse, bit for bit, at all 15 (D, H);
  f. g_absmax under a pool descriptor;  g. determinism and refusals.
Bounds: pooled_cases.BOUNDS / G_E_TOL, whole-tensor and per (head, node type, hub or not) block; the worst error / bound of every group is printed."""
import ctypes
import functools

import pytest
import torch

import pooled_cases as C

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAN = float("nan")
W = {k: C.Worst() for k in ("a: (D, H) sweep", "b: node types", "c: gtab", "d: coeff", "f: absmax", "g: determinism")}


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for title, w in W.items():
        w.report(title)


class _Graph:
    pass


@functools.lru_cache(maxsize=None)
def on_device(T, B, hub):
    """The case's graph on the GPU with a plan of its own (hub: built under graph.HEAVY_DEGREE = 8), checked against the CPU plan."""
    from wsi_hgnn_amd import ops
    from wsi_hgnn_amd.pooling.readout import all_types_plan
    c = C.graph_case(T, B)
    d = _Graph()
    d.g = c.g.to(DEV)
    if hub:
        with C.heavy_degree(C.HUB_DEGREE):
            d.plan = d.g.plan()
    else:
        d.plan = d.g.plan()
    want = c.hub_plan if hub else c.plan
    for name in ("src", "rowptr", "node_seg", "colptr", "csc_eid", "csc_dst"):
        assert torch.equal(getattr(d.plan, name).cpu(), getattr(want, name)), name
    assert d.plan.num_src_rows == d.plan.num_nodes == c.n and d.plan.heavy_degree == want.heavy_degree
    assert (d.plan.num_heavy > 0) == hub
    d.hub = C.hub_mask(d.plan)
    assert bool(d.hub.any()) == hub                      # the cooperative kernels do get rows
    d.rp = all_types_plan(d.g, torch.device(DEV))
    d.row_seg = d.rp.row_segment()
    assert torch.equal(d.row_seg.cpu().long(), c.row_seg) and d.rp.num_segs == T * B
    d.sim = d.g.cat_edata_csr("sim")
    assert torch.equal(d.sim.cpu(), c.sim)
    d.edge_seg, d.seg_dst = ops._edge_segments(d.plan), ops._segment_dst(d.plan)
    return d


def _graph_args(d):
    from wsi_hgnn_amd import ops, _native as N
    p = d.plan
    return (N.ptr(p.node_seg), N.ptr(p.rowptr), N.ptr(p.src), N.ptr(d.sim), N.ptr(p.order_dst), p.num_heavy, ops._attn_flags(p))


@functools.lru_cache(maxsize=2)
def forward_state(T, B, D, H, hub):
    """Inputs on the device and the forward's state through the product's entry points: scores, lse, ctab."""
    from wsi_hgnn_amd import _native as N
    c, x, d = C.graph_case(T, B), C.inputs(T, B, D, H), on_device(T, B, hub)
    lib, p = N.load(), d.plan
    s = {k: x[k].to(DEV).contiguous() for k in ("kq", "h", "gt_seg", "g_row", "omg", "ew", "eb", "y", "beta", "v")}
    s["kqv"] = torch.cat([s["kq"], s["v"]], dim=1).contiguous()
    s["score"] = torch.full((c.E, H), NAN, device=DEV)
    s["lse"] = torch.zeros(p.num_segs, H, device=DEV)                   # (rows of empty segments are never written)
    N.check(lib.wsi_heat_attn_scores_fwd(N.ptr(s["kq"], D * 4), 2 * D, N.ptr(s["kq"]), 2 * D, c.n, D, H, *_graph_args(d), N.ptr(s["ew"]), N.ptr(s["eb"]),
                                         N.ptr(s["score"]), N.ptr(s["lse"]), N.context(), N.stream()), "scores")
    s["ctab"] = torch.full((c.n, T, H), NAN, device=DEV)
    N.check(lib.wsi_heat_pool_coeff(N.ptr(s["score"]), N.ptr(s["lse"]), N.ptr(d.edge_seg), N.ptr(p.colptr), N.ptr(p.csc_eid), N.ptr(p.csc_dst),
                                    N.ptr(p.inv_rd), N.ptr(d.row_seg), B, T, H, c.n, N.ptr(s["ctab"]), N.stream()), "coeff")
    torch.cuda.synchronize()
    return s


def _gtab(d, s, T, B, D, H, out):
    from wsi_hgnn_amd import _native as N
    return N.load().wsi_heat_pool_gtab(N.ptr(s["h"]), D, D, H, N.ptr(s["y"]), N.ptr(s["beta"]), N.ptr(d.rp.chunk_row), N.ptr(d.rp.chunk_seg),
                                       d.rp.num_chunks, B, T, N.ptr(out), N.stream())


def run_bwd(T, B, D, H, variant, hub, absmax=False):
    """One wsi_heat_attn_bwd call under a pool descriptor; every output starts as NaN (r_out, g_k|g_q, a, scratch) so an unwritten entry shows.
    Returns the outputs and the variant the call really ran as (gtab falls back to gather_h where wsi_heat_pool_gtab refuses the shape)."""
    from wsi_hgnn_amd import ops, _native as N
    c, d, s = C.graph_case(T, B), on_device(T, B, hub), forward_state(T, B, D, H, hub)
    lib, p, n, E = N.load(), d.plan, c.n, c.E
    out = {}
    gtab = None
    if variant == "gtab":
        gtab = torch.full((n, T, H), -7.5, device=DEV)
        rc = _gtab(d, s, T, B, D, H, gtab)
        if C.gtab_fits(T, H, D):
            N.check(rc, "gtab")
            out["gtab"] = gtab
        else:
            torch.cuda.synchronize()
            assert rc == N.WSI_ENOSYS and bool((gtab == -7.5).all()), (rc, "wsi_heat_pool_gtab must refuse T*H > 32 or a table over 64 KB and write nothing")
            gtab, variant = None, "gather_h"
    no_v = variant != "with_v"
    ctab = s["ctab"].clone() if no_v else torch.zeros(n, T, H, device=DEV)
    r_out = torch.full((n, D), NAN, device=DEV)
    desc = N.AttnPool(row_seg=N.ptr(d.row_seg), segs_per_type=B, n_types=T, y=N.ptr(s["y"]), g_row=N.ptr(s["g_row"]), omg=N.ptr(s["omg"]),
                      r_out=N.ptr(r_out), ldr=D, ctab=N.ptr(ctab), ctab_ready=1 if no_v else 0, h=N.ptr(s["h"]) if no_v else None, ldh=D,
                      beta=N.ptr(s["beta"]) if no_v else None, gtab=N.ptr(gtab),
                      edge_seg=N.ptr(d.edge_seg) if gtab is not None else None, seg_dst=N.ptr(d.seg_dst) if gtab is not None else None)
    a = torch.full((E, H), NAN, device=DEV)
    scratch = torch.full((3, E, H), NAN, device=DEV)
    red_ws = torch.empty(1024, device=DEV)
    ldp = 2 * D if no_v else 3 * D
    tab = s["kq"] if no_v else s["kqv"]
    g_tab = torch.full((n, ldp), NAN, device=DEV)
    g_e = torch.full((2,), NAN, device=DEV)
    am = torch.zeros(n, 2, dtype=torch.int32, device=DEV) if absmax else None
    score = s["score"].clone()
    N.check(lib.wsi_heat_attn_bwd(
        N.ptr(tab, D * 4), ldp, N.ptr(tab), ldp, None if no_v else N.ptr(tab, 2 * D * 4), ldp, n, p.num_src_rows, E, D, H,
        N.ptr(p.node_seg), N.ptr(p.rowptr), N.ptr(p.src), N.ptr(d.sim), N.ptr(p.colptr), N.ptr(p.csc_eid), N.ptr(p.csc_dst),
        N.ptr(p.inv_rd), N.ptr(p.order_dst), p.num_heavy, N.ptr(p.order_src), ops._attn_flags(p), N.ptr(s["ew"]), N.ptr(s["eb"]),
        N.ptr(s["gt_seg"]), D, N.ptr(d.row_seg), N.ptr(score), N.ptr(a), N.ptr(s["lse"]), N.ptr(scratch[0]), N.ptr(scratch[1]), N.ptr(scratch[2]),
        N.ptr(red_ws), N.ptr(g_tab, D * 4), ldp, N.ptr(g_tab), ldp, None, ldp, N.ptr(g_e), N.ptr(am), ctypes.byref(desc), N.context(), N.stream()), "bwd")
    torch.cuda.synchronize()
    assert torch.equal(score, s["score"]), "the saved logits are read only"
    if not no_v:
        assert bool(torch.isnan(g_tab[:, 2 * D:]).all()), "g_v is never formed: its columns stay untouched"
    out.update(a=a, g_k=g_tab[:, :D], g_q=g_tab[:, D:2 * D], r_out=r_out, ctab=ctab, g_e=g_e, ran_as=variant, absmax=am, g_tab=g_tab)
    return out


def _hold(w, out, T, B, D, H, hub, label):
    c, d, x = C.graph_case(T, B), on_device(T, B, hub), C.inputs(T, B, D, H)
    got = {k: out[k] for k in ("a", "g_q", "g_k", "r_out", "ctab", "g_e", "gtab") if k in out}
    got["g_v_from_ctab"] = C.g_v_from_ctab(out["ctab"], c, x["gt_seg"], H)
    w.hold(C.ratios(got, C.reference(T, B, D, H), c, d.hub, H), label)
    # rows without edges: zeros, not leftovers
    indeg, outdeg = torch.bincount(c.dst, minlength=c.n), torch.bincount(c.src, minlength=c.n)
    assert bool((out["g_q"][indeg == 0] == 0).all()) and bool((out["g_k"][outdeg == 0] == 0).all()) and bool((out["ctab"][outdeg == 0] == 0).all())


# ------------------------------------------------------------------------------------------ a. instantiation sweep
@pytest.mark.parametrize("D,H,hub,variant", [(D, H, hub, v) for D, H in C.ALL_DH for hub in (False, True) for v in C.VARIANTS])
def test_every_instantiation_against_float64(D, H, hub, variant):
    out = run_bwd(3, 2, D, H, variant, hub)
    assert out["ran_as"] == (variant if (variant != "gtab" or C.gtab_fits(3, H, D)) else "gather_h")
    _hold(W["a: (D, H) sweep"], out, 3, 2, D, H, hub, f"D={D} H={H} {'hub' if hub else 'plain'} {variant}")


# ------------------------------------------------------------------------------------------ b. node-type counts
@pytest.mark.parametrize("T,B,D,H,variant", [(T, B, D, H, v) for T in (1, 2, 4, 5, 8) for B in (1, 3) for D, H in ((128, 4), (256, 8), (512, 2))
                                             for v in C.VARIANTS])
def test_node_type_counts_against_float64(T, B, D, H, variant):
    out = run_bwd(T, B, D, H, variant, True)
    assert out["ran_as"] == (variant if (variant != "gtab" or C.gtab_fits(T, H, D)) else "gather_h")
    _hold(W["b: node types"], out, T, B, D, H, True, f"T={T} B={B} D={D} H={H} {variant}")


def test_nine_node_types_are_refused_by_all_three_entry_points():
    from wsi_hgnn_amd import ops, _native as N
    T, B, D, H = 3, 2, 128, 4
    c, d, s = C.graph_case(T, B), on_device(T, B, True), forward_state(T, B, D, H, True)
    lib, p, n, E = N.load(), d.plan, c.n, c.E
    big = lambda *shape: torch.full(shape, -3.25, device=DEV)
    y9, beta9, ctab9, gtab9 = torch.zeros(9, 9 * B, H, D, device=DEV), torch.zeros(9, 9 * B, H, device=DEV), big(n, 9, H), big(n, 9, H)
    rc = lib.wsi_heat_pool_coeff(N.ptr(s["score"]), N.ptr(s["lse"]), N.ptr(d.edge_seg), N.ptr(p.colptr), N.ptr(p.csc_eid), N.ptr(p.csc_dst),
                                 N.ptr(p.inv_rd), N.ptr(d.row_seg), B, 9, H, n, N.ptr(ctab9), N.stream())
    assert rc == N.WSI_EINVAL
    rc = lib.wsi_heat_pool_gtab(N.ptr(s["h"]), D, D, H, N.ptr(y9), N.ptr(beta9), N.ptr(d.rp.chunk_row), N.ptr(d.rp.chunk_seg), d.rp.num_chunks, B, 9,
                                N.ptr(gtab9), N.stream())
    assert rc == N.WSI_EINVAL
    r_out, a, scratch, g_tab, g_e = big(n, D), big(E, H), big(3, E, H), big(n, 2 * D), big(2)
    omg9 = torch.zeros(9, device=DEV)
    desc = N.AttnPool(row_seg=N.ptr(d.row_seg), segs_per_type=B, n_types=9, y=N.ptr(y9), g_row=N.ptr(s["g_row"]), omg=N.ptr(omg9),
                      r_out=N.ptr(r_out), ldr=D, ctab=N.ptr(ctab9), ctab_ready=1, h=N.ptr(s["h"]), ldh=D, beta=N.ptr(beta9), gtab=None, edge_seg=None,
                      seg_dst=None)
    rc = _raw_bwd(lib, d, s, n, n, E, D, H, s["kq"], 2 * D, a, scratch, g_tab, g_e, desc)
    torch.cuda.synchronize()
    assert rc == N.WSI_EINVAL
    for t in (ctab9, gtab9, r_out, a, scratch, g_tab, g_e):
        assert bool((t == -3.25).all())


def _raw_bwd(lib, d, s, n, num_src, E, D, H, tab, ldp, a, scratch, g_tab, g_e, desc, score=None, lse=None):
    """wsi_heat_attn_bwd without V on the K|Q table ``tab``; returns the code."""
    from wsi_hgnn_amd import ops, _native as N
    p = d.plan
    red_ws = torch.empty(1024, device=DEV)
    return lib.wsi_heat_attn_bwd(
        N.ptr(tab, D * 4), ldp, N.ptr(tab), ldp, None, ldp, n, num_src, E, D, H,
        N.ptr(p.node_seg), N.ptr(p.rowptr), N.ptr(p.src), N.ptr(d.sim), N.ptr(p.colptr), N.ptr(p.csc_eid), N.ptr(p.csc_dst),
        N.ptr(p.inv_rd), N.ptr(p.order_dst), p.num_heavy, N.ptr(p.order_src), ops._attn_flags(p), N.ptr(s["ew"]), N.ptr(s["eb"]),
        N.ptr(s["gt_seg"]), D, N.ptr(d.row_seg), N.ptr(s["score"] if score is None else score), N.ptr(a), N.ptr(s["lse"] if lse is None else lse),
        N.ptr(scratch[0]), N.ptr(scratch[1]), N.ptr(scratch[2]), N.ptr(red_ws), N.ptr(g_tab, D * 4), ldp, N.ptr(g_tab), ldp, None, ldp, N.ptr(g_e), None,
        ctypes.byref(desc), N.context(), N.stream())


# ------------------------------------------------------------------------------------------ c. wsi_heat_pool_gtab alone
def _gtab_alone(k, T, H, D, ldh, out, h=None, h_offset=0):
    from wsi_hgnn_amd import ops, _native as N
    rp = ops.ReducePlan.from_ptr(k["ptr"], torch.device(DEV))
    hd = k["h"].to(DEV) if h is None else h
    y, beta = k["y"].to(DEV), k["beta"].to(DEV)
    rc = N.load().wsi_heat_pool_gtab(N.ptr(hd, h_offset), ldh, D, H, N.ptr(y), N.ptr(beta), N.ptr(rp.chunk_row), N.ptr(rp.chunk_seg), rp.num_chunks,
                                     k["B"], T, N.ptr(out), N.stream())
    torch.cuda.synchronize()
    return rc


@pytest.mark.parametrize("D", [128, 256, 512])
@pytest.mark.parametrize("T,H", C.GTAB_TH)
def test_gtab_alone_against_the_float64_contraction(T, H, D):
    from wsi_hgnn_amd import _native as N
    for ldh in (D, D + 4):
        k = C.gtab_case(T, H, D, ldh)
        out = torch.full((k["n"], T, H), -7.5, device=DEV)
        rc = _gtab_alone(k, T, H, D, ldh, out)
        if not C.gtab_fits(T, H, D):
            assert (T * H, D) == (32, 512)                    # the only combination of this sweep outside the limits: 32 x 516 floats > 64 KB
            assert rc == N.WSI_ENOSYS and bool((out == -7.5).all())
            continue
        N.check(rc, "gtab")
        none = torch.zeros(k["n"], dtype=torch.bool)
        r = C.block_ratio(out.double().cpu().transpose(1, 2), k["ref"].transpose(1, 2).contiguous(), k["row_type"], none, T, H, *C.BOUNDS["gtab"])
        W["c: gtab"].hold({"gtab": r}, f"J={T * H} (T={T} H={H}) D={D} ldh={ldh}")


def test_gtab_refuses_misaligned_rows_and_writes_nothing():
    from wsi_hgnn_amd import _native as N
    T, H, D = 3, 4, 128
    k = C.gtab_case(T, H, D, D + 4)
    out = torch.full((k["n"], T, H), -7.5, device=DEV)
    assert _gtab_alone(k, T, H, D, D + 2, out) == N.WSI_EINVAL                       # ldh % 4 != 0
    wide = torch.zeros(k["n"] + 1, D + 4, device=DEV)
    assert _gtab_alone(k, T, H, D, D + 4, out, h=wide, h_offset=4) == N.WSI_EINVAL    # h 4 bytes off a 16-byte boundary
    assert _gtab_alone(k, T, H, 64, D + 4, out) == N.WSI_ENOSYS                      # D outside {128, 256, 512}
    assert bool((out == -7.5).all())


# ------------------------------------------------------------------------------------------ d. wsi_heat_pool_coeff
@pytest.mark.parametrize("T", [1, 3, 8])
@pytest.mark.parametrize("H", [1, 2, 4, 8, 16])
def test_coeff_against_the_float64_scatter_and_the_forward(H, T):
    from wsi_hgnn_amd import _native as N
    B, D = 2, 128
    c, d, s = C.graph_case(T, B), on_device(T, B, True), forward_state(T, B, D, H, True)
    lib, p, n, S, dk = N.load(), d.plan, c.n, T * B, D // H
    ctab = s["ctab"]
    # the project's check: a float64 scatter of the probabilities the kernels' own score / lse give
    a = torch.exp(s["score"].double().cpu() - s["lse"].double().cpu()[c.seg]) * c.inv_rd[c.dst].unsqueeze(1)
    ref = torch.zeros(n * T, H, dtype=torch.float64).index_add_(0, c.src * T + c.type_of[c.dst], a).view(n, T, H)
    r = C.block_ratio(ctab.double().cpu().transpose(1, 2), ref.transpose(1, 2).contiguous(), c.type_of, d.hub, T, H, *C.BOUNDS["ctab"])
    # ... and against float64 from the inputs
    r64 = C.ratios({"ctab": ctab}, C.reference(T, B, D, H), c, d.hub, H)["ctab"]
    outdeg = torch.bincount(c.src, minlength=n)
    assert bool((outdeg == 0).any()) and bool((ctab[outdeg == 0] == 0).all())
    # what the coefficients mean: segment sums of the full forward's t from ctab and v alone
    t = torch.full((n, D), NAN, device=DEV)
    sc2, ls2 = torch.empty_like(s["score"]), torch.zeros_like(s["lse"])
    N.check(lib.wsi_heat_attn_fwd(N.ptr(s["kqv"], D * 4), 3 * D, N.ptr(s["kqv"]), 3 * D, N.ptr(s["kqv"], 8 * D), 3 * D, n, D, H, *_graph_args(d),
                                  N.ptr(s["ew"]), N.ptr(s["eb"]), N.ptr(t), D, N.ptr(sc2), N.ptr(ls2), None, N.context(), N.stream()), "fwd")
    torch.cuda.synchronize()
    want = torch.zeros(S, D, dtype=torch.float64).index_add_(0, c.row_seg, t.double().cpu())
    got = torch.zeros(S, H, dk, dtype=torch.float64)
    v = s["v"].double().cpu().view(n, H, dk)
    for b in range(T):
        got.index_add_(0, b * B + c.graph_of, ctab.double().cpu()[:, b, :].unsqueeze(-1) * v)
    ident = (got.view(S, D) - want).abs().max().item() / (2e-5 * max(1.0, want.abs().max().item()))
    W["d: coeff"].hold({"ctab vs scatter": r, "ctab": r64, "segment sums of t": ident}, f"T={T} H={H}")


# ------------------------------------------------------------------------------------------ e. scores forward == full forward
@pytest.mark.parametrize("hub", [False, True])
@pytest.mark.parametrize("D,H", C.ALL_DH)
def test_scores_fwd_equals_the_full_forward_bit_for_bit(D, H, hub):
    from wsi_hgnn_amd import _native as N
    c, d, s = C.graph_case(3, 2), on_device(3, 2, hub), forward_state(3, 2, D, H, hub)
    t = torch.full((c.n, D), NAN, device=DEV)
    sc, ls = torch.full_like(s["score"], NAN), torch.zeros_like(s["lse"])
    N.check(N.load().wsi_heat_attn_fwd(N.ptr(s["kqv"], D * 4), 3 * D, N.ptr(s["kqv"]), 3 * D, N.ptr(s["kqv"], 8 * D), 3 * D, c.n, D, H, *_graph_args(d),
                                       N.ptr(s["ew"]), N.ptr(s["eb"]), N.ptr(t), D, N.ptr(sc), N.ptr(ls), None, N.context(), N.stream()), "fwd")
    torch.cuda.synchronize()
    assert torch.equal(sc, s["score"]) and torch.equal(ls, s["lse"]) and bool(torch.isfinite(sc).all())


# ------------------------------------------------------------------------------------------ f. g_absmax under a pool descriptor
@pytest.mark.parametrize("variant", C.VARIANTS)
@pytest.mark.parametrize("D,H", [(128, 16), (256, 1), (512, 4)])
def test_absmax_slots_under_a_pool_descriptor(D, H, variant):
    plain, tabled = run_bwd(3, 2, D, H, variant, True), run_bwd(3, 2, D, H, variant, True, absmax=True)
    for k in ("a", "g_tab", "r_out", "ctab", "g_e"):
        assert torch.equal(plain[k].view(torch.int32), tabled[k].view(torch.int32)), f"{k} changes when the table is passed"
    am = tabled["absmax"].cpu()
    assert torch.equal(am[:, 0], C.absmax_bits(tabled["g_q"]).cpu()), "slot 2w: g_q[w]"
    assert torch.equal(am[:, 1], C.absmax_bits(tabled["g_k"]).cpu()), "slot 2u+1: g_k[u]"
    assert int((am[:, 0] != 0).sum()) > 0 and int((am[:, 1] != 0).sum()) > 0
    _hold(W["f: absmax"], tabled, 3, 2, D, H, True, f"D={D} H={H} {variant} absmax")


# ------------------------------------------------------------------------------------------ g. determinism and refusals
@pytest.mark.parametrize("variant", C.VARIANTS)
@pytest.mark.parametrize("D,H", [(128, 2), (512, 8)])
def test_identical_calls_give_identical_bytes(D, H, variant):
    one, two = run_bwd(3, 2, D, H, variant, True), run_bwd(3, 2, D, H, variant, True)
    for k in ("a", "g_tab", "r_out", "ctab", "g_e") + (("gtab",) if "gtab" in one else ()):
        assert torch.equal(one[k].view(torch.int32), two[k].view(torch.int32)), k
    _hold(W["g: determinism"], two, 3, 2, D, H, True, f"D={D} H={H} {variant} repeat")


@pytest.mark.parametrize("what", ["D=64", "D=512 H=32", "misaligned r_out", "num_src != num_nodes"])
def test_refusals_under_a_pool_descriptor_leave_the_outputs_alone(what):
    from wsi_hgnn_amd import _native as N
    T, B = 3, 2
    D, H = {"D=64": (64, 4), "D=512 H=32": (512, 32)}.get(what, (128, 4))
    c, d, x = C.graph_case(T, B), on_device(T, B, True), C.inputs(T, B, D, H)
    n, E, lib = c.n, c.E, N.load()
    s = {k: x[k].to(DEV).contiguous() for k in ("kq", "h", "gt_seg", "g_row", "omg", "ew", "eb", "y", "beta")}
    big = lambda *shape: torch.full(shape, -3.25, device=DEV)
    score, lse = torch.zeros(E, H, device=DEV), torch.zeros(d.plan.num_segs, H, device=DEV)
    r_out, a, scratch, g_tab, g_e, ctab = big(n + 1, D), big(E, H), big(3, E, H), big(n, 2 * D), big(2), big(n, T, H)
    desc = N.AttnPool(row_seg=N.ptr(d.row_seg), segs_per_type=B, n_types=T, y=N.ptr(s["y"]), g_row=N.ptr(s["g_row"]), omg=N.ptr(s["omg"]),
                      r_out=N.ptr(r_out, 4 if what == "misaligned r_out" else 0), ldr=D, ctab=N.ptr(ctab), ctab_ready=0, h=N.ptr(s["h"]), ldh=D,
                      beta=N.ptr(s["beta"]), gtab=None, edge_seg=None, seg_dst=None)
    rc = _raw_bwd(lib, d, s, n, n - 1 if what == "num_src != num_nodes" else n, E, D, H, s["kq"], 2 * D, a, scratch, g_tab, g_e, desc, score=score, lse=lse)
    torch.cuda.synchronize()
    assert rc == (N.WSI_ENOSYS if what.startswith("D=") else N.WSI_EINVAL), (what, rc)
    assert lib.wsi_last_error()
    for t in (r_out, a, scratch, g_tab, g_e, ctab):
        assert bool((t == -3.25).all())
