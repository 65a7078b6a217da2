"""Every instantiation of csrc/gat_attn.hip's dispatch table against float64, on the GPU.  ``row_cfg(H * D, D, H, vec4_ok)`` (csrc/row_group.h) maps the head
count, the per-head width and the alignment onto one of 20 (VEC, G, NK) codes; tests/test_gat.py's ``ga_cfg`` restates it and holds the shape table
(``GA_SWEEP``) that reaches each of them, and checks that without a GPU.  Here:
  1. the table through ``ops.gat_attention`` - scores, forward, every gradient - plain and with the explainer's per-edge message scale;
  2. graphs built for the kernels' edges, one per group size G, with n = 128 * (256 / G) + 37 nodes: the fixed-grid loops of
     gat_act_bwd_kernel / gat_bwd_attn_kernel make a second trip, the last workgroup is partly empty, n is no multiple of 256 / G;
     duplicate edges, a self-loop-only destination, in-degrees 2..15, 17 (the 16-lane stride of gat_bwd_dst_kernel) and 150, and 24 nodes
     without any out-edge (an empty colptr range); and two degenerate graphs (one node; a directed ring of three);
  3. the scalar fallback for widths that are multiples of 4, reachable only through the C ABI: row strides of F + 1 with a sentinel column,
     and tensors that start 4 bytes into their buffers;
  4. attn_drop replayed from the host mask at odd head counts and at 16 heads, plain and scaled;
  5. ``wsi_sddmm_dot`` at the widths that reach the rest of its kernels.
The float64 restatement, ``_close`` and the tolerance are tests/test_gat_gpu.py's: 1e-4 of the largest reference entry of each tensor.

The side of relu's / leaky_relu's kink is decided in fp32; the reference replays the GPU's decisions (``pos``, as test_gat_gpu.py's
``_model_check`` does), and every entry where the GPU's side differs from float64's must have a float64 pre-activation value within the
tolerance of zero - the only place where the two may legitimately differ."""
import pytest
import torch

from test_gat import GA_SWEEP, SDDMM_WIDTHS, ga_cfg, ga_group
from test_gat_gpu import DEV, TOL, _close, _csr, _graph, _inputs, ref_attention

pytestmark = pytest.mark.gpu

SLOPE = 0.2
N_SINKS = 24                       # nodes without an out-edge
LONELY, DEG17, DEG150 = 0, 1, 2    # destinations of in-degree 1 (its self loop), 17 and 150; nodes 3..16 have in-degrees 2..15
GRADS = ("g_ft", "g_attn_l", "g_attn_r", "g_bias", "g_edge_scale")
RATIOS = {}                        # tensor name -> (largest error / bound over the module's run, the case it came from)


def _nodes_for(G):
    return 128 * (256 // G) + 37


def _sweep_edges(G):
    """Edge lists of the graph of group size G.  Only nodes [0, R) have a self loop and only they are sources."""
    gen = torch.Generator().manual_seed(100 + G)
    n = _nodes_for(G)
    R = n - N_SINKS
    src, dst = [torch.arange(R)], [torch.arange(R)]

    def feed(v, k):                                                   # k in-edges of v from sources other than v
        s = torch.randint(0, R - 1, (k,), generator=gen)
        src.append(s + (s >= v))
        dst.append(torch.full((k,), v))

    feed(DEG17, 16)
    feed(DEG150, 149)
    for i in range(14):
        feed(3 + i, 1 + i)
    cnt = torch.randint(0, 6, (R - 17,), generator=gen)               # every other looped node: 0..5 more in-edges
    d = torch.repeat_interleave(torch.arange(17, R), cnt)
    s = torch.randint(0, R, (d.numel(),), generator=gen)
    m = d.numel() // 10
    src += [s, s[:m]]                                                 # a tenth of them twice
    dst += [d, d[:m]]
    for i in range(N_SINKS):                                          # the sinks: fed by 1..3 others, feeding nobody, no self loop
        k = 1 + i % 3
        src.append(torch.randint(0, R, (k,), generator=gen))
        dst.append(torch.full((k,), R + i))
    src, dst = torch.cat(src), torch.cat(dst)
    o = torch.randperm(src.numel(), generator=gen)
    return n, src[o], dst[o]


def _sweep_graph(G):
    from wsi_hgnn_amd.models.GAT import gat_plan
    n, src, dst = _sweep_edges(G)
    R = n - N_SINKS
    plan = gat_plan(_graph(n, src, dst).to(DEV))
    indeg = (plan.rowptr[1:n + 1] - plan.rowptr[:n]).cpu()
    outdeg = (plan.colptr[1:n + 1] - plan.colptr[:n]).cpu()
    assert plan.num_nodes == n and n % (256 // G) != 0 and n > 128 * (256 // G)
    assert int(indeg[LONELY]) == 1 and int(indeg[DEG17]) == 17 and int(indeg[DEG150]) == 150 and int(indeg.min()) >= 1
    assert indeg[3:17].tolist() == list(range(2, 16))
    assert int((outdeg == 0).sum()) == N_SINKS >= 20 and bool((outdeg[R:] == 0).all())
    s2, d2 = _csr(plan)
    assert torch.unique(s2 * n + d2).numel() < plan.num_edges         # duplicate edges
    return plan


@pytest.fixture(scope="module")
def graphs():
    """plan of the group size asked for, built once per G."""
    cache = {}

    def get(G):
        if G not in cache:
            cache[G] = _sweep_graph(G)
        return cache[G]
    return get


@pytest.fixture(scope="module", autouse=True)
def _report_ratios():
    yield
    for name, (r, case) in sorted(RATIOS.items()):
        print(f"\nlargest error / bound, {name}: {r:.3e} ({case})", end="")
    print()


class _Checks:
    """``_close`` over several tensors: every figure is printed and recorded before the first failure is raised."""

    def __init__(self, case):
        self.case, self.failed = case, []

    def close(self, got, ref, what):
        r64, g64 = ref.detach().double().cpu(), got.detach().double().cpu()
        assert g64.shape == r64.shape, f"{what}: shape {tuple(g64.shape)} != {tuple(r64.shape)}"
        ratio = float((g64 - r64).abs().max()) / (TOL * max(float(r64.abs().max()), 1e-30))
        print(f"{self.case} {what}: error / bound {ratio:.3e}, reference max {float(r64.abs().max()):.3e}")
        if ratio > RATIOS.get(what, (-1.0, None))[0]:
            RATIOS[what] = (ratio, self.case)
        try:
            _close(got, ref, what)
        except AssertionError as e:
            self.failed.append(str(e))

    def done(self):
        assert not self.failed, f"{self.case}: " + "; ".join(self.failed)


def _edge_scale(E, seed):
    gen = torch.Generator().manual_seed(seed)
    return torch.rand(E, generator=gen) * 1.5 + 0.05                  # positive, on both sides of 1


def _run_gpu(ft, al, ar, bias, g, plan, act, scale=None, drop=None):
    from wsi_hgnn_amd import ops
    leaves = [t.to(DEV).requires_grad_(True) for t in (ft, al, ar, bias)]
    s = scale.to(DEV).requires_grad_(True) if scale is not None else None
    out = ops.gat_attention(*leaves, plan, SLOPE, activation=act, attn_drop=drop, edge_scale=s)
    out.backward(g.to(DEV))
    torch.cuda.synchronize()
    return out.detach().cpu(), [t.grad.detach().cpu() for t in leaves + ([s] if s is not None else [])]


def _run_ref(ft, al, ar, bias, g, plan, act, out_gpu, scale=None, keep=None, keep_scale=1.0):
    """float64 ``ref_attention`` with the GPU run's kink decisions replayed.  The message scale enters as ``ref_attention``'s keep factor
    (a * keep * scale multiplies the message after the softmax: exactly the scaled op).  Returns out, the gradients, and the float64
    pre-activation values at the entries where the GPU took the other side of the kink."""
    src, dst = _csr(plan)
    n, H = plan.num_nodes, al.shape[-2]
    leaves = [t.to(torch.float64).requires_grad_(True) for t in (ft, al, ar, bias)]
    factor = None
    if scale is not None:
        leaves.append(scale.to(torch.float64).requires_grad_(True))
        factor = leaves[4][:, None].expand(-1, H)
    if keep is not None:
        factor = keep.to(torch.float64) if factor is None else factor * keep.to(torch.float64)
    pos, flipped = None, torch.zeros(0, dtype=torch.float64)
    if act:
        with torch.no_grad():
            pre = ref_attention(*leaves[:4], src, dst, n, SLOPE, None, factor, keep_scale)
        pos = out_gpu > 0
        flipped = pre[pos != (pre > 0)]
    out = ref_attention(*leaves[:4], src, dst, n, SLOPE, act, factor, keep_scale, pos=pos)
    out.backward(g.to(torch.float64))
    return out.detach(), [t.grad for t in leaves], flipped


def _compare(case, plan, H, D, act, scaled, drop=None, keep=None):
    ft, al, ar, bias, g = _inputs(plan.num_nodes, H, D, False, seed=H * 1000 + D)
    scale = _edge_scale(plan.num_edges, seed=D) if scaled else None
    out, grads = _run_gpu(ft, al, ar, bias, g, plan, act, scale, drop)
    rout, rgrads, flipped = _run_ref(ft, al, ar, bias, g, plan, act, out, scale, keep, drop.scale if drop is not None else 1.0)
    c = _Checks(case)
    c.close(out, rout, "out")
    for name, a, b in zip(GRADS, grads, rgrads):
        c.close(a, b, name)
    # a kink decision may differ from float64's only where float64's value is zero within the tolerance
    bound = TOL * max(float(rout.abs().max()), 1e-30)
    worst = float(flipped.abs().max()) if flipped.numel() else 0.0
    print(f"{case} kink: {flipped.numel()} decisions differ, largest |float64 value| there {worst:.3e}, bound {bound:.3e}")
    assert worst <= bound, f"{case}: the GPU took the other side of the activation's kink at a float64 value of {worst:.3e} > {bound:.3e}"
    c.done()


# ---------------------------------------------------------------------------------------------------- 1, 2: the shape sweep
@pytest.mark.parametrize("scaled", [False, True], ids=["plain", "scaled"])
@pytest.mark.parametrize("H,D,act", GA_SWEEP, ids=[f"{h}x{d}-{a or 'none'}" for h, d, a in GA_SWEEP])
def test_every_instantiation_matches_float64(graphs, H, D, act, scaled):
    """wsi_gat_scores, wsi_gat_attn_fwd[_scaled] and wsi_gat_attn_bwd[_scaled] at the code ga_cfg(H, D) - one row of the table per code,
    H == G at 8 and 16 heads in both families, the full width F = 4096, ragged last chunks - on the graph of that code's group size."""
    plan = graphs(ga_group(H, D))
    _compare(f"{ga_cfg(H, D)} ({H},{D}) {act or 'none'} {'scaled' if scaled else 'plain'}", plan, H, D, act, scaled)


DEGENERATE = {"one-node": (1, [0], [0]), "ring-of-three": (3, [0, 1, 2], [1, 2, 0])}


@pytest.mark.parametrize("scaled", [False, True], ids=["plain", "scaled"])
@pytest.mark.parametrize("H,D,act", [(7, 260, "leaky_relu"), (5, 25, "relu")], ids=["7x260", "5x25"])
@pytest.mark.parametrize("which", sorted(DEGENERATE))
def test_degenerate_graphs(which, H, D, act, scaled):
    """One node with a self loop, and a directed ring of three without self loops: all but one or three rows of the column partials are
    zero, most groups of the only workgroup are idle, and every softmax has one term: the attention-vector gradients are exactly zero
    in float64, so ``_close`` accepts nothing but an exact zero from the kernels either (gat_bwd_dst_kernel rounds d loss / d a once and
    uses that number for both delta and g_pre for this reason: with attn_drop or a message scale a fused g_a * f - delta left 1e-7 here)."""
    from wsi_hgnn_amd.models.GAT import gat_plan
    n, src, dst = DEGENERATE[which]
    plan = gat_plan(_graph(n, src, dst).to(DEV))
    _compare(f"{which} ({H},{D}) {'scaled' if scaled else 'plain'}", plan, H, D, act, scaled)


# ---------------------------------------------------------------------------------------------------- 3: the alignment fallback
SENTINEL = -12345.678


def _strided(t, variant):
    """A device copy of the [n, F] tensor t laid out as the variant asks, with the buffer it lives in: 'stride' = rows F + 1 apart, the
    extra column holding the sentinel; 'offset' = contiguous rows that start 4 bytes into the buffer."""
    n, F = t.shape
    if variant == "stride":
        buf = torch.full((n, F + 1), SENTINEL, device=DEV)
        view = buf[:, :F]
    else:
        buf = torch.full((n * F + 4,), SENTINEL, device=DEV)
        view = buf[1:1 + n * F].view(n, F)
        assert view.data_ptr() % 16 == 4
    view.copy_(t.to(DEV))
    return buf, view


_CAPI_REF = {}                     # (H, D) -> (the kink decisions of the run it was computed for, out, gradients)


@pytest.mark.parametrize("variant", ["stride", "offset"])
@pytest.mark.parametrize("H,D", [(4, 8), (4, 512)])
def test_scalar_fallback_through_the_c_abi(graphs, H, D, variant):
    """D % 4 == 0 but a row stride that is no multiple of 4, or pointers 4 bytes off a 16-byte boundary: row_cfg must pick the scalar
    family (codes 103201 and 106432 here, G = 32 and 64).  Same float64 reference and tolerance; with the strides of F + 1 the column
    after every row of out and g_ft must come back bit for bit - a 16-byte store on this path would overwrite it."""
    from wsi_hgnn_amd import _native as N
    assert ga_cfg(H, D, True) // 100000 == 4 and ga_cfg(H, D, False) // 100000 == 1
    plan = graphs(ga_group(H, D, False))
    n, E, F = plan.num_nodes, plan.num_edges, H * D
    ft, al, ar, bias, g = _inputs(n, H, D, False, seed=H * 1000 + D)
    ld = F + 1 if variant == "stride" else F
    _, ft_d = _strided(ft, variant)
    _, g_d = _strided(g, variant)
    out_buf, out_d = _strided(torch.zeros(n, F), variant)
    gft_buf, gft_d = _strided(torch.zeros(n, F), variant)
    al_d, ar_d, b_d = al.reshape(-1).to(DEV), ar.reshape(-1).to(DEV), bias.to(DEV)
    assert (ld % 4 != 0) or all(t.data_ptr() % 16 != 0 for t in (ft_d, g_d, out_d, gft_d))
    lib = N.load()
    eler = torch.empty(n, 2 * H, device=DEV)
    lse = torch.empty(n, 2 * H, device=DEV)
    act = 2                                                           # leaky_relu: g_rst goes through the workspace
    N.check(lib.wsi_gat_scores(N.ptr(ft_d), ld, n, H, D, N.ptr(al_d), N.ptr(ar_d), N.ptr(eler), N.stream()), "wsi_gat_scores")
    N.check(lib.wsi_gat_attn_fwd(N.ptr(ft_d), ld, N.ptr(eler), n, H, D, N.ptr(plan.rowptr), N.ptr(plan.src), N.ptr(plan.order_dst), SLOPE,
                                 0, None, 0, 1.0, N.ptr(b_d), act, 0.01, N.ptr(out_d), ld, N.ptr(lse), N.stream()), "wsi_gat_attn_fwd")
    ws_bytes = int(lib.wsi_gat_attn_bwd_workspace_bytes(n, E, H, D, act))
    assert ws_bytes > 0
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=DEV)
    assert ws.data_ptr() % 16 == 0
    g_al, g_ar, g_b = (torch.empty(F, device=DEV) for _ in range(3))
    N.check(lib.wsi_gat_attn_bwd(N.ptr(ft_d), ld, N.ptr(eler), N.ptr(lse), N.ptr(out_d), ld, N.ptr(g_d), ld, n, E, H, D,
                                 N.ptr(plan.rowptr), N.ptr(plan.src), N.ptr(plan.colptr), N.ptr(plan.csc_eid), N.ptr(plan.csc_dst),
                                 N.ptr(plan.order_src), N.ptr(al_d), N.ptr(ar_d), SLOPE, 0, None, 0, 1.0, act, 0.01,
                                 N.ptr(ws), ws_bytes, N.ptr(gft_d), ld, N.ptr(g_al), N.ptr(g_ar), N.ptr(g_b), N.stream()), "wsi_gat_attn_bwd")
    torch.cuda.synchronize()
    out = out_d.cpu()
    cached = _CAPI_REF.get((H, D))
    if cached is None or not torch.equal(cached[0], out > 0):         # one reference per shape unless a kink decision differs
        rout, rgrads, flipped = _run_ref(ft, al, ar, bias, g, plan, "leaky_relu", out)
        assert float(flipped.abs().max() if flipped.numel() else 0.0) <= TOL * float(rout.abs().max())
        cached = _CAPI_REF[(H, D)] = (out > 0, rout, rgrads)
    _, rout, rgrads = cached
    c = _Checks(f"{ga_cfg(H, D, False)} ({H},{D}) {variant}")
    c.close(out, rout, "out")
    for name, a, b in zip(GRADS, (gft_d, g_al.view(1, H, D), g_ar.view(1, H, D), g_b), rgrads):
        c.close(a, b, name)
    c.done()
    sentinel = torch.tensor(SENTINEL).view(torch.int32)
    for name, buf in (("out", out_buf), ("g_ft", gft_buf)):
        pad = buf[:, F] if variant == "stride" else torch.cat([buf[:1], buf[1 + n * F:]])
        assert bool((pad.contiguous().cpu().view(torch.int32) == sentinel).all()), f"{name}: the floats next to the rows were overwritten"


# ---------------------------------------------------------------------------------------------------- 4: attn_drop
@pytest.mark.parametrize("scaled", [False, True], ids=["plain", "scaled"])
@pytest.mark.parametrize("H,D", [(1, 1001), (3, 10), (5, 24), (16, 4)])
def test_attn_drop_at_odd_and_maximal_head_counts(graphs, H, D, scaled):
    """edge_factor packs two heads into one hash with (H + 1) / 2 pairs per edge: an odd head count leaves the last pair half used, 16
    heads use all eight.  The host mask ``ops.dropout_keep_mask`` replays the draw into float64; the comparison is element-wise."""
    from wsi_hgnn_amd import ops
    plan = graphs(ga_group(H, D))
    drop = ops.CounterDropout(0.2, 4242)
    keep = ops.dropout_keep_mask(drop, plan.num_edges, H)
    assert tuple(keep.shape) == (plan.num_edges, H) and not bool(keep.all()) and bool(keep.any())
    _compare(f"attn_drop ({H},{D}) {'scaled' if scaled else 'plain'}", plan, H, D, "leaky_relu", scaled, drop, keep)
    if (H, D) == (16, 4):                                             # E * H is large enough here for the 6 sigma bound to bind
        m = keep.numel()
        frac = float(keep.float().mean())
        assert abs(frac - (1 - drop.threshold / 65536)) < 6 * (0.2 * 0.8 / m) ** 0.5


# ---------------------------------------------------------------------------------------------------- 5: wsi_sddmm_dot
@pytest.mark.parametrize("full", [False, True], ids=["plain", "relu-iscale-oscale"])
@pytest.mark.parametrize("D", SDDMM_WIDTHS)
def test_sddmm_dot_widths(graphs, D, full):
    """g_w[e] = oscale[w] iscale[u] <g[w] (masked by relu_ref[w] > 0), x[u]> per CSR entry, against the float64 dot product, at one width
    per kernel that the widths of tests/test_gnn_explainer_gpu.py do not reach."""
    from wsi_hgnn_amd import _native as N
    plan = graphs(64)
    n, E = plan.num_nodes, plan.num_edges
    gen = torch.Generator().manual_seed(D)
    g, x, ref = (torch.randn(n, D, generator=gen) for _ in range(3))
    iscale, oscale = (torch.rand(n, generator=gen) + 0.5 for _ in range(2))
    gw = torch.full((E,), float("nan"), device=DEV)
    gd, xd, rd, isd, osd = (t.to(DEV) for t in (g, x, ref, iscale, oscale))
    N.check(N.load().wsi_sddmm_dot(N.ptr(gd), D, N.ptr(xd), D, n, D, N.ptr(plan.rowptr), N.ptr(plan.src), N.ptr(isd) if full else None,
                                   N.ptr(osd) if full else None, N.ptr(rd) if full else None, D, N.ptr(gw), N.stream()), "wsi_sddmm_dot")
    torch.cuda.synchronize()
    src, dst = _csr(plan)
    gm = (g * (ref > 0)).double() if full else g.double()
    want = (gm[dst] * x.double()[src]).sum(1)
    if full:
        want = oscale.double()[dst] * iscale.double()[src] * want
    c = _Checks(f"sddmm {ga_cfg(1, D)} D={D} {'full' if full else 'plain'}")
    c.close(gw, want, "g_w")
    c.done()
