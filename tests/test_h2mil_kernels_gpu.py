"""``ops.ra_attention`` (wsi_ra_attn_fwd / _bwd) and ``ops.ihpool_assign`` (wsi_ihpool_assign) on the GPU against float64 on the SAME fp32 inputs.
Tolerance (tests/test_gtn_kernels_gpu.py's norm): error <= 1e-4 x the largest float64 entry of each tensor.

ra_attention: the graph of h2mil_cases.ra_kernel_graph - in-degrees 0, 1, 2, 63, 64, 65 and 200 (a row shorter than, equal to and longer than
a wave's worth of edges for every group width), groups of one edge, destinations with 1, 2 and 3 types present, repeated edges - at
C in {1, 3, 4, 32, 256, 260}; out, g_ft, g_sc and g_bias are each checked.  ihpool_assign: segments of 1, 2, 63, 64, 65 and 300 members under
1, 2, 7 and 65 seeds and an empty segment, inputs under the margin condition: clusters equal the float64 restatement exactly.

The dispatch sweep.  ``row_cfg(C, C, 1, vec4_ok)`` (csrc/row_group.h) maps the width and the alignment onto one of 20 (VEC, G, NK) codes;
tests/test_h2mil.py's ``ra_cfg`` restates it, holds the widths (h2mil_cases.RA_SWEEP) to the table and every case below to its conditions without a GPU.  Here, all on
h2mil_cases.ra_sweep_graph (n = 333, no multiple of any 256 / G; the destinations above; sources of out-degree >= 17, 65 and 200, so the
stride loops of ra_bwd_score_kernel and ra_bwd_src_kernel over a source's edges go round again; 24 nodes without an out-edge, one without
any edge, repeated edges, a self loop):
  1. every RA_SWEEP width through ``ops.ra_attention``: out, g_ft, g_sc, g_bias, identical bits on a repeat;
  2. sc x 30 (nearly one-hot rows) at one width per G and at 2052 and 2050; negative_slope 0.05 and 0.0 at one width per VEC;
  3. a node without an edge, and a ring of three among five nodes (fewer rows than WSI_RA_BIAS_PARTS);
  4. the scalar fallback at C in {8, 44, 200, 772} through ops: ft as the leading and as the trailing columns of a [n, C + 1] buffer, and
     a bias 4 bytes into its buffer, which makes the forward scalar and leaves the backward vector; the padding's gradient is exactly 0;
  5. the raw C ABI: ldo = ldg = ldgf = C + 1 and C + 4 with a sentinel in the padding of out and g_ft; g_bias and bias_ws NULL; E = 0 with
     edge_ws NULL; n = 0 with a g_bias that must be zeroed; ``stat`` against float64 (counts exact, absent groups exactly (+inf, 0, 0, 0),
     max, max + log-sum and beta within the tolerance, the present betas summing to 1 within 1e-6);
  6. wsi_ihpool_assign with member, seed and segment indices outside their tables (raw ABI, xyf inside a larger buffer), and segments of
     128 and 129 seeds (two full tiles; a third tile of one).
Norms of 1-5 (``_hold``): every whole tensor under TOL x its largest float64 entry; the rows out[3..6] and g_ft[10..12] (the long rows,
the hubs) each under TOL x ITS OWN largest entry; the four columns of g_sc each under max(TOL, 4 e32) x its largest entry, e32 being the
fp32 CPU run of the restatement on the same inputs in the same norm (g_er and g_pr are cancelling sums).  No per-row norm for g_sc: the
gradients of a one-edge group cancel exactly.  The fp32 run stays under TOL / 4 in every norm and no leaky_relu argument is nearer to zero
than 1e-5 x the score scale (``h2mil_cases.ra_case``, asserted in tests/test_h2mil.py), so fp32 cannot take the other side of a kink."""
import pytest
import torch

import h2mil_cases as C
from mil_cases import Ratios
from test_h2mil import ra_code

pytestmark = pytest.mark.gpu

DEV = "cuda"
TOL = 1e-4
R = Ratios(TOL)
WIDTHS = (1, 3, 4, 32, 256, 260)


@pytest.fixture(scope="module", autouse=True)
def _report_ratios():
    yield
    R.report()


@pytest.fixture(scope="module")
def graph():
    from wsi_hgnn_amd import ops
    n, nt, ei = C.ra_kernel_graph()
    ec = ops.edge_csr_by_source_type(ei[0].to(DEV), ei[1].to(DEV), nt.to(DEV), n)
    return n, nt, ei, ec


_inputs = C.ra_inputs


def _reference(ft, sc, bias, w, ei, nt):
    return C.ra_run(ft, sc, bias, w, ei, nt)


def _through_ops(ft, sc, bias, w, ec, nt, slope=0.2):
    from wsi_hgnn_amd import ops
    f, s, b = (t.to(DEV).requires_grad_(True) for t in (ft, sc, bias))
    out = ops.ra_attention(f, s, b, ec, nt.to(DEV), slope)
    out.backward(w.to(DEV))
    return out.detach(), f.grad, s.grad, b.grad


NAMES = ("out", "g_ft", "g_sc", "g_bias")


@pytest.mark.parametrize("Cw", WIDTHS)
def test_ra_attention_against_float64(graph, Cw):
    n, nt, ei, ec = graph
    args = _inputs(n, Cw)
    got = _through_ops(*args, ec, nt)
    for name, g, r in zip(NAMES, got, _reference(*args, ei, nt)):
        R.check(g, r, name, f"C={Cw}")
    again = _through_ops(*args, ec, nt)
    for name, a, b in zip(NAMES, got, again):
        assert torch.equal(a, b), f"C={Cw}: {name} differs between identical calls"
    bias = args[2].to(DEV)
    assert torch.equal(got[0][0], bias), "a node without in-edges gives the bias"
    # a softmax of one term has gradient zero: destination 1 has one in-edge, so its er receives exactly nothing
    assert float(got[2][1, 1]) == 0.0


@pytest.mark.parametrize("Cw", (4, 260))
def test_ra_attention_with_nearly_one_hot_rows(graph, Cw):
    n, nt, ei, ec = graph
    args = _inputs(n, Cw, seed=1, scale=30.0)
    for name, g, r in zip(NAMES, _through_ops(*args, ec, nt), _reference(*args, ei, nt)):
        R.check(g, r, name, f"one-hot C={Cw}")


def test_ra_attention_without_bias_and_on_a_strided_projection(graph):
    """bias None; ft as the leading columns of a wider matrix (the layer's own call: ft | pl | pr | 0 | 0 from one GEMM)."""
    from wsi_hgnn_amd import ops
    n, nt, ei, ec = graph
    ft, sc, _, w = _inputs(n, 32, seed=2)
    wide = torch.cat([ft, torch.randn(n, 4)], 1).to(DEV).requires_grad_(True)
    s = sc.to(DEV).requires_grad_(True)
    out = ops.ra_attention(wide[:, :32], s, None, ec, nt.to(DEV))
    out.backward(w.to(DEV))
    f64, s64 = ft.double().requires_grad_(True), sc.double().requires_grad_(True)
    ref = C.ra_attention_ref(f64, s64, None, ei, nt)
    (ref * w.double()).sum().backward()
    R.check(out.detach(), ref.detach(), "out", "strided")
    R.check(wide.grad[:, :32], f64.grad, "g_ft", "strided")
    R.check(s.grad, s64.grad, "g_sc", "strided")
    assert not wide.grad[:, 32:].any()


def test_one_node_type_equals_gat_attention(graph):
    """With every node of one type there is one group per destination and beta = 1: GATConv at one head."""
    from wsi_hgnn_amd import ops
    n, _, ei, _ = graph
    nt = torch.ones(n, dtype=torch.int64)
    ec = ops.edge_csr_by_source_type(ei[0].to(DEV), ei[1].to(DEV), nt.to(DEV), n)
    ec.order_dst = ec.order_src = None
    g = torch.Generator().manual_seed(5)
    Cw = 32
    ft, al, ar, bias = torch.randn(n, Cw, generator=g), torch.randn(1, 1, Cw, generator=g), torch.randn(1, 1, Cw, generator=g), torch.randn(Cw, generator=g)
    ftd = ft.to(DEV)
    sc = torch.stack([ftd @ al.view(Cw).to(DEV), ftd @ ar.view(Cw).to(DEV), torch.randn(n, generator=g).to(DEV), torch.randn(n, generator=g).to(DEV)], 1)
    ra = ops.ra_attention(ftd, sc, bias.to(DEV), ec, nt.to(DEV), 0.2)
    gat = ops.gat_attention(ftd, al.to(DEV), ar.to(DEV), bias.to(DEV), ec, 0.2)
    ref = C.ra_attention_ref(ft.double(), sc.double().cpu(), bias.double(), ei, nt)
    R.check(ra, ref, "out", "one type")
    R.check(gat, ref, "gat out", "one type")
    R.check(ra, gat.double(), "ra against gat", "one type")


# ------------------------------------------------------------------------------------------------ the dispatch sweep
COLUMNS = ("g_el", "g_er", "g_pl", "g_pr")


@pytest.fixture(scope="module")
def sweep():
    """The hub-source graph on the device, its promises asserted from the plan's own rowptr / colptr."""
    from wsi_hgnn_amd import ops
    n, nt, ei = C.ra_graph("sweep")
    ec = ops.edge_csr_by_source_type(ei[0].to(DEV), ei[1].to(DEV), nt.to(DEV), n)
    _, outdeg = C.ra_sweep_facts(n, nt, ei, ec.rowptr, ec.colptr)
    return n, nt, ei, ec, (outdeg == 0).nonzero().view(-1)


def _hold(got, case, label):
    """Every figure of ``h2mil_cases.ra_norms`` against its bound, all printed and recorded before the first failure is raised: the whole
    tensors and the single rows under TOL, the columns of g_sc under max(TOL, 4 e32) with e32 the fp32 CPU run's figure in the same norm."""
    assert all(bool(torch.isfinite(t).all()) for t in got), f"{label}: not finite"
    failed = []
    for name, e in C.ra_norms(got, case["ref"]).items():
        if name in COLUMNS:
            e32 = case["e32"][name]
            bound = max(TOL, 4 * e32)
            print(f"{label} {name}: e_gpu {e:.3e}, e32 {e32:.3e}, bound {bound:.3e}, e_gpu / e32 {e / max(e32, 1e-30):.2f}")
        else:
            bound = TOL
            print(f"{label} {name}: error / bound {e / bound:.3e}")
        what = name if "[" not in name else name[:name.index("[")] + " single row"
        if e / bound > R.worst.get(what, (-1.0, None))[0]:
            R.worst[what] = (e / bound, f"{label} {name}")
        if not e <= bound:
            failed.append(f"{name}: {e:.3e} > {bound:.3e}")
    assert not failed, f"{label}: " + "; ".join(failed)


def _exact_facts(got, bias, n, sinks, label):
    out, g_ft, g_sc, _ = got
    b = bias.to(DEV)
    assert torch.equal(out[0], b) and torch.equal(out[n - 1], b), f"{label}: a node without in-edges gives the bias"
    assert float(g_sc[1, 1]) == 0.0, f"{label}: a softmax of one term has gradient zero"
    s = sinks.to(DEV)
    assert not g_ft[s].any() and not g_sc[s, 0].any() and not g_sc[s, 2].any(), f"{label}: a node without out-edges receives no source-side gradient"


@pytest.mark.parametrize("Cw", C.RA_SWEEP)
def test_every_instantiation_matches_float64(sweep, Cw):
    """One width per (VEC, G, NK) code, on the graph whose hubs send the source-side loops round again."""
    n, nt, ei, ec, sinks = sweep
    case = C.ra_case((n, nt, ei), Cw)
    label = f"{ra_code(Cw)} C={Cw}"
    got = _through_ops(*case["inputs"], ec, nt)
    again = _through_ops(*case["inputs"], ec, nt)
    for name, a, b in zip(NAMES, got, again):
        assert torch.equal(a, b), f"{label}: {name} differs between identical calls"
    _exact_facts(got, case["inputs"][2], n, sinks, label)
    _hold(got, case, label)


@pytest.mark.parametrize("Cw", C.RA_ONE_HOT_WIDTHS)
def test_nearly_one_hot_scores_at_every_group_size(sweep, Cw):
    n, nt, ei, ec, sinks = sweep
    case = C.ra_case((n, nt, ei), Cw, scale=30.0)
    label = f"{ra_code(Cw)} C={Cw} sc x 30"
    got = _through_ops(*case["inputs"], ec, nt)
    _exact_facts(got, case["inputs"][2], n, sinks, label)
    _hold(got, case, label)


@pytest.mark.parametrize("Cw,slope", C.RA_SLOPE_CASES)
def test_other_negative_slopes(sweep, Cw, slope):
    n, nt, ei, ec, sinks = sweep
    case = C.ra_case((n, nt, ei), Cw, slope=slope)
    label = f"{ra_code(Cw)} C={Cw} slope {slope}"
    got = _through_ops(*case["inputs"], ec, nt, slope)
    _exact_facts(got, case["inputs"][2], n, sinks, label)
    _hold(got, case, label)


@pytest.mark.parametrize("Cw", C.RA_DEGENERATE_WIDTHS)
@pytest.mark.parametrize("which", sorted(C.ra_degenerate_graphs()))
def test_degenerate_graphs(which, Cw):
    """One node without an edge; a ring of three among five nodes.  Every softmax has one term, so float64's score gradients are exactly
    zero and the whole-tensor norm accepts nothing but exact zeros; with n < WSI_RA_BIAS_PARTS most column partials sum no row."""
    from wsi_hgnn_amd import ops
    n, nt, ei = C.ra_graph(which)
    ec = ops.edge_csr_by_source_type(ei[0].to(DEV), ei[1].to(DEV), nt.to(DEV), n)
    case = C.ra_case((n, nt, ei), Cw)
    got = _through_ops(*case["inputs"], ec, nt)
    assert not got[2].any()
    _hold(got, case, f"{which} C={Cw}")


@pytest.mark.parametrize("variant", ["stride", "offset", "bias"])
@pytest.mark.parametrize("Cw", C.RA_FALLBACK_WIDTHS)
def test_scalar_fallback_through_ops(sweep, Cw, variant):
    """Widths that are multiples of 4 sent down the scalar family by what ops passes on as it is: ft as the leading columns of a [n, C + 1]
    buffer (ldf = C + 1), ft as its trailing columns (4 bytes into the buffer as well), and a bias 4 bytes into its buffer - which makes
    the forward scalar while the backward, which never sees the bias, stays vector.  The padding's gradient is exactly zero."""
    from wsi_hgnn_amd import ops
    n, nt, ei, ec, sinks = sweep
    case = C.ra_case((n, nt, ei), Cw)
    ft, sc, bias, w = case["inputs"]
    s = sc.to(DEV).requires_grad_(True)
    if variant == "bias":
        f = ft.to(DEV).requires_grad_(True)
        buf = torch.zeros(Cw + 4, device=DEV)
        buf[1:Cw + 1] = bias.to(DEV)
        buf.requires_grad_(True)
        b = buf[1:Cw + 1]
        assert buf.data_ptr() % 16 == 0 and f.data_ptr() % 16 == 0 and b.data_ptr() % 16 == 4 and b.is_contiguous()
        fwd_code, bwd_code = ra_code(Cw, False), ra_code(Cw, True)
        assert fwd_code != bwd_code
    else:
        wide = torch.zeros(n, Cw + 1, device=DEV)
        first = 0 if variant == "stride" else 1
        wide[:, first:first + Cw] = ft.to(DEV)
        wide.requires_grad_(True)
        f = wide[:, first:first + Cw]
        b = bias.to(DEV).requires_grad_(True)
        assert f.stride() == (Cw + 1, 1) and f.data_ptr() % 16 == 4 * first
        fwd_code = bwd_code = ra_code(Cw, False)
    assert fwd_code // 100000 == 1 and ra_code(Cw) // 100000 == 4
    out = ops.ra_attention(f, s, b, ec, nt.to(DEV))
    out.backward(w.to(DEV))
    if variant == "bias":
        g_ft, g_b = f.grad, buf.grad[1:Cw + 1]
        assert float(buf.grad[0]) == 0.0 and not buf.grad[Cw + 1:].any()
    else:
        g_ft, g_b = wide.grad[:, first:first + Cw], b.grad
        assert not wide.grad[:, Cw if variant == "stride" else 0].any(), "the padding column's gradient is exactly zero"
    got = (out.detach(), g_ft, s.grad, g_b)
    label = f"fwd {fwd_code} bwd {bwd_code} C={Cw} {variant}"
    _exact_facts(got, bias, n, sinks, label)
    _hold(got, case, label)


# ------------------------------------------------------------------------------------------------ the raw C ABI
SENTINEL = 777.0


def _padded(t, pad):
    """A device view of ``t``'s values whose row stride is its width + pad; the padding holds SENTINEL."""
    buf = torch.full((t.shape[0], t.shape[1] + pad), SENTINEL, device=DEV)
    buf[:, :t.shape[1]] = t.to(DEV)
    return buf, buf[:, :t.shape[1]]


def _raw(ec, nt32, ft, sc, bias, g_out, out, g_ft, slope=0.2, want_bias=True):
    """wsi_ra_attn_fwd and wsi_ra_attn_bwd on 2-D device views (row strides as they are); out and g_ft are written in place.  ``ec``: the
    plan's five index arrays and E.  Returns (stat, g_sc, g_bias or None)."""
    from wsi_hgnn_amd import _native as N
    lib = N.load()
    rowptr, src, colptr, csc_eid, csc_dst, E = ec
    n, Cw = ft.shape
    stat = torch.full((n, 3, 4), SENTINEL, device=DEV)
    N.check(lib.wsi_ra_attn_fwd(N.ptr(ft), ft.stride(0), N.ptr(sc), N.ptr(nt32), n, Cw, N.ptr(rowptr), N.ptr(src), slope, N.ptr(bias),
                                N.ptr(out), out.stride(0), N.ptr(stat), N.stream()), "wsi_ra_attn_fwd")
    edge_ws = torch.empty(E, device=DEV) if E else None
    group_ws = torch.empty(3 * n, device=DEV)
    bias_ws = torch.empty(N.WSI_RA_BIAS_PARTS * Cw, device=DEV) if want_bias else None
    g_sc = torch.full((n, 4), SENTINEL, device=DEV)
    g_b = torch.full((Cw,), SENTINEL, device=DEV) if want_bias else None
    N.check(lib.wsi_ra_attn_bwd(N.ptr(ft), ft.stride(0), N.ptr(sc), N.ptr(nt32), N.ptr(stat), N.ptr(g_out), g_out.stride(0), n, E, Cw,
                                N.ptr(rowptr), N.ptr(src), N.ptr(colptr), N.ptr(csc_eid), N.ptr(csc_dst), slope, N.ptr(edge_ws), N.ptr(group_ws),
                                N.ptr(bias_ws), N.ptr(g_ft), g_ft.stride(0), N.ptr(g_sc), N.ptr(g_b), N.stream()), "wsi_ra_attn_bwd")
    torch.cuda.synchronize()
    return stat, g_sc, g_b


def _plan(ec):
    return ec.rowptr, ec.src, ec.colptr, ec.csc_eid, ec.csc_dst, ec.num_edges


@pytest.mark.parametrize("Cw,pad", [(44, 1), (44, 4), (772, 1), (772, 4)])
def test_raw_abi_row_strides_leave_the_padding_alone(sweep, Cw, pad):
    """ldo = ldg = ldgf = C + pad.  C + 1 sends both directions down the scalar family; C + 4 keeps the 16-byte accesses, and a store that
    ran past C would land on the sentinel."""
    n, nt, ei, ec, sinks = sweep
    case = C.ra_case((n, nt, ei), Cw)
    ft, sc, bias, w = case["inputs"]
    code = ra_code(Cw, pad % 4 == 0)
    assert code // 100000 == (4 if pad == 4 else 1)
    _, g_v = _padded(w, pad)
    out_buf, out_v = _padded(torch.zeros(n, Cw), pad)
    gft_buf, gft_v = _padded(torch.zeros(n, Cw), pad)
    assert out_v.stride(0) == g_v.stride(0) == gft_v.stride(0) == Cw + pad
    _, g_sc, g_b = _raw(_plan(ec), ec.node_type, ft.to(DEV), sc.to(DEV), bias.to(DEV), g_v, out_v, gft_v)
    got = (out_v, gft_v, g_sc, g_b)
    label = f"{code} C={Cw} row strides C+{pad}"
    _exact_facts(got, bias, n, sinks, label)
    _hold(got, case, label)
    for name, buf in (("out", out_buf), ("g_ft", gft_buf)):
        assert bool((buf[:, Cw:] == SENTINEL).all()), f"{label}: the padding of {name} was overwritten"


def test_raw_abi_without_g_bias(sweep):
    """g_bias and bias_ws NULL: the other gradients are what they are with them."""
    n, nt, ei, ec, _ = sweep
    Cw = 44
    ft, sc, bias, w = (t.to(DEV) for t in C.ra_case((n, nt, ei), Cw)["inputs"])
    runs = []
    for want_bias in (True, False):
        out, g_ft = torch.empty(n, Cw, device=DEV), torch.empty(n, Cw, device=DEV)
        stat, g_sc, g_b = _raw(_plan(ec), ec.node_type, ft, sc, bias, w, out, g_ft, want_bias=want_bias)
        runs.append((out, g_ft, stat, g_sc))
        assert (g_b is None) != want_bias
    for a, b in zip(*runs):
        assert torch.equal(a, b)


def test_raw_abi_without_edges_and_without_nodes():
    """E = 0 with edge_ws NULL: out = bias, every group absent, g_ft = g_sc = 0, g_bias = the column sums of g_out.  n = 0: nothing is read,
    and a g_bias that is given is zeroed."""
    from wsi_hgnn_amd import _native as N
    n, Cw = 5, 13
    ft, sc, bias, w = (t.to(DEV) for t in C.ra_inputs(n, Cw))
    zeros = torch.zeros(n + 1, dtype=torch.int32, device=DEV)
    dummy = torch.zeros(1, dtype=torch.int32, device=DEV)
    nt32 = torch.tensor([0, 1, 2, 0, 1], dtype=torch.int32, device=DEV)
    out, g_ft = torch.full((n, Cw), SENTINEL, device=DEV), torch.full((n, Cw), SENTINEL, device=DEV)
    stat, g_sc, g_b = _raw((zeros, dummy, zeros, dummy, dummy, 0), nt32, ft, sc, bias, w, out, g_ft)
    assert torch.equal(out, bias.expand(n, Cw)) and not g_ft.any() and not g_sc.any()
    assert bool((stat == torch.tensor([float("inf"), 0.0, 0.0, 0.0], device=DEV)).all())
    R.check(g_b, w.double().sum(0), "g_bias", "E = 0")
    lib = N.load()
    g_b = torch.full((8,), SENTINEL, device=DEV)
    N.check(lib.wsi_ra_attn_fwd(None, 8, None, None, 0, 8, None, None, 0.2, None, None, 8, None, N.stream()), "wsi_ra_attn_fwd(n = 0)")
    N.check(lib.wsi_ra_attn_bwd(None, 8, None, None, None, None, 8, 0, 0, 8, None, None, None, None, None, 0.2, None, None, None, None, 8, None,
                                N.ptr(g_b), N.stream()), "wsi_ra_attn_bwd(n = 0)")
    torch.cuda.synchronize()
    assert not g_b.any()


@pytest.mark.parametrize("scale,slope", [(1.0, 0.2), (30.0, 0.2), (1.0, 0.0)])
def test_stat_is_what_the_header_defines(sweep, scale, slope):
    """stat [n, 3, 4] = max | log-sum | count | beta, the forward's message to the backward, against float64: counts exact, an absent group
    exactly (+inf, 0, 0, 0), the maximum, max + log-sum (the group's logsumexp) and beta within the tolerance, the betas present at a node
    summing to 1 within 1e-6."""
    n, nt, ei, ec, _ = sweep
    Cw = 44 if slope else 257
    case = C.ra_case((n, nt, ei), Cw, scale=scale, slope=slope)
    ft, sc, bias, w = case["inputs"]
    out, g_ft = torch.empty(n, Cw, device=DEV), torch.empty(n, Cw, device=DEV)
    stat, _, _ = _raw(_plan(ec), ec.node_type, ft.to(DEV), sc.to(DEV), bias.to(DEV), w.to(DEV), out, g_ft, slope=slope)
    stat = stat.cpu()
    ref = C.ra_stat_ref(sc, ei, nt, slope)
    present = ref[:, :, 2] > 0
    assert 0 < int(present.sum()) < 3 * n and int((present.sum(1) == 0).sum()) >= 2
    assert torch.equal(stat[:, :, 2].double(), ref[:, :, 2]), "the counts are exact"
    assert bool((stat[~present] == torch.tensor([float("inf"), 0.0, 0.0, 0.0])).all()), "an absent group is (+inf, 0, 0, 0)"
    label = f"stat sc x {scale:g} slope {slope}"
    R.check(stat[:, :, 0][present], ref[:, :, 0][present], "stat max", label)
    R.check((stat[:, :, 0].double() + stat[:, :, 1].double())[present], (ref[:, :, 0] + ref[:, :, 1])[present], "stat logsumexp", label)
    R.check(stat[:, :, 3], ref[:, :, 3], "stat beta", label)
    assert bool((stat[:, :, 1][present] >= 0).all())
    sums = stat[:, :, 3].double().sum(1)[present.any(1)]
    print(f"{label}: largest |sum of the present betas - 1| {float((sums - 1).abs().max()):.3e}")
    assert float((sums - 1).abs().max()) <= 1e-6
    assert not stat[:, :, 3][~present].any()


# ------------------------------------------------------------------------------------------------ wsi_ihpool_assign
@pytest.fixture(scope="module")
def assign_case():
    case, _ = C.find_case(C.assign_case, lambda c: float(C.assign_ref(*c)[1].min()))
    return case


def test_ihpool_assign_equals_the_restatement_exactly(assign_case):
    from wsi_hgnn_amd import ops
    sizes = torch.bincount(assign_case[2].long())
    assert sorted(set(sizes.tolist())) == [0, 1, 2, 63, 64, 65, 300]
    want, gaps = C.assign_ref(*assign_case)
    assert float(gaps.min()) >= C.MARGIN
    dev = [t.to(DEV) for t in assign_case]
    got = ops.ihpool_assign(*dev)
    assert got.dtype == torch.int32 and torch.equal(got.cpu().long(), want)
    assert torch.equal(got, ops.ihpool_assign(*dev))
    # every seed sits in its own cluster
    pos = torch.arange(assign_case[4].shape[0]) - assign_case[3].long()[torch.repeat_interleave(torch.arange(len(sizes)), assign_case[3].long().diff())]
    where = {int(nd): i for i, nd in enumerate(assign_case[1].tolist())}
    assert all(int(want[where[int(nd)]]) == int(p) for nd, p in zip(assign_case[4].tolist(), pos.tolist()))


def test_ihpool_assign_ties_and_edges():
    from wsi_hgnn_amd import ops
    i32 = lambda *v: torch.tensor(v, dtype=torch.int32, device=DEV)
    # segment 0: seeds at nodes 0 and 1, node 2 exactly between them -> the lowest seed; nodes 0 and 1 coincide with seeds 3 and 4 of segment 1,
    # where node 4 is a seed at the very place of seed 3: it still owns its cluster; segment 2 is empty; segment 3 has a member and no seed
    xyf = torch.tensor([[0.0, 0.0, 0.0], [0.5, 0.0, 0.0], [0.25, 0.0, 0.0], [0.3, 0.3, 0.1], [0.3, 0.3, 0.1], [0.3, 0.3, 0.1], [0.9, 0.9, 0.9]], device=DEV)
    got = ops.ihpool_assign(xyf, i32(0, 1, 2, 3, 4, 5, 6), i32(0, 0, 0, 1, 1, 1, 3), i32(0, 2, 4, 4, 4), i32(0, 1, 3, 4))
    assert got.tolist() == [0, 1, 0, 0, 1, 0, -1]
    assert ops.ihpool_assign(xyf, i32(), i32(), i32(0), i32()).numel() == 0


def test_ihpool_assign_over_three_tiles_of_seeds():
    """128 seeds (two full tiles of 64) and 129 (a third tile of one seed)."""
    from wsi_hgnn_amd import ops
    case, _ = C.find_case(C.assign_tiles_case, lambda c: float(C.assign_ref(*c)[1].min()))
    assert case[3].diff().tolist() == list(C.ASSIGN_TILE_SEEDS)
    want = C.assign_ref(*case)[0]
    got = ops.ihpool_assign(*[t.to(DEV) for t in case])
    assert torch.equal(got.cpu().long(), want)
    assert int(want[case[2] == 1].max()) == 128                  # the third tile's only seed owns its cluster


def test_ihpool_assign_ignores_indices_outside_the_tables():
    """The header's promise, through the raw ABI: xyf points ASSIGN_LEAD rows into a larger buffer and num_nodes ends before the buffer does,
    so every outside index of the case, followed or not, names allocated memory.  Outside member_node: -1; an outside seed is never
    chosen (the row it names holds a member's own coordinates: distance 0 if it were read), -1 if it is the segment's only one;
    member_seg >= num_segs: -1; everything else equals the float64 restatement on the cleaned case."""
    from wsi_hgnn_amd import _native as N
    case, _ = C.find_case(C.assign_outside_case, lambda c: c[6])
    buf, member_node, member_seg, seed_ptr, seed_node, want, _ = case
    T, lead = C.ASSIGN_TABLE, C.ASSIGN_LEAD
    assert tuple(buf.shape) == (C.ASSIGN_ROWS, 3) and lead + T < C.ASSIGN_ROWS
    for t in (member_node, seed_node):
        assert int(t.min()) >= -lead and int(t.max()) < C.ASSIGN_ROWS - lead and (int(t.min()) < 0 or int(t.max()) >= T)
    num_segs, m = seed_ptr.numel() - 1, member_node.numel()
    assert int(member_seg.max()) == num_segs + 1 and int(seed_ptr[-1]) == seed_node.numel()
    d_buf, d_node, d_seg, d_ptr, d_seed = (t.to(DEV).contiguous() for t in (buf, member_node, member_seg, seed_ptr, seed_node))
    runs = []
    for _ in range(2):
        assign = torch.full((m,), -7, dtype=torch.int32, device=DEV)
        N.check(N.load().wsi_ihpool_assign(N.ptr(d_buf, lead * 3 * 4), T, N.ptr(d_node), N.ptr(d_seg), m, N.ptr(d_ptr), N.ptr(d_seed), num_segs,
                                           seed_node.numel(), N.ptr(assign), N.stream()), "wsi_ihpool_assign")
        torch.cuda.synchronize()
        runs.append(assign.cpu().long())
    got = runs[0]
    outside = (member_node < 0) | (member_node >= T)
    assert bool((got[outside] == -1).all()), "a member outside the node table gets -1"
    assert bool((got[(member_seg >= num_segs) | (member_seg < 0)] == -1).all()), "a member of a segment before the first or past the last gets -1"
    assert bool((got[member_seg == 1] == -1).all()), "a segment whose only seed lies outside the table has no seed"
    wrong = (got != want).nonzero().view(-1).tolist()
    assert not wrong, [(i, int(member_seg[i]), int(got[i]), int(want[i])) for i in wrong[:8]]
    assert torch.equal(runs[0], runs[1])
    assert torch.equal(d_buf.cpu(), buf)                         # read only
