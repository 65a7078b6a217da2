"""The segment dots, the weighted sums and the loss kernel (csrc/segment.hip, csrc/loss.hip) through the raw C ABI against float64, at the
widths, strides, bases and segment sizes where a tail, tile or chunk-edge mistake would show.  Cases, layouts, references and bounds:
tests/segment_tail_cases.py (checked without a GPU by tests/test_segment_tail_cases.py).

  A. wsi_segment_dot_diff       D on both sides of 4 and of the 256-column tile x five layouts (16-byte path, scalar tail, scalar path by
                                stride, by base, by ONE operand's base) x {integers, gaussian, cancelling}; a plan that starts at row 7; a
                                segment of 71 chunks; no chunk, no segment; two calls bit for bit.
  B. wsi_gate_grad              from the rows in float64 (never through wsi_segment_dot_diff): gate maps with shared, unfed, empty-fed and
                                -1 gates, n_gates 1 / 3 / 300, skip randn / +-30 / 0, exact at skip = -100, num_segs 8192 and 8193.
  C. wsi_segment_weighted_sums  D x J on both sides of the 16-wide weight groups x layouts of x x padded w; J = 1024 and 1025.
     wsi_pool_factors           hp / csum / x_mean with the ones column in an open group, alone in a new one, behind a full one.
  D. wsi_cross_entropy          logits whose expf overflows, -inf rows, equal maxima, the B * C limit from both sides, ignored rows where a
                                thread's first and second row meet.  (1, 65536) found the serial denominator: its partial sum swallowed
                                the row's small terms, loss 1.9 x and gradient 5.3 x their tolerances; csrc/loss.hip now sums in blocks.

``integers``: torch.equal with the float64 reference cast down.  ``gaussian``: every entry within n_chain * 2^-24 * (float64 sum of the
absolute values of ITS terms).  NaN lies in every padding column, every row outside the plan, every output, the scratch and the margins
around outputs and scratch before each call; outputs come back finite and fully written, margins bit for bit as they were.  The largest
error / bound per kernel is printed at the end of the module."""
import pytest
import torch

import segment_tail_cases as C

pytestmark = pytest.mark.gpu

DEV = "cuda"
MARGIN = 64                         # floats of NaN on either side of every output and scratch buffer (256 bytes: the body stays aligned)
RATIOS = {}                         # kernel output -> (largest error / bound over the module's run, the case it came from)


@pytest.fixture(scope="module", autouse=True)
def _report_ratios():
    yield
    for name, (r, case) in sorted(RATIOS.items()):
        print(f"\nlargest error / bound, {name}: {r:.3e} ({case})", end="")
    print()


@pytest.fixture(scope="module")
def api():
    from wsi_hgnn_amd import _native as N
    return N, N.load()


# ---------------------------------------------------------------------------------------------------- helpers
class _Out:
    """n floats of NaN between two NaN margins."""

    def __init__(self, n):
        self.n = n
        self.buf = torch.full((n + 2 * MARGIN,), C.NAN, dtype=torch.float32, device=DEV)
        self.before = self.buf.view(torch.int32).clone()

    def ptr(self, N):
        return N.ptr(self.buf, MARGIN * 4)

    def body(self):
        return self.buf[MARGIN:MARGIN + self.n]

    def margins_untouched(self):
        now = self.buf.view(torch.int32)
        return torch.equal(now[:MARGIN], self.before[:MARGIN]) and torch.equal(now[MARGIN + self.n:], self.before[MARGIN + self.n:])

    def untouched(self):
        return torch.equal(self.buf.view(torch.int32), self.before)

    def written(self):
        """The body, after checking that every entry was written with a finite value and nothing around it was touched."""
        assert self.margins_untouched(), "wrote outside its output"
        b = self.body()
        assert bool(torch.isfinite(b).all()), "an output entry was not written (or is not finite)"
        return b


def _upload(table, layout, live, N):
    """(keep-alive buffer, device pointer of the first element, row stride) of a table embedded under a layout."""
    buf, off, ld = C.embed(table, layout, live)
    d = buf.to(DEV)
    assert d.data_ptr() % 16 == 0
    return d, N.ptr(d, off * 4), ld


_PLANS = {}


def _tables(plan):
    """The plan's chunk tables on the device, from ops.ReducePlan.from_ranges (they equal the cases file's)."""
    if plan not in _PLANS:
        from wsi_hgnn_amd import ops
        rp = ops.ReducePlan.from_ranges(plan.ranges, DEV)
        assert rp.chunk_row.tolist() == plan.chunk_row and rp.seg_chunk.tolist() == plan.seg_chunk
        assert (rp.num_chunks, rp.num_segs, rp.first_row) == (plan.num_chunks, plan.num_segs, plan.first_row)
        _PLANS[plan] = rp
    return _PLANS[plan]


def _record(what, case, ratio):
    print(f"{case} {what}: error / bound {ratio:.3e}")
    if ratio > RATIOS.get(what, (-1.0, None))[0]:
        RATIOS[what] = (ratio, case)


def _exact(what, case, got, ref):
    want = ref.float()
    assert torch.equal(want.double(), ref), f"{case} {what}: the reference is no fp32 number"
    got = got.detach().cpu().reshape(want.shape)
    bad = int((got != want).sum())
    assert torch.equal(got, want), f"{case} {what}: {bad} of {want.numel()} entries differ from the exact result"


def _within(what, case, got, ref, bound):
    """|got - ref| <= bound entry by entry (equality where the bound is 0); records the largest error / bound."""
    got = got.detach().double().cpu().reshape(ref.shape)
    assert bool(torch.isfinite(got).all()), f"{case} {what}: not finite"
    err = (got - ref).abs()
    zero = bound == 0
    assert bool((err[zero] == 0).all()), f"{case} {what}: an entry with bound 0 is not exact"
    ratio = float((err[~zero] / bound[~zero]).max()) if bool((~zero).any()) else 0.0
    _record(what, case, ratio)
    assert ratio <= 1.0, f"{case} {what}: error / bound {ratio:.3e}"


# ---------------------------------------------------------------------------------------------------- A. wsi_segment_dot_diff
def _dot_operands(family, plan, D, layout, N):
    live = plan.live()
    return [_upload(t, name, live, N) for t, name in zip(C.dot_inputs(family, plan, D), C.dot_layouts(layout, D))]


def _n_partial(plan, D):
    return plan.num_chunks * C.cdiv(D, 256)


def _dot_call(api, plan, D, ops3):
    N, lib = api
    rp = _tables(plan)
    out, partial = _Out(plan.num_segs), _Out(_n_partial(plan, D))
    (_, pg, ldg), (_, pa, lda), (_, pb, ldb) = ops3
    N.check(lib.wsi_segment_dot_diff(pg, ldg, pa, lda, pb, ldb, D, N.ptr(rp.chunk_row), rp.num_chunks, N.ptr(rp.seg_chunk), rp.num_segs,
                                     partial.ptr(N), out.ptr(N), N.stream()), "wsi_segment_dot_diff")
    torch.cuda.synchronize()
    assert partial.margins_untouched(), "wrote outside its scratch"
    return out.written().clone()


def _check_dots(api, plan, D, layout):
    N, _ = api
    empty = torch.tensor(plan.sizes) == 0
    for family in C.DOT_FAMILIES:
        case = f"dot {plan.name} D={D} {layout} {family}"
        ops3 = _dot_operands(family, plan, D, layout, N)
        vec = all(p % 16 == 0 and ld % 4 == 0 for _, p, ld in ops3)
        assert vec == C.dot_vec(layout, D), case
        got = _dot_call(api, plan, D, ops3)
        ref, scale, bound = C.dot_reference(family, plan, D)
        assert bool((got.cpu()[empty] == 0).all()), f"{case}: an empty segment is not exactly 0"
        if family == "integers":
            _exact("segment_dot_diff", case, got, ref)
        else:
            _within("segment_dot_diff", case, got, ref, bound)
        assert torch.equal(got, _dot_call(api, plan, D, ops3)), f"{case}: two identical calls differ"


@pytest.mark.parametrize("layout", C.DOT_LAYOUTS)
@pytest.mark.parametrize("D", C.DOT_D)
def test_segment_dot_diff(api, D, layout):
    _check_dots(api, C.PLAN, D, layout)


@pytest.mark.parametrize("layout", C.DOT_LAYOUTS)
@pytest.mark.parametrize("D", C.DOT_D_ROW7)
def test_segment_dot_diff_plan_from_row_7(api, D, layout):
    _check_dots(api, C.PLAN7, D, layout)


@pytest.mark.parametrize("layout", ["plain", "pad4", "offset"])
@pytest.mark.parametrize("D", C.DOT_D_LONG)
def test_segment_dot_diff_more_partials_than_lanes(api, D, layout):
    _check_dots(api, C.PLAN_LONG, D, layout)


def test_segment_dot_diff_without_chunks_and_without_segments(api):
    N, lib = api
    plan = C.PLAN_EMPTY
    rp = _tables(plan)
    out = _Out(plan.num_segs)
    rc = lib.wsi_segment_dot_diff(None, 5, None, 5, None, 5, 5, N.ptr(rp.chunk_row), 0, N.ptr(rp.seg_chunk), plan.num_segs, None, out.ptr(N), N.stream())
    torch.cuda.synchronize()
    assert rc == N.WSI_OK
    assert bool((out.written() == 0).all())
    out = _Out(4)
    rc = lib.wsi_segment_dot_diff(None, 5, None, 5, None, 5, 5, None, 0, None, 0, None, out.ptr(N), N.stream())
    torch.cuda.synchronize()
    assert rc == N.WSI_OK and out.untouched()


# ---------------------------------------------------------------------------------------------------- B. wsi_gate_grad
def _gate_call(api, plan, D, ops3, seg_gate, skip, n_gates):
    N, lib = api
    rp = _tables(plan)
    out, partial = _Out(n_gates), _Out(_n_partial(plan, D))
    sg = torch.tensor(seg_gate, dtype=torch.int32, device=DEV)
    sk = skip.to(DEV)
    (_, pg, ldg), (_, pa, lda), (_, pb, ldb) = ops3
    rc = lib.wsi_gate_grad(pg, ldg, pa, lda, pb, ldb, D, N.ptr(rp.chunk_row), rp.num_chunks, N.ptr(rp.seg_chunk), rp.num_segs,
                           N.ptr(sg), N.ptr(sk), n_gates, partial.ptr(N), out.ptr(N), N.stream())
    torch.cuda.synchronize()
    assert partial.margins_untouched(), "wrote outside its scratch"
    return rc, out


def _check_gates(api, plan, D, layout, maps):
    N, _ = api
    for family in C.DOT_FAMILIES:
        ops3 = _dot_operands(family, plan, D, layout, N)
        dots, _, dot_bounds = C.dot_reference(family, plan, D)
        for n_gates, seg_gate in maps.items():
            fed = {gt for gt in seg_gate if gt >= 0}
            for kind in ((-100.0,) if family == "integers" else C.SKIP_KINDS):
                case = f"gate {plan.name} D={D} {layout} {family} n_gates={n_gates} skip={kind}"
                skip = C.gate_skip(kind, n_gates)
                rc, out = _gate_call(api, plan, D, ops3, seg_gate, skip, n_gates)
                assert rc == N.WSI_OK, case
                got = out.written().clone()
                ref, bound, sums = C.gate_reference(dots, dot_bounds, seg_gate, skip, n_gates)
                unfed = torch.tensor([gt not in fed for gt in range(n_gates)])
                assert bool((got.cpu()[unfed] == 0).all()), f"{case}: a gate that nothing feeds is not exactly 0"
                if family == "integers":
                    _exact("gate_grad", case, got, sums)          # the factor is exactly 1.0: the integer sums of the gates
                else:
                    _within("gate_grad", case, got, ref, bound)
            rc, again = _gate_call(api, plan, D, ops3, seg_gate, skip, n_gates)
            assert torch.equal(got, again.written()), f"{case}: two identical calls differ"


@pytest.mark.parametrize("layout", C.DOT_LAYOUTS)
@pytest.mark.parametrize("D", C.GATE_D)
def test_gate_grad(api, D, layout):
    _check_gates(api, C.PLAN, D, layout, C.GATE_MAPS)


def test_gate_grad_more_partials_than_lanes(api):
    _check_gates(api, C.PLAN_LONG, 5, "plain", {3: (1, 0, 2), 1: (-1, 0, 0)})


def test_gate_grad_num_segs_limit(api):
    N, _ = api
    for num_segs, want in ((8192, N.WSI_OK), (8193, N.WSI_EINVAL)):
        plan, seg_gate = C.many_segments(num_segs)
        ops3 = _dot_operands("integers", plan, 4, "plain", N)
        skip = C.gate_skip(-100.0, 3)
        rc, out = _gate_call(api, plan, 4, ops3, seg_gate, skip, 3)
        assert rc == want, num_segs
        if want == N.WSI_OK:
            dots, scale, dot_bounds = C.dot_reference("integers", plan, 4)
            assert C.exact_condition(scale)
            _exact("gate_grad", f"gate num_segs={num_segs}", out.written(), C.gate_reference(dots, dot_bounds, seg_gate, skip, 3)[2])
        else:
            assert out.untouched(), "a refused call wrote g_skip"


# ---------------------------------------------------------------------------------------------------- C. the weighted sums
def _wsum_call(api, plan, x_up, w_up, D, J, expect=None):
    N, lib = api
    rp = _tables(plan)
    out, partial = _Out(plan.num_segs * J * D), _Out(plan.num_chunks * J * D)
    (_, px, ldx), (wd, ldw) = x_up, w_up
    rc = lib.wsi_segment_weighted_sums(px, ldx, D, N.ptr(wd), ldw, J, N.ptr(rp.chunk_row), rp.num_chunks, N.ptr(rp.seg_chunk), rp.num_segs,
                                       partial.ptr(N), out.ptr(N), N.stream())
    torch.cuda.synchronize()
    assert partial.margins_untouched(), "wrote outside its scratch"
    if expect is not None:
        assert rc == expect
        return out
    assert rc == N.WSI_OK, lib.wsi_last_error()
    return out.written().view(plan.num_segs, J, D).clone()


def _check_close_or_exact(what, case, family, got, ref, bound):
    if family == "integers":
        _exact(what, case, got, ref)
    else:
        _within(what, case, got, ref, bound)


@pytest.mark.parametrize("J", C.WSUM_J)
@pytest.mark.parametrize("D", C.WSUM_D)
def test_segment_weighted_sums(api, D, J):
    N, _ = api
    plan = C.PLAN
    for family in C.WSUM_FAMILIES:
        x, w = C.wsum_inputs(family, plan, D, J)
        r = C.wsum_reference(family, plan, D, J)
        first = None
        for layout in C.X_LAYOUTS:
            x_up = _upload(x, layout, plan.live(), N)
            for ldw in (J, J + 3):
                case = f"wsum D={D} J={J} {layout} ldw={ldw} {family}"
                got = _wsum_call(api, plan, x_up, (C.embed_ld(w, ldw).to(DEV), ldw), D, J)
                _check_close_or_exact("segment_weighted_sums", case, family, got, r["out"], r["bound"])
                first = got if first is None else first
        x_up = _upload(x, "plain", plan.live(), N)
        assert torch.equal(first, _wsum_call(api, plan, x_up, (C.embed_ld(w, J).to(DEV), J), D, J)), "two identical calls differ"


def test_segment_weighted_sums_weight_limit(api):
    N, _ = api
    plan = C.PLAN
    x, w = C.wsum_inputs("integers", plan, 1, 1024)
    r = C.wsum_reference("integers", plan, 1, 1024)
    x_up = _upload(x, "plain", plan.live(), N)
    got = _wsum_call(api, plan, x_up, (C.embed_ld(w, 1024).to(DEV), 1024), 1, 1024)
    _exact("segment_weighted_sums", "wsum D=1 J=1024", got, r["out"])
    out = _wsum_call(api, plan, x_up, (C.embed_ld(w, 1028).to(DEV), 1028), 1, 1025, expect=N.WSI_EINVAL)
    assert out.untouched(), "a refused call wrote its output"


def _pool_call(api, plan, x_up, w_up, D, T, H, Bg, with_mean):
    N, lib = api
    rp = _tables(plan)
    S, J = T * Bg, T * H
    hp, csum, xm = _Out(S * H * T * D), _Out(T * S * H), _Out(S * D)
    partial = _Out(plan.num_chunks * (J + 1) * (D + 1))
    (_, px, ldx), (wd, ldw) = x_up, w_up
    N.check(lib.wsi_pool_factors(px, ldx, D, N.ptr(wd), ldw, T, H, Bg, N.ptr(rp.chunk_row), rp.num_chunks, N.ptr(rp.seg_chunk),
                                 partial.ptr(N), hp.ptr(N), csum.ptr(N), xm.ptr(N) if with_mean else None, N.stream()), "wsi_pool_factors")
    torch.cuda.synchronize()
    assert partial.margins_untouched(), "wrote outside its scratch"
    if not with_mean:
        assert xm.untouched()
    return hp.written().view(S, H, T, D).clone(), csum.written().view(T, S, H).clone(), (xm.written().view(S, D).clone() if with_mean else None)


@pytest.mark.parametrize("D", C.POOL_D)
@pytest.mark.parametrize("T,H,Bg", C.POOL_SHAPES)
def test_pool_factors(api, T, H, Bg, D):
    N, _ = api
    J = T * H
    for variant in C.pool_variants(T, Bg):
        plan = C.pool_plan(T, Bg, variant)
        for family in C.WSUM_FAMILIES:
            x, w = C.wsum_inputs(family, plan, D, J)
            r = C.pool_reference(x, w, plan, T, H, Bg)
            mean_bound = C.integer_mean_bound(r["x_mean"], plan) if family == "integers" else r["x_mean_bound"]
            for layout in C.X_LAYOUTS:
                case = f"pool T={T} H={H} Bg={Bg} sizes={plan.name} D={D} {layout} {family}"
                x_up = _upload(x, layout, plan.live(), N)
                ldw = J if layout in ("plain", "offset") else J + 3
                w_up = (C.embed_ld(w, ldw).to(DEV), ldw)
                hp, csum, _ = _pool_call(api, plan, x_up, w_up, D, T, H, Bg, False)
                _check_close_or_exact("pool_factors hp", case, family, hp, r["hp"], r["hp_bound"])
                _check_close_or_exact("pool_factors csum", case, family, csum, r["csum"], r["csum_bound"])
                hp2, csum2, xm = _pool_call(api, plan, x_up, w_up, D, T, H, Bg, True)
                assert torch.equal(hp2, hp) and torch.equal(csum2, csum), f"{case}: hp / csum change with x_mean"
                _within("pool_factors x_mean", case, xm, r["x_mean"], mean_bound)
                old = _wsum_call(api, plan, x_up, w_up, D, J)
                assert torch.equal(C.permute_hp(old, T, H, Bg), hp), f"{case}: hp is not the permuted segment_weighted_sums"


# ---------------------------------------------------------------------------------------------------- D. wsi_cross_entropy
def _ce_call(api, B, C_, logits, labels):
    N, lib = api
    loss, dl = _Out(1), _Out(B * C_)
    bad = torch.zeros(1, dtype=torch.int32, device=DEV)
    rc = lib.wsi_cross_entropy(N.ptr(logits), N.ptr(labels), B, C_, loss.ptr(N), dl.ptr(N), N.ptr(bad), N.stream())
    torch.cuda.synchronize()
    return rc, loss, dl, int(bad.item())


@pytest.mark.parametrize("name", sorted(C.ce_cases()))
def test_cross_entropy(api, name):
    N, _ = api
    x, y = C.ce_cases()[name]
    B, C_ = x.shape
    xd, yd = x.to(DEV), y.to(DEV)
    rc, loss, dl, bad = _ce_call(api, B, C_, xd, yd)
    assert rc == N.WSI_OK and bad == 0
    got_loss, got_grad = loss.written().clone(), dl.written().view(B, C_).clone()
    ref_loss, ref_grad = C.ce_reference(x, y)
    e_loss = abs(float(got_loss.double().cpu()[0] - ref_loss)) / (C.CE_LOSS_TOL * max(1.0, abs(float(ref_loss))))
    e_grad = float((got_grad.double().cpu() - ref_grad).abs().max()) / C.CE_GRAD_TOL
    _record("cross_entropy loss", name, e_loss)
    _record("cross_entropy dlogits", name, e_grad)
    assert e_loss <= 1.0 and e_grad <= 1.0, f"{name}: loss error / tolerance {e_loss:.3e}, gradient error / tolerance {e_grad:.3e}"
    assert bool((got_grad.cpu()[y == C.CE_IGNORE] == 0).all()), "an ignored row has a gradient"
    if C_ == 1:
        assert float(got_loss[0]) == 0.0 and bool((got_grad == 0).all())
    rc, loss2, dl2, _ = _ce_call(api, B, C_, xd, yd)
    assert torch.equal(loss2.written(), got_loss) and torch.equal(dl2.written().view(B, C_), got_grad), "two identical calls differ"


@pytest.mark.parametrize("B,C_", C.CE_OVER_LIMIT)
def test_cross_entropy_refuses_what_it_cannot_hold(api, B, C_):
    N, _ = api
    x = torch.zeros(B, C_, device=DEV)
    y = torch.zeros(B, dtype=torch.int64, device=DEV)
    rc, loss, dl, _ = _ce_call(api, B, C_, x, y)
    assert rc == N.WSI_ENOSYS
    assert loss.untouched() and dl.untouched(), "a refused call wrote its outputs"


# ---------------------------------------------------------------------------------------------------- ops.segment_dot_diff's argument checks
def test_ops_segment_dot_diff_checks_its_arguments():
    from wsi_hgnn_amd import ops
    plan, D = C.PLAN, 5
    rp = _tables(plan)
    g, a, b = (t.contiguous() for t in C.dot_inputs("integers", plan, D))
    ref = C.dot_reference("integers", plan, D)[0]
    gd, ad, bd = g.to(DEV), a.to(DEV), b.to(DEV)
    _exact("ops.segment_dot_diff", "contiguous", ops.segment_dot_diff(gd, ad, bd, rp), ref)
    # 1. device, dtype and shape are checked
    with pytest.raises(RuntimeError):
        ops.segment_dot_diff(gd, a, bd, rp)
    with pytest.raises(ValueError):
        ops.segment_dot_diff(gd, ad.double(), bd, rp)
    with pytest.raises(ValueError):
        ops.segment_dot_diff(gd, ad[:, :4], bd, rp)
    with pytest.raises(ValueError):
        ops.segment_dot_diff(gd[:-1], ad[:-1], bd[:-1], rp)
    with pytest.raises(ValueError):
        ops.segment_dot_diff(gd.view(-1), ad.view(-1), bd.view(-1), rp)
    # 2. a column stride that is not 1 (a transposed view, every second column of a wider table) is copied: the same numbers
    at = ad.t().contiguous().t()
    wide = torch.full((plan.total_rows, 2 * D), C.NAN, device=DEV)
    wide[:, ::2] = bd
    assert at.stride(1) != 1 and wide[:, ::2].stride(1) == 2
    assert ops._unit_columns(at) is not at and ops._unit_columns(at).is_contiguous()
    _exact("ops.segment_dot_diff", "column-strided", ops.segment_dot_diff(gd, at, wide[:, ::2], rp), ref)
    # 3. a row-strided view (a column slice of a wider table, NaN around it) is read in place
    table = torch.full((plan.total_rows, 3 * D + 2), C.NAN, device=DEV)
    views = [table[:, 1 + i * D:1 + (i + 1) * D] for i in range(3)]
    for v, t in zip(views, (gd, ad, bd)):
        v.copy_(t)
        assert ops._unit_columns(v) is v and v.stride(0) == 3 * D + 2
    _exact("ops.segment_dot_diff", "row-strided", ops.segment_dot_diff(*views, rp), ref)
