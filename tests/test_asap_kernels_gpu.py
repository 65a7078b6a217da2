"""The four kernel families of csrc/asap.hip on the GPU, on the paths the model-level ASAP tests never take, against float64 on the SAME fp32
inputs.  The cases come from tests/asap_cases.py; tests/test_asap_cases.py proves without a GPU that each has the property it is here for.
  a. wsi_csr_gather_max_* / wsi_asap_attend_* at D in {1, 63, 64, 65, 128, 129, 256, 257, 512, 513, 1024} (every NV instantiation, both sides of a
     64-column boundary) on a 259-node graph (n % 4 == 3) with segments of 1, 63, 64, 65, 70, 128, 129 and 150 edges, nodes without a segment
     and nodes never gathered; forward and every gradient; csr_gather_max bit-equal, the rows that get nothing exactly 0;
  b. ``arg`` read through the C ABI == "first maximum in CSR order" for every (node, column), ties included, and the max backward == the
     routing that arg implies, for all elements;
  c. peaked (30 * randn) and exact-grid scores with and without a common offset of 4096, at D = 65 and 200;
  d. row strides ldx = D + 1, ldo = D + 2, ldg = D + 3, ldgx = D + 5 through the C ABI: bit-equal to the contiguous run, padding untouched;
  e. D = 1025: WSI_ENOSYS from each of the four entry points, outputs untouched;
  f. one node, a ring of five, six nodes without an edge; identical bits from two identical calls;
  g. wsi_graph_topk == the sort formulation at n up to 24575 (grid.y = 1, 2 and 3), four ratios, NaN / inf / signed zeros across the chunks;
  h. wsi_stas at 384 / 385 / 1536 / 1537 distinct columns per row (both table sizes from both sides, the overflow report), and a graph whose rows
     are split between the two launches, with and without per-edge weights.

Bounds: the project's own for these kernels - 2e-6 (out, score) and 5e-6 (gradients) of the largest float64 entry of the tensor, for wsi_stas
1e-6 * max(1, max|want|).  The same bound also holds row by row on nodes 0..6 and n - 1 (``NAMED_ROWS``), relative to the row's own largest
reference entry: out[w], g_x[w] and the scores of w's segment against their own maximum; g_a[w] and g_b[u] are sums of the centred per-edge
terms score_e * (g_out[i_e] . x[j_e] - mean) over w's segment / over the edges that gather u, which cancel (a softmax's score gradients sum to
zero; over a one-edge segment the sum IS zero), so their row scale is the largest float64 |score_e * g_out[i_e] . x[j_e]| under that sum, not
the sum itself.  On the grid regimes every pre-activation is positive, so g_a as a whole cancels to zero and is measured against the largest
term as well.  A (case, figure) listed in ``DERIVED`` did not meet the project bound; its bound is 4 x the error of the same eager scatter
composition run in fp32 on the CPU against float64 on that case in that norm (asap_cases.edge_reference(dtype=float32)), never above 1e-4.
The grid+4096 runs are compared with the grid runs of the GPU itself under the same forward / gradient bounds: sums and differences of those
scores are exact in fp32, so no new number is needed.

Measured on an MI355X (largest error / bound, printed at the end of the module's run): every figure met the project bound, ``DERIVED`` is empty.
  out 0.487 (peaked D=65), score 0.479 (peaked D=65), g_a 0.380 (peaked D=200), g_b 0.136 (peaked D=65), g_x 0.074 (peaked D=200),
  gx_max 0.019 (normal D=256); row by row: out 0.337 (node 6, 150 edges), score 0.189 (node 258), g_x 0.308, g_a 0.264, g_b 0.248, gx_max 0.026;
  grid+4096 against grid: identical bits (0 for every tensor); wsi_stas values 0.051 (combined graph, unit weights).
"""
import pytest
import torch

import asap_cases as AC

pytestmark = pytest.mark.gpu

DEV = "cuda"
FWD, GRAD, CAP = 2e-6, 5e-6, 1e-4
BASE = {"out": FWD, "score": FWD, "g_x": GRAD, "g_a": GRAD, "g_b": GRAD, "gx_max": GRAD}
WIDTHS = (1, 63, 64, 65, 128, 129, 256, 257, 512, 513, 1024)
REGIME_DS = (65, 200)
PADS = (1, 2, 3, 5)                  # ldx - D, ldo - D, ldg - D, ldgx - D
SENTINEL = 777.0
# (case prefix, figure) -> bound by the 4x rule instead of the project bound (see the module docstring)
DERIVED = ()
RATIOS = {}                          # figure -> (largest error / bound over the module's run, case)


@pytest.fixture(scope="module", autouse=True)
def _report_ratios():
    yield
    for name, (r, case) in sorted(RATIOS.items()):
        print(f"\nlargest error / bound, {name}: {r:.3e} ({case})", end="")
    if RATIOS:
        print(f"\nlargest error / bound of the module: {max(r for r, _ in RATIOS.values()):.3e}")


@pytest.fixture(scope="module")
def graph():
    from wsi_hgnn_amd import ops
    n, i, j = AC.edge_graph()
    ec = ops.EdgeCSR(i.to(DEV), j.to(DEV), n)
    assert torch.equal(ec.perm.cpu(), AC.csr_order(i))                 # stable: CSR order inside a segment is the input order
    return n, i, j, ec


# ------------------------------------------------------------------------------------------------ running the kernels
def _run_ops(ec, x, a, b, g_max, g_out):
    from wsi_hgnn_amd import ops
    xd, ad, bd = (t.to(DEV).requires_grad_() for t in (x, a, b))
    mx = ops.csr_gather_max(xd, ec)
    out, score = ops.asap_attend(ad, bd, xd, ec, AC.SLOPE)
    mx.backward(g_max.to(DEV))
    gx_max, xd.grad = xd.grad.clone(), None
    out.backward(g_out.to(DEV))
    torch.cuda.synchronize()
    return {"mx": mx.detach(), "out": out.detach(), "score": score.detach(), "gx_max": gx_max, "g_x": xd.grad, "g_a": ad.grad, "g_b": bd.grad}


def _padded(t, pad):
    """(buffer, view): the values of ``t`` under a row stride of its width + pad; the padding holds SENTINEL."""
    buf = torch.full((t.shape[0], t.shape[1] + pad), SENTINEL, device=DEV)
    buf[:, :t.shape[1]] = t.to(DEV)
    return buf, buf[:, :t.shape[1]]


def _run_raw(ec, x, a, b, g_max, g_out, pads=(0, 0, 0, 0)):
    """The same four calls through the C ABI with row strides D + pads; returns the results (views), arg and the padded buffers."""
    from wsi_hgnn_amd import _native as N
    lib = N.load()
    n, D, E = x.shape[0], x.shape[1], ec.num_edges
    px, po, pg, pgx = pads
    xbuf, xv = _padded(x, px)
    g1buf, g1v = _padded(g_max, pg)
    g2buf, g2v = _padded(g_out, pg)
    blank = torch.full((n, D), SENTINEL)
    mxbuf, mxv = _padded(blank, po)
    outbuf, outv = _padded(blank, po)
    gmbuf, gmv = _padded(blank, pgx)
    gxbuf, gxv = _padded(blank, pgx)
    ad, bd = a.to(DEV).contiguous().view(-1), b.to(DEV).contiguous().view(-1)
    arg = torch.full((n, D), -7, dtype=torch.int32, device=DEV)
    score, gpre = torch.zeros(max(E, 1), device=DEV), torch.zeros(max(E, 1), device=DEV)
    g_a, g_b = torch.empty(n, device=DEV), torch.empty(n, device=DEV)
    P, st = N.ptr, N.stream()
    N.check(lib.wsi_csr_gather_max_fwd(P(xv), xv.stride(0), n, D, P(ec.rowptr), P(ec.src), P(mxv), mxv.stride(0), P(arg), st), "gather_max_fwd")
    N.check(lib.wsi_csr_gather_max_bwd(P(g1v), g1v.stride(0), P(arg), n, D, P(ec.colptr), P(ec.csc_eid), P(ec.csc_dst), P(gmv), gmv.stride(0), st),
            "gather_max_bwd")
    N.check(lib.wsi_asap_attend_fwd(P(ad), P(bd), P(xv), xv.stride(0), n, D, P(ec.rowptr), P(ec.src), AC.SLOPE, P(score), P(outv), outv.stride(0), st),
            "asap_attend_fwd")
    N.check(lib.wsi_asap_attend_bwd(P(ad), P(bd), P(xv), xv.stride(0), n, D, P(ec.rowptr), P(ec.src), P(ec.colptr), P(ec.csc_eid), P(ec.csc_dst),
                                    AC.SLOPE, P(score), P(g2v), g2v.stride(0), P(gpre), P(g_a), P(g_b), P(gxv), gxv.stride(0), st), "asap_attend_bwd")
    torch.cuda.synchronize()
    score_in = torch.empty(E, device=DEV)
    score_in[ec.perm] = score[:E]
    res = {"mx": mxv, "out": outv, "score": score_in, "gx_max": gmv, "g_x": gxv, "g_a": g_a.view(a.shape), "g_b": g_b.view(b.shape)}
    return res, arg, (xbuf, g1buf, g2buf, mxbuf, outbuf, gmbuf, gxbuf)


# ------------------------------------------------------------------------------------------------ comparing
def _errors(res, ref, i, j, named, figures=("out", "score", "g_x", "g_a", "g_b"), cancelling=False):
    """figure -> error relative to its scale: every tensor against its largest float64 entry, and the ``named`` rows one by one.
    ``cancelling``: every pre-activation is positive (the grid regimes), so each g_a[w] is a sum of centred terms that cancel exactly and the
    float64 g_a is 0 up to its own rounding; g_a as a whole is then measured against the largest term, as its rows are."""
    cpu = lambda t: t.detach().double().cpu()
    err = {k: AC.rel_err(res[k], ref[k]) for k in figures}
    gpre = ref["gterm"]
    if cancelling and "g_a" in figures:
        assert float(ref["g_a"].abs().max()) < 1e-12 * float(gpre.max())
        err["g_a"] = float((cpu(res["g_a"]) - ref["g_a"]).abs().max()) / float(gpre.max())
    for w in named:
        seg, gat = i == w, j == w
        for k in ("out", "g_x"):
            err[f"{k}[{w}]"] = AC.rel_err(res[k][w], ref[k][w]) if bool(ref[k][w].any()) else float(cpu(res[k][w]).abs().max())
        if bool(seg.any()) and "score" in figures:
            err[f"score[{w}]"] = AC.rel_err(res["score"][seg.to(res["score"].device)], ref["score"][seg])
        if bool(seg.any()) and "g_a" in figures:
            err[f"g_a[{w}]"] = abs(float(cpu(res["g_a"]).view(-1)[w] - ref["g_a"].view(-1)[w])) / max(float(gpre[seg].max()), 1e-30)
        if bool(gat.any()) and "g_b" in figures:
            err[f"g_b[{w}]"] = abs(float(cpu(res["g_b"]).view(-1)[w] - ref["g_b"].view(-1)[w])) / max(float(gpre[gat].max()), 1e-30)
    return err


class _Checks:
    """Every figure is printed and recorded before the first failure is raised."""

    def __init__(self, case):
        self.case, self.failed = case, []

    def ratio(self, figure, err, bound, note=""):
        r = err / bound
        print(f"{self.case} {figure}: error / bound {r:.3e} (bound {bound:.2e}{note})")
        kind = figure.split("[")[0] + (" (row)" if "[" in figure else "")
        if r > RATIOS.get(kind, (-1.0, None))[0]:
            RATIOS[kind] = (r, f"{self.case} {figure}")
        if not r <= 1.0:
            self.failed.append(f"{figure}: error {err:.3e} > {bound:.2e}{note}")

    def against(self, res, ref, i, j, named, yardstick=None, figures=("out", "score", "g_x", "g_a", "g_b"), cancelling=False):
        """``yardstick``: callable giving the fp32 eager composition's results on this case (the 4x rule), evaluated only when DERIVED asks."""
        got = _errors(res, ref, i, j, named, figures, cancelling)
        derived = [f for c, f in DERIVED if self.case.startswith(c)]
        yard = _errors(yardstick(), ref, i, j, named, figures, cancelling) if derived and yardstick is not None else {}
        for figure, e in got.items():
            base = BASE[figure.split("[")[0]]
            if figure in derived and figure in yard:
                self.ratio(figure, e, min(CAP, 4 * yard[figure]), " = 4 x fp32 eager")
            else:
                self.ratio(figure, e, base)

    def close(self, got, want, figure, bound):
        self.ratio(figure, AC.rel_err(got, want), bound)

    def done(self):
        assert not self.failed, f"{self.case}: " + "; ".join(self.failed)


def _finite(res):
    for k, t in res.items():
        assert torch.isfinite(t).all(), k


def _exact_zeros(res, n, i, j):
    seg, gathered = AC.degrees(n, i, j)
    no_seg, never = (seg == 0).to(DEV), (gathered == 0).to(DEV)
    assert set(AC.NO_SEGMENT) <= set(torch.nonzero(seg == 0).view(-1).tolist())
    assert set(AC.NEVER_GATHERED) <= set(torch.nonzero(gathered == 0).view(-1).tolist())
    for k in ("mx", "out", "g_a"):
        assert not res[k][no_seg].any(), f"{k}: a row without a segment is not exactly 0"
    for k in ("gx_max", "g_x", "g_b"):
        assert not res[k][never].any(), f"{k}: a row that is never gathered is not exactly 0"


# ------------------------------------------------------------------------------------------------ a, b: width sweep, arg
@pytest.mark.parametrize("D", WIDTHS)
def test_width_sweep_against_float64(graph, D):
    n, i, j, ec = graph
    x, g_max, g_out = AC.features(n, D)
    a, b = AC.scores("normal", n)
    ref = AC.edge_reference(i, j, x, a, b, g_out)
    res = _run_ops(ec, x, a, b, g_max, g_out)
    raw, arg, _ = _run_raw(ec, x, a, b, g_max, g_out)
    _finite(res)
    for k in res:
        assert torch.equal(res[k], raw[k]), f"{k}: ops and the C ABI disagree"
    assert torch.equal(res["mx"].cpu().double(), ref["mx"])                                  # a maximum is one of its inputs: bit-equal
    _exact_zeros(res, n, i, j)
    # b. arg == the first maximum in CSR order, ties included; -1 without a segment; the backward routes by it
    want_arg, src = AC.first_max_arg(n, i, j, x)
    assert torch.equal(arg.cpu().long(), want_arg)
    assert bool((want_arg[list(AC.NO_SEGMENT)] == -1).all())
    routed = AC.max_backward_from_arg(want_arg, src, g_max, n)
    c = _Checks(f"normal D={D}")
    c.against(res, ref, i, j, AC.NAMED_ROWS, lambda: AC.edge_reference(i, j, x, a, b, g_out, dtype=torch.float32))
    c.close(res["gx_max"], routed, "gx_max", GRAD)
    for w in AC.NAMED_ROWS:
        if bool(routed[w].any()):
            c.close(res["gx_max"][w], routed[w], f"gx_max[{w}]", GRAD)
    c.done()


# ------------------------------------------------------------------------------------------------ c: score regimes
@pytest.fixture(scope="module")
def regime_runs(graph):
    n, i, j, ec = graph
    cache = {}

    def get(regime, D):
        if (regime, D) not in cache:
            x, g_max, g_out = AC.features(n, D)
            a, b = AC.scores(regime, n)
            cache[regime, D] = (_run_ops(ec, x, a, b, g_max, g_out), AC.edge_reference(i, j, x, a, b, g_out), (x, a, b, g_out))
        return cache[regime, D]
    return get


@pytest.mark.parametrize("D", REGIME_DS)
@pytest.mark.parametrize("regime", ["peaked", "grid", "grid+4096"])
def test_score_regimes_against_float64(graph, regime_runs, regime, D):
    n, i, j, ec = graph
    res, ref, (x, a, b, g_out) = regime_runs(regime, D)
    _finite(res)
    _exact_zeros(res, n, i, j)
    assert torch.equal(res["mx"].cpu().double(), ref["mx"])
    c = _Checks(f"{regime} D={D}")
    c.against(res, ref, i, j, AC.NAMED_ROWS, lambda: AC.edge_reference(i, j, x, a, b, g_out, dtype=torch.float32), cancelling=regime.startswith("grid"))
    c.done()


@pytest.mark.parametrize("D", REGIME_DS)
def test_a_common_offset_of_the_scores_changes_nothing(regime_runs, D):
    """a + 4096 on the exact grid: every sum and every difference from the segment's maximum is the same fp32 number as without the offset, so the
    forward and gradient bounds apply between the two GPU runs as they are (a softmax without the max subtraction gives inf / inf here)."""
    (shifted, ref, _), plain = regime_runs("grid+4096", D), regime_runs("grid", D)[0]
    c = _Checks(f"grid+4096 vs grid D={D}")
    for k in ("out", "score", "g_x", "g_b"):
        c.close(shifted[k], plain[k], k, BASE[k])
    # g_a cancels to 0 on the grid (see _errors): the two runs' g_a against the largest term under its sums
    c.ratio("g_a", float((shifted["g_a"] - plain["g_a"]).abs().max()) / float(ref["gterm"].max()), GRAD)
    c.done()
    assert torch.equal(shifted["mx"], plain["mx"]) and torch.equal(shifted["gx_max"], plain["gx_max"])


# ------------------------------------------------------------------------------------------------ d: padded row strides
@pytest.mark.parametrize("D", REGIME_DS)
def test_raw_abi_row_strides_leave_the_padding_alone(graph, D):
    n, i, j, ec = graph
    x, g_max, g_out = AC.features(n, D, seed=3)
    a, b = AC.scores("normal", n, seed=3)
    dense, arg_d, _ = _run_raw(ec, x, a, b, g_max, g_out)
    padded, arg_p, bufs = _run_raw(ec, x, a, b, g_max, g_out, PADS)
    strides = [padded[k].stride(0) for k in ("mx", "out", "gx_max", "g_x")]
    assert strides == [D + 2, D + 2, D + 5, D + 5]
    assert torch.equal(arg_d, arg_p)
    for k in dense:
        assert torch.equal(dense[k], padded[k]), k
    for buf in bufs:
        assert buf.shape[1] > D and bool((buf[:, D:] == SENTINEL).all())
    ref = AC.edge_reference(i, j, x, a, b, g_out)
    assert AC.rel_err(padded["out"], ref["out"]) < FWD and AC.rel_err(padded["g_x"], ref["g_x"]) < GRAD


# ------------------------------------------------------------------------------------------------ e: width 1025
def test_width_1025_is_refused_by_every_entry_point():
    from wsi_hgnn_amd import _native as N, ops
    lib = N.load()
    n, i, j = AC.small_graphs()["ring5"]
    ec = ops.EdgeCSR(i.to(DEV), j.to(DEV), n)
    D = 1025
    x = torch.randn(n, D, device=DEV)
    a, b = torch.randn(n, device=DEV), torch.randn(n, device=DEV)
    mk = lambda *shape: torch.full(shape, SENTINEL, device=DEV)
    out, gx, score, gpre, g_a, g_b = mk(n, D), mk(n, D), mk(n), mk(n), mk(n), mk(n)
    arg = torch.full((n, D), -7, dtype=torch.int32, device=DEV)
    P, st = N.ptr, N.stream()
    calls = {
        "gather_max_fwd": lambda: lib.wsi_csr_gather_max_fwd(P(x), D, n, D, P(ec.rowptr), P(ec.src), P(out), D, P(arg), st),
        "gather_max_bwd": lambda: lib.wsi_csr_gather_max_bwd(P(x), D, P(arg), n, D, P(ec.colptr), P(ec.csc_eid), P(ec.csc_dst), P(gx), D, st),
        "attend_fwd": lambda: lib.wsi_asap_attend_fwd(P(a), P(b), P(x), D, n, D, P(ec.rowptr), P(ec.src), AC.SLOPE, P(score), P(out), D, st),
        "attend_bwd": lambda: lib.wsi_asap_attend_bwd(P(a), P(b), P(x), D, n, D, P(ec.rowptr), P(ec.src), P(ec.colptr), P(ec.csc_eid), P(ec.csc_dst),
                                                      AC.SLOPE, P(a), P(x), D, P(gpre), P(g_a), P(g_b), P(gx), D, st),
    }
    for name, call in calls.items():
        assert call() == N.WSI_ENOSYS, name
        msg = lib.wsi_last_error().decode()
        assert "unsupported" in msg and "1025" in msg, (name, msg)
    torch.cuda.synchronize()
    for t in (out, gx, score, gpre, g_a, g_b):
        assert bool((t == SENTINEL).all())
    assert bool((arg == -7).all())
    with pytest.raises(RuntimeError, match="feature width 1025 > 1024 unsupported"):
        ops.csr_gather_max(x, ec)


# ------------------------------------------------------------------------------------------------ f: small graphs, determinism
@pytest.mark.parametrize("name", ["one_node", "ring5", "no_edges"])
@pytest.mark.parametrize("D", [3, 65])
def test_small_graphs(name, D):
    from wsi_hgnn_amd import ops
    n, i, j = AC.small_graphs()[name]
    ec = ops.EdgeCSR(i.to(DEV), j.to(DEV), n)
    x, g_max, g_out = AC.features(n, D)
    a, b = AC.scores("normal", n)
    ref = AC.edge_reference(i, j, x, a, b, g_out)
    res = _run_ops(ec, x, a, b, g_max, g_out)
    _finite(res)
    assert res["score"].numel() == i.numel()
    assert torch.equal(res["mx"].cpu().double(), ref["mx"])
    want_arg, src = AC.first_max_arg(n, i, j, x)
    c = _Checks(f"{name} D={D}")
    single = name in ("one_node", "ring5")       # one edge per segment: g_a and g_b are exactly 0, float64's are artefacts of the 1e-16 in the denominator
    c.against(res, ref, i, j, range(n), figures=("out", "score", "g_x") if single else ("out", "score", "g_x", "g_a", "g_b"))
    if single:
        assert not res["g_a"].any() and not res["g_b"].any() and float(ref["g_a"].abs().max()) < 1e-12 and float(ref["g_b"].abs().max()) < 1e-12
    c.close(res["gx_max"], AC.max_backward_from_arg(want_arg, src, g_max, n), "gx_max", GRAD)
    c.done()
    if name == "no_edges":
        for k, t in res.items():
            assert not t.any(), k
    if name == "one_node":                   # a softmax over one edge is 1 (up to the 1e-16 of the denominator): out == x, no score gradient
        assert torch.equal(res["out"].cpu(), x) and float(res["score"][0]) == 1.0
        assert not res["g_a"].any() and not res["g_b"].any() and torch.equal(res["g_x"].cpu(), g_out) and torch.equal(res["gx_max"].cpu(), g_max)


def test_identical_calls_give_identical_bits(graph):
    n, i, j, ec = graph
    x, g_max, g_out = AC.features(n, 200, seed=5)
    a, b = AC.scores("peaked", n, seed=5)
    first, second = _run_ops(ec, x, a, b, g_max, g_out), _run_ops(ec, x, a, b, g_max, g_out)      # atomic-free kernels: one repeat, no loop
    for k in first:
        assert torch.equal(first[k], second[k]), k


# ------------------------------------------------------------------------------------------------ g: top-k
def _topk_check(score, batch, B, ratios, case):
    from wsi_hgnn_amd.pooling import ASAP as PA
    n = score.numel()
    sd, bd = score.to(DEV), batch.to(DEV)
    counts = torch.bincount(batch, minlength=B).tolist()
    for ratio in ratios:
        want = PA.topk(score, ratio, batch)                              # CPU: the sort formulation
        got = PA.topk(sd, ratio, bd).cpu()
        assert torch.equal(got, want), (case, ratio)
        assert got.unique().numel() == got.numel() and (got.numel() == 0 or (int(got.min()) >= 0 and int(got.max()) < n)), (case, ratio)
        assert torch.equal(PA.topk(sd, ratio, bd, num_per_graph=counts).cpu(), want), (case, ratio)
        k = torch.ceil(ratio * torch.tensor(counts).float()).long()
        assert want.numel() == int(k.sum()) and torch.equal(torch.bincount(batch[want], minlength=B), k)


@pytest.mark.parametrize("n,B,arrangement", AC.TOPK_CASES)
def test_graph_topk_matches_the_sort_formulation_across_chunks(n, B, arrangement):
    score, batch = AC.topk_case(n, B, arrangement)
    _topk_check(score, batch, B, AC.TOPK_RATIOS, (n, B, arrangement))


def test_graph_topk_total_order_across_chunks():
    score, batch = AC.topk_special_case()
    _topk_check(score, batch, 4, AC.TOPK_RATIOS, "nan/inf/zeros")


# ------------------------------------------------------------------------------------------------ h: S^T A S
def _stas_native(N_, ei, score, w, perm):
    from wsi_hgnn_amd import ops
    from wsi_hgnn_amd.pooling import ASAP as PA
    ec = ops.EdgeCSR(ei[0].to(DEV), ei[1].to(DEV), N_)
    if w is not None:
        ec = ec.with_weights(w.to(DEV))
    run = lambda: PA.graph_connectivity_native(ec, score.to(DEV), perm.to(DEV), N_)
    return run(), run


def _stas_check(case, N_, ei, score, w, perm):
    want_i, want_v, rows = AC.stas_reference(N_, ei, score, w, perm)
    got, run = _stas_native(N_, ei, score, w, perm)
    assert got is not None, f"{case}: the native path declined"
    assert torch.equal(got[0].cpu(), want_i), f"{case}: index list"
    bound = 1e-6 * max(1.0, float(want_v.abs().max()))
    err = float((got[1].cpu().double() - want_v).abs().max())
    print(f"{case} value_E: error / bound {err / bound:.3e} (bound {bound:.2e}, rows hold {int(rows.min())}..{int(rows.max())} columns)")
    if err / bound > RATIOS.get("value_E", (-1.0, None))[0]:
        RATIOS["value_E"] = (err / bound, case)
    assert err <= bound, f"{case}: value_E error {err:.3e} > {bound:.2e}"
    again = run()
    assert torch.equal(again[0], got[0]) and torch.equal(again[1], got[1]), f"{case}: a second call gives other bits"
    return rows


@pytest.mark.parametrize("m", [384, 385, 1536])
def test_stas_stars_at_the_table_boundaries(m):
    rows = _stas_check(f"star m={m}", *AC.star(m))
    assert bool((rows == m).all())


def test_stas_star_beyond_the_large_table_is_reported():
    N_, ei, score, w, perm = AC.star(1537)
    got, _ = _stas_native(N_, ei, score, w, perm)
    assert got is None


@pytest.mark.parametrize("m", [384, 385])
def test_stas_weighted_stars(m):
    _stas_check(f"weighted star m={m}", *AC.star(m, weighted=True))


@pytest.mark.parametrize("weighted", [False, True])
def test_stas_rows_split_between_the_two_launches(weighted):
    N_, ei, score, w, perm, _ = AC.combined(weighted)
    rows = _stas_check(f"combined weighted={weighted}", N_, ei, score, w, perm)
    assert int((rows > AC.ST_SMALL_ROWS).sum()) == 386 and int(((rows > 0) & (rows <= AC.ST_SMALL_ROWS)).sum()) > 385
