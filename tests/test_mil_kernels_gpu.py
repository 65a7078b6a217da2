"""The bag softmax pooling kernels (wsi_bag_softmax_pool_fwd / _bwd) and the DSMIL score step (wsi_bag_scores_fwd / _bwd) on the GPU
against float64 on the SAME fp32 inputs, through ``ops`` and through the raw ABI.  Tolerance (tests/test_gat_gpu.py's norm): error <=
1e-4 x the largest float64 entry of each tensor (out, lse, g_scores, g_values).

One plan: bags of 1, 127, 128, 129, 0, 293, 0, 1061 and 2 rows with the default chunk of 128 rows - a single row, the chunk boundary
from both sides, two empty bags (one between non-empty ones), multi-chunk combines (3 and 9 chunks) and a short last bag."""
import numpy as np
import pytest
import torch

import mil_cases as MC

pytestmark = pytest.mark.gpu

DEV = "cuda"
TOL = 1e-4
SIZES = MC.KERNEL_SIZES
OFF = MC.offsets(SIZES)
NROWS = OFF[-1]
S = len(SIZES)
BIG = SIZES.index(1061)
R = MC.Ratios(TOL)


@pytest.fixture(scope="module", autouse=True)
def _report_ratios():
    yield
    R.report()


@pytest.fixture(scope="module")
def rp():
    from wsi_hgnn_amd import mil
    return mil.bag_plan(SIZES, DEV)


def _inputs(C, D, seed=0):
    g = torch.Generator().manual_seed(1000 * C + D + seed)
    return (torch.randn(NROWS, C, generator=g), torch.randn(NROWS, D, generator=g), torch.randn(S, C, D, generator=g))


def _reference(scores, values, g_out, scale):
    s64 = scores.double().requires_grad_(True)
    v64 = values.double().requires_grad_(True)
    out, lse, p = MC.softmax_pool(s64, v64, SIZES, scale)
    (out * g_out.double()).sum().backward()
    return out.detach(), lse.detach(), s64.grad, v64.grad, p.detach()


def _through_ops(rp, scores, values, g_out, scale):
    from wsi_hgnn_amd import ops
    s = scores.to(DEV).requires_grad_(True)
    v = values.to(DEV).requires_grad_(True)
    out, lse, stats = ops.bag_softmax_pool_lse(s, v, rp, scale)
    assert torch.equal(stats.sum(-1), lse) and not lse.requires_grad and not stats.requires_grad
    out.backward(g_out.to(DEV))
    return out.detach(), lse, s.grad, v.grad


def _check_all(got, ref, case):
    for name, g, r in zip(("out", "lse", "g_scores", "g_values"), got, ref):
        R.check(g, r, name, case)
    # a softmax ignores a shift of its scores: the score gradients of a (bag, column) sum to 0
    gs = got[2].double().cpu()
    sums = torch.stack([gs[a:b].sum(0) for a, b in zip(OFF[:-1], OFF[1:])])
    assert float(sums.abs().max()) <= TOL * float(ref[2].abs().max()), f"{case}: score gradients sum to {float(sums.abs().max()):.3e}"
    for s_, n in enumerate(SIZES):
        if n == 0:
            assert not got[0][s_].any() and not got[1][s_].any(), f"{case}: empty bag {s_}"


@pytest.mark.parametrize("D", MC.KERNEL_DS)
@pytest.mark.parametrize("C", MC.KERNEL_CS)
def test_sweep_against_float64(rp, C, D):
    scores, values, g_out = _inputs(C, D)
    got = _through_ops(rp, scores, values, g_out, 1.0)
    _check_all(got, _reference(scores, values, g_out, 1.0), f"C={C} D={D}")


def _patterns():
    base, values, g_out = _inputs(3, 128, seed=7)
    # multiples of 2^-8 within +-4: adding -1e4 is then exact in float32, so the shifted case has the very same softmax
    quant = (base.clamp(-4, 4) * 256).round() / 256
    last = base.clone(); last[OFF[BIG + 1] - 5, :] = 60.0           # in the last of the 1061-row bag's 9 chunks
    first = base.clone(); first[OFF[BIG] + 3, :] = 60.0             # in its first chunk
    return {"normal": (base, 1.0), "equal": (torch.full_like(base, 0.75), 1.0), "quantised": (quant, 1.0), "shifted": (quant - 1.0e4, 1.0),
            "peak_last_chunk": (last, 1.0), "peak_first_chunk": (first, 1.0), "scaled": (base, MC.SCALE_128)}, values, g_out


@pytest.fixture(scope="module")
def pattern_runs(rp):
    pats, values, g_out = _patterns()
    return {k: (_through_ops(rp, sc, values, g_out, scale), _reference(sc, values, g_out, scale)) for k, (sc, scale) in pats.items()}


@pytest.mark.parametrize("name", ["normal", "equal", "quantised", "shifted", "peak_last_chunk", "peak_first_chunk", "scaled"])
def test_score_patterns(pattern_runs, name):
    got, ref = pattern_runs[name]
    _check_all(got, ref, name)
    if name == "equal":            # uniform weights: every bag's out is the mean of its rows
        _, values, _ = _patterns()
        for s_, (a, b) in enumerate(zip(OFF[:-1], OFF[1:])):
            if b > a:
                R.check(got[0][s_, 1], values[a:b].double().mean(0), "out", "equal/mean")


def test_a_shift_of_the_scores_changes_nothing(pattern_runs):
    (out_s, lse_s, gs_s, gv_s), _ = pattern_runs["shifted"]
    (out_q, lse_q, gs_q, gv_q), _ = pattern_runs["quantised"]
    for t in (out_s, lse_s, gs_s, gv_s):
        assert torch.isfinite(t).all()
    R.check(out_s, out_q, "out", "shifted vs unshifted")
    R.check(gs_s, gs_q, "g_scores", "shifted vs unshifted")
    R.check(gv_s, gv_q, "g_values", "shifted vs unshifted")
    live = torch.tensor([n > 0 for n in SIZES], device=DEV).view(-1, 1)
    R.check(torch.where(live, lse_s.double() + 1.0e4, lse_s.double()), lse_q, "lse", "shifted vs unshifted")


def test_identical_calls_give_identical_bits(rp):
    scores, values, g_out = _inputs(3, 128, seed=11)
    scores[OFF[BIG] + 3] = 9.0
    a = _through_ops(rp, scores, values, g_out, MC.SCALE_128)
    b = _through_ops(rp, scores, values, g_out, MC.SCALE_128)
    for name, x, y in zip(("out", "lse", "g_scores", "g_values"), a, b):
        assert torch.equal(x, y), name


def test_a_bag_without_gradient_gets_exact_zeros(rp):
    scores, values, g_out = _inputs(3, 128, seed=13)
    g_out[BIG] = 0.0
    g_out[1] = 0.0
    got = _through_ops(rp, scores, values, g_out, 1.0)
    _check_all(got, _reference(scores, values, g_out, 1.0), "zeroed g_out")
    for s_ in (BIG, 1):
        assert not got[2][OFF[s_]:OFF[s_ + 1]].any() and not got[3][OFF[s_]:OFF[s_ + 1]].any()
    assert got[2][OFF[2]:OFF[3]].any() and got[3][OFF[2]:OFF[3]].any()


def test_bag_attention_returns_the_normalised_weights(rp):
    from wsi_hgnn_amd import ops
    scores, values, g_out = _inputs(3, 128, seed=17)
    out, lse, stats = ops.bag_softmax_pool_lse(scores.to(DEV).requires_grad_(True), values.to(DEV), rp, MC.SCALE_128)
    ref = _reference(scores, values, g_out, MC.SCALE_128)[4]
    for form, t in (("lse", lse), ("stats", stats)):
        A = ops.bag_attention(scores.to(DEV).requires_grad_(True), t, rp, MC.SCALE_128)
        assert not A.requires_grad
        R.check(A, ref, "A", "bag_attention from " + form)


def test_ops_take_non_contiguous_inputs_and_honour_needs_input_grad(rp):
    from wsi_hgnn_amd import ops
    scores, values, g_out = _inputs(2, 50, seed=19)
    ref = _reference(scores, values, g_out, 1.0)
    wide_s = torch.zeros(NROWS, 5, device=DEV); wide_s[:, 1:3] = scores.to(DEV)
    wide_v = torch.zeros(NROWS, 77, device=DEV); wide_v[:, 20:70] = values.to(DEV)
    wide_s.requires_grad_(True)
    out = ops.bag_softmax_pool(wide_s[:, 1:3], wide_v[:, 20:70], rp)             # values need no gradient: only g_scores is computed
    out.backward(g_out.to(DEV))
    R.check(out, ref[0], "out", "views")
    R.check(wide_s.grad[:, 1:3], ref[2], "g_scores", "views")
    assert not wide_s.grad[:, 0].any() and not wide_s.grad[:, 3:].any()
    v = values.to(DEV).requires_grad_(True)
    ops.bag_softmax_pool(scores.to(DEV), v, rp).backward(g_out.to(DEV))           # and the other way round
    R.check(v.grad, ref[3], "g_values", "values only")
    with pytest.raises(ValueError):
        ops.bag_softmax_pool(scores.to(DEV)[:-1], values.to(DEV)[:-1], rp)
    with pytest.raises(RuntimeError, match="at most 8"):
        ops.bag_softmax_pool(torch.zeros(NROWS, 9, device=DEV), values.to(DEV), rp)


# ------------------------------------------------------------------------------------------------ raw ABI
SENTINEL = 777.0


def _padded(t, pad_cols):
    """A view of ``t``'s values whose row stride is its width + pad_cols; the padding holds SENTINEL."""
    buf = torch.full((t.shape[0], t.shape[1] + pad_cols), SENTINEL, device=DEV)
    buf[:, :t.shape[1]] = t.to(DEV)
    return buf, buf[:, :t.shape[1]]


def _shifted(t):
    """A contiguous copy of ``t`` that starts 4 bytes into its buffer: never 16-byte aligned."""
    buf = torch.full((t.numel() + 1,), SENTINEL, device=DEV)
    view = buf[1:].view(t.shape)
    view.copy_(t.to(DEV))
    assert view.data_ptr() % 16 == 4
    return buf, view


def _raw(rp, scores, values, g_out, scale, g_scores, g_values):
    """Forward and backward through the C ABI on (possibly strided / offset) 2-D views; gradients are written into the given views (or None)."""
    from wsi_hgnn_amd import _native as N
    lib = N.load()
    C, D = scores.shape[1], values.shape[1]
    out = torch.empty(S, C, D, device=DEV)
    lse = torch.empty(S, C, device=DEV)
    stats = torch.empty(S, C, 2, device=DEV)
    partial = torch.empty(rp.num_chunks * C * (D + 2), device=DEV)
    delta = torch.empty(S * C, device=DEV)
    N.check(lib.wsi_bag_softmax_pool_fwd(N.ptr(scores), scores.stride(0), C, scale, N.ptr(values), values.stride(0), D, N.ptr(rp.chunk_row),
                                         rp.num_chunks, N.ptr(rp.seg_chunk), rp.num_segs, N.ptr(partial), N.ptr(out), N.ptr(lse), N.ptr(stats), N.stream()), "fwd")
    N.check(lib.wsi_bag_softmax_pool_bwd(N.ptr(g_out), N.ptr(out), N.ptr(scores), scores.stride(0), C, scale, N.ptr(stats), N.ptr(values),
                                         values.stride(0), D, N.ptr(rp.chunk_row), N.ptr(rp.chunk_seg), rp.num_chunks, rp.num_segs,
                                         N.ptr(delta), N.ptr(g_scores), g_scores.stride(0) if g_scores is not None else 0,
                                         N.ptr(g_values), g_values.stride(0) if g_values is not None else 0, N.stream()), "bwd")
    torch.cuda.synchronize()
    return out, lse


@pytest.mark.parametrize("C,D", [(3, 128), (2, 50), (8, 4)])
def test_raw_abi_row_strides_leave_the_padding_alone(rp, C, D):
    scores, values, g_out = _inputs(C, D, seed=23)
    ref = _reference(scores, values, g_out, 1.0)
    sbuf, sv = _padded(scores, 1)
    vbuf, vv = _padded(values, 1)
    gsbuf, gsv = _padded(torch.zeros_like(scores), 1)
    gvbuf, gvv = _padded(torch.zeros_like(values), 1)
    out, lse = _raw(rp, sv, vv, g_out.to(DEV).contiguous(), 1.0, gsv, gvv)
    _check_all((out, lse, gsv, gvv), ref, f"strided C={C} D={D}")
    for buf in (sbuf, vbuf, gsbuf, gvbuf):
        assert (buf[:, -1] == SENTINEL).all()


def test_raw_abi_unaligned_tensors_take_the_scalar_path(rp):
    scores, values, g_out = _inputs(3, 128, seed=29)
    ref = _reference(scores, values, g_out, 1.0)
    _, vv = _shifted(values)
    _, go = _shifted(g_out)
    gvbuf, gvv = _shifted(torch.zeros_like(values))
    gs = torch.zeros(NROWS, 3, device=DEV)
    out, lse = _raw(rp, scores.to(DEV), vv, go, 1.0, gs, gvv)
    _check_all((out, lse, gs, gvv), ref, "unaligned D=128")
    assert float(gvbuf[0]) == SENTINEL


def test_raw_abi_null_gradient_pointers(rp):
    scores, values, g_out = _inputs(3, 128, seed=31)
    ref = _reference(scores, values, g_out, 1.0)
    s, v, go = scores.to(DEV), values.to(DEV), g_out.to(DEV)
    gs = torch.full((NROWS, 3), SENTINEL, device=DEV)
    gv = torch.full((NROWS, 128), SENTINEL, device=DEV)
    _raw(rp, s, v, go, 1.0, gs, None)
    R.check(gs, ref[2], "g_scores", "g_values = NULL")
    _raw(rp, s, v, go, 1.0, None, gv)
    R.check(gv, ref[3], "g_values", "g_scores = NULL")
    gs2, gv2 = torch.empty_like(gs), torch.empty_like(gv)
    _raw(rp, s, v, go, 1.0, gs2, gv2)
    assert torch.equal(gs, gs2) and torch.equal(gv, gv2)        # either alone computes what both together compute
    _raw(rp, s, v, go, 1.0, None, None)


# ------------------------------------------------------------------------------------------------ DSMIL score step
@pytest.mark.parametrize("C,D", [(1, 128), (3, 128), (8, 128), (3, 50), (2, 3)])
def test_dsmil_score_step_against_float64(rp, C, D):
    from wsi_hgnn_amd import ops
    g = torch.Generator().manual_seed(41 * C + D)
    q = torch.randn(NROWS, D, generator=g)
    g_sc = torch.randn(NROWS, C, generator=g)
    idx = [[OFF[s_] + int(torch.randint(0, n, (1,), generator=g)) if n else -1 for _ in range(C)] for s_, n in enumerate(SIZES)]
    if C > 1:
        idx[BIG][1] = idx[BIG][0]                                # one row critical for two classes
    onehot = torch.zeros(NROWS, C)
    for s_ in range(S):
        for c in range(C):
            if idx[s_][c] >= 0:
                onehot[idx[s_][c], c] = 1.0
    q64 = q.double().requires_grad_(True)
    ref = torch.cat([q64[a:b] @ q64[torch.tensor(idx[s_])].t() for s_, (a, b) in enumerate(zip(OFF[:-1], OFF[1:])) if b > a], 0)
    (ref * g_sc.double()).sum().backward()
    runs = []
    for _ in range(2):
        qd = q.to(DEV).requires_grad_(True)
        sc = ops.bag_scores(qd, onehot.to(DEV), rp)
        sc.backward(g_sc.to(DEV))
        runs.append((sc.detach(), qd.grad))
    R.check(runs[0][0], ref, "scores", f"score step C={C} D={D}")
    R.check(runs[0][1], q64.grad, "g_q", f"score step C={C} D={D}")
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
