"""The relevance-propagation kernels (wsi_lrp_linear / _residual / _attention) on the GPU against the float64 restatement
(tests/graphcam_cases.py) on the SAME fp32 inputs.  Tolerance (tests/test_gtn_kernels_gpu.py's norm): error <= 1e-4 x the largest float64 entry of
each tensor, on sign-coherent inputs - q, k, v in [0.1, 1.1], B = sign(A) |.|, relevances >= 0, so that no denominator cancels - with planted
exact zeros (a zero v row, A = -B elements, a zero X row, an all-negative W column and row), whose outputs must be exact zeros.

One signed (cancelling) case per entry point runs under the measured yardstick e_gpu <= max(1e-4, 4 e32'), e32' the float32 CPU run of the
restatement on the same inputs (seeds fixed so that e32' <= 1e-2: tests/test_gtn_graphcam.py).

G = 3, C in {1, 3}, H in {1, 8}, d in {8, 16}, n in {1, 2, 63, 64, 65, 101, 128}; the widths of graphcam_cases.LINEAR_WIDTHS."""
import pytest
import torch

import graphcam_cases as Q
from mil_cases import Ratios, rel_err

pytestmark = pytest.mark.gpu

DEV = "cuda"
TOL = 1e-4
G = 3
R = Ratios(TOL)
ENOSYS = -38


@pytest.fixture(scope="module", autouse=True)
def _report_ratios():
    yield
    R.report()


def dev(*ts):
    return [None if t is None else t.to(DEV) for t in ts]


def f64(*ts):
    return [None if t is None else t.double() for t in ts]


# ------------------------------------------------------------------------------------------------ linear
@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("widths", Q.LINEAR_WIDTHS, ids=lambda w: f"{w[0]}x{w[1]}")
def test_linear(widths, C):
    from wsi_hgnn_amd import ops
    fin, fout = widths
    assert ops.lrp_linear_supported(fin, fout)
    n = Q.SEQ_LENGTHS[(Q.LINEAR_WIDTHS.index(widths) + C) % len(Q.SEQ_LENGTHS)]
    X, W, Rel = Q.linear_case(G, C, n, fin, fout, seed=10 * fin + fout + C)
    got = ops.lrp_linear(*dev(X, W, Rel))
    R.check(got, Q.lin(*f64(X, W, Rel)), "lrp_linear", f"{fin}->{fout} n={n} C={C}")
    assert torch.equal(got[G - 1, :, n // 2].cpu(), torch.zeros(C, fin))                       # the zero X row
    assert torch.equal(got, ops.lrp_linear(*dev(X, W, Rel)))


@pytest.mark.parametrize("n", Q.SEQ_LENGTHS)
def test_linear_every_length(n):
    from wsi_hgnn_amd import ops
    X, W, Rel = Q.linear_case(G, 3, n, 64, 192, seed=n)
    R.check(ops.lrp_linear(*dev(X, W, Rel)), Q.lin(*f64(X, W, Rel)), "lrp_linear", f"64->192 n={n}")


def test_linear_head_and_many_classes():
    """The head's use (n = 1, out = n_class) and more (token, class) pairs than one pass of the kernel takes."""
    from wsi_hgnn_amd import ops
    for C, fout in ((3, 3), (16, 16), (7, 5)):
        X, W, Rel = Q.linear_case(G, C, 1, 64, fout, seed=C)
        R.check(ops.lrp_linear(*dev(X, W, Rel)), Q.lin(*f64(X, W, Rel)), "lrp_linear", f"head C={C} out={fout}")


# ------------------------------------------------------------------------------------------------ clone + add
@pytest.mark.parametrize("single", [False, True], ids=["two", "single"])
@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("n", Q.SEQ_LENGTHS)
def test_residual(n, C, single):
    from wsi_hgnn_amd import ops
    X, r1, r2, A, B = Q.residual_case(G, C, n, 64, seed=n + C, single=single)
    a, b = ops.lrp_residual(*dev(X, r1, r2, A, B))
    ra, rb = Q.residual(*f64(X, r1, r2, A, B))
    case = f"n={n} C={C} {'single' if single else 'two'}"
    R.check(a, ra, "lrp_residual a", case)
    R.check(b, rb, "lrp_residual b", case)
    planted = ((A + B) == 0).unsqueeze(1).expand(G, C, n, 64)
    assert planted.any() and float(a.cpu()[planted].abs().max()) == 0 and float(b.cpu()[planted].abs().max()) == 0
    a2, b2 = ops.lrp_residual(*dev(X, r1, r2, A, B))
    assert torch.equal(a, a2) and torch.equal(b, b2)


@pytest.mark.parametrize("E", [4, 32, 256])
def test_residual_widths(E):
    from wsi_hgnn_amd import ops
    X, r1, r2, A, B = Q.residual_case(G, 3, 101, E, seed=E)
    a, b = ops.lrp_residual(*dev(X, r1, r2, A, B))
    ra, rb = Q.residual(*f64(X, r1, r2, A, B))
    R.check(a, ra, "lrp_residual a", f"E={E}")
    R.check(b, rb, "lrp_residual b", f"E={E}")


# ------------------------------------------------------------------------------------------------ attention
def _attention(qkv, Rel, g_out, H):
    from wsi_hgnn_amd import ops
    qd, Rd, gd = dev(qkv, Rel, g_out)
    _, lse = ops.seq_attention_lse(qd, H)
    return ops.lrp_attention(qd, lse, Rd, gd, H), lse


@pytest.mark.parametrize("rollout", [False, True], ids=["grad", "rollout"])
@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("d", [8, 16])
@pytest.mark.parametrize("H", [1, 8])
@pytest.mark.parametrize("n", Q.SEQ_LENGTHS)
def test_attention(n, H, d, C, rollout):
    qkv, Rel, g_out = Q.attention_case(G, C, n, H, d, seed=1000 * n + 10 * H + d + C, rollout=rollout)
    (cam, M), lse = _attention(qkv, Rel, g_out, H)
    ref_cam, ref_M, ref_lse = Q.attention_reference(*f64(qkv, Rel, g_out), H)
    case = f"n={n} H={H} d={d} C={C} {'rollout' if rollout else 'grad'}"
    R.check(lse, ref_lse, "lse", case)
    R.check(cam, ref_cam, "lrp_attention cam_qkv", case)
    R.check(M, ref_M, "lrp_attention layer map", case)
    assert cam.shape == (G, C, n, 3 * H * d) and M.shape == (G, C, n, n) and float(M.min()) >= 0
    assert float(cam[:, :, n // 2, 2 * H * d:].abs().max()) == 0                                # the zero v row: cam_v = v * (.) = 0
    (cam2, M2), _ = _attention(qkv, Rel, g_out, H)
    assert torch.equal(cam, cam2) and torch.equal(M, M2)


# ------------------------------------------------------------------------------------------------ signed inputs under the measured yardstick
@pytest.mark.parametrize("entry", ["lrp_linear", "lrp_residual", "lrp_attention"])
def test_signed_case(entry):
    from wsi_hgnn_amd import ops
    name, fn, inputs = [c for c in Q.signed_cases() if c[0] == entry][0]
    e32 = Q.rel_err_f32(fn, *inputs)
    bound = max(1e-4, 4 * e32)
    ref = fn(*f64(*inputs))
    if entry == "lrp_linear":
        got = (ops.lrp_linear(*dev(*inputs)),)
        ref = (ref,)
    elif entry == "lrp_residual":
        got = ops.lrp_residual(*dev(*inputs))
    else:
        got = _attention(*inputs, Q.SIGNED_HEADS)[0]
    errs = [rel_err(a, b) for a, b in zip(got, ref)]
    print(f"{entry} signed: e_gpu {max(errs):.3e}, e32' {e32:.3e}, bound {bound:.3e}, e_gpu / e32' {max(errs) / e32:.2f}")
    assert e32 <= 1e-2 and all(torch.isfinite(t).all() for t in got)
    assert max(errs) <= bound, errs


# ------------------------------------------------------------------------------------------------ what the kernels refuse
def test_unsupported_shapes_answer_enosys():
    from wsi_hgnn_amd import _native as N, ops
    lib = N.load()
    buf = torch.zeros(3 * 129 * 3 * 8 * 8 + 260 * 260, device=DEV)
    p = N.ptr(buf)
    for fin, fout in Q.LINEAR_REFUSED:
        assert not ops.lrp_linear_supported(fin, fout)
        assert lib.wsi_lrp_linear(p, p, p, 1, 1, 2, fin, fout, p, N.stream()) == ENOSYS
        with pytest.raises(RuntimeError):
            ops.lrp_linear(torch.zeros(1, 2, fin, device=DEV), torch.zeros(fout, fin, device=DEV), torch.zeros(1, 1, 2, fout, device=DEV))
    assert ops.lrp_linear_supported(32, 96) and ops.lrp_linear_supported(256, 256) and ops.lrp_linear_supported(64, 3)
    assert lib.wsi_lrp_attention(p, p, p, None, 3, 1, 129, 8, 8, 1.0, p, p, p, N.stream()) == ENOSYS            # n = 129
    assert lib.wsi_lrp_attention(p, p, p, None, 1, 1, 64, 2, 32, 1.0, p, p, p, N.stream()) == ENOSYS            # head width 32
    assert lib.wsi_lrp_attention(p, p, p, None, 1, 1, 64, 2, 12, 1.0, p, p, p, N.stream()) == ENOSYS
    assert lib.wsi_lrp_residual(p, p, p, p, p, 1, 1, 5, 6, p, p, N.stream()) == ENOSYS                           # width 6
    assert not ops.lrp_residual_supported(6) and ops.lrp_residual_supported(64)
    with pytest.raises(RuntimeError):
        ops.lrp_attention(torch.zeros(1, 129, 3 * 8, device=DEV), torch.zeros(1, 1, 129, device=DEV), torch.zeros(1, 1, 129, 8, device=DEV), None, 1)
    torch.cuda.synchronize()


def test_empty_calls_do_nothing():
    from wsi_hgnn_amd import _native as N
    lib = N.load()
    assert lib.wsi_lrp_linear(None, None, None, 0, 3, 5, 64, 64, None, N.stream()) == 0
    assert lib.wsi_lrp_residual(None, None, None, None, None, 3, 0, 5, 64, None, None, N.stream()) == 0
    assert lib.wsi_lrp_attention(None, None, None, None, 3, 3, 0, 8, 8, 1.0, None, None, None, N.stream()) == 0
