"""The mincut assignment kernels (wsi_mincut_fwd / _bwd) and the short-sequence attention (wsi_seq_attn_fwd / _bwd) on the GPU against float64
on the SAME fp32 inputs.  Tolerance (tests/test_mil_kernels_gpu.py's norm): error <= 1e-4 x the largest float64 entry of each tensor.

Mincut: graphs of 1, 127, 128, 129, 293 and 2 rows under the default chunk of 128 rows, K in {1, 2, 64, 100, 128} (one lane column, both,
a full first column, a partial and a full second one), the entry list of gtn_cases.kernel_edges.  Attention: B = 3, H in {1, 8},
d in {8, 16}, n in {1, 2, 63, 64, 65, 101, 128}."""
import pytest
import torch

import gtn_cases as C
from mil_cases import Ratios, rel_err

pytestmark = pytest.mark.gpu

DEV = "cuda"
TOL = 1e-4
SIZES = C.KERNEL_SIZES
NROWS = sum(SIZES)
G = len(SIZES)
R = Ratios(TOL)
ENOSYS = -38


@pytest.fixture(scope="module", autouse=True)
def _report_ratios():
    yield
    R.report()


@pytest.fixture(scope="module")
def edges():
    return C.kernel_edges()


@pytest.fixture(scope="module")
def rp():
    from wsi_hgnn_amd import ops
    ptr = [0]
    for n in SIZES:
        ptr.append(ptr[-1] + n)
    return ops.ReducePlan.from_ptr(ptr, DEV)


def _ec(row, col, w):
    from wsi_hgnn_amd import ops
    return ops.EdgeCSR(row.to(DEV), col.to(DEV), NROWS).with_weights(None if w is None else w.to(DEV))


@pytest.fixture(scope="module")
def ec(edges):
    return _ec(*edges)


def _inputs(K, seed=0):
    g = torch.Generator().manual_seed(100 * K + seed)
    return (torch.randn(NROWS, K, generator=g), torch.randn(NROWS, K, generator=g), torch.randn(G, generator=g), torch.randn(G, generator=g))


def _reference(z, g_s, g_num, g_den, row, col, w):
    z64 = z.double().requires_grad_(True)
    s, t, num, den = C.mincut_sparse(z64, row, col, None if w is None else w.double(), list(SIZES))
    ((s * g_s.double()).sum() + (num * g_num.double()).sum() + (den * g_den.double()).sum()).backward()
    return s.detach(), t.detach(), num.detach(), den.detach(), z64.grad


def _through_ops(z, g_s, g_num, g_den, ec, rp):
    from wsi_hgnn_amd import ops
    zd = z.to(DEV).requires_grad_(True)
    s, num, den, t = ops.mincut_assign_t(zd, ec, rp)
    assert not t.requires_grad and s.requires_grad and num.requires_grad and den.requires_grad
    torch.autograd.backward([s, num, den], [g_s.to(DEV), g_num.to(DEV), g_den.to(DEV)])
    return s.detach(), t, num.detach(), den.detach(), zd.grad


def _check_all(got, ref, case):
    for name, g, r in zip(("s", "t", "num", "den", "g_logits"), got, ref):
        R.check(g, r, name, case)
    gz = got[4].double().cpu()
    assert float(gz.sum(1).abs().max()) <= TOL * max(float(ref[4].abs().max()), 1e-30), f"{case}: a row of g_logits sums to {float(gz.sum(1).abs().max()):.3e}"


@pytest.mark.parametrize("K", C.KERNEL_KS)
def test_mincut_against_float64(edges, ec, rp, K):
    z, g_s, g_num, g_den = _inputs(K)
    got = _through_ops(z, g_s, g_num, g_den, ec, rp)
    _check_all(got, _reference(z, g_s, g_num, g_den, *edges), f"K={K}")
    again = _through_ops(z, g_s, g_num, g_den, ec, rp)
    for name, a, b in zip(("s", "t", "num", "den", "g_logits"), got, again):
        assert torch.equal(a, b), f"K={K}: {name} differs between identical calls"
    if K == 1:
        assert not got[4].any(), "K = 1: g_logits must be exactly 0"
        assert bool((got[0] == 1).all())


@pytest.mark.parametrize("K", C.KERNEL_KS)
def test_mincut_on_the_symmetrised_list(edges, rp, K):
    row, col, w = edges
    sym = (torch.cat([row, col]), torch.cat([col, row]), torch.cat([w, w]))
    z, g_s, g_num, g_den = _inputs(K, seed=1)
    _check_all(_through_ops(z, g_s, g_num, g_den, _ec(*sym), rp), _reference(z, g_s, g_num, g_den, *sym), f"symmetric K={K}")


@pytest.mark.parametrize("K", C.KERNEL_KS)
def test_mincut_with_a_saturated_softmax(edges, ec, rp, K):
    z, g_s, g_num, g_den = _inputs(K, seed=2)
    z = z * 30
    _check_all(_through_ops(z, g_s, g_num, g_den, ec, rp), _reference(z, g_s, g_num, g_den, *edges), f"saturated K={K}")


@pytest.mark.parametrize("K", (2, 100))
def test_mincut_ignores_a_constant_added_to_a_row(edges, ec, rp, K):
    z, g_s, g_num, g_den = _inputs(K, seed=3)
    shift = torch.randn(NROWS, 1, generator=torch.Generator().manual_seed(9)) * 5
    ref = _reference(z, g_s, g_num, g_den, *edges)
    _check_all(_through_ops(z + shift, g_s, g_num, g_den, ec, rp), ref, f"shifted K={K}")


def test_mincut_without_weights_and_with_parts_of_the_gradient(edges, rp):
    """Unit weights (edge_w NULL); a backward in which only one of the three outputs carries a gradient; no gradient asked for at all."""
    from wsi_hgnn_amd import ops
    row, col, _ = edges
    ec1 = _ec(row, col, None)
    K = 100
    z, g_s, g_num, g_den = _inputs(K, seed=4)
    _check_all(_through_ops(z, g_s, g_num, g_den, ec1, rp), _reference(z, g_s, g_num, g_den, row, col, None), "unit weights")
    zero_s, zero_g = torch.zeros_like(g_s), torch.zeros_like(g_num)
    for name, parts in (("g_s only", (g_s, zero_g, zero_g)), ("g_num only", (zero_s, g_num, zero_g)), ("g_den only", (zero_s, zero_g, g_den))):
        zd = z.to(DEV).requires_grad_(True)
        s, num, den = ops.mincut_assign(zd, ec1, rp)
        out = {"g_s only": lambda: (s * g_s.to(DEV)).sum(), "g_num only": lambda: (num * g_num.to(DEV)).sum(),
               "g_den only": lambda: (den * g_den.to(DEV)).sum()}[name]()
        out.backward()
        R.check(zd.grad, _reference(z, *parts, row, col, None)[4], "g_logits", name)
    s, num, den = ops.mincut_assign(z.to(DEV), ec1, rp)
    assert not s.requires_grad and not num.requires_grad and not den.requires_grad


def test_mincut_accepts_non_contiguous_inputs(edges, ec, rp):
    from wsi_hgnn_amd import ops
    K = 64
    z, g_s, g_num, g_den = _inputs(K, seed=5)
    ref = _reference(z, g_s, g_num, g_den, *edges)
    wide = torch.zeros(NROWS, K + 7, device=DEV)
    wide[:, 3:3 + K] = z.to(DEV)
    for case, view in (("row stride", wide[:, 3:3 + K]), ("transposed", z.to(DEV).t().contiguous().t())):
        assert not view.is_contiguous()
        zd = view.detach().requires_grad_(True)
        s, num, den = ops.mincut_assign(zd, ec, rp)
        gs_wide = torch.zeros(NROWS, 2 * K, device=DEV)
        gs_wide[:, ::2] = g_s.to(DEV)
        torch.autograd.backward([s, num, den], [gs_wide[:, ::2], g_num.to(DEV), g_den.to(DEV)])
        for name, g, r in zip(("s", "num", "den", "g_logits"), (s, num, den, zd.grad), (ref[0], ref[2], ref[3], ref[4])):
            R.check(g, r, name, case)


def test_mincut_refuses_more_than_128_columns(edges, ec, rp):
    from wsi_hgnn_amd import ops
    with pytest.raises(RuntimeError, match="code -38"):
        ops.mincut_assign(torch.zeros(NROWS, 129, device=DEV), ec, rp)
    with pytest.raises(ValueError, match="rows"):
        ops.mincut_assign(torch.zeros(NROWS - 1, 4, device=DEV), ec, rp)


def test_dense_mincut_pool_against_the_dense_formula(edges, rp):
    """gtn.dense_mincut_pool(..., return_adj=True) against torch_geometric's definition over padded float64 tensors: all four outputs, and the
    gradients of both losses and of a seeded functional of ``out`` with respect to x and the logits."""
    from wsi_hgnn_amd import gtn
    row, col, w = edges
    K, D = 10, 24
    g = torch.Generator().manual_seed(77)
    x, z, w_out = torch.randn(NROWS, D, generator=g), torch.randn(NROWS, K, generator=g), torch.randn(G, K, D, generator=g)
    gb = gtn.GraphBatch(x.to(DEV), row.to(DEV), col.to(DEV), w.to(DEV), list(SIZES))
    xd, zd = x.to(DEV).requires_grad_(True), z.to(DEV).requires_grad_(True)
    out, out_adj, mc, ortho = gtn.dense_mincut_pool(xd, zd, gb, return_adj=True)
    assert not out_adj.requires_grad and gtn.dense_mincut_pool(xd, zd, gb)[1] is None
    nmax = max(SIZES)
    X, Z = torch.zeros(G, nmax, D, dtype=torch.float64), torch.zeros(G, nmax, K, dtype=torch.float64)
    A, M = torch.zeros(G, nmax, nmax, dtype=torch.float64), torch.zeros(G, nmax)
    x64, z64 = x.double().requires_grad_(True), z.double().requires_grad_(True)
    off = 0
    for b, n in enumerate(SIZES):
        sel = (row >= off) & (row < off + n)
        X[b, :n], Z[b, :n], M[b, :n] = x64[off:off + n], z64[off:off + n], 1.0
        A[b, :n, :n] = C.dense_adjacency(n, row[sel] - off, col[sel] - off, w[sel])
        off += n
    r_out, r_adj, r_mc, r_ortho = C.mincut_dense(X, A, Z, M)
    for name, a, b in (("pool out", out, r_out), ("pool out_adj", out_adj, r_adj), ("mincut_loss", mc, r_mc), ("ortho_loss", ortho, r_ortho)):
        R.check(a, b, name, "dense_mincut_pool")
    for name, f_got, f_ref in (("mincut_loss", mc, r_mc), ("ortho_loss", ortho, r_ortho), ("out", (out * w_out.to(DEV)).sum(), (r_out * w_out.double()).sum())):
        gx, gz = torch.autograd.grad(f_got, [xd, zd], retain_graph=True, allow_unused=True)
        rx, rz = torch.autograd.grad(f_ref, [x64, z64], retain_graph=True, allow_unused=True)
        R.check(gz, rz, "g_logits of " + name, "dense_mincut_pool")
        if rx is not None:
            R.check(gx, rx, "g_x of " + name, "dense_mincut_pool")
        else:
            assert gx is None or not gx.any()


# ------------------------------------------------------------------------------------------------ attention
def _attn_reference(qkv, heads, w_out):
    q64 = qkv.double().requires_grad_(True)
    out, lse = C.attention_ref(q64, heads)
    (out * w_out.double()).sum().backward()
    return out.detach(), lse.detach(), q64.grad


def _attn_through_ops(qkv, heads, w_out):
    from wsi_hgnn_amd import ops
    qd = qkv.to(DEV).requires_grad_(True)
    out, lse = ops.seq_attention_lse(qd, heads)
    assert not lse.requires_grad
    out.backward(w_out.to(DEV))
    return out.detach(), lse, qd.grad


@pytest.mark.parametrize("n", (1, 2, 63, 64, 65, 101, 128))
@pytest.mark.parametrize("d", (8, 16))
@pytest.mark.parametrize("H", (1, 8))
def test_attention_against_float64(H, d, n):
    B = 3
    g = torch.Generator().manual_seed(1000 * H + 10 * d + n)
    qkv = torch.randn(B, n, 3 * H * d, generator=g)
    w_out = torch.randn(B, n, H * d, generator=g)
    peaked = qkv.clone()
    peaked[:, :, :2 * H * d] *= 8                                   # q and k x 8: rows of the softmax close to one-hot
    for case, x in ((f"H={H} d={d} n={n}", qkv), (f"peaked H={H} d={d} n={n}", peaked)):
        got, ref = _attn_through_ops(x, H, w_out), _attn_reference(x, H, w_out)
        for name, a, b in zip(("attn out", "attn lse", "g_qkv"), got, ref):
            R.check(a, b, name, case)
        again = _attn_through_ops(x, H, w_out)
        for name, a, b in zip(("out", "lse", "g_qkv"), got, again):
            assert torch.equal(a, b), f"{case}: {name} differs between identical calls"


def test_attention_accepts_a_non_contiguous_qkv():
    from wsi_hgnn_amd import ops
    B, n, H, d = 3, 101, 8, 8
    g = torch.Generator().manual_seed(5)
    qkv, w_out = torch.randn(B, n, 3 * H * d, generator=g), torch.randn(B, n, H * d, generator=g)
    ref = _attn_reference(qkv, H, w_out)
    view = qkv.to(DEV).transpose(0, 1).contiguous().transpose(0, 1)
    assert not view.is_contiguous()
    qd = view.detach().requires_grad_(True)
    out = ops.seq_attention(qd, H)
    g_wide = torch.zeros(B, n, 2 * H * d, device=DEV)
    g_wide[:, :, ::2] = w_out.to(DEV)
    out.backward(g_wide[:, :, ::2])
    R.check(out, ref[0], "attn out", "non-contiguous")
    R.check(qd.grad, ref[2], "g_qkv", "non-contiguous")
    assert not ops.seq_attention(view, H).requires_grad


def test_attention_refuses_what_is_not_compiled():
    from wsi_hgnn_amd import _native as N
    from wsi_hgnn_amd import ops
    with pytest.raises(RuntimeError, match="code -38"):
        ops.seq_attention(torch.zeros(2, 129, 3 * 8 * 8, device=DEV), 8)
    with pytest.raises(RuntimeError, match="code -38"):
        ops.seq_attention(torch.zeros(2, 64, 3 * 2 * 32, device=DEV), 2)
    x = torch.zeros(2, 129, 3 * 8 * 8, device=DEV)
    out, lse = torch.zeros(2, 129, 64, device=DEV), torch.zeros(2, 8, 129, device=DEV)
    lib = N.load()
    assert lib.wsi_seq_attn_fwd(N.ptr(x), 2, 129, 8, 8, 1.0, N.ptr(out), N.ptr(lse), N.stream()) == ENOSYS
    assert lib.wsi_seq_attn_bwd(N.ptr(out), N.ptr(x), N.ptr(lse), 2, 129, 8, 8, 1.0, N.ptr(x), N.stream()) == ENOSYS
    assert lib.wsi_seq_attn_fwd(N.ptr(x), 2, 64, 2, 32, 1.0, N.ptr(out), N.ptr(lse), N.stream()) == ENOSYS
