"""Every instantiation of csrc/gin.hip's dispatch table against float64, on the GPU.  ``row_cfg(D, D, 1, aligned)`` (csrc/row_group.h) maps a row width onto
one of its 16 narrow (VEC, G, NK) codes; tests/gin_cases.py's ``gin_cfg`` restates it and holds the width table (``GIN_SWEEP``) that reaches each of them
(tests/test_gin.py checks that without a GPU).  Here:
  1. the table x {sum, mean, max} x {plain, scaled} through ``ops.gin_aggregate``: forward, ``arg``, g_x, g_eps, g_bias, g_edge_scale;
  2. graphs built for the kernels' edges, one per group size G, with n = 128 * (256 / G) + 37 nodes (the last workgroup is partly empty, n is
     no multiple of 256 / G): in-degrees 0 (8 nodes), 1, 2..15, 17 and 150, duplicate edges, self loops, 24 nodes without an out-edge,
     shuffled edge order; and the degenerate graphs (one node without edges, one node with a self loop, a ring of three, no node);
  3. eps in {0, 0.3, -1} and eps as a buffer (no gradient, nothing launched for it), x without a gradient (nothing launched for it);
  4. an exact case that pins the first-position rule of max with equality (integer features with many zeros, power-of-two scales);
  5. the C ABI alone: row strides of D + 1 with a sentinel column, tensors that start 4 bytes into their buffers (the scalar path at
     D % 4 == 0), outputs inside poisoned margins, D = 1028;
  6. two identical calls give identical bits.
Tolerance: 1e-4 of the largest float64 entry of each tensor; g_eps, one sum of N * D signed terms, 1e-4 x sqrt(sum (g x)^2).

The side of a near-tie of max is decided in fp32: the reference replays the GPU's ``arg`` (taken from a C-ABI call that is bit-identical to the
op's own), after checking that every arg lies in its row's CSR range (-1 exactly for empty rows) and that the float64 message there is within
the tolerance of the float64 maximum."""
import pytest
import torch

import gin_cases as C

pytestmark = pytest.mark.gpu

DEV = "cuda"
TOL = C.TOL
MARGIN, POISON = 64, -12345.0
RATIOS = {}                        # tensor name -> (largest error / bound over the module's run, the case it came from)


@pytest.fixture(scope="module")
def graphs():
    """(csr on the CPU, plan on the device) of the group size asked for, built once per G."""
    cache = {}

    def get(G):
        if G not in cache:
            csr = C.csr_of(*C.sweep_edges(G))
            C.check_sweep_graph(G, csr)
            cache[G] = (csr, C.Plan(csr, DEV))
        return cache[G]
    return get


@pytest.fixture(scope="module", autouse=True)
def _report_ratios():
    yield
    for name, (r, case) in sorted(RATIOS.items()):
        print(f"\nlargest error / bound, {name}: {r:.3e} ({case})", end="")
    print()


class _Checks:
    """Every figure is printed and recorded before the first failure is raised."""

    def __init__(self, case):
        self.case, self.failed = case, []

    def close(self, got, ref, what, bound=None):
        r64, g64 = ref.detach().double().cpu(), got.detach().double().cpu().reshape(ref.shape)
        if not r64.numel():
            return
        bound = TOL * max(float(r64.abs().max()), 1e-30) if bound is None else max(bound, 1e-30)
        ratio = float((g64 - r64).abs().max()) / bound
        print(f"{self.case} {what}: error / bound {ratio:.3e}")
        if ratio > RATIOS.get(what, (-1.0, None))[0]:
            RATIOS[what] = (ratio, self.case)
        if not ratio <= 1.0:
            self.failed.append(f"{what}: error / bound {ratio:.3e}")

    def done(self):
        assert not self.failed, f"{self.case}: " + "; ".join(self.failed)


def _inputs(n, D, E, seed, integers=False):
    gen = torch.Generator().manual_seed(seed)
    if integers:
        x = (torch.randint(0, 4, (n, D), generator=gen) * (torch.rand(n, D, generator=gen) < 0.5)).float()
        g = torch.randint(-3, 4, (n, D), generator=gen).float()
        scale = 2.0 ** torch.randint(-1, 2, (E,), generator=gen).float()
        bias = torch.randint(-2, 3, (D,), generator=gen).float()
    else:
        x, g, bias = torch.randn(n, D, generator=gen), torch.randn(n, D, generator=gen), torch.randn(D, generator=gen)
        scale = torch.rand(E, generator=gen) * 1.5 + 0.05             # positive, on both sides of 1
    return x, g, bias, scale


def _run_gpu(x, eps, plan, mode, bias, scale, g, learn=True, x_grad=True):
    from wsi_hgnn_amd import ops
    xv = x.to(DEV).requires_grad_(x_grad)
    ev = torch.tensor([eps], dtype=torch.float32, device=DEV).requires_grad_(learn)
    bv = bias.to(DEV).requires_grad_(True) if bias is not None else None
    sv = scale.to(DEV).requires_grad_(True) if scale is not None else None
    out = ops.gin_aggregate(xv, ev, plan, mode, bias=bv, edge_scale=sv)
    out.backward(g.to(DEV))
    torch.cuda.synchronize()
    grad = lambda t: None if t is None or t.grad is None else t.grad.detach().cpu()
    return out.detach().cpu(), {"g_x": grad(xv), "g_eps": grad(ev), "g_bias": grad(bv), "g_scale": grad(sv)}


def _ld(t):
    return t.stride(0) if t.shape[0] > 1 else t.shape[1]


def _capi_fwd(x, eps, plan, mode, bias, scale, out, arg):
    """wsi_gin_aggregate_fwd on device tensors (views allowed: the row strides are taken from them)."""
    from wsi_hgnn_amd import _native as N, ops
    n, D = x.shape
    return N.load().wsi_gin_aggregate_fwd(N.ptr(x), _ld(x), n, D, N.ptr(plan.rowptr), N.ptr(plan.src), N.ptr(scale), N.ptr(eps), ops.GIN_MODES[mode],
                                          N.ptr(bias), N.ptr(out), _ld(out), N.ptr(arg), N.stream())


def _gpu_arg(x, eps, plan, bias, scale, out_op):
    """The op's own arg table: an identical C-ABI call (whose out must equal the op's bit for bit)."""
    xd = x.to(DEV)
    out = torch.empty_like(xd)
    arg = torch.full(tuple(xd.shape), -7, dtype=torch.int32, device=DEV)
    ev = torch.tensor([eps], dtype=torch.float32, device=DEV)
    rc = _capi_fwd(xd, ev, plan, "max", None if bias is None else bias.to(DEV), None if scale is None else scale.to(DEV), out, arg)
    torch.cuda.synchronize()
    assert rc == 0 and torch.equal(out.cpu(), out_op)
    return arg.cpu().long()


def _check_arg(arg, csr, x, eps, bias, scale, case):
    """Range of every arg, and the float64 message at arg against the float64 maximum."""
    rowptr = csr["rowptr"]
    lo, hi = rowptr[:-1].view(-1, 1), rowptr[1:].view(-1, 1)
    empty = (hi == lo).expand_as(arg)
    assert bool((arg[empty] == -1).all()) and bool(((arg >= lo) & (arg < hi))[~empty].all()), f"{case}: arg outside its row"
    free = C.closed_form(x, eps, csr, "max", bias, scale)
    held = C.closed_form(x, eps, csr, "max", bias, scale, arg=arg)
    bound = TOL * max(float(free["top"].abs().max()), 1e-30)
    assert float((held["out"] - free["out"]).abs().max()) <= bound, f"{case}: the message at arg is not the maximum"


def _compare(case, csr, plan, x, eps, mode, bias, scale, g, learn=True):
    out, grads = _run_gpu(x, eps, plan, mode, bias, scale, g, learn)
    d = lambda t: None if t is None else t.double()
    arg = None
    if mode == "max" and csr["n"] > 0:
        arg = _gpu_arg(x, eps, plan, bias, scale, out)
        _check_arg(arg, csr, d(x), eps, d(bias), d(scale), case)
    ref = C.closed_form(d(x), eps, csr, mode, d(bias), d(scale), d(g), arg=arg)
    ck = _Checks(case)
    ck.close(out, ref["out"], "out")
    ck.close(grads["g_x"], ref["g_x"], "g_x")
    if bias is not None:
        ck.close(grads["g_bias"], ref["g_bias"], "g_bias")
    if scale is not None:
        ck.close(grads["g_scale"], ref["g_scale"], "g_edge_scale")
    if learn:
        ck.close(grads["g_eps"], ref["g_eps"], "g_eps", bound=ref["g_eps_bound"])
    else:
        assert grads["g_eps"] is None
    ck.done()
    return out, grads, arg


# ---------------------------------------------------------------------------------------------------- 1, 2: the table
@pytest.mark.parametrize("scaled", [False, True], ids=["plain", "scaled"])
@pytest.mark.parametrize("mode", C.MODES)
@pytest.mark.parametrize("D", C.GIN_SWEEP)
def test_sweep(D, mode, scaled, graphs):
    vec, G, nk = C.gin_cfg(D, True)
    csr, plan = graphs(G)
    x, g, bias, scale = _inputs(csr["n"], D, plan.num_edges, 1000 + D)
    _compare(f"D={D} VEC={vec} G={G} NK={nk} {mode} {'scaled' if scaled else 'plain'}", csr, plan, x, 0.3, mode, bias, scale if scaled else None, g)


@pytest.mark.parametrize("mode", C.MODES)
@pytest.mark.parametrize("name", list(C.DEGENERATE))
def test_degenerate_graphs(name, mode):
    n, src, dst = C.DEGENERATE[name]
    csr = C.csr_of(n, src, dst)
    plan = C.Plan(csr, DEV)
    for D in (12, 5):
        x, g, bias, scale = _inputs(n, D, plan.num_edges, 7)
        out, grads, _ = _compare(f"{name} D={D} {mode}", csr, plan, x, 0.3, mode, bias, scale, g)
        assert tuple(out.shape) == (n, D) and tuple(grads["g_scale"].shape) == (plan.num_edges,)
        if n == 0:
            assert float(grads["g_eps"]) == 0.0


# ---------------------------------------------------------------------------------------------------- 3: eps
@pytest.mark.parametrize("mode", C.MODES)
@pytest.mark.parametrize("eps", [0.0, 0.3, -1.0])
def test_eps_values(eps, mode, graphs):
    csr, plan = graphs(16)
    x, g, bias, scale = _inputs(csr["n"], 40, plan.num_edges, 31)
    out, _, _ = _compare(f"eps={eps} {mode}", csr, plan, x, eps, mode, None, scale, g)
    if eps == -1.0:                                                   # the self term is gone: a node without in-edges is exactly 0
        assert float(out[:C.N_EMPTY].abs().max()) == 0.0


@pytest.mark.parametrize("mode", C.MODES)
def test_eps_buffer_and_constant_input_launch_nothing_for_them(mode, graphs, monkeypatch):
    from wsi_hgnn_amd import _native as N
    csr, plan = graphs(64)
    x, g, bias, scale = _inputs(csr["n"], 200, plan.num_edges, 32)

    def boom(*a):
        raise AssertionError("launched")
    monkeypatch.setattr(N.load(), "wsi_gin_eps_grad", boom)
    _compare(f"eps buffer {mode}", csr, plan, x, 0.3, mode, bias, scale, g, learn=False)
    monkeypatch.undo()
    monkeypatch.setattr(N.load(), "wsi_gin_aggregate_bwd", boom)
    monkeypatch.setattr(N.load(), "wsi_gin_edge_grad", boom)
    out, grads = _run_gpu(x, 0.3, plan, mode, bias, None, g, learn=True, x_grad=False)
    assert grads["g_x"] is None and grads["g_eps"] is not None and grads["g_bias"] is not None


# ---------------------------------------------------------------------------------------------------- 4: the first-position rule, exactly
@pytest.mark.parametrize("scaled", [False, True], ids=["plain", "scaled"])
@pytest.mark.parametrize("D", [40, 101, 512])
def test_max_first_position_rule_is_exact(D, scaled, graphs):
    G = C.gin_cfg(D, True)[1]
    csr, plan = graphs(G)
    x, g, bias, scale = _inputs(csr["n"], D, plan.num_edges, 41, integers=True)
    scale = scale if scaled else None
    out, grads = _run_gpu(x, 0.5, plan, "max", bias, scale, g)
    arg = _gpu_arg(x, 0.5, plan, bias, scale, out)
    d = lambda t: None if t is None else t.double()
    ref = C.closed_form(d(x), 0.5, csr, "max", d(bias), d(scale), d(g))            # no replay: the rule itself
    deg = csr["rowptr"][1:] - csr["rowptr"][:-1]
    ties = (C.closed_form(d(x), 0.5, csr, "max", scale=d(scale))["top"][deg > 1] == 0).float().mean()
    assert float(ties) > 0.05                                                      # many rows whose maximum is a tie of zeros
    assert torch.equal(arg, ref["arg"])
    assert torch.equal(out.double(), ref["out"]) and torch.equal(grads["g_x"].double(), ref["g_x"])
    if scaled:
        assert torch.equal(grads["g_scale"].double(), ref["g_scale"])


# ---------------------------------------------------------------------------------------------------- 5: the C ABI alone
def _framed(shape, dtype, skew):
    """A tensor of ``shape`` inside a poisoned buffer, MARGIN words on either side; ``skew``: it starts 4 bytes past a 16-byte boundary."""
    n = 1
    for s in shape:
        n *= s
    whole = torch.full((2 * MARGIN + n + 1,), POISON, dtype=dtype, device=DEV)
    lo = MARGIN + (1 if skew else 0)
    return whole, whole[lo:lo + n].view(shape), lo


def _frame_ok(whole, lo, n):
    return bool((whole[:lo] == POISON).all()) and bool((whole[lo + n:] == POISON).all())


@pytest.mark.parametrize("mode", C.MODES)
@pytest.mark.parametrize("layout", ["stride D + 1", "4 bytes in"])
@pytest.mark.parametrize("D", [40, 512])
def test_capi_strides_offsets_and_margins(D, layout, mode, graphs):
    """Both layouts force the scalar kernels at D % 4 == 0.  Inputs and outputs are views: columns [0, D) of [n, D + 1] tables whose last
    column is a sentinel, or tensors 4 bytes into poisoned buffers."""
    from wsi_hgnn_amd import _native as N, ops
    lib = N.load()
    G = C.gin_cfg(D, False)[1]
    csr, plan = graphs(G)
    n, E = csr["n"], plan.num_edges
    x, g, bias, scale = _inputs(n, D, E, 51)
    wide = layout == "stride D + 1"
    cols = D + 1 if wide else D
    frames = {}

    def place(name, t=None, dtype=torch.float32):
        whole, view, lo = _framed((n, cols), dtype, not wide)
        if wide:
            view[:, D] = 777
        if t is not None:
            view[:, :D] = t.to(DEV)
        frames[name] = (whole, lo)
        return view[:, :D]

    xv, gv, out, gx, arg = place("x", x), place("g", g), place("out"), place("gx"), place("arg", dtype=torch.int32)
    if wide:
        arg = torch.full((n, D), -7, dtype=torch.int32, device=DEV)    # (arg is a dense table: it has no stride argument)
    gs_whole, gs, gs_lo = _framed((E,), torch.float32, not wide)
    ev, bv, sv = torch.tensor([0.3], device=DEV), bias.to(DEV), scale.to(DEV)
    code = ops.GIN_MODES[mode]
    assert _capi_fwd(xv, ev, plan, mode, bv, sv, out, arg if mode == "max" else None) == 0
    assert lib.wsi_gin_aggregate_bwd(N.ptr(gv), _ld(gv), n, D, N.ptr(plan.rowptr), N.ptr(plan.colptr), N.ptr(plan.csc_eid), N.ptr(plan.csc_dst),
                                     N.ptr(sv), N.ptr(ev), code, N.ptr(arg) if mode == "max" else None, N.ptr(gx), _ld(gx), N.stream()) == 0
    assert lib.wsi_gin_edge_grad(N.ptr(gv), _ld(gv), N.ptr(xv), _ld(xv), n, D, N.ptr(plan.rowptr), N.ptr(plan.src), code,
                                 N.ptr(arg) if mode == "max" else None, N.ptr(gs), N.stream()) == 0
    partial = torch.empty(lib.wsi_gin_eps_partials(), device=DEV)
    ge = torch.empty(1, device=DEV)
    assert lib.wsi_gin_eps_grad(N.ptr(gv), _ld(gv), N.ptr(xv), _ld(xv), n, D, N.ptr(partial), N.ptr(ge), N.stream()) == 0
    torch.cuda.synchronize()
    d = lambda t: t.double()
    a = arg.cpu().long() if mode == "max" else None
    case = f"C ABI D={D} {layout} {mode}"
    if mode == "max":
        _check_arg(a, csr, d(x), 0.3, d(bias), d(scale), case)
    ref = C.closed_form(d(x), 0.3, csr, mode, d(bias), d(scale), d(g), arg=a)
    ck = _Checks(case)
    ck.close(out, ref["out"], "out")
    ck.close(gx, ref["g_x"], "g_x")
    ck.close(gs, ref["g_scale"], "g_edge_scale")
    ck.close(ge, ref["g_eps"], "g_eps", bound=ref["g_eps_bound"])
    ck.done()
    for name, (whole, lo) in frames.items():
        if name == "arg" and (wide or mode != "max"):
            continue
        assert _frame_ok(whole, lo, n * cols), f"{name}: written outside the tensor"
        if wide:
            assert bool((whole[lo:lo + n * cols].view(n, cols)[:, D] == 777).all()), f"{name}: sentinel column touched"
    assert _frame_ok(gs_whole, gs_lo, E)
    # and the same numbers as the aligned (vector) path gives through the op, within the tolerance
    out_op, grads = _run_gpu(x, 0.3, plan, mode, bias, scale, g)
    ck = _Checks(case + " against the op")
    ck.close(out, out_op, "out (scalar against vector path)")
    ck.done()


def test_capi_width_beyond_1024_is_enosys():
    from wsi_hgnn_amd import _native as N
    lib = N.load()
    x = torch.zeros((4, 1028), device=DEV)
    ptr = torch.zeros(5, dtype=torch.int32, device=DEV)
    ev = torch.zeros(1, device=DEV)
    assert lib.wsi_gin_aggregate_fwd(N.ptr(x), 1028, 4, 1028, N.ptr(ptr), N.ptr(ptr), None, N.ptr(ev), 0, None, N.ptr(x), 1028, None, N.stream()) == N.WSI_ENOSYS
    assert lib.wsi_gin_aggregate_bwd(N.ptr(x), 1028, 4, 1028, N.ptr(ptr), N.ptr(ptr), N.ptr(ptr), N.ptr(ptr), None, N.ptr(ev), 0, None, N.ptr(x), 1028,
                                     N.stream()) == N.WSI_ENOSYS
    assert lib.wsi_gin_edge_grad(N.ptr(x), 1028, N.ptr(x), 1028, 4, 1028, N.ptr(ptr), N.ptr(ptr), 0, None, N.ptr(ev), N.stream()) == N.WSI_ENOSYS
    assert lib.wsi_gin_eps_grad(N.ptr(x), 1028, N.ptr(x), 1028, 4, 1028, N.ptr(ev), N.ptr(ev), N.stream()) == N.WSI_ENOSYS
    from wsi_hgnn_amd import ops
    csr = C.csr_of(4, [0, 1], [1, 2])
    with pytest.raises(RuntimeError, match="wsi_gin_aggregate_fwd failed"):
        ops.gin_aggregate(x, ev, C.Plan(csr, DEV), "sum")


# ---------------------------------------------------------------------------------------------------- 6: determinism
@pytest.mark.parametrize("mode,D", [("sum", 1023), ("mean", 512), ("max", 200)])
def test_identical_calls_give_identical_bits(mode, D, graphs):
    csr, plan = graphs(64)
    x, g, bias, scale = _inputs(csr["n"], D, plan.num_edges, 61)
    a_out, a = _run_gpu(x, 0.3, plan, mode, bias, scale, g)
    b_out, b = _run_gpu(x, 0.3, plan, mode, bias, scale, g)
    assert torch.equal(a_out, b_out)
    for k in a:
        assert torch.equal(a[k], b[k]), k
