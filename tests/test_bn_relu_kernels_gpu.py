"""wsi_masked_bn_relu_fwd / _bwd and wsi_slot_live_rows through the raw C ABI on the GPU, over the cases of
tests/bn_relu_cases.py: bit-equality with the composite of the unfused entries (wsi_masked_bn_fwd then clamp_min(0); g * (y > 0) then
wsi_masked_bn_bwd) - which pins the sign the backward recomputes to the sign the forward used - the float64 restatement under the GPU's own
ReLU sides, exact zeros in dead rows, bit-equal repeats, the argument checks, and the live-row launch against the tensor formulation.

Largest error / bound against float64 reached on an MI355X: 0.244 (``test_against_float64``, which prints the figure per shape)."""
import ctypes

import numpy as np
import pytest
import torch

import bn_relu_cases as B
import gin_slot_cases as S

pytestmark = pytest.mark.gpu

DEV = "cuda"


def _lib():
    from wsi_hgnn_amd import _native as N
    return N, N.load()


def _table(a, layout):
    """A device copy of the float32 matrix ``a`` laid out as the shape asks: (tensor view, row stride)."""
    rows, C = a.shape
    t = torch.from_numpy(a)
    if layout == "stride":
        buf = torch.full((rows, C + 1), 7.0, device=DEV)
        buf[:, :C] = t.to(DEV)
        return buf[:, :C], C + 1
    if layout == "offset":
        buf = torch.full((rows * C + 1,), 7.0, device=DEV)
        v = buf[1:].view(rows, C)
        v.copy_(t.to(DEV))
        return v, C
    return t.to(DEV).contiguous(), C


def _vec(a, layout):
    if a is None:
        return None
    if layout == "offset":
        buf = torch.zeros(a.shape[0] + 1, device=DEV)
        buf[1:] = torch.from_numpy(a).to(DEV)
        return buf[1:]
    return torch.from_numpy(a).to(DEV)


def _run(case, layout, affine, running, train, fused):
    """Forward and backward through the raw entries: the fused ones, or the composite of the unfused ones around elementwise ReLU steps.
    Returns dict of out, stats, running_mean, running_var, dx, dgamma, dbeta (device tensors)."""
    N, lib = _lib()
    rows, C = case["x"].shape
    x, ldx = _table(case["x"], layout)
    g, ldg = _table(case["g"], layout)
    out, ldy = _table(np.full((rows, C), 3.0, dtype=np.float32), layout)
    dx, lddx = _table(np.full((rows, C), 3.0, dtype=np.float32), layout)
    live, n = torch.from_numpy(case["live"]).to(DEV), torch.tensor([case["n"]], device=DEV)
    gamma, beta = (_vec(case["gamma"], layout), _vec(case["beta"], layout)) if affine else (None, None)
    rm, rv = (_vec(case["rm"], layout), _vec(case["rv"], layout)) if running else (None, None)
    chunks = lib.wsi_masked_bn_chunks(rows)
    stats = torch.empty((2, C), device=DEV)
    part = torch.empty(3 * chunks * C, device=DEV)
    dgamma, dbeta = torch.empty(C, device=DEV), torch.empty(C, device=DEV)
    fwd = lib.wsi_masked_bn_relu_fwd if fused else lib.wsi_masked_bn_fwd
    N.check(fwd(N.ptr(x), ldx, rows, C, N.ptr(live), N.ptr(n), N.ptr(gamma), N.ptr(beta), N.ptr(rm), N.ptr(rv), 1 if train else 0,
                B.MOMENTUM, B.EPS, N.ptr(part), N.ptr(stats), N.ptr(out), ldy, N.stream()), "fwd")
    head = lambda gg: (N.ptr(gg), ldg, N.ptr(x), ldx, rows, C, N.ptr(live), N.ptr(n), N.ptr(gamma))
    tail = (N.ptr(stats), 1 if train else 0, N.ptr(part), N.ptr(dgamma), N.ptr(dbeta), N.ptr(dx), lddx, N.stream())
    if fused:
        N.check(lib.wsi_masked_bn_relu_bwd(*head(g), N.ptr(beta), *tail), "bwd")
    else:
        g.mul_(out > 0)                                # ReLU's backward, on the unfused forward's y; g keeps its layout
        out.clamp_(min=0)
        N.check(lib.wsi_masked_bn_bwd(*head(g), *tail), "bwd")
    torch.cuda.synchronize()
    return dict(out=out, stats=stats, running_mean=rm, running_var=rv, dx=dx, dgamma=dgamma, dbeta=dbeta)


def _cases(rows, C):
    for pattern in B.live_patterns(rows):
        case = B.make(rows, C, pattern)
        for affine, running, train in B.VARIANTS:
            yield pattern, case, affine, running, train


@pytest.mark.parametrize("rows,C,layout", B.SHAPES, ids=B.SHAPE_IDS)
def test_bit_equal_to_the_composite_of_the_unfused_entries(rows, C, layout):
    """Same sums in the same order, so every output is the composite's bit for bit - and the sign the backward kernels recompute is the
    forward's: one flipped side would change dx, dgamma or dbeta."""
    seen = 0
    for pattern, case, affine, running, train in _cases(rows, C):
        a = _run(case, layout, affine, running, train, fused=True)
        b = _run(case, layout, affine, running, train, fused=False)
        what = (pattern, affine, running, train)
        for k in a:
            assert (a[k] is None) == (b[k] is None)
            if a[k] is not None:
                assert torch.equal(a[k], b[k]), (what, k)
        dead = torch.from_numpy(case["live"] == 0).to(DEV)
        assert not a["out"][dead].any() and not a["dx"][dead].any(), what                 # exact zeros in dead rows
        assert bool((a["out"] >= 0).all())
        if C >= 4 and affine:
            assert not a["out"][:, :2].any() and not a["dx"][:, :2].any()                  # y == 0 and y < 0: the zero side, no gradient
            assert bool((a["out"][~dead][:, 2] > 0).all())
        c = _run(case, layout, affine, running, train, fused=True)                         # the same call again: the same bits
        assert all(a[k] is None or torch.equal(a[k], c[k]) for k in a), what
        seen += 1
    assert seen == 6 * len(B.live_patterns(rows))


@pytest.mark.parametrize("rows,C,layout", B.SHAPES, ids=B.SHAPE_IDS)
def test_against_float64(rows, C, layout):
    """Every block within 1e-4 of its largest float64 entry, the float64 restatement replaying the GPU's own ReLU sides (``out > 0``); first,
    what float32 itself costs on the case (the restatement in float32 on the CPU): a quarter of each bound at most.  The GPU's sides may
    differ from float64's only within 1e-5 of the column's largest |y|, on 1 % of the entries at most.
    Largest error / bound reached on an MI355X: 0.244, at 300 x 132 in every layout ('out' at two live rows without affine terms, where
    two rows of a 0.01-wide column lie 1e-4 apart and x - mean loses the bits; the float32 restatement on the CPU reaches the same
    0.244 there), 0.174 at 2 x 132, 0.097 at 300 x 67, under 0.04 at every other shape; no ReLU side differed from float64's."""
    worst, flipped = 0.0, 0
    for pattern, case, affine, running, train in _cases(rows, C):
        what = f"{rows}x{C}-{layout} {pattern} affine={affine} running={running} train={train}"
        r32 = B.restate(case, affine, running, train, dtype=np.float32)
        B.worst_ratio(r32, B.restate(case, affine, running, train, sides=r32["side"]), 0.25, what + " (float32 on the CPU)")
        got = _run(case, layout, affine, running, train, fused=True)
        cpu = {k: None if v is None else v.cpu().numpy() for k, v in got.items()}
        cpu["mean"], cpu["rstd"] = cpu["stats"][0], cpu["stats"][1]
        ref = B.restate(case, affine, running, train, sides=cpu["out"] > 0)
        flipped += B.check_sides(cpu["out"] > 0, ref, what)
        worst = max(worst, B.worst_ratio(cpu, ref, 1.0, what))
    print(f"{rows}x{C}-{layout}: largest error / bound {worst:.3f}, {flipped} ReLU sides differ from float64's")


def test_argument_checks_are_those_of_the_unfused_entries():
    N, lib = _lib()
    P = ctypes.c_void_p(1 << 40)          # a fake device address: the calls below fail their argument check before touching it
    E = N.WSI_EINVAL

    def fwd(f, **k):
        return f(k.get("x", P), k.get("ldx", 8), k.get("rows", 4), k.get("C", 8), k.get("live", P), k.get("n", P), P, P, k.get("rm", P), P,
                 k.get("train", 1), 0.1, k.get("eps", 1e-5), k.get("part", P), k.get("stats", P), k.get("y", P), k.get("ldy", 8), None)

    def bwd(f, relu, **k):
        head = (k.get("g", P), k.get("ldg", 8), P, k.get("ldx", 8), k.get("rows", 4), k.get("C", 8), P, k.get("n", P), P)
        tail = (k.get("stats", P), k.get("train", 1), k.get("part", P), k.get("dgamma", P), P, k.get("dx", P), k.get("lddx", 8), None)
        return f(*head, P, *tail) if relu else f(*head, *tail)

    bad_fwd = [dict(rows=-1), dict(C=0), dict(ldx=7), dict(ldy=7), dict(eps=-1.0), dict(eps=float("nan")), dict(x=None), dict(live=None),
               dict(stats=None), dict(y=None), dict(n=None), dict(part=None), dict(train=0, rm=None)]
    for kw in bad_fwd:
        assert fwd(lib.wsi_masked_bn_fwd, **kw) == E and fwd(lib.wsi_masked_bn_relu_fwd, **kw) == E, kw
    assert b"masked_bn_relu_fwd" in lib.wsi_last_error()
    assert fwd(lib.wsi_masked_bn_fwd, rows=0) == 0 and fwd(lib.wsi_masked_bn_relu_fwd, rows=0) == 0
    bad_bwd = [dict(rows=-1), dict(C=0), dict(ldg=7), dict(ldx=7), dict(lddx=7), dict(dgamma=None), dict(g=None), dict(stats=None),
               dict(part=None), dict(dx=None), dict(n=None)]
    for kw in bad_bwd:
        assert bwd(lib.wsi_masked_bn_bwd, False, **kw) == E and bwd(lib.wsi_masked_bn_relu_bwd, True, **kw) == E, kw
    assert b"masked_bn_relu_bwd" in lib.wsi_last_error()
    live = lambda **k: lib.wsi_slot_live_rows(k.get("seg", P), k.get("counts", P), k.get("n", 4), k.get("graphs", 3), k.get("b_cap", 2),
                                              k.get("live", P), k.get("out", P), None)
    for kw in (dict(n=-1), dict(graphs=-1), dict(b_cap=-1), dict(b_cap=4), dict(out=None), dict(counts=None), dict(seg=None), dict(live=None)):
        assert live(**kw) == E, kw


@pytest.mark.parametrize("idxs", [[0], [0, 5], [1, 3], [6]])
def test_live_row_launch_equals_the_tensor_formulation(idxs):
    """The GPU slot's tables against the CPU slot's (``graph.derive_live_rows``'s tensor operations), exactly; every word written."""
    from wsi_hgnn_amd.data import BatchSlot
    gpu, cpu = BatchSlot(S.loader(torch.device("cuda", torch.cuda.current_device())), S.WIDE), BatchSlot(S.loader("cpu"), S.WIDE)
    for t in gpu.live_rows:
        t.fill_(-7.5)
    gpu.load(idxs)
    cpu.load(idxs)
    assert torch.equal(gpu.live_rows[0].cpu(), cpu.live_rows[0]) and torch.equal(gpu.live_rows[1].cpu(), cpu.live_rows[1])
    assert gpu.live_rows[1].item() == float(sum(S.SIZES[i] for i in idxs)) and gpu.graph.__dict__["_gin_live"] is gpu.live_rows


def test_live_row_launch_without_rows_still_writes_the_count():
    N, lib = _lib()
    counts = torch.tensor([3.0, 4.0, 50.0], device=DEV)
    out = torch.full((1,), -1.0, device=DEV)
    N.check(lib.wsi_slot_live_rows(None, N.ptr(counts), 0, 3, 2, None, N.ptr(out), N.stream()), "wsi_slot_live_rows")
    assert out.item() == 7.0
    N.check(lib.wsi_slot_live_rows(None, None, 0, 3, 0, None, N.ptr(out), N.stream()), "wsi_slot_live_rows")
    assert out.item() == 0.0
