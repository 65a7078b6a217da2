"""The attention readout kernels (wsi_attn_readout_fwd / _bwd) on the GPU against the float64 restatement of tests/attn_readout_cases.py on
the SAME float32 inputs, through the raw ABI (row strides, g_x = NULL) and through ``ops.attention_readout``.

Bound (as the other kernel tests): error <= 1e-4 x the largest float64 entry of each block - out, gate, stats, g_x, g_w | g_b.
Every case first shows that the bound is not within reach of float32 rounding alone: the restatement run in float32 on the CPU stays under a
quarter of it.  Then: exact zeros for empty segments and for the segment whose g_out row is zero, two runs bit-equal, the backward with and
without g_x giving the same g_w | g_b bits, WSI_ENOSYS above the width limit and WSI_EINVAL on null pointers."""
import ctypes

import numpy as np
import pytest
import torch

import attn_readout_cases as AC

pytestmark = pytest.mark.gpu

DEV = "cuda"


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__
    __graft_entry__.build()
    from wsi_hgnn_amd import _native
    return _native.load()


@pytest.fixture(scope="module")
def rp():
    from wsi_hgnn_amd import ops
    return ops.ReducePlan.from_ptr(AC.OFF, DEV, AC.CHUNK)


@pytest.fixture(scope="module")
def refs():
    """inputs and float64 restatement of every case, computed once."""
    return {AC.case_id(c): (AC.inputs(c), AC.restate(*AC.inputs(c))) for c in AC.CASES}


def _raw(lib, rp, case, args, want_gx=True, x_offset=0):
    """Forward and backward through the C ABI; x lives in a buffer with the case's row stride, ``x_offset`` floats into it."""
    from wsi_hgnn_amd import _native as N
    D, _, ld = case
    x, w, b, g_out = args
    buf = torch.zeros(AC.ROWS * ld + x_offset, device=DEV)
    buf[x_offset:].view(AC.ROWS, ld)[:, :D] = x.to(DEV)
    w, b, g_out = w.to(DEV), b.to(DEV), g_out.to(DEV).contiguous()
    S, nch = rp.num_segs, rp.num_chunks
    out = torch.full((S, D), -7.5, device=DEV)
    gate = torch.full((AC.ROWS,), -7.5, device=DEV)
    stats = torch.full((S, 2), -7.5, device=DEV)
    partial = torch.empty(nch * (D + 2), device=DEV)
    N.check(lib.wsi_attn_readout_fwd(N.ptr(buf, 4 * x_offset), ld, D, N.ptr(w), N.ptr(b), N.ptr(rp.chunk_row), nch, N.ptr(rp.seg_chunk), S,
                                     N.ptr(partial), N.ptr(out), N.ptr(gate), N.ptr(stats), N.stream()), "wsi_attn_readout_fwd")
    g_x = torch.full((AC.ROWS, D), -7.5, device=DEV) if want_gx else None
    g_wb = torch.full((D + 1,), -7.5, device=DEV)
    scratch = torch.empty(S + nch * (D + 1), device=DEV)
    N.check(lib.wsi_attn_readout_bwd(N.ptr(g_out), N.ptr(out), N.ptr(gate), N.ptr(stats), N.ptr(buf, 4 * x_offset), ld, D, N.ptr(w),
                                     N.ptr(rp.chunk_row), N.ptr(rp.chunk_seg), nch, S, N.ptr(scratch), N.ptr(g_x), D, N.ptr(g_wb),
                                     N.stream()), "wsi_attn_readout_bwd")
    got = {"out": out, "gate": gate, "stats": stats, "g_wb": g_wb}
    if want_gx:
        got["g_x"] = g_x
    return {k: v.cpu() for k, v in got.items()}


def _check(got, ref, what):
    for k, v in got.items():
        r = AC.error_ratio(v.numpy(), ref[k])
        print(f"{what}: {k} error / bound = {r:.4f}")
        assert r <= 1.0, (what, k, r)
    for s, n in enumerate(AC.LENS):
        if n == 0:
            assert not got["out"][s].any() and not got["stats"][s].any(), f"{what}: empty segment {s}"
    if "g_x" in got:
        a, e = AC.OFF[AC.ZERO_SEG], AC.OFF[AC.ZERO_SEG + 1]
        assert not got["g_x"][a:e].any(), f"{what}: rows of the segment without gradient"
        assert got["g_x"][AC.OFF[2]:AC.OFF[3]].any()


@pytest.mark.parametrize("case", AC.CASES, ids=AC.case_id)
def test_kernels_against_float64(lib, rp, refs, case):
    args, ref = refs[AC.case_id(case)]
    f32 = AC.restate(*args, dtype=np.float32)
    for k in ref:
        r = AC.error_ratio(f32[k], ref[k])
        assert r <= 0.25, (k, r, "float32 arithmetic alone uses more than a quarter of the bound")
    got = _raw(lib, rp, case, args)
    _check(got, ref, AC.case_id(case))
    again = _raw(lib, rp, case, args)
    for k in got:
        assert torch.equal(got[k], again[k]), f"{k}: two runs differ"
    no_gx = _raw(lib, rp, case, args, want_gx=False)
    assert "g_x" not in no_gx and torch.equal(no_gx["g_wb"], got["g_wb"])
    if case[1] == "ties":                         # equal gates: the mean of the segment's rows
        x = args[0].double()
        for s, (a, e) in enumerate(zip(AC.OFF[:-1], AC.OFF[1:])):
            if e > a:
                assert AC.error_ratio(got["out"][s].numpy(), x[a:e].mean(0).numpy()) <= 1.0


def test_unaligned_base_pointer_takes_the_scalar_path(lib, rp, refs):
    case = (256, "ordinary", 256)
    args, ref = refs[AC.case_id(case)]
    got = _raw(lib, rp, case, args, x_offset=1)
    _check(got, ref, "x one float off a 16-byte boundary")
    aligned = _raw(lib, rp, case, args)
    for k in ("gate", "out"):                     # the same arithmetic in the same order, whatever the width of the loads
        assert torch.equal(got[k], aligned[k]), k


def _through_ops(rp, args, x_grad=True):
    from wsi_hgnn_amd import ops
    x, w, b, g_out = args
    x = x.to(DEV).requires_grad_(x_grad)
    w = w.to(DEV).view(1, -1).requires_grad_(True)
    b = b.to(DEV).requires_grad_(True)
    out = ops.attention_readout(x, w, b, rp)
    out.backward(g_out.to(DEV))
    return out.detach().cpu(), (x.grad.cpu() if x_grad else None), torch.cat([w.grad.reshape(-1), b.grad.reshape(-1)]).cpu()


@pytest.mark.parametrize("case", [(67, "twomax", 67), (1028, "peaked", 1028), (256, "ordinary", 257)], ids=AC.case_id)
def test_autograd_node_against_float64(lib, rp, refs, case):
    args, ref = refs[AC.case_id(case)]
    out, g_x, g_wb = _through_ops(rp, args)
    assert g_x.shape == args[0].shape
    for k, v in (("out", out), ("g_x", g_x), ("g_wb", g_wb)):
        assert AC.error_ratio(v.numpy(), ref[k]) <= 1.0, k
    out2, none, g_wb2 = _through_ops(rp, args, x_grad=False)          # layer 0: the feature table needs no gradient and none is formed
    assert none is None and torch.equal(out2, out) and torch.equal(g_wb2, g_wb)
    raw = _raw(lib, rp, case, args)
    assert torch.equal(raw["out"], out) and torch.equal(raw["g_x"], g_x) and torch.equal(raw["g_wb"], g_wb)


def test_module_switch_on_the_gpu(rp, refs):
    """``GlobalAttentionPooling`` with the switch on equals its composite path (switch off) within the bound, on one node type's rows."""
    from wsi_hgnn_amd import ops
    from wsi_hgnn_amd.pooling import GlobalAttentionPooling
    case = (256, "ordinary", 256)
    (x, w, b, _), ref = refs[AC.case_id(case)]

    class G:
        ntypes = ["n"]
        def batch_num_nodes(self, ntype=None):
            return torch.tensor(AC.LENS)
    pool = GlobalAttentionPooling(torch.nn.Linear(256, 1)).to(DEV)
    with torch.no_grad():
        pool.gate_nn.weight.copy_(w.view(1, -1)); pool.gate_nn.bias.copy_(b)
    composite = pool(G(), x.to(DEV)).detach().cpu()
    ops.set_fused_attention_readout(True)
    try:
        fused = pool(G(), x.to(DEV)).detach().cpu()
    finally:
        ops.set_fused_attention_readout(False)
    assert AC.error_ratio(composite.numpy(), ref["out"]) <= 1.0 and AC.error_ratio(fused.numpy(), ref["out"]) <= 1.0


def test_refused_shapes_and_null_pointers(lib):
    from wsi_hgnn_amd import _native as N
    P = ctypes.c_void_p(1 << 40)          # a fake device address: every call below must fail its argument check before touching it
    fwd = lambda x=P, ldx=16, D=16, w=P, cr=P, nch=2, sc=P, ns=2, part=P, out=P, gate=P, stats=P: lib.wsi_attn_readout_fwd(
        x, ldx, D, w, P, cr, nch, sc, ns, part, out, gate, stats, None)
    bwd = lambda g=P, out=P, gate=P, stats=P, x=P, ldx=16, D=16, w=P, cr=P, cs=P, nch=2, ns=2, scr=P, gx=P, ldgx=16, gwb=P: lib.wsi_attn_readout_bwd(
        g, out, gate, stats, x, ldx, D, w, cr, cs, nch, ns, scr, gx, ldgx, gwb, None)
    assert fwd(D=2049, ldx=2049) == N.WSI_ENOSYS and b"2049" in lib.wsi_last_error()
    assert bwd(D=2049, ldx=2049, ldgx=2049) == N.WSI_ENOSYS
    for kw in ({"x": None}, {"w": None}, {"cr": None}, {"sc": None}, {"part": None}, {"out": None}, {"gate": None}, {"stats": None}):
        assert fwd(**kw) == N.WSI_EINVAL, kw
    for kw in ({"g": None}, {"out": None}, {"gate": None}, {"stats": None}, {"x": None}, {"w": None}, {"cr": None}, {"cs": None}, {"scr": None},
               {"gwb": None}):
        assert bwd(**kw) == N.WSI_EINVAL, kw
    assert fwd(D=0) == N.WSI_EINVAL and fwd(ldx=15) == N.WSI_EINVAL and fwd(nch=-1) == N.WSI_EINVAL
    assert bwd(D=0) == N.WSI_EINVAL and bwd(ldx=15) == N.WSI_EINVAL and bwd(ldgx=15) == N.WSI_EINVAL
    # (g_x = NULL is a valid call: it would launch, so it is made with real tensors only - test_kernels_against_float64)
