"""Kernel-level tests of what the sibling models (HGT, GCN, ASAP) and the readouts run: relation attention on the HGT table layout,
LayerNorm, GELU, the GraphConv neighbour sum and the segment readouts, each against a float64 restatement computed on the CPU from
the inputs and the plan tensors (oracle/kernel_ref.py), at the widths, row counts and edges where these kernels branch.

Tolerances are those of tests/test_kernels_gpu.py (relative to the largest reference value) unless a case says otherwise.
"""
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu


def _dev():
    return torch.device("cuda:0")


def _relerr(a, b):
    a = a.double().cpu()
    b = b.double().cpu()
    return ((a - b).abs().max() / b.abs().max().clamp(min=1e-30)).item()


def _poison_allocator():
    """Fill a large block of the caching allocator with NaN and hand it back, so that the next allocations (the kernel's outputs)
    start out as NaN and an element the kernel never writes shows up as NaN instead of as a lucky zero."""
    torch.cuda.empty_cache()            # (otherwise an allocation may reuse some other cached block)
    junk = torch.full((64 << 20,), float("nan"), device=_dev())
    del junk


# ------------------------------------------------------------------------------------------ HGT relation attention
# (Dp, H, hidden): hidden = None -> every column is live; otherwise HGT's zero-padded layout (models/HGT.py: padded_head_dim)
_REL_CASES = [(128, 8, None), (256, 4, None), (512, 8, None), (256, 16, None),   # the specialised kernels
              (256, 4, 200),                                                     # hidden 200, 4 heads: d_k 50 padded to 64
              (96, 3, None)]                                                     # generic kernels


@pytest.mark.parametrize("Dp,H,hidden,weighted", [c + (False,) for c in _REL_CASES] + [(256, 4, None, True), (96, 3, None, True)])
@pytest.mark.parametrize("dst_mode", ["uniform", "hub", "hub-coop"])
def test_relation_attention_fwd_bwd(Dp, H, hidden, weighted, dst_mode, monkeypatch):
    """ops.relation_attention (wsi_heat_attn_fwd/bwd with separate q and k|v tables over per-relation source rows) against float64.
    HGT runs it with e_weight = 0 and sim = 0; ``weighted`` adds a nonzero weight and a random sim.  Inputs at the scale of
    test_heat_attention_fwd_bwd, with its tolerances."""
    from wsi_hgnn_amd import ops, synthetic, batch as gbatch, graph as graph_mod
    from wsi_hgnn_amd.models.HGT import padded_head_dim
    from oracle import kernel_ref
    if dst_mode == "hub-coop":
        monkeypatch.setattr(graph_mod, "HEAVY_DEGREE", 8)
    gs = [synthetic.hetero_graph(400, 8, seed=31 + i, dst_mode="hub" if dst_mode == "hub-coop" else dst_mode) for i in range(2)]
    plan = gbatch(gs).to(_dev()).plan(per_relation_src=True)
    if dst_mode == "hub-coop" and Dp in (128, 256, 512):
        assert plan.num_heavy > 0 and plan.heavy_degree == 8
    n, R, E = plan.num_nodes, plan.num_src_rows, plan.num_edges
    assert R > n                                                   # per-relation rows, not one row per node
    torch.manual_seed(Dp * 5 + H)
    q = torch.randn(n, Dp, device=_dev()) * 0.5
    kv = torch.randn(R, 2 * Dp, device=_dev()) * 0.5
    live = torch.ones(Dp, dtype=torch.bool)
    if hidden is not None:
        dkp = padded_head_dim(hidden, H)
        assert dkp * H == Dp and hidden % H == 0 and hidden // H < dkp
        live = (torch.arange(Dp) % dkp) < hidden // H             # the d_k live columns of every head
        q[:, ~live.to(_dev())] = 0
        kv[:, torch.cat([~live, ~live]).to(_dev())] = 0
        eb = torch.full((1,), math.sqrt(dkp * H / hidden), device=_dev())      # exactly as HgtContext.one_b
    else:
        eb = torch.tensor([0.3], device=_dev())
    if weighted:
        ew = torch.tensor([[0.7]], device=_dev())
        sim = torch.rand(max(E, 1), device=_dev()) * 2 - 1
    else:
        ew = torch.zeros(1, 1, device=_dev())
        sim = torch.zeros(max(E, 1), device=_dev())
    q.requires_grad_()
    kv.requires_grad_()
    ew.requires_grad_()
    eb.requires_grad_()
    t = ops.relation_attention(q, kv, ew, eb, plan, sim, Dp, H)
    gt = torch.randn_like(t)
    _poison_allocator()
    t.backward(gt)

    pc = kernel_ref.plan_to_cpu(plan)
    qd = q.detach().double().cpu().requires_grad_()
    kvd = kv.detach().double().cpu().requires_grad_()
    ewd = ew.detach().double().cpu().requires_grad_()
    ebd = eb.detach().double().cpu().requires_grad_()
    ref = kernel_ref.relation_attention_ref(qd, kvd, ewd, ebd, pc, sim.double().cpu()[:E], Dp, H)
    ref.backward(gt.double().cpu())
    assert _relerr(t, ref) < 1e-5, _relerr(t, ref)
    assert _relerr(q.grad, qd.grad) < 1e-4, ("g_q", _relerr(q.grad, qd.grad))
    assert _relerr(kv.grad[:, :Dp], kvd.grad[:, :Dp]) < 1e-4, ("g_k", _relerr(kv.grad[:, :Dp], kvd.grad[:, :Dp]))
    assert _relerr(kv.grad[:, Dp:], kvd.grad[:, Dp:]) < 1e-4, ("g_v", _relerr(kv.grad[:, Dp:], kvd.grad[:, Dp:]))
    assert abs(ew.grad.item() - ewd.grad.item()) < 1e-4 * max(1.0, abs(ewd.grad.item())), (ew.grad.item(), ewd.grad.item())
    assert abs(eb.grad.item() - ebd.grad.item()) < 1e-4 * max(1.0, abs(ebd.grad.item())), (eb.grad.item(), ebd.grad.item())
    if hidden is not None:
        gq, gkv = q.grad.cpu(), kv.grad.cpu()
        assert torch.count_nonzero(gq[:, ~live]) == 0, "g_q pad columns"
        assert torch.count_nonzero(gkv[:, :Dp][:, ~live]) == 0, "g_k pad columns"
        assert torch.count_nonzero(t.detach().cpu()[:, ~live]) == 0, "t pad columns"
        # the padded layout computes HGT's attention at the true width: d_k = hidden / H, logits scaled by 1/sqrt(d_k)
        qt = qd.detach()[:, live]
        kvt = torch.cat([kvd.detach()[:, :Dp][:, live], kvd.detach()[:, Dp:][:, live]], 1)
        one = torch.ones(1, dtype=torch.float64)
        ref_true = kernel_ref.relation_attention_ref(qt, kvt, 0 * one, one, pc, torch.zeros(E, dtype=torch.float64), hidden, H)
        assert _relerr(t.detach()[:, live.to(_dev())], ref_true) < 1e-5, "true-width HGT attention"
    # k|v rows of (relation, source node) pairs that send no edge: exactly zero gradient (the allocator was poisoned with NaN)
    outdeg = torch.bincount(pc.src.long(), minlength=R)
    idle = outdeg == 0
    assert int(idle.sum()) > 0
    assert torch.count_nonzero(kv.grad.cpu()[idle]) == 0 and not torch.isnan(kv.grad).any()
    assert not torch.isnan(q.grad).any()


# ------------------------------------------------------------------------------------------ LayerNorm
def _ln_setup(n, D, seed):
    """Segments [(0,a), (a,b), (b,n), (n,n)] -> parameter rows [0, 1, 0, 2]: two segments share row 0 and row 2 owns an empty range."""
    from wsi_hgnn_amd import ops
    a, b = n // 3, n // 3 + (n + 1) // 3
    ranges = [(0, a), (a, b), (b, n), (n, n)]
    seg_param = [0, 1, 0, 2]
    row_param = torch.cat([torch.full((hi - lo,), p, dtype=torch.int32) for (lo, hi), p in zip(ranges, seg_param)])
    rp = ops.ReducePlan.from_ranges(ranges, _dev())
    g = torch.Generator().manual_seed(seed)
    gamma = torch.randn(3, D, generator=g) * 0.5 + 1.0
    beta = torch.randn(3, D, generator=g)
    return rp, seg_param, row_param, gamma, beta


def _ln_ref(x, gamma, beta, row_param, eps=1e-5):
    """float64 reference on the CPU: F.layer_norm without affine, then the per-row parameter rows (autograd gives all three gradients)."""
    D = x.shape[1]
    rpl = row_param.long()
    return F.layer_norm(x, (D,), eps=eps) * gamma[rpl] + beta[rpl]


def _ln_run(x, gamma, beta, row_param, rp, seg_param, gy):
    from wsi_hgnn_amd import ops
    xg = x.to(_dev()).requires_grad_()
    gg = gamma.to(_dev()).requires_grad_()
    bg = beta.to(_dev()).requires_grad_()
    y = ops.layer_norm(xg, gg, bg, row_param.to(_dev()), rp, seg_param)
    _poison_allocator()
    y.backward(gy.to(_dev()))
    xd, gd, bd = (t.detach().double().requires_grad_() for t in (x, gamma, beta))
    ref = _ln_ref(xd, gd, bd, row_param)
    ref.backward(gy.double())
    return (y, xg.grad, gg.grad, bg.grad), (ref, xd.grad, gd.grad, bd.grad)


@pytest.mark.parametrize("D", [1, 50, 64, 65, 128, 200, 256, 300, 512, 700, 1024])
@pytest.mark.parametrize("n", [1, 3, 517])
def test_layer_norm_fwd_bwd(D, n):
    """ops.layer_norm over every NV bucket of wsi_layernorm_fwd/bwd (NV = 1, 2, 4, 8, 16 lanes of 64 columns) and both sides of each
    bucket edge, row counts that leave the last 4-row block partly empty, per-type parameter rows with a shared and an empty one.
    Rows 0 and n-1 (when n > 1) are constant (zero variance); the constants are dyadic so that the kernel's mean is exact and the
    output must equal beta."""
    rp, seg_param, row_param, gamma, beta = _ln_setup(n, D, seed=D * 7 + n)
    g = torch.Generator().manual_seed(D + 1000 * n)
    x = torch.randn(n, D, generator=g) * 2 + 0.5
    const_rows = [0, n - 1] if n > 1 else []
    if D > 1:                           # (at D = 1 every row is constant)
        for r, c in zip(const_rows, (-2.75, 6.5)):
            x[r] = c
    gy = torch.randn(n, D, generator=g)
    (y, gx, ggam, gbet), (ref, rx, rg, rb) = _ln_run(x, gamma, beta, row_param, rp, seg_param, gy)
    assert _relerr(y, ref) < 1e-5, ("y", _relerr(y, ref))
    assert _relerr(gx, rx) < 1e-4, ("g_x", _relerr(gx, rx))
    assert _relerr(ggam, rg) < 1e-4, ("g_gamma", _relerr(ggam, rg))
    assert _relerr(gbet, rb) < 1e-4, ("g_beta", _relerr(gbet, rb))
    assert torch.count_nonzero(ggam[2]) == 0 and torch.count_nonzero(gbet[2]) == 0      # parameter row of the empty range
    yc, gxc = y.detach().cpu(), gx.cpu()
    assert torch.isfinite(yc).all() and torch.isfinite(gxc).all()
    for r in (const_rows if D > 1 else range(n)):
        assert torch.equal(yc[r], beta[row_param[r].long()]), r          # zero variance: xhat = 0 exactly, y = beta


@pytest.mark.parametrize("D", [64, 200, 700, 1024])
def test_layer_norm_large_offset_rows(D):
    """Rows with mean 1e3 and spread 1e-2: the fp32 floor is set by the input itself.  The kernel's error against float64 stays within
    2x the error of torch's own fp32 F.layer_norm on the GPU for the same input, + 1e-6."""
    n = 517
    rp, seg_param, row_param, gamma, beta = _ln_setup(n, D, seed=D)
    g = torch.Generator().manual_seed(D + 5)
    x = 1e3 + 1e-2 * torch.randn(n, D, generator=g)
    gy = torch.randn(n, D, generator=g)
    (y, gx, ggam, gbet), (ref, rx, rg, rb) = _ln_run(x, gamma, beta, row_param, rp, seg_param, gy)
    # torch fp32 on the GPU, same formulation (affine applied per row)
    xt = x.to(_dev()).requires_grad_()
    gt_ = gamma.to(_dev()).requires_grad_()
    bt = beta.to(_dev()).requires_grad_()
    rpl = row_param.long().to(_dev())
    yt = F.layer_norm(xt, (D,)) * gt_[rpl] + bt[rpl]
    yt.backward(gy.to(_dev()))
    for name, k, t, r in (("y", y, yt, ref), ("g_x", gx, xt.grad, rx), ("g_gamma", ggam, gt_.grad, rg), ("g_beta", gbet, bt.grad, rb)):
        ek = (k.detach().double().cpu() - r.detach()).abs().max().item()
        et = (t.detach().double().cpu() - r.detach()).abs().max().item()
        assert ek <= 2 * et + 1e-6, (name, ek, et)


def test_layer_norm_rejects_width_over_1024():
    rp, seg_param, row_param, gamma, beta = _ln_setup(8, 1025, seed=0)
    from wsi_hgnn_amd import ops
    x = torch.randn(8, 1025, device=_dev())
    with pytest.raises(RuntimeError, match="feature width 1025 > 1024 unsupported"):
        ops.layer_norm(x, gamma.to(_dev()), beta.to(_dev()), row_param.to(_dev()), rp, seg_param)


# ------------------------------------------------------------------------------------------ GELU
def _gelu64(x):
    return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))


def _gelu64_grad(x):
    return 0.5 * (1.0 + torch.erf(x / math.sqrt(2.0))) + x * torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)


def _ulp32(r):
    """1 ulp (fp32) of max(|r|, 1e-30), elementwise, as float64."""
    m = r.abs().clamp(min=1e-30).float()
    return (torch.nextafter(m, torch.full_like(m, float("inf"))) - m).double()


def test_gelu_fwd_bwd_every_element():
    """wsi_gelu_fwd/bwd, every element against float64 erf-GELU: a dense grid over [-12, 12] plus +-0, +-1e-30, +-1e4, at a length
    (2 * 4096 * 256 + 77) where the 4096-block grid-stride loop wraps twice and ends in a partial block.  The negative tail cancels in
    any fp32 erf form, so the bound per element is 2x torch's own fp32 F.gelu error on that element + 1 ulp."""
    from wsi_hgnn_amd import ops
    L = 2 * 4096 * 256 + 77
    special = torch.tensor([0.0, -0.0, 1e-30, -1e-30, 1e4, -1e4, 1.0, -1.0], dtype=torch.float32)
    grid = torch.linspace(-12.0, 12.0, L - special.numel(), dtype=torch.float32)
    x = torch.cat([grid[: L // 2], special, grid[L // 2:]])          # specials in the middle: a wrapped iteration of the loop
    assert x.numel() == L
    gy = torch.rand(L, generator=torch.Generator().manual_seed(3)) + 0.5
    xg = x.to(_dev()).requires_grad_()
    y = ops.gelu(xg)
    _poison_allocator()
    y.backward(gy.to(_dev()))
    xt = x.to(_dev()).requires_grad_()
    yt = F.gelu(xt)
    yt.backward(gy.to(_dev()))
    xd = x.double()
    ref = _gelu64(xd)
    gref = gy.double() * _gelu64_grad(xd)
    for name, k, t, r in (("fwd", y, yt, ref), ("bwd", xg.grad, xt.grad, gref)):
        k, t = k.detach().double().cpu(), t.detach().double().cpu()
        ek, et = (k - r).abs(), (t - r).abs()
        bad = ~(ek <= 2 * et + _ulp32(r))
        assert not bad.any(), (name, int(bad.sum()), x[bad][:5].tolist(), k[bad][:5].tolist(), r[bad][:5].tolist())


# ------------------------------------------------------------------------------------------ GraphConv aggregation
def _gcn_graph(seed):
    """Edges (dst, src) over n nodes with in-degree-0 nodes, out-degree-0 nodes, self-loops, duplicate edges, one destination with
    in-degree >= 5000 and one source with out-degree >= 5000."""
    g = torch.Generator().manual_seed(seed)
    n = 3000
    # nodes [n - 60, n) are never a destination, nodes [n - 120, n - 60) never a source
    srcs_ok = n - 120
    hub_dst, hub_src = 7, 11

    def rsrc(k):
        s = torch.randint(0, srcs_ok + 60, (k,), generator=g)
        return torch.where(s >= srcs_ok, s + 60, s)         # skip the no_out block

    def rdst(k):
        return torch.randint(0, n - 60, (k,), generator=g)

    src = [rsrc(4 * n), rsrc(5200), torch.full((5100,), hub_src)]
    dst = [rdst(4 * n), torch.full((5200,), hub_dst), rdst(5100)]
    loops = torch.arange(0, n - 120, 3)
    src.append(loops)
    dst.append(loops)
    src, dst = torch.cat(src), torch.cat(dst)
    dup = torch.randint(0, src.numel(), (500,), generator=g)
    src, dst = torch.cat([src, src[dup]]), torch.cat([dst, dst[dup]])
    return n, src, dst


@pytest.mark.parametrize("D", [1, 37, 64, 100, 128, 512, 1024])
@pytest.mark.parametrize("relu,has_bias", [(False, False), (False, True), (True, False), (True, True)])
@pytest.mark.parametrize("weighted", [False, True])
def test_graph_conv_aggregate(D, relu, has_bias, weighted):
    """ops.graph_conv_aggregate (wsi_spmm_sum forward over the CSR, backward over the CSC) with GraphConv norm='both' (in/out norms as
    models/GCN.py computes them), bias, ReLU and signed edge weights, against a float64 scatter.  For the ReLU backward the output
    gradient is zeroed where the float64 pre-activation lies within fp32 rounding of 0, so the mask at those elements cannot matter."""
    from wsi_hgnn_amd import ops
    n, src, dst = _gcn_graph(seed=5)
    ec = ops.EdgeCSR(dst.to(_dev()), src.to(_dev()), n)
    indeg = (ec.rowptr[1:] - ec.rowptr[:-1]).to(torch.float32)
    outdeg = (ec.colptr[1:] - ec.colptr[:-1]).to(torch.float32)
    assert indeg.max() >= 5000 and outdeg.max() >= 5000 and (indeg == 0).any() and (outdeg == 0).any()
    ec.in_norm = indeg.clamp(min=1).pow(-0.5).contiguous()
    ec.out_norm = outdeg.clamp(min=1).pow(-0.5).contiguous()
    gen = torch.Generator().manual_seed(D * 3 + relu * 2 + has_bias + 10 * weighted)
    w = (torch.rand(src.numel(), generator=gen) * 2 - 1) if weighted else None
    if weighted:
        ec = ec.with_weights(w.to(_dev()))
    z = torch.randn(n, D, generator=gen)
    bias = torch.randn(D, generator=gen) * 0.5 if has_bias else None
    # float64 reference from the edge list
    zd = z.double().requires_grad_()
    bd = bias.double().requires_grad_() if has_bias else None
    inn, outn = ec.in_norm.double().cpu(), ec.out_norm.double().cpu()
    coef = outn[src] * (w.double() if weighted else 1.0)
    pre = torch.zeros(n, D, dtype=torch.float64).index_add_(0, dst, zd[src] * coef.unsqueeze(1)) * inn.unsqueeze(1)
    if has_bias:
        pre = pre + bd
    ref = torch.relu(pre) if relu else pre
    gy = torch.randn(n, D, generator=gen)
    if relu:
        mag = torch.zeros(n, D, dtype=torch.float64).index_add_(0, dst, (zd.detach()[src] * coef.unsqueeze(1)).abs()) * inn.unsqueeze(1)
        near0 = pre.detach().abs() <= 1e-5 * (mag + (bd.detach().abs() if has_bias else 0))
        gy[near0] = 0
    ref.backward(gy.double())
    zg = z.to(_dev()).requires_grad_()
    bg = bias.to(_dev()).requires_grad_() if has_bias else None
    y = ops.graph_conv_aggregate(zg, bg, ec, relu)
    _poison_allocator()
    y.backward(gy.to(_dev()))
    assert _relerr(y, ref) < 1e-5, ("y", _relerr(y, ref))
    assert _relerr(zg.grad, zd.grad) < 1e-5, ("g_z", _relerr(zg.grad, zd.grad))
    if has_bias:
        assert _relerr(bg.grad, bd.grad) < 1e-5, ("g_bias", _relerr(bg.grad, bd.grad))
    yc = y.detach().cpu()
    no_in = indeg.cpu() == 0
    exp_empty = (torch.relu(bias) if relu else bias) if has_bias else torch.zeros(D)
    assert torch.equal(yc[no_in], exp_empty.expand(int(no_in.sum()), D))       # nothing gathered: bias (through the ReLU) or 0
    assert torch.count_nonzero(zg.grad.cpu()[outdeg.cpu() == 0]) == 0


def test_graph_conv_aggregate_rejects_width_over_1024():
    from wsi_hgnn_amd import ops
    n, src, dst = _gcn_graph(seed=5)
    ec = ops.EdgeCSR(dst.to(_dev()), src.to(_dev()), n)
    with pytest.raises(RuntimeError, match="feature width 1025 > 1024 unsupported"):
        ops.graph_conv_aggregate(torch.randn(n, 1025, device=_dev()), None, ec, False)


# ------------------------------------------------------------------------------------------ segment readouts
_SEG_COUNTS = [0, 1, 3, 128, 129, 0, 512, 20000]


def _seg_ranges(counts, first=0):
    ranges, pos = [], first
    for c in counts:
        ranges.append((pos, pos + c))
        pos += c
    return ranges


def _sumlike_check(out, gx, x, g, ranges, op):
    """sum / mean: |err| <= 1e-6 * sum|x| per (segment, column) (/ count for mean); gx rows = g (/ count) of their segment."""
    xd, gd = x.double().cpu(), g.double().cpu()
    outc, gxc = out.detach().double().cpu(), gx.double().cpu()
    ref_gx = torch.zeros_like(xd)
    for s, (a, b) in enumerate(ranges):
        cnt = max(b - a, 1)
        div = cnt if op == "mean" else 1
        ref = xd[a:b].sum(0) / div
        bound = 1e-6 * xd[a:b].abs().sum(0) / div
        assert ((outc[s] - ref).abs() <= bound).all(), (op, s, (outc[s] - ref).abs().max().item())
        ref_gx[a:b] = (gd[s] / div).float().double()
    assert _relerr(gxc, ref_gx) < 1e-6 and torch.equal(gxc == 0, ref_gx == 0), op


def _max_inputs(n, D, ranges, neg_segments, seed):
    """Integer-valued rows in [-3, 3] (in [-3, -1] for the segments in ``neg_segments``): ties everywhere.  In two of every three
    columns the maximum is planted first at a row that walks over wave (stride 4) and 128-row chunk boundaries, and repeated after it
    in the same wave, the next wave and the next chunk."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randint(-3, 4, (n, D), generator=g).float()
    first = [0, 1, 2, 3, 4, 5, 7, 124, 127, 128, 129, 131, 255, 256, 300, 511, 512, 4097, 19999]
    for s, (a, b) in enumerate(ranges):
        L = b - a
        if L == 0:
            continue
        neg = s in neg_segments
        top = -1.0 if neg else 3.0
        x[a:b] = torch.randint(-3, 0, (L, D), generator=g).float() if neg else x[a:b]
        for c in range(D):
            if c % 3 == 2:
                continue
            p = first[(c // 3 * 2 + c % 3 + s) % len(first)] % L
            x[a:b, c] = x[a:b, c].clamp(max=top - 1)
            for k in (0, 1, 3, 4, 127, 128, 129):
                if p + k < L:
                    x[a + p + k, c] = top
    return x


def _max_check(out, gx, x, g, ranges):
    xd, gc = x.double().cpu(), g.cpu()
    outc, gxc = out.detach().cpu(), gx.cpu()
    ref_gx = torch.zeros_like(x.cpu())
    for s, (a, b) in enumerate(ranges):
        if b == a:
            assert torch.count_nonzero(outc[s]) == 0
            continue
        blk = xd[a:b]
        mx = blk.max(0).values
        assert torch.equal(outc[s].double(), mx), s                   # exact
        first = (blk == mx).to(torch.int64).argmax(0)                 # lowest row holding the maximum
        ref_gx[a + first, torch.arange(x.shape[1])] = gc[s]
    assert torch.equal(gxc, ref_gx)


@pytest.mark.parametrize("D", [1, 4, 255, 256, 257, 1000, 1027])
def test_segment_readouts(D):
    """ops.segment_reduce sum / mean / max over segments of 0, 1, 3, 128, 129, 512 and 20000 rows (256-column tiles: D = 255 / 256 / 257,
    1000, 1027).  Max runs on integer-valued inputs with ties everywhere: the forward equals the float64 max exactly and the backward sends
    every (segment, column) gradient to exactly one row, the lowest-index row holding the maximum (csrc/segment.hip, seg_stage1)."""
    from wsi_hgnn_amd import ops
    ranges = _seg_ranges(_SEG_COUNTS)
    n = ranges[-1][1]
    rp = ops.ReducePlan.from_ranges(ranges, _dev())
    g = torch.Generator().manual_seed(D)
    x = torch.randn(n, D, generator=g) * 3 + 1
    gout = torch.randn(len(ranges), D, generator=g)
    for op in ("sum", "mean"):
        xg = x.to(_dev()).requires_grad_()
        out = ops.segment_reduce(xg, rp, op)
        _poison_allocator()
        out.backward(gout.to(_dev()))
        _sumlike_check(out, xg.grad, x, gout, ranges, op)
    xm = _max_inputs(n, D, ranges, neg_segments={2, 4}, seed=D + 1)
    gm = torch.rand(len(ranges), D, generator=g) + 0.5             # nonzero: a misrouted gradient cannot hide as 0
    xg = xm.to(_dev()).requires_grad_()
    out = ops.segment_reduce(xg, rp, "max")
    out.backward(gm.to(_dev()))
    _max_check(out, xg.grad, xm, gm, ranges)


@pytest.mark.parametrize("op", ["sum", "mean", "max"])
def test_segment_readout_partial_plan(op):
    """A plan over rows [100, 600) of a 700-row x (the backward's covered = False path): rows outside the plan get exactly zero gradient."""
    from wsi_hgnn_amd import ops
    D = 130
    ranges = _seg_ranges([129, 0, 3, 368], first=100)
    assert ranges[-1][1] == 600
    rp = ops.ReducePlan.from_ranges(ranges, _dev())
    g = torch.Generator().manual_seed(17)
    if op == "max":
        x = _max_inputs(700, D, ranges, neg_segments={2}, seed=4)
        gout = torch.rand(len(ranges), D, generator=g) + 0.5
    else:
        x = torch.randn(700, D, generator=g)
        gout = torch.randn(len(ranges), D, generator=g)
    xg = x.to(_dev()).requires_grad_()
    out = ops.segment_reduce(xg, rp, op)
    _poison_allocator()
    out.backward(gout.to(_dev()))
    gx = xg.grad.cpu()
    assert torch.count_nonzero(gx[:100]) == 0 and torch.count_nonzero(gx[600:]) == 0
    local = [(a - 100, b - 100) for a, b in ranges]
    if op == "max":
        _max_check(out, gx[100:600], x[100:600], gout, local)
    else:
        _sumlike_check(out, gx[100:600], x[100:600], gout, local, op)


@pytest.mark.parametrize("D", [4, 256, 1000])
@pytest.mark.parametrize("layout", ["ldx", "offset"])
def test_segment_reduce_fwd_scalar_path(D, layout):
    """wsi_segment_reduce_fwd through the C-ABI on an x the 16-byte path cannot take although D is a multiple of 4: row stride
    D + 3, or rows that start one float past a 16-byte boundary (seg_stage1 with vec = false)."""
    from wsi_hgnn_amd import ops, _native as N
    lib = N.load()
    ranges = _seg_ranges([0, 1, 3, 129, 512, 2000])
    n = ranges[-1][1]
    rp = ops.ReducePlan.from_ranges(ranges, _dev())
    ldx, off = (D + 3, 0) if layout == "ldx" else (D, 1)
    g = torch.Generator().manual_seed(D + 7)
    buf = torch.randn(n * ldx + off, generator=g).to(_dev())
    xv = buf[off:].view(n, ldx)[:, :D]                              # the D columns the kernel reads
    if layout == "offset":
        assert (buf.data_ptr() + 4 * off) % 16 != 0
    xm = _max_inputs(n, D, ranges, neg_segments={3}, seed=D)
    for op, code in (("sum", N.WSI_RED_SUM), ("mean", N.WSI_RED_MEAN), ("max", N.WSI_RED_MAX)):
        if op == "max":
            xv.copy_(xm.to(_dev()))
        extra = 2 if op == "max" else 1
        partial = torch.empty(max(rp.num_chunks * D * extra, 1), device=_dev())
        out = torch.full((rp.num_segs, D), float("nan"), device=_dev())
        argmax = torch.empty(rp.num_segs, D, dtype=torch.int32, device=_dev()) if op == "max" else None
        N.check(lib.wsi_segment_reduce_fwd(N.ptr(buf, 4 * off), ldx, D, code, N.ptr(rp.chunk_row), rp.num_chunks, N.ptr(rp.seg_chunk),
                                           rp.num_segs, N.ptr(partial), N.ptr(out), D, N.ptr(argmax), N.stream()), "wsi_segment_reduce_fwd")
        xc = xv.cpu().double()
        oc = out.cpu().double()
        for s, (a, b) in enumerate(ranges):
            if op == "max":
                if b == a:
                    assert torch.count_nonzero(oc[s]) == 0 and torch.equal(argmax[s].cpu(), torch.full((D,), -1, dtype=torch.int32))
                    continue
                mx = xc[a:b].max(0).values
                first = (xc[a:b] == mx).to(torch.int64).argmax(0)
                assert torch.equal(oc[s], mx) and torch.equal(argmax[s].cpu().long(), a + first), (op, s)
            else:
                div = max(b - a, 1) if op == "mean" else 1
                ref = xc[a:b].sum(0) / div
                assert ((oc[s] - ref).abs() <= 1e-6 * xc[a:b].abs().sum(0) / div).all(), (op, s)
