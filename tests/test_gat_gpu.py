"""GAT on the GPU against a float64 restatement of DGL's GATConv (written here from DGL's documented semantics): the edge kernels
(forward and every gradient) on graphs with several members, duplicate edges, a destination of in-degree >= 4096, peaked scores
and self-loop-only members; zero in-degree refused; bit-reproducibility; attn_drop / feat_drop replayed from the counter-based
mask; the whole model at the GAT_Kimia_v2 shape under every GEMM mode; all four readouts.  Tolerance (DESIGN): 1e-4 of the
largest reference entry of each tensor."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = "cuda"
TOL = 1e-4


def _close(got, ref, what):
    ref = ref.detach().to(torch.float64).cpu()
    got = got.detach().to(torch.float64).cpu()
    scale = max(float(ref.abs().max()), 1e-30)
    err = float((got - ref).abs().max())
    assert err <= TOL * scale, f"{what}: max error {err:.3e} > {TOL} x {scale:.3e}"


def _graph(n, src, dst):
    from wsi_hgnn_amd.graph import HeteroGraph
    return HeteroGraph.homogeneous(n, torch.as_tensor(src, dtype=torch.int64), torch.as_tensor(dst, dtype=torch.int64))


def _edge_batch(seed=5):
    """Three graphs in one batch: random edges with duplicates + self loops; a hub whose in-degree is 4200; self loops only."""
    import wsi_hgnn_amd as W
    gen = torch.Generator().manual_seed(seed)
    n1 = 300
    s1 = torch.randint(0, n1, (2400,), generator=gen)
    d1 = torch.randint(0, n1, (2400,), generator=gen)
    s1 = torch.cat([s1, s1[:200], torch.arange(n1)])                 # 200 duplicated edges, then the self loops
    d1 = torch.cat([d1, d1[:200], torch.arange(n1)])
    n2 = 4300
    s2 = torch.cat([torch.arange(1, 4201), torch.arange(n2), torch.randint(0, n2, (3000,), generator=gen)])
    d2 = torch.cat([torch.zeros(4200, dtype=torch.int64), torch.arange(n2), torch.randint(0, n2, (3000,), generator=gen)])
    n3 = 50
    g = W.batch([_graph(n1, s1, d1), _graph(n2, s2, d2), _graph(n3, torch.arange(n3), torch.arange(n3))])
    return g.to(DEV)


def _csr(plan):
    n = plan.num_nodes
    rowptr = plan.rowptr.long().cpu()
    src = plan.src.long().cpu()
    dst = torch.repeat_interleave(torch.arange(n), rowptr[1:] - rowptr[:-1])
    return src, dst


def ref_attention(ft, al, ar, bias, src, dst, n, slope, act, keep=None, scale=1.0, pos=None, terms=None):
    """float64 DGL GATConv after fc: el/er, leaky_relu, edge softmax over in-edges (max-subtracted, no epsilon), attn_drop as a
    replayed keep mask [E, H] (CSR order), weighted sum, bias, activation."""
    H, D = al.shape[-2], al.shape[-1]
    f3 = ft.view(n, H, D)
    el = (f3 * al).sum(-1)
    er = (f3 * ar).sum(-1)
    if terms is not None:                                            # (el, er, ft) for the rounding bound of the attention-vector gradients
        el.retain_grad()
        er.retain_grad()
        terms.append((el, er, f3.detach()))
    s = F.leaky_relu(el[src] + er[dst], slope)
    m = torch.full((n, H), -float("inf"), dtype=s.dtype).scatter_reduce(0, dst[:, None].expand(-1, H), s, "amax")
    ex = torch.exp(s - m[dst])
    den = torch.zeros((n, H), dtype=s.dtype).index_add(0, dst, ex)
    a = ex / den[dst]
    if keep is not None:
        a = a * keep.to(a.dtype) * scale
    rst = torch.zeros((n, H, D), dtype=ft.dtype).index_add(0, dst, a[:, :, None] * f3[src]).reshape(n, H * D)
    if bias is not None:
        rst = rst + bias
    if act == "relu" and pos is not None:
        rst = torch.where(pos, rst, torch.zeros_like(rst))
    elif act == "relu":
        rst = F.relu(rst)
    elif act == "leaky_relu" and pos is not None:                    # the side of the kink the GPU run took, replayed (see _model_check)
        rst = torch.where(pos, rst, 0.01 * rst)
    elif act == "leaky_relu":
        rst = F.leaky_relu(rst, 0.01)
    return rst


def _inputs(n, H, D, peaked, seed):
    gen = torch.Generator().manual_seed(seed)
    ft = torch.randn(n, H * D, generator=gen)
    al = torch.randn(1, H, D, generator=gen)
    ar = torch.randn(1, H, D, generator=gen)
    target = 30.0 if peaked else 1.0                                  # |el|, |er| ~ target
    al = al * (target / D ** 0.5)
    ar = ar * (target / D ** 0.5)
    bias = torch.randn(H * D, generator=gen) * 0.1
    g = torch.randn(n, H * D, generator=gen)
    return ft, al, ar, bias, g


def _run_ours(ft, al, ar, bias, g, plan, slope, act, drop=None):
    from wsi_hgnn_amd import ops
    leaves = [t.to(DEV).requires_grad_(True) for t in (ft, al, ar, bias)]
    out = ops.gat_attention(*leaves, plan, slope, activation=act, attn_drop=drop)
    out.backward(g.to(DEV))
    torch.cuda.synchronize()
    return out.detach(), [t.grad for t in leaves]


def _run_ref(ft, al, ar, bias, g, plan, slope, act, keep=None, scale=1.0):
    src, dst = _csr(plan)
    leaves = [t.to(torch.float64).requires_grad_(True) for t in (ft, al, ar, bias)]
    out = ref_attention(*leaves, src, dst, plan.num_nodes, slope, act, keep, scale)
    out.backward(g.to(torch.float64))
    return out.detach(), [t.grad for t in leaves]


@pytest.fixture(scope="module")
def edge_graph():
    from wsi_hgnn_amd.models.GAT import gat_plan
    g = _edge_batch()
    p = gat_plan(g)
    indeg = (p.rowptr[1:] - p.rowptr[:-1]).cpu()
    assert int(indeg.max()) >= 4096 and int(indeg.min()) >= 1
    return g, p


@pytest.mark.parametrize("peaked", [False, True], ids=["normal", "peaked"])
@pytest.mark.parametrize("act", [None, "leaky_relu"], ids=["none", "leaky"])
@pytest.mark.parametrize("H,D", [(1, 2), (4, 8), (4, 512), (3, 40)])
def test_attention_matches_float64(edge_graph, H, D, act, peaked):
    _, plan = edge_graph
    ft, al, ar, bias, g = _inputs(plan.num_nodes, H, D, peaked, seed=H * 1000 + D)
    out, grads = _run_ours(ft, al, ar, bias, g, plan, 0.2, act)
    rout, rgrads = _run_ref(ft, al, ar, bias, g, plan, 0.2, act)
    _close(out, rout, "out")
    for name, a, b in zip(("g_ft", "g_attn_l", "g_attn_r", "g_bias"), grads, rgrads):
        _close(a, b, name)


def test_relu_and_no_bias(edge_graph):
    from wsi_hgnn_amd import ops
    _, plan = edge_graph
    ft, al, ar, _, g = _inputs(plan.num_nodes, 2, 24, False, seed=3)
    leaves = [t.to(DEV).requires_grad_(True) for t in (ft, al, ar)]
    out = ops.gat_attention(*leaves, None, plan, 0.2, activation="relu")
    out.backward(g.to(DEV))
    rl = [t.to(torch.float64).requires_grad_(True) for t in (ft, al, ar)]
    src, dst = _csr(plan)
    rout = ref_attention(*rl, None, src, dst, plan.num_nodes, 0.2, "relu")
    rout.backward(g.to(torch.float64))
    _close(out, rout, "out")
    for a, b in zip(leaves, rl):
        _close(a.grad, b.grad, "grad")


def test_zero_in_degree_is_rejected():
    from wsi_hgnn_amd.models.GAT import GATConv
    g = _graph(4, [0, 1, 2], [1, 2, 3]).to(DEV)                    # node 0 has no in-edge
    conv = GATConv(8, 4, 2).to(DEV)
    with pytest.raises(ValueError, match="zero in-degree"):
        conv(g, torch.randn(4, 8, device=DEV))


def test_bit_reproducible(edge_graph):
    from wsi_hgnn_amd import ops
    _, plan = edge_graph
    ft, al, ar, bias, g = _inputs(plan.num_nodes, 4, 512, True, seed=9)
    drop = ops.CounterDropout(0.2, 12345)
    a = _run_ours(ft, al, ar, bias, g, plan, 0.2, "leaky_relu", drop)
    b = _run_ours(ft, al, ar, bias, g, plan, 0.2, "leaky_relu", drop)
    assert torch.equal(a[0], b[0])
    for x, y in zip(a[1], b[1]):
        assert torch.equal(x, y)


@pytest.mark.parametrize("H,D", [(4, 8), (4, 512)])
def test_attn_drop_replayed_into_float64(edge_graph, H, D):
    from wsi_hgnn_amd import ops
    _, plan = edge_graph
    ft, al, ar, bias, g = _inputs(plan.num_nodes, H, D, False, seed=77)
    drop = ops.CounterDropout(0.2, 4242)
    out, grads = _run_ours(ft, al, ar, bias, g, plan, 0.2, "leaky_relu", drop)
    keep = ops.dropout_keep_mask(drop, plan.num_edges, H)
    rout, rgrads = _run_ref(ft, al, ar, bias, g, plan, 0.2, "leaky_relu", keep, drop.scale)
    _close(out, rout, "out")
    for name, a, b in zip(("g_ft", "g_attn_l", "g_attn_r", "g_bias"), grads, rgrads):
        _close(a, b, name)
    # the kept fraction of the [E, H] draw lies within binomial bounds (6 sigma), and a new seed draws a new mask
    m = keep.numel()
    frac = float(keep.float().mean())
    assert abs(frac - (1 - drop.threshold / 65536)) < 6 * (0.2 * 0.8 / m) ** 0.5
    out2, _ = _run_ours(ft, al, ar, bias, g, plan, 0.2, "leaky_relu", ops.CounterDropout(0.2, 4243))
    assert not torch.equal(out, out2)
    assert not torch.equal(keep, ops.dropout_keep_mask(ops.CounterDropout(0.2, 4243), plan.num_edges, H))


def test_feat_drop_replayed():
    from wsi_hgnn_amd import ops
    x = torch.randn(3000, 1024, device=DEV, requires_grad=True)
    drop = ops.CounterDropout(0.2, 99)
    y = ops.counter_dropout(x, drop)
    g = torch.randn_like(y)
    y.backward(g)
    keep = ops.dropout_keep_mask(drop, 3000, 1024, device=DEV)
    ref = x.detach() * keep * drop.scale
    assert float((y - ref).abs().max()) <= TOL * float(ref.abs().max())
    assert float((x.grad - g * keep * drop.scale).abs().max()) <= TOL * float(g.abs().max()) * drop.scale
    frac = float((y != 0).float().mean())
    assert abs(frac - 0.8) < 6 * (0.16 / y.numel()) ** 0.5
    y2 = ops.counter_dropout(x.detach(), ops.CounterDropout(0.2, 100))
    assert not torch.equal(y2 != 0, y != 0)


# ---------------------------------------------------------------------------------------------------- whole model
def _ref_pool(kind, h, gid, B, gate=None):
    if kind == "sum":
        return torch.zeros(B, h.shape[1], dtype=h.dtype).index_add(0, gid, h)
    if kind == "mean":
        cnt = torch.zeros(B, dtype=h.dtype).index_add(0, gid, torch.ones_like(h[:, 0]))
        return torch.zeros(B, h.shape[1], dtype=h.dtype).index_add(0, gid, h) / cnt[:, None]
    if kind == "max":
        return torch.full((B, h.shape[1]), -float("inf"), dtype=h.dtype).scatter_reduce(0, gid[:, None].expand_as(h), h, "amax")
    w, b = gate
    z = h @ w.t() + b                                                 # [N, 1]
    m = torch.full((B, 1), -float("inf"), dtype=h.dtype).scatter_reduce(0, gid[:, None], z, "amax")
    ex = torch.exp(z - m[gid])
    den = torch.zeros((B, 1), dtype=h.dtype).index_add(0, gid, ex)
    return torch.zeros(B, h.shape[1], dtype=h.dtype).index_add(0, gid, h * (ex / den[gid]))


def ref_gat_model(params, n_layers, heads, hidden, pool, x, src, dst, gid, B, slope=0.2, signs=None, terms=None):
    """float64 models/GAT.py forward (eval mode): readout of every layer's INPUT, the last GATConv's output unused."""
    h = x
    outs = []
    n = x.shape[0]
    for i in range(n_layers + 1):
        gate = (params[f"pools.{i}.gate_nn.weight"], params[f"pools.{i}.gate_nn.bias"]) if pool == "att" else None
        p = _ref_pool(pool, h, gid, B, gate)
        outs.append(p @ params[f"linears_prediction.{i}.weight"].t() + params[f"linears_prediction.{i}.bias"])
        if i < n_layers:
            ft = h @ params[f"layers.{i}.fc.weight"].t()
            h = ref_attention(ft, params[f"layers.{i}.attn_l"], params[f"layers.{i}.attn_r"], params[f"layers.{i}.bias"], src, dst, n,
                              slope, "leaky_relu", pos=signs[i] if signs else None, terms=terms)
    return torch.stack(outs).mean(0)


def _model_check(m, g, labels, pool, n_layers, heads, hidden):
    from wsi_hgnn_amd.models.GAT import gat_plan
    gd = g.to(DEV)
    m.zero_grad(set_to_none=True)
    # Which side of the leaky_relu kink an entry takes is decided in fp32: an entry within fp32 resolution of 0 may take the other side
    # than in float64, and each such entry moves a bias gradient (a sum over ALL nodes) by 0.99 |g| - at 8M entries several do.  The
    # reference therefore replays the GPU run's decisions (the sign of every hidden layer's output), as it replays dropout masks; the
    # forward values of the two sides differ by 0.99 |z| there, i.e. by nothing measurable.
    signs = []
    hooks = [l.register_forward_hook(lambda mod, inp, out: signs.append(out.detach().flatten(1).cpu() > 0)) for l in m.layers[:n_layers]]
    logits = m(gd)
    for hk in hooks:
        hk.remove()
    loss = F.cross_entropy(logits, labels.to(DEV))
    loss.backward()
    torch.cuda.synchronize()
    plan = gat_plan(gd)
    src, dst = _csr(plan)
    bnn = g.batch_num_nodes(g.ntypes[0])
    gid = torch.repeat_interleave(torch.arange(len(bnn)), bnn)
    params = {k: v.detach().cpu().to(torch.float64).requires_grad_(True) for k, v in m.named_parameters()}
    x = g.ndata["feat"].to(torch.float64)
    terms = []
    rl = ref_gat_model(params, n_layers, heads, hidden, pool, x, src, dst, gid, len(bnn), signs=signs, terms=terms)
    rloss = F.cross_entropy(rl, labels)
    rloss.backward()
    assert float((logits.detach().cpu().double() - rl.detach()).abs().max()) < 1e-4
    assert abs(loss.item() - rloss.item()) < 1e-4
    dead = set(m.dead_parameter_names())
    largest = max(float(p.grad.abs().max()) for p in params.values() if p.grad is not None)
    for k, p in m.named_parameters():
        if k in dead:
            assert p.grad is None, k
            continue
        ref = params[k].grad
        assert p.grad is not None and ref is not None, k
        # the readout gate's bias has an exact gradient of ZERO (the softmax over a graph's nodes ignores a shift): float64 leaves
        # 1e-19 there, fp32 the rounding of a cancelling sum, ~1e-9 of the model's largest gradient
        allow = TOL * float(ref.abs().max()) if float(ref.abs().max()) > 1e-12 * largest else 1e-8 * largest
        err = (p.grad.detach().double().cpu() - ref).abs()
        if k.startswith("layers.") and k.endswith(("attn_l", "attn_r")):
            # g_attn[h, d] = sum over nodes of g_el[u, h] ft[u, h, d]: at the model's shape a sum of terms that cancel to ~1e-3 of their
            # absolute sum (the softmax gradient a (g_a - delta) of similar rows).  Its fp32 rounding bound is added: 1e-5 of the
            # absolute sum of the terms (eps 6e-8 x a random walk over thousands of terms)
            el, er, f3 = terms[int(k.split(".")[1])]
            gs = (el if k.endswith("attn_l") else er).grad.abs()
            err = err - 1e-5 * (gs[:, :, None] * f3.abs()).sum(0, keepdim=True)
        err = float(err.max())
        assert err <= allow, f"{k}: error {err:.3e} > {allow:.3e}"


def test_model_at_gat_kimia_v2_shape(gemm_mode):
    import wsi_hgnn_amd as W
    from wsi_hgnn_amd import models, synthetic
    torch.manual_seed(1)
    m = models.GAT(2, 1024, 512, 2, [4, 4, 1], F.leaky_relu, 0.2, 0.2, 0.2, False, "mean").to(DEV).eval()
    g = W.batch([synthetic.homogeneous_graph(n, 1024, seed=20 + n) for n in (2000, 3000, 2500)])
    _model_check(m, g, torch.tensor([0, 1, 1]), "mean", 2, [4, 4, 1], 512)


@pytest.mark.parametrize("pool", ["sum", "mean", "max", "att"])
def test_poolings(pool):
    import wsi_hgnn_amd as W
    from wsi_hgnn_amd import models, synthetic
    torch.manual_seed(2)
    m = models.GAT(2, 32, 8, 3, [4, 4, 1], F.leaky_relu, 0.0, 0.0, 0.2, False, pool).to(DEV)
    g = W.batch([synthetic.homogeneous_graph(n, 32, seed=n) for n in (300, 500)])
    _model_check(m, g, torch.tensor([0, 2]), pool, 2, [4, 4, 1], 8)
