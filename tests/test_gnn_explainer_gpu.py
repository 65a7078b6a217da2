"""GNNExplainer on the GPU against float64 restatements written here: the edge kernels with a per-edge message scale (GAT attention
with its scale gradient, the GraphConv aggregation with ``wsi_sddmm_dot``), the mask gradients of whole GCN / GAT models, and the
explainer's training loop against the same loop in float64 with torch's Adam.  One adversarial graph of 400 nodes: a self-loop on
every node, duplicate edges, a destination of in-degree 1, a destination of in-degree 300, a source whose only out-edge is its
self-loop, and a shuffled edge order (CSR order != edge order).  Tolerance (DESIGN): 1e-4 of the largest reference entry of each
tensor; the per-epoch loss is compared at 1e-4 relative."""
from math import sqrt

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = "cuda"
TOL = 1e-4
N_NODES, HUB, LONELY_DST, LONELY_SRC = 400, 0, 399, 398


def _close(got, ref, what):
    ref = ref.detach().to(torch.float64).cpu()
    got = got.detach().to(torch.float64).cpu()
    assert got.shape == ref.shape, f"{what}: shape {tuple(got.shape)} != {tuple(ref.shape)}"
    scale = max(float(ref.abs().max()), 1e-30)
    err = float((got - ref).abs().max())
    print(f"{what}: max error {err:.3e}, reference max {scale:.3e}")
    assert err <= TOL * scale, f"{what}: max error {err:.3e} > {TOL} x {scale:.3e}"


def make_graph(in_dim=24, seed=5):
    """The adversarial graph (CPU).  Node 0: in-degree 300 (299 sources + its self-loop); node 399: in-degree 1 (its self-loop only);
    node 398: no out-edge but its self-loop; 120 duplicated edges; the edge list is shuffled."""
    from wsi_hgnn_amd.graph import HeteroGraph
    gen = torch.Generator().manual_seed(seed)
    n = N_NODES
    s = torch.randint(1, LONELY_SRC, (2200,), generator=gen)             # sources in [1, 397]: never 398
    d = torch.randint(1, LONELY_DST, (2200,), generator=gen)             # destinations in [1, 398]: never 0 or 399
    loop = torch.arange(n)
    u = torch.cat([s, s[:120], torch.arange(1, 300), loop])
    v = torch.cat([d, d[:120], torch.full((299,), HUB), loop])
    o = torch.randperm(u.numel(), generator=gen)
    g = HeteroGraph.homogeneous(n, u[o], v[o], feat=torch.randn(n, in_dim, generator=gen))
    return g


def make_scale(E, seed):
    """Scales in (0, 1) with some entries forced to exactly 0 and exactly 1."""
    gen = torch.Generator().manual_seed(seed)
    s = torch.rand(E, generator=gen) * 0.98 + 0.01
    idx = torch.randperm(E, generator=gen)
    s[idx[:25]] = 0.0
    s[idx[25:50]] = 1.0
    return s


def _csr(plan):
    n = plan.num_nodes
    rowptr = plan.rowptr.long().cpu()
    src = plan.src.long().cpu()
    dst = torch.repeat_interleave(torch.arange(n), rowptr[1:n + 1] - rowptr[:n])
    return src, dst


@pytest.fixture(scope="module")
def graph():
    from wsi_hgnn_amd.models.GAT import gat_plan
    from wsi_hgnn_amd.models.GCN import homo_plan
    g = make_graph().to(DEV)
    p = gat_plan(g)
    indeg = (p.rowptr[1:] - p.rowptr[:-1]).cpu()
    outdeg = (p.colptr[1:] - p.colptr[:-1]).cpu()
    assert int(indeg[HUB]) == 300 and int(indeg[LONELY_DST]) == 1 and int(outdeg[LONELY_SRC]) == 1 and int(indeg.min()) >= 1
    assert not torch.equal(g._csr_perm().cpu(), torch.arange(g.num_edges()))
    return g, p, homo_plan(g)


# ------------------------------------------------------------------------------------------------ float64 restatements
def ref_attention(ft, al, ar, bias, escale, src, dst, n, slope, act, keep=None, keep_scale=1.0, pos=None):
    """DGL GATConv after fc with the explainer's message mask: el/er, leaky_relu, edge softmax over the in-edges, attn_drop as a
    replayed keep mask [E, H]; the message a_e ft[u] is multiplied by escale[e] AFTER the softmax; sum, bias, activation.
    ``pos`` (optional, [n, H*D] bool): the side of the activation's kink the GPU run took, replayed (see ``_kink``)."""
    H, D = al.shape[-2], al.shape[-1]
    f3 = ft.view(n, H, D)
    el = (f3 * al).sum(-1)
    er = (f3 * ar).sum(-1)
    s = F.leaky_relu(el[src] + er[dst], slope)
    m = torch.full((n, H), -float("inf"), dtype=s.dtype).scatter_reduce(0, dst[:, None].expand(-1, H), s, "amax")
    ex = torch.exp(s - m[dst])
    den = torch.zeros((n, H), dtype=s.dtype).index_add(0, dst, ex)
    a = ex / den[dst]
    if keep is not None:
        a = a * keep.to(a.dtype) * keep_scale
    msg = a[:, :, None] * f3[src]
    if escale is not None:
        msg = msg * escale[:, None, None]
    rst = torch.zeros((n, H, D), dtype=ft.dtype).index_add(0, dst, msg).reshape(n, H * D)
    if bias is not None:
        rst = rst + bias
    if act == "relu":
        rst = F.relu(rst)
    elif act == "leaky_relu":
        rst = torch.where(pos, rst, 0.01 * rst) if pos is not None else F.leaky_relu(rst, 0.01)
    return rst


def _kink(out):
    """Which side of relu's / leaky_relu's kink every output entry took on the GPU.  That is decided in fp32: an entry within fp32
    resolution of 0 (1e-7 of its terms) may take the other side than in float64, and one such entry among the 800k of a [400, 2048]
    output moves the gradients through it by 0.99 |g| - thousands of tolerances - while the two forward values differ by nothing
    measurable.  The float64 references therefore replay the GPU run's decisions, as they replay dropout masks (and as
    tests/test_gat_gpu.py::_model_check does); everything else is compared as before."""
    return out.detach().cpu() > 0


def ref_aggregate(z, bias, escale, src, dst, n, relu, pos=None):
    """DGL GraphConv(norm='both') message passing with the message mask; the degree norms are those of the UNMASKED graph.
    ``pos``: the replayed side of the ReLU's kink (``_kink``), used only next to the kink."""
    one = torch.ones(src.numel(), dtype=z.dtype)
    indeg = torch.zeros(n, dtype=z.dtype).index_add(0, dst, one)
    outdeg = torch.zeros(n, dtype=z.dtype).index_add(0, src, one)
    in_norm, out_norm = indeg.clamp(min=1).pow(-0.5), outdeg.clamp(min=1).pow(-0.5)
    msg = z[src] * out_norm[src][:, None]
    if escale is not None:
        msg = msg * escale[:, None]
    y = torch.zeros((n, z.shape[1]), dtype=z.dtype).index_add(0, dst, msg) * in_norm[:, None]
    if bias is not None:
        y = y + bias
    if relu and pos is not None:
        # the replay decides only the entries that the forward comparison cannot tell from 0 (|y| within TOL of the largest entry, far
        # above fp32 rounding); everywhere else float64's own sign does, so an entry the kernel wrongly zeroes still shows in ``y``
        near = y.abs() <= TOL * y.abs().max()
        return torch.where(torch.where(near, pos, y > 0), y, torch.zeros_like(y))
    return F.relu(y) if relu else y


def ref_graph_conv(x, w, b, escale, src, dst, n, relu):
    if w.shape[0] > w.shape[1]:
        return ref_aggregate(x @ w, b, escale, src, dst, n, relu)
    y = ref_aggregate(x, None, escale, src, dst, n, False) @ w + b
    return F.relu(y) if relu else y


def _ref_pool(kind, h, gate=None):
    if kind == "mean":
        return h.mean(0, keepdim=True)
    w, b = gate
    a = torch.softmax(h @ w.t() + b, dim=0)
    return (h * a).sum(0, keepdim=True)


def ref_gcn(params, n_layers, pool, x, escale, src, dst):
    """models/GCN.py forward in eval mode on one graph; every GraphConv's messages are masked, the readouts are not."""
    h, outs, n = x, [], x.shape[0]
    for i in range(n_layers):
        gate = (params[f"pools.{i}.gate_nn.weight"], params[f"pools.{i}.gate_nn.bias"]) if pool == "att" else None
        outs.append(_ref_pool(pool, h, gate) @ params[f"linears_prediction.{i}.weight"].t() + params[f"linears_prediction.{i}.bias"])
        h = ref_graph_conv(h, params[f"layers.{i}.weight"], params[f"layers.{i}.bias"], escale, src, dst, n, True)
    gate = (params[f"pools.{n_layers}.gate_nn.weight"], params[f"pools.{n_layers}.gate_nn.bias"]) if pool == "att" else None
    outs.append(_ref_pool(pool, h, gate) @ params["classify.weight"].t() + params["classify.bias"])
    return torch.stack(outs).mean(0)


def ref_gat(params, n_layers, pool, x, escale, src, dst, slope=0.2):
    """models/GAT.py forward in eval mode on one graph (readout of every layer's INPUT; the last GATConv's output is unused)."""
    h, outs, n = x, [], x.shape[0]
    for i in range(n_layers + 1):
        outs.append(_ref_pool(pool, h) @ params[f"linears_prediction.{i}.weight"].t() + params[f"linears_prediction.{i}.bias"])
        if i < n_layers:
            ft = h @ params[f"layers.{i}.fc.weight"].t()
            h = ref_attention(ft, params[f"layers.{i}.attn_l"], params[f"layers.{i}.attn_r"], params[f"layers.{i}.bias"], escale, src, dst, n,
                              slope, "leaky_relu")
    return torch.stack(outs).mean(0)


EXPLAINER_PARAMS = {"edge_size": 0.005, "feat_size": 0.1, "edge_ent": 1.0, "feat_ent": 0.1, "eps": 1e-15}


def ref_explainer_loss(forward, feat, node_mask, edge_mask, csr_perm, pred, p=EXPLAINER_PARAMS):
    """explainers/gnn_explainer.py:84-101,173-175 for graph classification; ``edge_mask`` is in EDGE order, ``forward(h, scale_csr)``
    the model restatement."""
    h = feat * node_mask.sigmoid()[:, None]
    me, mn = edge_mask.sigmoid(), node_mask.sigmoid()
    logits = forward(h, me[csr_perm])
    ent = lambda m: (-m * torch.log(m + p["eps"]) - (1 - m) * torch.log(1 - m + p["eps"])).mean()
    return -logits.view(-1)[pred] + me.sum() * p["edge_size"] + p["edge_ent"] * ent(me) + mn.mean() * p["feat_size"] + p["feat_ent"] * ent(mn)


def ref_explainer_loop(forward, feat, node0, edge0, csr_perm, pred, epochs, lr, dtype=torch.float64):
    """The explainer's loop with torch's Adam in ``dtype`` from the given initial masks: (losses, gradients per epoch, final masks)."""
    node = node0.detach().clone().to(dtype).requires_grad_(True)
    edge = edge0.detach().clone().to(dtype).requires_grad_(True)
    opt = torch.optim.Adam([node, edge], lr=lr)
    losses, grads = [], []
    for _ in range(epochs):
        loss = ref_explainer_loss(forward, feat.to(dtype), node, edge, csr_perm, pred)
        opt.zero_grad()
        loss.backward()
        grads.append((node.grad.detach().clone(), edge.grad.detach().clone()))
        opt.step()
        losses.append(float(loss.detach()))
    return losses, grads, node.detach(), edge.detach()


def trusted_elements(grads):
    """Elements whose gradient, in EVERY epoch, is at least 1e-5 of that epoch's largest gradient magnitude of the same mask.  Adam's
    first steps move an element by lr * sign(g): an element whose gradient is rounding noise may go either way."""
    keep_n = torch.ones_like(grads[0][0], dtype=torch.bool)
    keep_e = torch.ones_like(grads[0][1], dtype=torch.bool)
    for gn, ge in grads:
        keep_n &= gn.abs() >= 1e-5 * gn.abs().max()
        keep_e &= ge.abs() >= 1e-5 * ge.abs().max()
    return keep_n, keep_e


def build_model(kind, in_dim, pool="mean", seed=11):
    from wsi_hgnn_amd import models
    torch.manual_seed(seed)
    if kind == "gcn":
        m = models.GCN(in_dim, 32, 2, 2, F.relu, 0.0, pool)
        with torch.no_grad():                                            # DGL zero-initialises the biases: make them count
            for l in m.layers:
                l.bias.normal_(0, 0.1)
    else:
        m = models.GAT(2, in_dim, 16, 2, [2, 2, 1], F.leaky_relu, 0.0, 0.0, 0.2, False, pool)
        with torch.no_grad():
            for l in m.layers:
                l.bias.normal_(0, 0.1)
    return m.eval()


def ref_forward_of(kind, m, pool, src, dst, dtype=torch.float64):
    params = {k: v.detach().cpu().to(dtype) for k, v in m.named_parameters()}
    if kind == "gcn":
        return lambda h, s: ref_gcn(params, 2, pool, h, s, src, dst)
    return lambda h, s: ref_gat(params, 2, pool, h, s, src, dst)


# ------------------------------------------------------------------------------------------------ 1-4: scaled GAT attention
def _inputs(n, H, D, peaked, seed):
    gen = torch.Generator().manual_seed(seed)
    ft = torch.randn(n, H * D, generator=gen)
    target = 30.0 if peaked else 1.0                                  # |el|, |er| ~ target
    al = torch.randn(1, H, D, generator=gen) * (target / D ** 0.5)
    ar = torch.randn(1, H, D, generator=gen) * (target / D ** 0.5)
    bias = torch.randn(H * D, generator=gen) * 0.1
    g = torch.randn(n, H * D, generator=gen)
    return ft, al, ar, bias, g


def _run_ours(ft, al, ar, bias, g, plan, act, scale=None, drop=None):
    from wsi_hgnn_amd import ops
    leaves = [t.to(DEV).requires_grad_(True) for t in (ft, al, ar, bias)]
    s = scale.to(DEV).requires_grad_(True) if scale is not None else None
    out = ops.gat_attention(*leaves, plan, 0.2, activation=act, attn_drop=drop, edge_scale=s)
    out.backward(g.to(DEV))
    torch.cuda.synchronize()
    return out.detach(), [t.grad for t in leaves] + ([s.grad] if s is not None else [])


def _run_ref(ft, al, ar, bias, g, plan, act, scale, keep=None, keep_scale=1.0, pos=None):
    src, dst = _csr(plan)
    leaves = [t.to(torch.float64).requires_grad_(True) for t in (ft, al, ar, bias, scale)]
    out = ref_attention(*leaves, src, dst, plan.num_nodes, 0.2, act, keep, keep_scale, pos)
    out.backward(g.to(torch.float64))
    return out.detach(), [t.grad for t in leaves]


GRADS = ("g_ft", "g_attn_l", "g_attn_r", "g_bias", "g_edge_scale")


@pytest.mark.parametrize("peaked", [False, True], ids=["normal", "peaked"])
@pytest.mark.parametrize("act", [None, "leaky_relu"], ids=["none", "leaky"])
@pytest.mark.parametrize("H,D", [(1, 2), (4, 8), (3, 40), (4, 512)])
def test_scaled_attention_matches_float64(graph, H, D, act, peaked):
    _, plan, _ = graph
    ft, al, ar, bias, g = _inputs(plan.num_nodes, H, D, peaked, seed=H * 1000 + D)
    scale = make_scale(plan.num_edges, seed=D)
    out, grads = _run_ours(ft, al, ar, bias, g, plan, act, scale)
    rout, rgrads = _run_ref(ft, al, ar, bias, g, plan, act, scale, pos=_kink(out) if act else None)
    _close(out, rout, "out")
    for name, a, b in zip(GRADS, grads, rgrads):
        _close(a, b, name)
    zero = scale == 0
    assert int(zero.sum()) == 25 and int((scale == 1).sum()) == 25
    assert float(rgrads[4][zero].abs().max()) > 0 and float(grads[4].cpu()[zero].abs().max()) > 0      # a scale of 0 still has a gradient


@pytest.mark.parametrize("H,D", [(4, 8), (4, 512)])
def test_scale_of_ones_is_the_unscaled_op_bit_for_bit(graph, H, D):
    _, plan, _ = graph
    ft, al, ar, bias, g = _inputs(plan.num_nodes, H, D, True, seed=21)
    ones = torch.ones(plan.num_edges)
    out0, grads0 = _run_ours(ft, al, ar, bias, g, plan, "leaky_relu")
    out1, grads1 = _run_ours(ft, al, ar, bias, g, plan, "leaky_relu", ones)
    assert torch.equal(out0, out1)
    for name, a, b in zip(GRADS, grads0, grads1):
        assert torch.equal(a, b), name
    _, rgrads = _run_ref(ft, al, ar, bias, g, plan, "leaky_relu", ones, pos=_kink(out1))
    _close(grads1[4], rgrads[4], "g_edge_scale")


def test_scaled_attention_is_bit_reproducible(graph):
    from wsi_hgnn_amd import ops
    _, plan, _ = graph
    ft, al, ar, bias, g = _inputs(plan.num_nodes, 4, 512, True, seed=9)
    scale = make_scale(plan.num_edges, seed=1)
    drop = ops.CounterDropout(0.2, 12345)
    a = _run_ours(ft, al, ar, bias, g, plan, "leaky_relu", scale, drop)
    b = _run_ours(ft, al, ar, bias, g, plan, "leaky_relu", scale, drop)
    assert torch.equal(a[0], b[0])
    for x, y in zip(a[1], b[1]):
        assert torch.equal(x, y)


def test_scaled_attention_with_attn_drop_replayed(graph):
    from wsi_hgnn_amd import ops
    _, plan, _ = graph
    H, D = 4, 8
    ft, al, ar, bias, g = _inputs(plan.num_nodes, H, D, False, seed=77)
    scale = make_scale(plan.num_edges, seed=2)
    drop = ops.CounterDropout(0.2, 4242)
    out, grads = _run_ours(ft, al, ar, bias, g, plan, "leaky_relu", scale, drop)
    keep = ops.dropout_keep_mask(drop, plan.num_edges, H)
    assert 0.7 < float(keep.float().mean()) < 0.9
    rout, rgrads = _run_ref(ft, al, ar, bias, g, plan, "leaky_relu", scale, keep, drop.scale, pos=_kink(out))
    _close(out, rout, "out")
    for name, a, b in zip(GRADS, grads, rgrads):
        _close(a, b, name)


# ------------------------------------------------------------------------------------------------ 5: GraphConv with a scale
@pytest.mark.parametrize("relu", [False, True], ids=["linear", "relu"])
@pytest.mark.parametrize("with_bias", [False, True], ids=["nobias", "bias"])
@pytest.mark.parametrize("D", [1, 3, 64, 512, 1000])
def test_scaled_aggregate_matches_float64(graph, D, with_bias, relu):
    from wsi_hgnn_amd import ops
    _, plan, hp = graph
    n, E = plan.num_nodes, plan.num_edges
    gen = torch.Generator().manual_seed(D)
    z, g = torch.randn(n, D, generator=gen), torch.randn(n, D, generator=gen)
    bias = torch.randn(D, generator=gen) * 0.1 if with_bias else None
    scale = make_scale(E, seed=D + 1)
    leaves = [t.to(DEV).requires_grad_(True) if t is not None else None for t in (z, bias, scale)]
    y = ops.graph_conv_aggregate(leaves[0], leaves[1], hp, relu, edge_scale=leaves[2])
    y.backward(g.to(DEV))
    src, dst = _csr(plan)
    rl = [t.to(torch.float64).requires_grad_(True) if t is not None else None for t in (z, bias, scale)]
    ry = ref_aggregate(rl[0], rl[1], rl[2], src, dst, n, relu, pos=_kink(y))
    ry.backward(g.to(torch.float64))
    _close(y, ry, "y")
    for name, a, b in zip(("g_z", "g_bias", "g_edge_scale"), leaves, rl):
        if a is not None:
            _close(a.grad, b.grad, name)
    assert float(leaves[2].grad.cpu()[scale == 0].abs().max()) > 0


@pytest.mark.parametrize("fin,fout", [(48, 32), (24, 32), (32, 32)], ids=["project-first", "aggregate-first", "square"])
def test_graph_conv_under_message_scale(graph, fin, fout):
    from wsi_hgnn_amd import graph as G
    from wsi_hgnn_amd.models.GCN import GraphConv
    g, plan, _ = graph
    n, E = plan.num_nodes, plan.num_edges
    torch.manual_seed(fin)
    conv = GraphConv(fin, fout, activation=F.relu).to(DEV)
    with torch.no_grad():
        conv.bias.normal_(0, 0.1)
    x = torch.randn(n, fin)
    go = torch.randn(n, fout)
    scale = make_scale(E, seed=fin)                                   # EDGE order here: message_scale permutes it
    xd, sd = x.to(DEV).requires_grad_(True), scale.to(DEV).requires_grad_(True)
    with G.message_scale(g, sd):
        y = conv(g, xd)
    y.backward(go.to(DEV))
    src, dst = _csr(plan)
    perm = g._csr_perm().cpu()
    rl = [t.detach().cpu().to(torch.float64).requires_grad_(True) for t in (x, conv.weight, conv.bias, scale)]
    ry = ref_graph_conv(rl[0], rl[1], rl[2], rl[3][perm], src, dst, n, True)
    ry.backward(go.to(torch.float64))
    _close(y, ry, "y")
    for name, a, b in zip(("g_x", "g_weight", "g_bias", "g_edge_scale"), (xd.grad, conv.weight.grad, conv.bias.grad, sd.grad), rl):
        _close(a, b.grad, name)


def test_sddmm_dot_direct_with_relu_ref(graph):
    from wsi_hgnn_amd import _native as N
    _, plan, hp = graph
    n, E, D = plan.num_nodes, plan.num_edges, 40
    gen = torch.Generator().manual_seed(8)
    g, x, ref = (torch.randn(n, D, generator=gen) for _ in range(3))
    gw = torch.full((E,), float("nan"), device=DEV)
    gd, xd, rd = g.to(DEV), x.to(DEV), ref.to(DEV)
    N.check(N.load().wsi_sddmm_dot(N.ptr(gd), D, N.ptr(xd), D, n, D, N.ptr(hp.rowptr), N.ptr(hp.src), N.ptr(hp.out_norm), N.ptr(hp.in_norm),
                                   N.ptr(rd), D, N.ptr(gw), N.stream()), "wsi_sddmm_dot")
    torch.cuda.synchronize()
    src, dst = _csr(plan)
    gm = (g * (ref > 0)).double()
    want = hp.in_norm.cpu().double()[dst] * hp.out_norm.cpu().double()[src] * (gm[dst] * x.double()[src]).sum(1)
    _close(gw, want, "g_w")


# ------------------------------------------------------------------------------------------------ 6: whole-model mask gradients
MODELS = [("gcn", "mean"), ("gcn", "att"), ("gat", "mean")]


@pytest.mark.parametrize("kind,pool", MODELS, ids=[f"{k}-{p}" for k, p in MODELS])
def test_whole_model_mask_gradients(graph, kind, pool):
    from wsi_hgnn_amd import graph as G
    from wsi_hgnn_amd.explainers.gnn_explainer import mask_loss
    g, plan, _ = graph
    n, E = plan.num_nodes, plan.num_edges
    m = build_model(kind, 24, pool).to(DEV)
    gen = torch.Generator().manual_seed(4)
    node0 = torch.randn(n, generator=gen)
    edge0 = torch.randn(E, generator=gen)
    edge0[:4] = torch.tensor([30.0, -30.0, 0.0, 120.0])               # saturated masks: sigmoid = 1 - 1e-13, 1e-13, 0.5 and exactly 1
    feat = g.ndata["feat"]
    with torch.no_grad():
        pred = m(g).argmax(dim=-1)
    node, edge = node0.to(DEV).requires_grad_(True), edge0.to(DEV).requires_grad_(True)
    with G.message_scale(g, edge.sigmoid()):
        logits = m(g, feat * node.sigmoid()[:, None])
    loss = mask_loss(-logits.view(-1)[pred], edge.sigmoid(), node.sigmoid(), EXPLAINER_PARAMS)
    loss.backward()
    src, dst = _csr(plan)
    rn, re = node0.double().requires_grad_(True), edge0.double().requires_grad_(True)
    rloss = ref_explainer_loss(ref_forward_of(kind, m, pool, src, dst), feat.cpu().double(), rn, re, g._csr_perm().cpu(), pred.cpu())
    rloss.backward()
    assert abs(float(loss.detach()) - float(rloss.detach())) <= TOL * abs(float(rloss.detach()))
    _close(node.grad, rn.grad, "d loss / d node_mask")
    _close(edge.grad, re.grad, "d loss / d edge_mask")


# ------------------------------------------------------------------------------------------------ 7: the explainer loop
LOOP_SEED, LOOP_EPOCHS, LOOP_LR = 3, 5, 0.01


def initial_masks(n, E, seed):
    torch.manual_seed(seed)
    node = torch.randn(n) * 0.1
    edge = torch.randn(E) * (torch.nn.init.calculate_gain("relu") * sqrt(2.0 / (2 * n)))
    return node, edge


@pytest.mark.parametrize("kind", ["gcn", "gat"])
def test_explainer_loop_matches_float64_adam(graph, kind, capsys):
    from wsi_hgnn_amd.explainers import GNNExplainer, ExplainerTags
    g, plan, _ = graph
    n, E = plan.num_nodes, plan.num_edges
    m = build_model(kind, 24, "mean").to(DEV)
    before = {k: v.detach().clone() for k, v in m.state_dict().items()}
    ex = GNNExplainer(g, m, num_hops=2, epochs=LOOP_EPOCHS)
    torch.manual_seed(LOOP_SEED)
    subgraph, node_mask = ex.explain_node(node_idx=None)
    torch.cuda.synchronize()
    # the float64 restatement from the same initial masks
    node0, edge0 = initial_masks(n, E, LOOP_SEED)
    with torch.no_grad():
        pred = m(g).argmax(dim=-1).cpu()
    src, dst = _csr(plan)
    losses, grads, rnode, redge = ref_explainer_loop(ref_forward_of(kind, m, "mean", src, dst), g.ndata["feat"].cpu(), node0, edge0,
                                                     g._csr_perm().cpu(), pred, LOOP_EPOCHS, LOOP_LR)
    assert len(ex.history) == LOOP_EPOCHS and all(isinstance(x, float) for x in ex.history)
    for i, (a, b) in enumerate(zip(ex.history, losses)):
        print(f"epoch {i}: loss {a:.7f}, float64 {b:.7f}")
        assert abs(a - b) <= 1e-4 * abs(b), f"epoch {i}: loss {a} != {b}"
    keep_n, keep_e = trusted_elements(grads)
    excluded = int((~keep_n).sum()) + int((~keep_e).sum())
    print(f"excluded {excluded} of {n + E} mask elements")
    assert excluded <= 0.02 * (n + E)
    assert isinstance(node_mask, np.ndarray) and node_mask.shape == (n,)
    edge_mask = subgraph.edata[ExplainerTags.EDGE_MASK].detach().cpu()
    assert edge_mask.shape == (E,)
    _close(torch.from_numpy(node_mask)[keep_n], rnode.sigmoid()[keep_n], "sigmoid(node_mask)")
    _close(edge_mask[keep_e], redge[keep_e], "edge_mask")
    assert torch.equal(subgraph.ndata[ExplainerTags.ORIGINAL_ID].cpu(), torch.arange(n, dtype=torch.int))
    assert ExplainerTags.EDGE_MASK not in g.edata and ExplainerTags.ORIGINAL_ID not in g.ndata
    # the model is untouched: same parameters, still trainable, no gradient left behind
    for k, v in m.state_dict().items():
        assert torch.equal(v, before[k]), k
    assert all(p.grad is None and p.requires_grad for p in m.parameters())
    # the report runs on what explain_node returned: the all-ones mask leaves the original prediction
    capsys.readouterr()
    assert ex.test_explanation(None, subgraph, np.ones(n, dtype=np.float32)) is None
    report = capsys.readouterr().out
    assert f"{n} nodes, {E} edges" in report and f"{n} entries, total weight {n}" in report
    labels = [line.split(": ", 1)[1] for line in report.splitlines() if line.lstrip().startswith("label,")]
    assert len(labels) == 2 and labels[0] == labels[1] == str(pred.tolist())


# ------------------------------------------------------------------------------------------------ 8: nothing changes without an attachment
@pytest.mark.parametrize("kind", ["gcn", "gat"])
def test_models_without_an_attachment_are_untouched(graph, kind):
    from wsi_hgnn_amd import graph as G
    g, plan, _ = graph
    m = build_model(kind, 24, "mean").to(DEV)

    def run():
        m.zero_grad(set_to_none=True)
        x = g.ndata["feat"].clone().requires_grad_(True)
        out = m(g, x)
        out.sum().backward()
        torch.cuda.synchronize()
        return out.detach(), x.grad, [p.grad.clone() for p in m.parameters() if p.grad is not None]

    a = run()
    with G.message_scale(g, torch.full((plan.num_edges,), 0.5, device=DEV)):
        inside = m(g).detach()
    b = run()
    assert not torch.equal(a[0], inside)                               # the block did scale the messages
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert len(a[2]) == len(b[2]) > 0
    for x, y in zip(a[2], b[2]):
        assert torch.equal(x, y)
