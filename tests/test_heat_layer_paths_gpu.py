"""The branches of ops._HeatLayerFused that no model-level test reaches, each through ops.heat_layer_fused directly on one small synthetic
batch: output and EVERY gradient against the composed statement of the same arithmetic (ops.grouped_linear -> ops.heat_attention ->
ops.grouped_linear -> torch.lerp by the gate, then ops.segment_reduce where a readout is involved).

  - a readout of more than 8192 segments: the pooled backward without wsi_pool_bwd_prep (tensor form of the gradient factors, the skip-gate
    gradient through the segment -> gate matrix, 1 - sigmoid(skip) per type through the type -> gate matrix), with and without the V collapse;
  - the dropout mask as a tensor (the model passes a CounterDropout), with a node type that no relation enters;
  - a width that is no multiple of 32: one dX launch per column block of K | Q | V instead of the chunked one;
  - a readout plan whose segments straddle a node-type boundary: refused.

Low-rank readout gradients off and exact-fp32 GEMMs, so both forms run the same arithmetic in a different summation order.  Bounds: those of
test_kernels_gpu.py::test_readout_shortcuts_equal_the_full_depth_path, which compares the same kinds of forms - 2e-5 of the largest value on
outputs; on a gradient 2e-5 of its largest value + 1e-8 (1e-4 + 1e-6 under a sum readout).  Every figure is printed before it is checked."""
import pytest
import torch

pytestmark = pytest.mark.gpu

ND3 = {"0": 0, "1": 1, "2": 2}
# the synthetic schema without its two relations into node type 2: that type is passed through
NO_RELATION_INTO_2 = [("0", "pos", "0"), ("1", "pos", "0"), ("0", "pos", "1"), ("2", "neg", "1")]


def _dev():
    return torch.device("cuda:0")


def _synthetic(nodes, relations=None, fractions=(0.5, 0.3, 0.2), seed=7):
    from wsi_hgnn_amd import synthetic
    return [synthetic.hetero_graph(n, 8, seed=seed + i, dst_mode="hub", relations=relations, fractions=fractions) for i, n in enumerate(nodes)]


def _block_diagonal_graph(graphs, per, fan=4, seed=7):
    """A block-diagonal batch of ``graphs`` small graphs written as one graph: 3 node types, ``per`` nodes of each type in every small graph
    (rows [g * per, (g + 1) * per) of the type), and into every node ``fan`` edges per relation from random nodes of the SAME small graph."""
    from collections import OrderedDict
    from wsi_hgnn_amd import synthetic
    from wsi_hgnn_amd.graph import HeteroGraph
    gen = torch.Generator().manual_seed(seed)
    rows = graphs * per
    dst = torch.arange(rows, dtype=torch.int64).repeat(fan)
    edges, sim = OrderedDict(), {}
    for (s, e, d) in synthetic.HEAT_RELATIONS:
        src = (dst // per) * per + torch.randint(0, per, (rows * fan,), generator=gen, dtype=torch.int64)
        edges[(s, e, d)] = (src, dst.clone())
        mag = torch.rand(rows * fan, generator=gen, dtype=torch.float32)
        sim[(s, e, d)] = mag if e == "pos" else -mag
    counts = OrderedDict((str(t), rows) for t in range(3))
    return HeteroGraph.from_coo(counts, edges, feat={t: torch.zeros(rows, 8) for t in counts}, sim=sim)


def _case(graphs, D, H, seed=7):
    """(layer, ctx, h0, G): a HEATLayer's parameters, the context of one batch, an input table, and the batch (the context holds it weakly)."""
    import wsi_hgnn_amd as W
    from wsi_hgnn_amd.models.heat_layer import HEATLayer, heat_context
    torch.manual_seed(seed)
    layer = HEATLayer(D, D, ND3, H, dropout=0.0).to(_dev())
    with torch.no_grad():
        layer.skip.copy_(torch.tensor([0.3, 1.0, -0.7]))
    G = W.batch(graphs).to(_dev())
    ctx = heat_context(G, ND3, D, _dev())
    h0 = torch.randn(G.num_nodes(), D, device=_dev())
    return layer, ctx, h0, G


def _fused(layer, ctx, h, H, mask, pool):
    from wsi_hgnn_amd import ops
    params = []
    for nid in ctx.nid:
        params += [layer.k_linears[nid].weight, layer.q_linears[nid].weight, layer.v_linears[nid].weight, layer.a_linears[nid].weight,
                   layer.k_linears[nid].bias, layer.q_linears[nid].bias, layer.v_linears[nid].bias, layer.a_linears[nid].bias]
    return ops.heat_layer_fused(h, ctx, H, layer.skip, layer.e_linear.weight, layer.e_linear.bias, params, mask, pool)


def _composed(layer, ctx, h, H, mask, pool):
    from wsi_hgnn_amd import ops
    D = h.shape[1]
    ws, bs = [], []
    for nid in ctx.nid:
        for lin in (layer.k_linears[nid], layer.q_linears[nid], layer.v_linears[nid]):
            ws.append(lin.weight)
            bs.append(lin.bias)
    kqv = ops.grouped_linear(h, ctx.kqv_spec, ws, bs)
    t = ops.heat_attention(kqv, layer.e_linear.weight, layer.e_linear.bias, ctx.plan, ctx.sim_csr, D, H)
    y = ops.grouped_linear(t, ctx.a_spec, [layer.a_linears[ctx.nid[i]].weight for i in ctx.a_types],
                           [layer.a_linears[ctx.nid[i]].bias for i in ctx.a_types])
    if mask is not None:
        y = y * mask
    out = torch.lerp(h, y, ctx.row_gate(layer.skip))
    return out if pool is None else ops.segment_reduce(out, pool[0], pool[1])


def _compare(layer, ctx, h0, H, g_out, mask=None, pool=None, sum_bounds=False):
    """Both forms on the same input and output gradient; the figures, then the bounds of the module docstring."""
    from wsi_hgnn_amd import ops
    res = []
    ops.set_low_rank_readout_grad(False)
    ops.set_gemm_precision("fp32")
    try:
        for form in (_fused, _composed):
            layer.zero_grad(set_to_none=True)
            h = h0.clone().requires_grad_()
            out = form(layer, ctx, h, H, mask, pool)
            out.backward(g_out)
            grads = {"h": h.grad.clone()}
            grads.update({k: p.grad.clone() for k, p in layer.named_parameters() if p.grad is not None})
            res.append((out.detach().clone(), grads))
    finally:
        ops.set_low_rank_readout_grad(True)
    (o1, g1), (o2, g2) = res
    assert o1.shape == o2.shape and g1.keys() == g2.keys()
    rel, tiny = (1e-4, 1e-6) if sum_bounds else (2e-5, 1e-8)
    figures = [("out", (o1 - o2).abs().max().item(), 2e-5 * max(1.0, o2.abs().max().item()))]
    figures += [(k, (g1[k] - g).abs().max().item(), rel * g.abs().max().item() + tiny) for k, g in g2.items()]
    for name, err, bound in figures:
        print(f"{name}: error {err:.3e}, bound {bound:.3e}")
    for name, err, bound in figures:
        assert err <= bound, (name, err, bound)


@pytest.mark.parametrize("op", ["mean", "sum"])
@pytest.mark.parametrize("hidden", [64, 128])          # 64: the generic attention kernels (V kept); 128: the fast ones, V collapsed
def test_readout_of_more_than_8192_segments(hidden, op):
    """S = 9000 readout segments, type-major with 3000 per node type: above the 8192 that wsi_pool_bwd_prep takes.
    hidden 64: one synthetic graph, 3 node types of 3000 rows, a plan of one-row segments (with V kept a plan need only respect the node types).
    hidden 128: the V collapse takes every edge to stay inside one graph of the plan, and a graph needs two nodes of a type for a softmax
    over different sources - 3000 graphs of 2 nodes per type in one block-diagonal graph, a plan of two-row (type, graph) segments."""
    from wsi_hgnn_amd import ops
    H, per = 4, (1 if hidden == 64 else 2)
    graph = _synthetic([9000], fractions=(1 / 3, 1 / 3, 1 / 3))[0] if hidden == 64 else _block_diagonal_graph(3000, per)
    layer, ctx, h0, G = _case([graph], hidden, H)
    n = 9000 * per
    assert ctx.rows == [(0, n // 3), (n // 3, 2 * n // 3), (2 * n // 3, n)] and all(ctx.incoming)
    prp = ops.ReducePlan.from_ranges([(r, r + per) for r in range(0, n, per)], _dev())
    assert prp.num_segs == 9000
    g_pool = torch.randn(9000, hidden, device=_dev())
    pooled_calls = []
    real_pool = ops.N.AttnPool
    ops.N.AttnPool = lambda **kw: (pooled_calls.append(1), real_pool(**kw))[1]
    ops.set_value_collapse(True, min_work=0.0)          # (the size threshold would keep V at this test's size)
    try:
        assert ops._value_collapse_applies(ctx, prp, n, hidden, H) == (hidden == 128)
        _compare(layer, ctx, h0, H, g_pool, pool=(prp, op), sum_bounds=(op == "sum"))
    finally:
        ops.N.AttnPool = real_pool
        ops.set_value_collapse(True, min_work=4e9)
    assert len(pooled_calls) == (1 if hidden == 128 else 0)


@pytest.mark.parametrize("hidden", [64, 128])
def test_dropout_mask_as_a_tensor(hidden):
    """An explicit [N, D] keep mask (scaled by 1 / keep) through the fused node, the same tensor applied by hand in the composed form; node
    type 2 has no incoming relation."""
    H = 4
    layer, ctx, h0, G = _case(_synthetic([500, 431], NO_RELATION_INTO_2), hidden, H)
    assert ctx.incoming == [True, True, False]
    mask = torch.empty_like(h0).bernoulli_(0.7).mul_(1.0 / 0.7)
    _compare(layer, ctx, h0, H, torch.randn_like(h0), mask=mask)


@pytest.mark.parametrize("relations", [None, NO_RELATION_INTO_2], ids=["all_types_entered", "one_type_passed_through"])
def test_width_that_is_no_multiple_of_32(relations):
    """D = 48, H = 4: the K | Q | V dX as one launch per column block (the chunked launch needs D % 32 == 0)."""
    H = 4
    layer, ctx, h0, G = _case(_synthetic([500, 431], relations), 48, H)
    assert ctx.incoming == [True, True, relations is None]
    _compare(layer, ctx, h0, H, torch.randn_like(h0))


@pytest.mark.parametrize("op", ["mean", "sum"])
def test_readout_plan_that_straddles_a_node_type_is_refused(op):
    from wsi_hgnn_amd import ops
    H = 4
    layer, ctx, h0, G = _case(_synthetic([300]), 64, H)
    n = h0.shape[0]
    assert ctx.rows[0][1] not in (100, 200)
    prp = ops.ReducePlan.from_ranges([(0, 100), (100, 200), (200, n)], _dev())
    assert prp.segments_of(ctx.rows) is None
    launched = []
    real_gemm = ops._gemm
    ops._gemm = lambda *a, **kw: (launched.append(1), real_gemm(*a, **kw))[1]
    try:
        with pytest.raises(ValueError):
            _fused(layer, ctx, h0.clone().requires_grad_(), H, None, (prp, op))
    finally:
        ops._gemm = real_gemm
    assert not launched          # refused before the first launch (the K | Q | V projection)
