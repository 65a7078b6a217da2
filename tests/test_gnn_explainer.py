"""GNNExplainer without a GPU: the class surface against the reference's (tests/golden/reference_surface_explainer.json), the order
of the mask draws, the regularised loss against a float64 restatement, ``graph.message_scale`` (edge order <-> CSR order, refusals,
clean-up) and the argument checks of the new C-ABI entry points (they return before any HIP call)."""
import ctypes
import inspect
import json
import os
import re
from math import sqrt

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
SURFACE = json.load(open(os.path.join(HERE, "golden", "reference_surface_explainer.json")))


def _sig(fn):
    out = []
    for p in inspect.signature(fn).parameters.values():
        req = p.default is inspect.Parameter.empty
        out.append({"name": p.name, "default": None if req else p.default, "required": req})
    return out


def test_surface_matches_the_reference():
    from wsi_hgnn_amd.explainers import GNNExplainer, ExplainerTags, GemExplainer, HetGemExplainer  # noqa: F401  (the reference's three names + tags)
    import wsi_hgnn_amd.explainers as E
    assert E.__all__[0] == "GNNExplainer"
    assert _sig(GNNExplainer.__init__) == SURFACE["init"]
    assert _sig(GNNExplainer.explain_node) == SURFACE["explain_node"]
    assert GNNExplainer.params == SURFACE["params"]
    assert list(GNNExplainer.params) == list(SURFACE["params"])
    assert ExplainerTags.NODE_FEATURES == "feat" and ExplainerTags.EDGE_MASK != ExplainerTags.ORIGINAL_ID
    for name in ("test_explanation", "_predict", "_create_subgraph", "__loss__", "__set_masks__", "__apply_feature_mask__"):
        assert callable(getattr(GNNExplainer, name))


def _graph(n=23, seed=3, shuffle=True):
    """Homogeneous graph with self-loops, duplicate edges and (shuffle) an edge order that is not the CSR order."""
    from wsi_hgnn_amd.graph import HeteroGraph
    g = torch.Generator().manual_seed(seed)
    u = torch.randint(0, n, (4 * n,), generator=g)
    v = torch.randint(0, n, (4 * n,), generator=g)
    loop = torch.arange(n)
    u, v = torch.cat([u, loop, u[:5]]), torch.cat([v, loop, v[:5]])
    if shuffle:
        o = torch.randperm(u.numel(), generator=g)
        u, v = u[o], v[o]
    return HeteroGraph.homogeneous(n, u, v, feat=torch.randn(n, 6, generator=g))


def test_constructor_params_are_per_instance_and_model_flags_are_set():
    from wsi_hgnn_amd.explainers import GNNExplainer

    class M(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self._allow_zero_in_degree = False

    m = M()
    ex = GNNExplainer(_graph(), m, 2, edge_size=0.25, feat_size=0.75)
    assert ex.params["edge_size"] == 0.25 and ex.params["feat_size"] == 0.75 and ex.params["eps"] == 1e-15
    assert GNNExplainer.params == SURFACE["params"]
    assert (ex.epochs, ex.lr, ex.threshold, ex.num_hops) == (100, 0.01, 0.5, 2)
    assert m._allow_zero_in_degree is True
    assert ex.history == []


@pytest.mark.parametrize("seed", [0, 611])
def test_mask_initialisation_replays_the_reference_draw_order(seed):
    from wsi_hgnn_amd.explainers import GNNExplainer, ExplainerTags
    g = _graph()
    N, E = g.num_nodes(), g.num_edges()
    ex = GNNExplainer(g, torch.nn.Identity(), 2)
    torch.manual_seed(seed)
    ex.__set_masks__(g)
    torch.manual_seed(seed)
    node = torch.randn(N) * 0.1
    std = torch.nn.init.calculate_gain("relu") * sqrt(2.0 / (2 * N))
    edge = torch.randn(E) * std
    assert torch.equal(ex.node_mask.detach(), node)
    assert torch.equal(g.edata[ExplainerTags.EDGE_MASK].detach(), edge)
    assert isinstance(ex.node_mask, torch.nn.Parameter) and isinstance(g.edata[ExplainerTags.EDGE_MASK], torch.nn.Parameter)


def _loss64(logits, pred, me, mn, p):
    me, mn, logits = me.double(), mn.double(), logits.double()
    eps = p["eps"]
    ent = lambda m: (-m * torch.log(m + eps) - (1 - m) * torch.log(1 - m + eps)).mean()
    return -logits.view(-1)[pred] + me.sum() * p["edge_size"] + p["edge_ent"] * ent(me) + mn.mean() * p["feat_size"] + p["feat_ent"] * ent(mn)


def test_loss_matches_float64_restatement_including_saturated_masks():
    from wsi_hgnn_amd.explainers import GNNExplainer, ExplainerTags
    g = _graph()
    N, E = g.num_nodes(), g.num_edges()
    ex = GNNExplainer(g, torch.nn.Identity(), 2, edge_size=0.007, feat_size=0.3)
    gen = torch.Generator().manual_seed(5)
    node = torch.randn(N, generator=gen) * 2
    edge = torch.randn(E, generator=gen) * 2
    node[:3] = torch.tensor([-200.0, 200.0, 0.0])          # sigmoid -> exactly 0, exactly 1, 0.5: the eps terms keep the logs finite
    edge[:3] = torch.tensor([200.0, -200.0, 0.0])
    ex.node_mask = torch.nn.Parameter(node)
    g.edata[ExplainerTags.EDGE_MASK] = torch.nn.Parameter(edge)
    logits = torch.tensor([[0.3, -1.7]])
    pred = logits.argmax(dim=-1)
    got = ex.__loss__(g, None, logits, pred)
    assert got.shape == (1,) and torch.isfinite(got).all()
    assert float(edge.sigmoid()[1]) == 0.0 and float(edge.sigmoid()[0]) == 1.0
    want = _loss64(logits, pred, edge.sigmoid(), node.sigmoid(), ex.params)
    assert abs(float(got.detach()) - float(want)) <= 1e-6 * abs(float(want))
    # the edge size term is a SUM, every other term a mean: doubling edge_size moves the loss by sum(sigmoid(edge)) * edge_size
    ex.params["edge_size"] *= 2
    assert abs(float((ex.__loss__(g, None, logits, pred) - got).detach()) - 0.007 * float(edge.sigmoid().sum())) < 1e-5
    with pytest.raises(NotImplementedError):
        ex.__loss__(g, 0, logits, pred)


def test_message_scale_permutes_into_csr_order_and_back():
    from wsi_hgnn_amd import graph as G
    g = _graph()
    E = g.num_edges()
    u, v = g.edges()
    plan = g.plan()
    assert not torch.equal(g._csr_perm(), torch.arange(E))            # the edge order is not the CSR order
    scale = (torch.arange(E, dtype=torch.float32) + 1).requires_grad_(True)
    assert G.message_scale_of(g) is None
    with G.message_scale(g, scale) as gg:
        assert gg is g
        s = G.message_scale_of(g)
        assert s.shape == (E,)
        # CSR position j holds the scale of an edge with the same endpoints as the plan's j-th entry
        dst_csr = torch.repeat_interleave(torch.arange(g.num_nodes()), (plan.rowptr[1:] - plan.rowptr[:-1]).long())
        eid = (s.detach() - 1).long()
        assert torch.equal(u[eid], plan.src.long()) and torch.equal(v[eid], dst_csr)
        w = torch.zeros(E)
        w[plan.rowptr[3]:plan.rowptr[4]] = 1.0                          # weight 1 on the CSR entries of destination 3
        (s * w).sum().backward()
    assert G.message_scale_of(g) is None
    assert torch.equal(scale.grad, (v == 3).float())                    # ... lands on the edges that enter node 3, in edge order


def test_message_scale_refuses_hetero_graphs_and_bad_shapes_and_cleans_up():
    from wsi_hgnn_amd import graph as G
    from wsi_hgnn_amd import synthetic
    het = synthetic.hetero_graph(40, 8, seed=1)
    with pytest.raises(ValueError, match="homogeneous"):
        with G.message_scale(het, torch.ones(het.num_edges())):
            pass
    g = _graph()
    with pytest.raises(ValueError, match="one value per edge"):
        with G.message_scale(g, torch.ones(g.num_edges() + 1)):
            pass
    assert G.message_scale_of(g) is None
    with pytest.raises(RuntimeError, match="boom"):
        with G.message_scale(g, torch.ones(g.num_edges())):
            assert G.message_scale_of(g) is not None
            raise RuntimeError("boom")
    assert G.message_scale_of(g) is None and "_message_scale" not in g.__dict__
    outer = torch.full((g.num_edges(),), 2.0)
    with G.message_scale(g, outer):                                     # nested blocks restore the enclosing scale
        with G.message_scale(g, torch.ones(g.num_edges())):
            assert float(G.message_scale_of(g)[0]) == 1.0
        assert float(G.message_scale_of(g)[0]) == 2.0
    assert G.message_scale_of(g) is None


def test_ops_refuse_cpu_tensors_and_wrong_edge_counts():
    from wsi_hgnn_amd import ops
    from wsi_hgnn_amd.models.GCN import homo_plan
    from wsi_hgnn_amd.models.GAT import gat_plan
    g = _graph()
    E, n = g.num_edges(), g.num_nodes()
    hp, gp = homo_plan(g), gat_plan(g)
    assert hp.num_edges == gp.num_edges == E
    z = torch.randn(n, 6)
    with pytest.raises(ValueError, match="edge_scale"):
        ops.graph_conv_aggregate(z, None, hp, False, edge_scale=torch.ones(E - 1))
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.graph_conv_aggregate(z, None, hp, False, edge_scale=torch.ones(E))
    al = torch.randn(1, 2, 3)
    with pytest.raises(ValueError, match="edge_scale"):
        ops.gat_attention(z, al, al, None, gp, 0.2, edge_scale=torch.ones(E, 2))
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.gat_attention(z, al, al, None, gp, 0.2, edge_scale=torch.ones(E))


def test_node_idx_is_refused():
    from wsi_hgnn_amd.explainers import GNNExplainer
    ex = GNNExplainer(_graph(), torch.nn.Identity(), 2)
    with pytest.raises(NotImplementedError, match="one row of logits per graph"):
        ex.explain_node(0)
    with pytest.raises(NotImplementedError):
        ex._create_subgraph(3)


def test_subgraph_is_a_copy_with_the_original_ids():
    from wsi_hgnn_amd.explainers import GNNExplainer, ExplainerTags
    g = _graph()
    ex = GNNExplainer(g, torch.nn.Identity(), 2)
    sub = ex._create_subgraph(None)
    assert sub is not g and sub.num_nodes() == g.num_nodes() and sub.num_edges() == g.num_edges()
    assert torch.equal(sub.ndata[ExplainerTags.ORIGINAL_ID], torch.arange(g.num_nodes(), dtype=torch.int))
    assert torch.equal(sub.ndata["feat"], g.ndata["feat"])
    assert ExplainerTags.ORIGINAL_ID not in g.ndata                     # the copy has frames of its own


# ---------------------------------------------------------------------------------------------- C-ABI
def _lib():
    import __graft_entry__
    __graft_entry__.build()
    from wsi_hgnn_amd import _native
    return _native.load()


P = ctypes.c_void_p(1 << 40)            # a fake device address: every call below must fail its argument check before touching it
EINVAL = -22


def test_abi_26_in_header_library_and_binding():
    from wsi_hgnn_amd import _native
    lib = _lib()
    header = open(os.path.join(os.path.dirname(HERE), "include", "wsi_hgnn.h")).read()
    assert int(re.search(r"#define WSI_ABI_VERSION (\d+)", header).group(1)) == 26
    assert lib.wsi_abi_version() == 26 == _native.WSI_ABI_VERSION
    for name in ("wsi_gat_attn_fwd_scaled", "wsi_gat_attn_bwd_scaled", "wsi_sddmm_dot"):
        assert hasattr(lib, name) and re.search(r"\b%s\(" % name, header)


def test_capi_scaled_gat_rejects_bad_arguments():
    lib = _lib()
    H, D = 4, 8

    def fwd(**kw):
        return lib.wsi_gat_attn_fwd_scaled(kw.get("ft", P), kw.get("ld", 32), P, kw.get("n", 10), kw.get("H", H), D, kw.get("rowptr", P), P, None, 0.2,
                                           0, None, kw.get("thr", 0), 1.0, None, kw.get("act", 0), 0.01, kw.get("scale", P), kw.get("out", P), 32, P, None)
    assert fwd(scale=None) == EINVAL
    assert "null pointer" in lib.wsi_last_error().decode() and "gat_attn_fwd_scaled" in lib.wsi_last_error().decode()
    assert fwd(ft=None) == EINVAL and fwd(rowptr=None) == EINVAL and fwd(out=None) == EINVAL
    assert fwd(n=-1) == EINVAL and fwd(H=0) == EINVAL and fwd(H=17) == EINVAL
    assert fwd(ld=16) == EINVAL and fwd(act=3) == EINVAL and fwd(thr=65536) == EINVAL
    assert fwd(n=0) == 0                                    # nothing to do: no launch
    ws = lib.wsi_gat_attn_bwd_workspace_bytes(10, 20, H, D, 2)
    assert ws > 0

    def bwd(**kw):
        return lib.wsi_gat_attn_bwd_scaled(P, 32, P, P, kw.get("out", P), 32, kw.get("g_out", P), 32, kw.get("n", 10), kw.get("E", 20), H, D, P, P, P, P, P, None,
                                           P, P, 0.2, 0, None, 0, 1.0, kw.get("act", 2), 0.01, kw.get("scale", P), kw.get("ws", P), kw.get("ws_bytes", ws),
                                           kw.get("g_ft", P), 32, P, P, None, kw.get("g_scale", P), None)
    assert bwd(scale=None) == EINVAL and bwd(g_scale=None) == EINVAL
    assert bwd(g_out=None) == EINVAL and bwd(g_ft=None) == EINVAL and bwd(out=None) == EINVAL and bwd(ws=None) == EINVAL
    assert bwd(E=-1) == EINVAL and bwd(n=-1) == EINVAL and bwd(act=-1) == EINVAL
    assert bwd(ws_bytes=ws - 1) == -12                      # WSI_ENOMEM: the workspace of the unscaled backward, same size


def test_capi_sddmm_dot_rejects_bad_arguments():
    lib = _lib()

    def call(**kw):
        return lib.wsi_sddmm_dot(kw.get("g", P), kw.get("ldg", 64), kw.get("x", P), kw.get("ldx", 64), kw.get("n", 10), kw.get("D", 64),
                                 kw.get("rowptr", P), kw.get("src", P), None, None, kw.get("ref", None), kw.get("ldref", 0), kw.get("g_w", P), None)
    for k in ("g", "x", "rowptr", "src", "g_w"):
        assert call(**{k: None}) == EINVAL, k
    assert "sddmm_dot" in lib.wsi_last_error().decode()
    assert call(n=-1) == EINVAL and call(D=0) == EINVAL and call(D=-4) == EINVAL and call(D=1025, ldg=2048, ldx=2048) == EINVAL
    assert call(ldg=63) == EINVAL and call(ldx=8) == EINVAL and call(ref=P, ldref=32) == EINVAL
    assert call(n=0) == 0
