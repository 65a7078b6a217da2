"""H2MIL on the CPU: the float64 restatements of tests/h2mil_cases.py against the fixtures recorded from the reference's own RAConv.py and
IHPool.py (values and gradients to 1e-10, discrete outputs exactly), the ``kernels=False`` modules against the restatements, a packed batch
against its slides one at a time, the seed-count arithmetic, the state_dict surface, which parameters receive gradients, the stated decisions,
and the refusal of CPU tensors and bad arguments by the two new entry points."""
import math
import os

import numpy as np
import pytest
import torch

import h2mil_cases as C
import row_group_cases as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "h2mil")
TOL = 1e-10


def _close(got, want, what):
    got, want = torch.as_tensor(got).double(), torch.as_tensor(want).double()
    assert got.shape == want.shape, (what, got.shape, want.shape)
    err = float((got - want).abs().max()) if want.numel() else 0.0
    assert err <= TOL * max(1.0, float(want.abs().max()) if want.numel() else 1.0), f"{what}: error {err:.3e}"


@pytest.fixture(scope="module")
def ra_fix():
    return dict(np.load(os.path.join(GOLD, "reference_raconv.npz")))


@pytest.fixture(scope="module")
def ih_fix():
    return dict(np.load(os.path.join(GOLD, "reference_ihpool.npz")))


def _ra_state(fix):
    return {k: torch.from_numpy(fix["sd." + k]).double() for k in fix["keys"].tolist()}


# ------------------------------------------------------------------------------------------------ RAConv
def test_raconv_restatement_reproduces_the_reference(ra_fix):
    p = {k: v.clone().requires_grad_(True) for k, v in _ra_state(ra_fix).items() if not k.endswith("_r.weight")}
    x = torch.from_numpy(ra_fix["x"]).double().requires_grad_(True)
    ei, nt = torch.from_numpy(ra_fix["edge_index"]), torch.from_numpy(ra_fix["node_type"])
    indeg = torch.bincount(ei[1], minlength=x.shape[0])
    groups = {v: len({int(nt[u]) for u, w in ei.t().tolist() if w == v}) for v in range(x.shape[0])}
    assert int((indeg == 0).sum()) >= 4 and 1 in groups.values() and 3 in groups.values()          # what the fixture promises
    out = C.raconv_ref(x, ei, nt, p)
    (out * torch.from_numpy(ra_fix["w"])).sum().backward()
    _close(out.detach(), ra_fix["out"], "out")
    _close(x.grad, ra_fix["g.x"], "g.x")
    for k, v in p.items():
        _close(v.grad, ra_fix["g." + k], "g." + k)
    assert not out.detach()[indeg == 0].sub(p["bias"].detach()).any(), "a node without in-edges gives the bias"


def _our_raconv(fix, **kw):
    from wsi_hgnn_amd import h2mil
    cin, cout = fix["config"].tolist()
    m = h2mil.RAConv(cin, cout, **kw).double()
    m.load_state_dict(_ra_state(fix))
    return m


def test_raconv_module_equals_the_restatement_and_keeps_the_keys(ra_fix):
    m = _our_raconv(ra_fix, kernels=False)
    assert list(m.state_dict().keys()) == ra_fix["keys"].tolist()
    assert m.lin_r is m.lin_l and m.t_lin_r is m.t_lin_l
    x = torch.from_numpy(ra_fix["x"]).double().requires_grad_(True)
    ei, nt = torch.from_numpy(ra_fix["edge_index"]), torch.from_numpy(ra_fix["node_type"])
    out = m(x, ei, nt)
    (out * torch.from_numpy(ra_fix["w"])).sum().backward()
    _close(out.detach(), ra_fix["out"], "out")
    _close(x.grad, ra_fix["g.x"], "g.x")
    for k, p in m.named_parameters():
        _close(p.grad, ra_fix["g." + k], "g." + k)


def test_raconv_refuses_what_is_not_built():
    from wsi_hgnn_amd import h2mil
    with pytest.raises(ValueError, match="heads"):
        h2mil.RAConv(8, 4, heads=2)
    with pytest.raises(ValueError, match="tuple"):
        h2mil.RAConv((8, 8), 4)
    m = h2mil.RAConv(8, 4, kernels=False)
    with pytest.raises(ValueError, match="return_attention_weights"):
        m(torch.zeros(3, 8), torch.zeros(2, 0, dtype=torch.int64), torch.zeros(3, dtype=torch.int64), return_attention_weights=True)
    with pytest.raises(ValueError, match="select"):
        h2mil.IHPool(4, select="topk")
    with pytest.raises(ValueError, match="select"):
        h2mil.IHPool(4, dis="cos")


def test_edge_layout_orders_a_destination_by_source_type(ra_fix):
    from wsi_hgnn_amd import ops
    ei, nt = torch.from_numpy(ra_fix["edge_index"]), torch.from_numpy(ra_fix["node_type"])
    ec = ops.edge_csr_by_source_type(ei[0], ei[1], nt, 40)
    assert torch.equal(ei[0][ec.perm].to(torch.int32), ec.src) and ec.node_type.dtype == torch.int32
    dst = ei[1][ec.perm]
    key = dst * 3 + nt[ec.src.long()]
    assert bool((key[1:] >= key[:-1]).all())
    assert torch.equal(torch.bincount(dst, minlength=40).cumsum(0).to(torch.int32), ec.rowptr[1:])
    assert torch.equal(dst[ec.csc_eid.long()].to(torch.int32), ec.csc_dst)


# ------------------------------------------------------------------------------------------------ IHPool
FIELDS = ("x", "edge_index", "cluster", "node_type", "tree", "fitness", "x_y_index")
DISCRETE = ("edge_index", "cluster", "node_type", "tree")


def _ih_inputs(fix):
    return (torch.from_numpy(fix["x"]).double(), torch.from_numpy(fix["edge_index"]), torch.from_numpy(fix["node_type"]), torch.from_numpy(fix["tree"]),
            torch.from_numpy(fix["x_y_index"]).double())


def _compare_layer(fix, name, got):
    for f in FIELDS:
        want = torch.from_numpy(fix[f"{name}.{f}"])
        if f in DISCRETE:
            assert torch.equal(got[f], want), f"{name}.{f}"
        else:
            _close(got[f], want, f"{name}.{f}")


def test_ihpool_restatement_reproduces_the_reference(ih_fix):
    w = lambda n, k: torch.from_numpy(ih_fix[f"{n}.sd.{k}"]).double()
    a0 = _ih_inputs(ih_fix)
    ra = C.ihpool_ref(*a0, w("a", "weight_1"), w("a", "weight_2"), float(ih_fix["a.ratio"]))
    rb = C.ihpool_ref(ra["x"], ra["edge_index"], ra["node_type"], ra["tree"], ra["x_y_index"], w("b", "weight_1"), w("b", "weight_2"), float(ih_fix["b.ratio"]))
    rc = C.ihpool_ref(*a0, w("c", "weight_1"), w("c", "weight_2"), float(ih_fix["c.ratio"]))
    assert min(ra["margin"], rb["margin"], rc["margin"]) >= C.MARGIN
    for name, r in (("a", ra), ("b", rb), ("c", rc)):
        _compare_layer(ih_fix, name, r)
        assert ih_fix[f"{name}.edge_weight"].size == 0 and not ih_fix[f"{name}.batch"].any()


def _as_slide(x, ei, nt, tree, xy):
    return {"x": x, "edge_index_tree_8nb": ei, "node_type": nt, "node_tree": tree, "x_y_index": xy}


def _pool_one(layer, x, tb):
    """One slide through our layer, as the restatement's dict."""
    xn, nb, cluster, fit = layer(x, tb)
    return {"x": xn, "edge_index": nb.edge_index, "cluster": cluster, "node_type": nb.node_type, "tree": nb.tree, "fitness": fit,
            "x_y_index": nb.x_y_index, "batch": nb}


def test_ihpool_module_equals_the_reference_and_loads_its_state(ih_fix):
    from wsi_hgnn_amd import h2mil
    cin = int(ih_fix["config"][0])
    layers = {}
    for n in "abc":
        layers[n] = h2mil.IHPool(cin, ratio=float(ih_fix[f"{n}.ratio"]), kernels=False).double()
        ref_state = {k: torch.from_numpy(ih_fix[f"{n}.sd.{k}"]).double() for k in ih_fix["keys"].tolist()}
        assert any(k.startswith("gnn_score.") for k in ref_state)
        layers[n].load_state_dict(ref_state)                                         # gnn_score.* accepted and dropped
        ours = list(layers[n].state_dict().keys())
        assert ours == [k for k in ih_fix["keys"].tolist() if not k.startswith("gnn_score.")] and ours[:2] == ["weight_1", "weight_2"]
    x, ei, nt, tree, xy = _ih_inputs(ih_fix)
    tb = h2mil.from_slides([_as_slide(x, ei, nt, tree, xy)])
    ga = _pool_one(layers["a"], x, tb)
    gb = _pool_one(layers["b"], ga["x"], ga["batch"])
    gc = _pool_one(layers["c"], x, tb)
    for name, g in (("a", ga), ("b", gb), ("c", gc)):
        _compare_layer(ih_fix, name, g)
    assert layers["a"].readbacks == 2 and layers["c"].readbacks == 2                 # kernels=False: the one copy and the table width


@pytest.mark.parametrize("ratio", (0.1, 0.2, 0.3, 4))
def test_seed_count_arithmetic_matches_the_reference_expression(ratio):
    import importlib
    mod = importlib.import_module("wsi_hgnn_amd.h2mil.IHPool")       # (the package attribute of that name is the class)
    ns = torch.arange(1, 65)
    dev_steps = mod._steps_on_device(ns, ratio).tolist()
    for n in range(1, 65):
        want1 = len(range(0, n, C.reference_step(n, ratio, 1)))
        assert mod.seed_count(n, mod.level1_step(n, ratio)) == want1, (ratio, n)
        want2 = len(range(0, n, C.reference_step(n, ratio, 2)))
        assert mod.seed_count(n, dev_steps[n - 1]) == want2, (ratio, n)
        if ratio >= 1:
            assert want2 == min(n, 2)


# ------------------------------------------------------------------------------------------------ the model
@pytest.fixture(scope="module")
def model64():
    return C.make_model(kernels=False, dtype=torch.float64)


@pytest.fixture(scope="module")
def slides(model64):
    state = {k: v.detach() for k, v in model64.state_dict().items()}
    return C.model_slides(state)


def test_model_slides_meet_the_margin_condition(model64, slides):
    state = {k: v.detach() for k, v in model64.state_dict().items()}
    sizes = [s["x"].shape[0] for s in slides]
    assert 50 <= sizes[0] <= 75 and 120 <= sizes[1] <= 180 and 350 <= sizes[2] <= 450, sizes
    for s in slides:
        assert C.h2mil_ref(C.double(s), state)[2] >= C.MARGIN


def _check_outputs(outs, b, ref_pools):
    for layer in (0, 1):
        r = ref_pools[layer]
        assert torch.equal(outs[1][layer][b], r["cluster"])
        assert torch.equal(outs[2][layer][b], r["node_type"])
        _close(outs[3][layer][b], r["fitness"], "fitness")
        assert torch.equal(outs[4][layer][b], r["tree"])
        _close(outs[5][layer][b], r["x_y_index"], "x_y_index")
        assert torch.equal(outs[6][layer][b], r["edge_index"])


def test_model_equals_the_restatement_and_a_batch_equals_its_slides(model64, slides):
    from wsi_hgnn_amd import h2mil
    state = {k: v.detach() for k, v in model64.state_dict().items()}
    single = C.tree_slide(7, 1, (3, 3), feat=C.MODEL_CFG["in_feats"])               # a slide with ONE level-1 node
    three = [slides[0], single, slides[1]]
    model64.eval()
    labels = torch.tensor([0, 2, 1])
    batch = h2mil.from_slides(three, dtype=torch.float64)
    model64.zero_grad()
    outs = model64(batch)
    loss = h2mil.loss_fn(outs[0], labels)
    loss.backward()
    ref_loss, ref_p = 0.0, {k: v.clone().requires_grad_(True) for k, v in state.items()}
    for b, s in enumerate(three):
        probs, pools, _ = C.h2mil_ref(C.double(s), ref_p)
        _close(outs[0][b:b + 1].detach(), probs.detach(), f"probabilities of slide {b}")
        _check_outputs(outs, b, pools)
        ref_loss = ref_loss + torch.nn.functional.cross_entropy(probs, labels[b:b + 1])
        alone = model64(h2mil.from_slides([s], dtype=torch.float64))
        _close(alone[0], outs[0][b:b + 1], f"slide {b} alone")
        for t in range(1, 7):
            for layer in (0, 1):
                a, g = alone[t][layer][0], outs[t][layer][b]
                assert torch.equal(a, g) if not a.is_floating_point() else float((a - g).abs().max()) <= TOL, (b, t, layer)
    _close(loss.detach(), ref_loss.detach(), "loss")
    ref_loss.backward()
    for k, p in model64.named_parameters():
        if k.startswith(("pool_1.", "pool_2.")):
            assert p.grad is None, k                                             # weight_1 / weight_2 decide clusters only; lin / att never enter
        else:
            assert p.grad is not None and float(p.grad.abs().max()) > 0, k
            _close(p.grad, ref_p[k].grad, "g." + k)
    # the per-slide LayerNorm statistics
    x = torch.randn(batch.num_nodes, 5, dtype=torch.float64)
    y = model64.norm(x, batch.slide, 3, None)
    for b in range(3):
        _close(y[batch.starts[b]:batch.starts[b + 1]], C.graph_norm(x[batch.starts[b]:batch.starts[b + 1]], state["norm.weight"], state["norm.bias"]), "norm")
    assert tuple(model64.norm.weight.shape) == (1,) and tuple(model64.norm.bias.shape) == (1,)


@pytest.mark.parametrize("mpool", ("global_max_pool", "global_att_pool"))
def test_the_other_readouts_equal_the_restatement(slides, mpool):
    from wsi_hgnn_amd import h2mil
    torch.manual_seed(5)
    m = h2mil.H2MIL(**C.MODEL_CFG, drop_out_ratio=0.0, mpool_method=mpool, kernels=False).double().eval()
    state = {k: v.detach() for k, v in m.state_dict().items()}
    s = slides[0]
    probs = C.h2mil_ref(C.double(s), state, mpool=mpool)[0]
    _close(m(h2mil.from_slides([s], dtype=torch.float64))[0].detach(), probs, mpool)
    if mpool == "global_att_pool":
        assert [k for k in state if k.startswith("mpool.")] == ["mpool.gate_nn.0.weight", "mpool.gate_nn.0.bias", "mpool.gate_nn.2.weight", "mpool.gate_nn.2.bias"]


def test_model_state_dict_keys():
    from wsi_hgnn_amd import h2mil
    m = h2mil.H2MIL(32, 0, 16, 2)
    conv = ["att_l", "att_r", "t_att_l", "t_att_r", "bias", "lin_l.weight", "lin_r.weight", "t_lin_l.weight", "t_lin_r.weight"]
    pool = ["weight_1", "weight_2", "lin.weight", "lin.bias", "att.weight", "att.bias"]
    want = [f"conv1.{k}" for k in conv] + [f"conv2.{k}" for k in conv] + [f"pool_1.{k}" for k in pool] + [f"pool_2.{k}" for k in pool] + \
        ["lin1.weight", "lin1.bias", "lin2.weight", "lin2.bias", "norm.weight", "norm.bias"]
    assert list(m.state_dict().keys()) == want
    assert m.pool_1.ratio == 0.2 and m.pool_2.ratio == 4 and m.dropout.p == 0.2 and m.kernels


def test_train_one_step_lowers_the_loss_in_tensor_operations():
    from wsi_hgnn_amd import h2mil
    torch.manual_seed(3)
    m = h2mil.H2MIL(12, 0, 8, 2, drop_out_ratio=0.0, kernels=False)
    a, b = C.tree_slide(1, 6, (2, 4), feat=12), C.tree_slide(2, 6, (2, 4), feat=12)
    b["x"] = b["x"] + 1.5
    batch, labels = h2mil.from_slides([a, b]), torch.tensor([0, 1])
    opt = torch.optim.Adam(m.parameters(), lr=1e-2)
    losses = [float(h2mil.train_one_step(m, batch, labels, opt)) for _ in range(8)]
    assert all(math.isfinite(l) for l in losses) and losses[-1] < losses[0], losses


# ------------------------------------------------------------------------------------------------ decisions
def _tiny(xy1, f1_feat, kids_xy, kids_feat, parents):
    """A slide with hand-placed level-1 and level-2 nodes; the feature is one column, so fitness = tanh(feature) under weight 1."""
    n1, n2 = len(xy1), len(kids_xy)
    x = torch.tensor([[0.0]] + [[v] for v in f1_feat] + [[v] for v in kids_feat], dtype=torch.float64)
    xy = torch.tensor([[0.0, 0.0]] + list(xy1) + list(kids_xy), dtype=torch.float64)
    nt = torch.tensor([0] + [1] * n1 + [2] * n2)
    tree = torch.tensor([-1] + [0] * n1 + [1 + p for p in parents])
    ei = torch.tensor([[0] * n1, list(range(1, 1 + n1))])
    return _as_slide(x, ei, nt, tree, xy)


def _pool_tiny(slide, ratio):
    from wsi_hgnn_amd import h2mil
    layer = h2mil.IHPool(1, ratio=ratio, kernels=False).double()
    with torch.no_grad():
        layer.weight_1.fill_(1.0); layer.weight_2.fill_(1.0)
    tb = h2mil.from_slides([slide])
    return _pool_one(layer, slide["x"], tb)


def test_ties_and_duplicate_seeds_follow_the_stated_rules():
    # ratio 4 with four level-1 nodes: step 1, every node is a seed.  Nodes 1 and 2 coincide exactly (same place, same fitness): each seed
    # owns its cluster, so there are four clusters whatever the distances say (the reference's sort would put both into one).
    s = _tiny([(0.1, 0.1), (0.1, 0.1), (0.5, 0.5), (0.9, 0.9)], [0.3, 0.3, 0.1, 0.7], [], [], [])
    g = _pool_tiny(s, 4)
    assert g["cluster"].tolist() == [0, 2, 3, 1, 4]              # equal fitness in node order: sorted order is nodes 3, 1, 2, 4
    assert g["node_type"].tolist() == [0, 1, 1, 1, 1]
    # equal distance: node 2 lies exactly between the two seeds -> the lowest seed
    s = _tiny([(0.0, 0.0), (0.25, 0.0), (0.5, 0.0), (0.75, 0.0), (1.0, 0.0), (0.5, 0.0)], [0.0, 0.0, 0.0, 0.0, 0.0, 0.0], [], [], [])
    g = _pool_tiny(s, 0.2)                                        # six members, step 5: seeds = sorted positions 0 and 5 = nodes 1 and 6
    assert g["cluster"].tolist() == [0, 1, 1, 2, 2, 2, 2]        # node 2 is 0.25 from seed 1 and 0.25 from seed 6: the lowest; nodes 3, 4, 5 are nearer to seed 6


def test_a_childless_level1_cluster_contributes_no_level2_cluster():
    # three level-1 nodes, every one a seed (ratio 4); only nodes 1 and 3 have children
    s = _tiny([(0.0, 0.0), (0.5, 0.5), (1.0, 1.0)], [0.1, 0.2, 0.3], [(0.0, 0.1), (0.1, 0.0), (1.0, 0.9)], [0.5, 0.6, 0.7], [0, 0, 2])
    g = _pool_tiny(s, 4)
    assert g["node_type"].tolist() == [0, 1, 1, 1, 2, 2, 2]
    assert g["tree"].tolist() == [-1, 0, 0, 0, 1, 1, 3]          # two clusters under cluster 1, none under 2, one under 3
    assert g["cluster"].tolist() == [0, 1, 2, 3, 4, 5, 6]
    ref = C.ihpool_ref(s["x"], s["edge_index_tree_8nb"], s["node_type"], s["node_tree"], s["x_y_index"], torch.ones(1, 1, dtype=torch.float64),
                       torch.ones(1, 1, dtype=torch.float64), 4)
    for f in DISCRETE:
        assert torch.equal(g[f], ref[f]), f


def test_misordered_nodes_are_refused():
    from wsi_hgnn_amd import h2mil
    s = C.tree_slide(0, 3, (1, 2), feat=4)
    for bad_type in ([1, 0], [0, 2, 1]):
        t = dict(s)
        nt = s["node_type"].clone()
        nt[:len(bad_type)] = torch.tensor(bad_type)
        t["node_type"] = nt
        with pytest.raises(ValueError, match="ordered root, level 1, level 2"):
            h2mil.from_slides([t])
    t = dict(s)
    t["node_tree"] = s["node_tree"].clone()
    t["node_tree"][-1] = 0
    with pytest.raises(ValueError, match="node_tree"):
        h2mil.from_slides([t])
    t = dict(s)
    t["edge_index_tree_8nb"] = torch.tensor([[0], [99]])
    with pytest.raises(ValueError, match="outside the slide"):
        h2mil.from_slides([t])


# ------------------------------------------------------------------------------------------------ the boundary
def test_new_entry_points_refuse_cpu_tensors_and_bad_arguments():
    from wsi_hgnn_amd import ops, _native as N
    n, Cw = 5, 4
    nt = torch.tensor([0, 1, 1, 2, 2])
    ec = ops.edge_csr_by_source_type(torch.tensor([0, 1, 3]), torch.tensor([1, 2, 2]), nt, n)
    ft, sc, bias = torch.zeros(n, Cw), torch.zeros(n, 4), torch.zeros(Cw)
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.ra_attention(ft, sc, bias, ec, nt)
    with pytest.raises(ValueError, match=r"sc is an fp32 \[5, 4\]"):
        ops.ra_attention(ft, torch.zeros(n, 3), bias, ec, nt)
    with pytest.raises(ValueError, match="ft is an fp32"):
        ops.ra_attention(ft.double(), sc, bias, ec, nt)
    with pytest.raises(ValueError, match="bias"):
        ops.ra_attention(ft, sc, torch.zeros(Cw + 1), ec, nt)
    with pytest.raises(ValueError, match="node_type"):
        ops.ra_attention(ft, sc, bias, ec, nt[:4])
    with pytest.raises(ValueError, match="edge_csr_by_source_type"):
        ops.ra_attention(ft, sc, bias, ops.EdgeCSR(torch.tensor([1]), torch.tensor([0]), n), nt)
    i32 = lambda *v: torch.tensor(v, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.ihpool_assign(torch.zeros(3, 3), i32(0, 1), i32(0, 0), i32(0, 1), i32(0))
    with pytest.raises(ValueError, match="xyf"):
        ops.ihpool_assign(torch.zeros(3, 2), i32(0, 1), i32(0, 0), i32(0, 1), i32(0))
    with pytest.raises(ValueError, match="int32"):
        ops.ihpool_assign(torch.zeros(3, 3), torch.tensor([0, 1]), i32(0, 0), i32(0, 1), i32(0))
    lib = N.load()
    err = lambda: lib.wsi_last_error().decode()
    EINVAL = -22
    assert lib.wsi_ra_attn_fwd(None, 0, None, None, 4, 0, None, None, 0.2, None, None, 0, None, None) == EINVAL and "bad shape" in err()
    assert lib.wsi_ra_attn_fwd(None, 0, None, None, 4, 4097, None, None, 0.2, None, None, 0, None, None) == EINVAL and "bad shape" in err()
    assert lib.wsi_ra_attn_fwd(None, 2, None, None, 4, 4, None, None, 0.2, None, None, 4, None, None) == EINVAL and "row stride" in err()
    assert lib.wsi_ra_attn_fwd(None, 4, None, None, 4, 4, None, None, 0.2, None, None, 4, None, None) == EINVAL and "null pointer" in err()
    assert lib.wsi_ra_attn_fwd(None, 4, None, None, 0, 4, None, None, 0.2, None, None, 4, None, None) == 0
    bwd = lambda n_, E_, C_: lib.wsi_ra_attn_bwd(None, C_, None, None, None, None, C_, n_, E_, C_, None, None, None, None, None, 0.2, None, None, None,
                                                 None, C_, None, None, None)
    assert bwd(3, -1, 4) == EINVAL and "E=-1" in err()
    assert bwd(3, 2, 0) == EINVAL and "bad shape" in err()
    assert bwd(3, 2, 4) == EINVAL and "null pointer" in err()
    assert bwd(0, 0, 4) == 0
    assert lib.wsi_ihpool_assign(None, -1, None, None, 0, None, None, 0, 0, None, None) == EINVAL and "bad shape" in err()
    assert lib.wsi_ihpool_assign(None, 3, None, None, 2, None, None, 1, 1, None, None) == EINVAL and "null pointer" in err()
    assert lib.wsi_ihpool_assign(None, 3, None, None, 0, None, None, 1, 1, None, None) == 0
    assert N.WSI_RA_BIAS_PARTS == 64


# ------------------------------------------------------------------------------------------------ the ra_attention dispatch sweep
# What tests/test_h2mil_kernels_gpu.py runs on the GPU is decided and checked here, without one: which kernel instantiation every width
# reaches, what the sweep graph contains, and that every case leaves the kernels room (tests/h2mil_cases.py: ra_case).
def ra_cfg(C, vec4_ok=True):
    """The dispatch code of csrc/ra_attn.hip's call of row_cfg, and the chunks per lane the width needs."""
    vec, G, NK = R.row_cfg(C, C, 1, vec4_ok)
    return R.code(vec, G, NK), -(-(C // vec) // G)


def ra_code(C, vec4_ok=True):
    return ra_cfg(C, vec4_ok)[0]


def test_ra_sweep_reaches_every_dispatch_code():
    codes = R.family_codes("ra_attn.hip")
    assert len(codes) == len(set(codes)) == 20 and codes == sorted(sum(R.case_lists(), []))
    before = {ra_code(Cw) for Cw in C.RA_WIDTHS_BEFORE}
    assert before == {100401, 400401, 400801, 406401, 406402}
    assert all(Cw % 4 == 0 for Cw in C.RA_SWEEP_VEC4) and all(Cw % 4 for Cw in C.RA_SWEEP_VEC1) and len(set(C.RA_SWEEP)) == len(C.RA_SWEEP) == 22
    reached = {}
    for Cw in C.RA_SWEEP:
        reached.setdefault(ra_code(Cw), []).append(Cw)
    assert sorted(set(reached) | before) == codes, f"not reached: {sorted(set(codes) - set(reached) - before)}"
    assert sorted(reached) == codes                                                # the sweep alone reaches them too
    # no width repeats another's kernel, but for the partly filled and the full last chunk of the widest code of each family
    twice = {code: ws for code, ws in reached.items() if len(ws) > 1}
    assert twice == {406416: [2052, 4096], 106464: [2050, 4095]}
    assert ra_cfg(2052) == (406416, 9) and ra_cfg(4096) == (406416, 16) and ra_cfg(2050) == (106464, 33) and ra_cfg(4095) == (106464, 64)
    # no width on a boundary of the rule: but for the full width 4096, the last lane of a group has less to do than the first
    for Cw in C.RA_SWEEP:
        code = ra_code(Cw)
        vec, G, NK = code // 100000, code // 100 % 1000, code % 100
        assert (Cw // vec < G * NK) == (Cw != 4096), Cw
    # an idle chunk index (k with VEC * G * k >= C for every lane) exists at every NK >= 4
    for NK in (4, 8, 16, 32, 64):
        assert any(ra_cfg(Cw)[0] % 100 == NK and ra_cfg(Cw)[1] < NK for Cw in C.RA_SWEEP), NK
    # the scalar fallback at multiples of 4: its codes exist and differ from the vector family's
    for Cw in C.RA_FALLBACK_WIDTHS:
        assert Cw % 4 == 0 and Cw in C.RA_SWEEP and ra_code(Cw, False) in codes and ra_code(Cw, False) // 100000 == 1 and ra_code(Cw) // 100000 == 4
    assert [ra_code(Cw, False) for Cw in C.RA_FALLBACK_WIDTHS] == [100801, 106401, 106404, 106416]
    # what the other cases are there for: one width per group size at peaked scores, one width per family at the other slopes
    assert {ra_code(Cw) // 100 % 1000 for Cw in C.RA_ONE_HOT_WIDTHS} == {4, 8, 16, 32, 64} and {2052, 2050} <= set(C.RA_ONE_HOT_WIDTHS)
    for slope in (0.05, 0.0):
        assert sorted(ra_code(Cw) // 100000 for Cw, s in C.RA_SLOPE_CASES if s == slope) == [1, 4]
    assert all(Cw in C.RA_SWEEP for Cw in C.RA_ONE_HOT_WIDTHS + C.RA_DEGENERATE_WIDTHS + tuple(Cw for Cw, _ in C.RA_SLOPE_CASES))


def test_ra_sweep_graph_has_what_it_promises():
    from wsi_hgnn_amd import ops
    n, nt, ei = C.ra_graph("sweep")
    ec = ops.edge_csr_by_source_type(ei[0], ei[1], nt, n)
    indeg, outdeg = C.ra_sweep_facts(n, nt, ei, ec.rowptr, ec.colptr)
    print(f"sweep graph: E = {ei.shape[1]}, hub out-degrees {[int(outdeg[h]) for h, _ in C.RA_HUBS]}, sinks {int((outdeg == 0).sum())}, "
          f"largest in-degree {int(indeg.max())}")
    # the stride loops over a source's edges make a second trip: 16 lanes in pass C, up to 64 in pass A
    assert int(outdeg[10]) > 16 and int(outdeg[11]) > 64 and int(outdeg[12]) > 3 * 64
    old_n, old_nt, old_ei = C.ra_kernel_graph()
    assert int(torch.bincount(old_ei[0], minlength=old_n).max()) <= 16                         # why the old graph could not reach them
    deg = C.ra_degenerate_graphs()
    assert deg["one-node"][0] == 1 and deg["one-node"][2].shape == (2, 0)
    n5, nt5, ei5 = deg["ring-of-three"]
    assert n5 == 5 and ei5.t().tolist() == [[0, 1], [1, 2], [2, 0]] and n5 < 64


@pytest.mark.parametrize("name,Cw,scale,slope", C.ra_gpu_cases(), ids=[f"{g}-{w}-x{int(s)}-{sl}" for g, w, s, sl in C.ra_gpu_cases()])
def test_ra_cases_leave_the_kernels_their_margin(name, Cw, scale, slope):
    """Every case of the GPU tests, on the seed ``ra_case`` settles on (the first of 20 that meets both conditions): the fp32 CPU run of the
    restatement is within a quarter of the tolerance of float64 under every norm the GPU tests use, and no leaky_relu argument is nearer
    to zero than 1e-5 x the score scale."""
    n, nt, ei = C.ra_graph(name)
    case = C.ra_case((n, nt, ei), Cw, scale, slope)
    worst = max(case["e32"].items(), key=lambda kv: kv[1])
    print(f"{name} C={Cw} x{scale} slope {slope}: seed {case['seed']}, kink distance {case['kink']:.3e}, largest fp32 figure {worst[1]:.3e} ({worst[0]})")
    assert case["kink"] >= C.RA_KINK * scale
    assert C.ra_kink_distance(case["inputs"][1], ei, nt) == case["kink"]
    assert max(case["e32"].values()) <= C.RA_TOL / 4, case["e32"]
    names = set(case["e32"])
    assert {"out", "g_ft", "g_sc", "g_bias"} <= names
    if name == "sweep":
        assert {f"out[{r}]" for r in C.RA_OUT_ROWS} | {f"g_ft[{r}]" for r in C.RA_GFT_ROWS} | {"g_el", "g_er", "g_pl", "g_pr"} <= names
    else:
        assert not case["ref"][2].any()                          # every softmax has one term: the score gradients are exactly zero


def test_a_plan_without_edges_still_passes_addresses():
    """An empty tensor has no address and wsi_ra_attn_fwd / _bwd refuse NULL: ``ops.ra_attention`` on a graph without edges (the one-node
    case of the GPU tests; it answered 'null pointer' before) hands over one unread element per edge array, and the plan's own otherwise."""
    from wsi_hgnn_amd import ops
    n, nt, ei = C.ra_graph("one-node")
    ec = ops.edge_csr_by_source_type(ei[0], ei[1], nt, n)
    assert ec.num_edges == 0 and ec.rowptr.tolist() == [0, 0] and ec.colptr.tolist() == [0, 0]
    assert all(t.numel() == 1 and t.dtype == torch.int32 for t in ops._ra_edges(ec))
    n, nt, ei = C.ra_graph("ring-of-three")
    ec = ops.edge_csr_by_source_type(ei[0], ei[1], nt, n)
    src, eid, dst = ops._ra_edges(ec)
    assert src is ec.src and eid is ec.csc_eid and dst is ec.csc_dst


def test_ra_stat_restatement_agrees_with_the_attention_restatement():
    """``ra_stat_ref`` (the loops) against ``ra_attention_ref`` (the dense form): out rebuilt from stat's max, log-sum and beta."""
    n, nt, ei = C.ra_graph("sweep")
    ft, sc, bias, _ = C.ra_inputs(n, 7)
    stat = C.ra_stat_ref(sc, ei, nt)
    u, v = ei[0], ei[1]
    s = torch.nn.functional.leaky_relu(sc.double()[u, 0] + sc.double()[v, 1], 0.2)
    a = torch.exp(s - stat[v, nt[u], 0] - stat[v, nt[u], 1]) * stat[v, nt[u], 3]
    out = torch.zeros(n, 7, dtype=torch.float64).index_add(0, v, a[:, None] * ft.double()[u]) + bias.double()
    _close(out, C.ra_attention_ref(ft.double(), sc.double(), bias.double(), ei, nt), "out from stat")
    present = stat[:, :, 2] > 0
    assert torch.equal(stat[:, :, 2].sum(1).long(), torch.bincount(v, minlength=n))
    assert bool((stat[~present] == torch.tensor([math.inf, 0.0, 0.0, 0.0], dtype=torch.float64)).all())


def test_assign_cases_outside_the_tables_and_over_three_tiles():
    case, _ = C.find_case(C.assign_outside_case, lambda c: c[6])
    buf, member_node, member_seg, seed_ptr, seed_node, want, _ = case
    T, lead = C.ASSIGN_TABLE, C.ASSIGN_LEAD
    assert buf.shape == (C.ASSIGN_ROWS, 3) and seed_ptr.tolist() == [0, 5, 6, 71, 74]
    for t in (member_node, seed_node):                           # every index, followed or not, stays inside the buffer
        assert int(t.min()) >= -lead and int(t.max()) < C.ASSIGN_ROWS - lead
    out_seed = ((seed_node < 0) | (seed_node >= T)).nonzero().view(-1).tolist()
    assert out_seed == [1, 3, 5, 6 + 64] and int(seed_node[1]) < 0 and int(seed_node[3]) >= T
    out_member = (member_node < 0) | (member_node >= T)
    assert int(out_member.sum()) == 3 and bool((member_seg[out_member] == 3).all())
    assert bool((want[out_member] == -1).all()) and bool((want[member_seg == 1] == -1).all()) and bool((want[member_seg >= 4] == -1).all())
    assert int((member_seg >= 4).sum()) == 10 and bool((member_seg[1:] >= member_seg[:-1]).all())
    assert int((member_seg < 0).sum()) == 4 and bool((want[member_seg < 0] == -1).all())
    rest = ~out_member & (member_seg != 1) & (member_seg >= 0) & (member_seg < 4)
    assert bool((want[rest] >= 0).all())
    for s, bad in ((0, (1, 3)), (2, (64,))):                     # an outside seed is never chosen; its neighbours keep their positions
        got = set(want[member_seg == s].tolist())
        assert not got & set(bad) and max(got) > max(bad) - (s == 2) * 64
    # every lure is in place: following an outside index would have changed the answer
    for p in out_seed:
        seg = int((seed_ptr[1:] > p).nonzero()[0])
        mem = member_node[(member_seg == seg) & ~out_member].long()
        assert bool((buf[lead + mem] == buf[lead + int(seed_node[p])]).all(1).any())
    for i in out_member.nonzero().view(-1).tolist():
        assert torch.equal(buf[lead + int(member_node[i])], buf[lead + int(seed_node[seed_ptr[3]])])
    tiles, _ = C.find_case(C.assign_tiles_case, lambda c: float(C.assign_ref(*c)[1].min()))
    assert tiles[3].diff().tolist() == [128, 129]
    got = C.assign_ref(*tiles)[0]
    for s, k in enumerate((128, 129)):
        mine = got[tiles[2] == s]
        assert int(mine.min()) >= 0 and int(mine.max()) == k - 1 and int((mine >= 64).sum()) > 0       # the later tiles are chosen from
