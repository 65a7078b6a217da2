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
