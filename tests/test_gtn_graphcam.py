"""GraphCAM of the GTNMIL baseline on the CPU (``gtn.graphcam`` in its tensor-operation form) against the recorded run of the reference's own
``relprop`` (tests/golden/gtn/reference_graphcam.npz, made by tests/golden/make_reference_graphcam_fixture.py) and against the float64
restatement of tests/graphcam_cases.py.

Bounds.  float64 against the reference: 1e-6 x the largest entry of each tensor (a restatement that simplified the clone rule to r1 + r2
measured 4e-8; a wrong rule is off by order 1).  float32: max(1e-4, 4 E32), E32 the largest recorded float32 error of the REFERENCE's own code
at that shape (the chain divides by signed sums, so float32 is that ill-conditioned in the reference itself; the factor 4 covers another order
of summation)."""
import pytest
import torch

import graphcam_cases as Q

TOL64 = 1e-6
SIZES = Q.MODEL_SIZES
IN_FEATS = Q.MODEL_IN_FEATS


def rel(got, want):
    return float((got.double() - want.double()).abs().max()) / max(float(want.abs().max()), 1e-300)


@pytest.fixture(scope="module")
def fix():
    return Q.load_fixture()


@pytest.fixture(scope="module", params=["small", "ref"])
def shape(request, fix):
    tag = request.param
    cfg = dict((t, c) for t, c, _ in Q.fixture_shapes(fix))[tag]
    return tag, cfg


@pytest.fixture(scope="module")
def restated(fix, shape):
    tag, (n, E, depth, H, C) = shape
    return Q.vit_graphcam(Q.fixture_state(fix, tag), Q.fixture_inputs(fix, tag), H)


def make_classifier(fix, tag, cfg, dtype, **kw):
    from wsi_hgnn_amd import gtn
    n, E, depth, H, C = cfg
    m = gtn.Classifier(C, in_feats=IN_FEATS, embed_dim=E, node_cluster_num=n - 1, depth=depth, num_heads=H, kernels=False, **kw)
    m.load_state_dict(Q.model_state(fix, tag))
    return m.to(dtype)


def make_batch(tag="small", sizes=SIZES, seed=None):
    from wsi_hgnn_amd import gtn
    return gtn.GraphBatch(*Q.model_batch(tag, sizes, seed))


# ------------------------------------------------------------------------------------------------ the restatement against the reference
def test_restatement_matches_the_reference(fix, shape, restated):
    tag, (n, E, depth, H, C) = shape
    want = torch.from_numpy(fix[f"{tag}.cluster_cam"])
    assert rel(restated["prob"], torch.from_numpy(fix[f"{tag}.prob"])) <= TOL64
    for s in range(want.shape[0]):
        for c in range(C):
            assert rel(restated["cluster_cam"][s, c], want[s, c]) <= TOL64, (tag, s, c)
    if tag == "small":
        cams, grads = torch.from_numpy(fix["small.attn_cam"]), torch.from_numpy(fix["small.attn_grad"])
        for l in range(depth):
            for s in range(want.shape[0]):
                for c in range(C):
                    assert rel(restated["attn_cam"][l][s, c], cams[s, c, l]) <= TOL64, ("attn_cam", l, s, c)
                    assert rel(restated["attn_grad"][l][s, c], grads[s, c, l]) <= TOL64, ("attn_grad", l, s, c)


def test_recorded_cases_are_within_the_float32_condition(fix, shape):
    assert Q.fixture_e32(fix, shape[0]) <= 1e-2
    assert len(dict((t, s) for t, _, s in Q.fixture_shapes(fix))[shape[0]]) == 6


# ------------------------------------------------------------------------------------------------ the package against both
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_token_maps_match_the_reference(fix, shape, dtype):
    from wsi_hgnn_amd import gtn
    from wsi_hgnn_amd.gtn import graphcam
    tag, (n, E, depth, H, C) = shape
    vt = gtn.VisionTransformer(num_classes=C, embed_dim=E, depth=depth, num_heads=H, kernels=False).to(dtype).eval()
    vt.load_state_dict(Q.fixture_state(fix, tag, dtype))
    prob, cam, maps = graphcam.token_maps(vt, Q.fixture_inputs(fix, tag, dtype), keep_layer_maps=True)
    want = torch.from_numpy(fix[f"{tag}.cluster_cam"])
    bound = TOL64 if dtype == torch.float64 else max(1e-4, 4 * Q.fixture_e32(fix, tag))
    worst = max(rel(cam[s, c], want[s, c]) for s in range(want.shape[0]) for c in range(C))
    print(f"{tag} {dtype}: cluster map error {worst:.3e}, bound {bound:.3e}")
    assert cam.dtype == dtype and worst <= bound
    assert len(maps) == depth and maps[0].shape == (want.shape[0], C, n, n)


@pytest.mark.parametrize("method", Q.METHODS)
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_class_maps_match_the_restatement(fix, shape, dtype, method):
    from wsi_hgnn_amd.gtn import graphcam
    tag, cfg = shape
    n, E, depth, H, C = cfg
    model = make_classifier(fix, tag, cfg, dtype)
    res = graphcam.class_maps(model, make_batch(tag), method=method, keep_layer_maps=True)
    sd64 = {k: v.double() for k, v in model.state_dict().items() if v.dtype.is_floating_point}
    ref = Q.vit_graphcam(sd64, res.tokens.double(), H, method=method, prefix="transformer.")
    bound = TOL64 if dtype == torch.float64 else max(1e-4, 4 * Q.fixture_e32(fix, tag))
    errs = Q.field_errors(res.cluster_cam, res.layer_maps, ref, len(SIZES), C)
    print(f"{tag} {dtype} {method}: " + ", ".join(f"{k} {v:.3e}" for k, v in errs.items()) + f"; bound {bound:.3e}")
    assert rel(res.prob, ref["prob"]) <= (TOL64 if dtype == torch.float64 else 1e-5)
    assert res.cluster_cam.shape == (len(SIZES), C, n - 1) and res.cluster_cam.dtype == dtype
    assert max(errs.values()) <= bound, errs
    # the node maps against the dense formula of src/vis_graphcam.py:71-101 on the same cluster maps
    assign, node_cam, node_heat = Q.node_maps(res.pool_logits.double(), SIZES, res.cluster_cam.double(), res.prob.double())
    tol = 1e-12 if dtype == torch.float64 else 1e-5
    assert res.assign.shape == (sum(SIZES), n - 1) and rel(res.assign, assign) <= tol
    assert res.node_cam.shape == (sum(SIZES), C) and rel(res.node_cam, node_cam) <= tol
    assert float((res.node_heat.double() - node_heat).abs().max()) <= (1e-9 if dtype == torch.float64 else 1e-3)
    assert float(res.node_heat.min()) >= 0 and float(res.node_heat.max()) <= 1


@pytest.mark.parametrize("method", Q.METHODS)
def test_the_model_case_is_within_the_float32_condition(fix, shape, method):
    """The admission condition of the model case (graphcam_cases.MODEL_BATCH_SEED): the restatement's OWN float32 run on the case's tokens stays
    within 1 / MODEL_CONDITION of the float32 bound (the reasons: graphcam_cases.py)."""
    from wsi_hgnn_amd.gtn import graphcam
    tag, cfg = shape
    model = make_classifier(fix, tag, cfg, torch.float32)
    tokens = graphcam.class_maps(model, make_batch(tag)).tokens
    sd32 = {k: v for k, v in model.state_dict().items() if v.dtype.is_floating_point}
    r64 = Q.vit_graphcam({k: v.double() for k, v in sd32.items()}, tokens.double(), cfg[3], method=method, prefix="transformer.")
    r32 = Q.vit_graphcam(sd32, tokens, cfg[3], method=method, prefix="transformer.")
    errs = Q.field_errors(r32["cluster_cam"], r32["layer_maps"], r64, len(SIZES), cfg[4])
    print(f"{tag} {method}: e32' of the restatement " + ", ".join(f"{k} {v:.3e}" for k, v in errs.items()))
    assert max(errs.values()) <= max(1e-4, 4 * Q.fixture_e32(fix, tag)) / Q.MODEL_CONDITION, errs


def test_classes_subset_and_a_slide_alone(fix):
    from wsi_hgnn_amd.gtn import graphcam
    tag, cfg = "small", dict((t, c) for t, c, _ in Q.fixture_shapes(fix))["small"]
    model = make_classifier(fix, tag, cfg, torch.float64)
    full = graphcam.class_maps(model, make_batch())
    one = graphcam.class_maps(model, make_batch(), classes=[1])
    assert one.classes == [1] and one.cluster_cam.shape[1] == 1 and one.node_heat.shape[1] == 1
    assert torch.equal(one.cluster_cam[:, 0], full.cluster_cam[:, 1]) and torch.equal(one.node_heat[:, 0], full.node_heat[:, 1])
    both = graphcam.class_maps(model, make_batch(), classes=[2, 0])
    assert torch.equal(both.cluster_cam[:, 0], full.cluster_cam[:, 2]) and torch.equal(both.cluster_cam[:, 1], full.cluster_cam[:, 0])
    alone = graphcam.class_maps(model, make_batch(sizes=SIZES[1:2], seed=1823))
    three = graphcam.class_maps(model, make_batch(sizes=(SIZES[1],) * 3, seed=1823))      # (the first slide of a seeded batch is the same slide)
    assert torch.equal(alone.tokens[0], three.tokens[0])
    assert rel(three.cluster_cam[0], alone.cluster_cam[0]) <= 1e-6 and rel(three.node_cam[:SIZES[1]], alone.node_cam) <= 1e-6


def test_start_layer(fix):
    from wsi_hgnn_amd.gtn import graphcam
    tag, cfg = "ref", dict((t, c) for t, c, _ in Q.fixture_shapes(fix))["ref"]
    model = make_classifier(fix, tag, cfg, torch.float64)
    sd64 = {k: v.double() for k, v in model.state_dict().items() if v.dtype.is_floating_point}
    for start in (1, 2):
        res = graphcam.class_maps(model, make_batch("ref", sizes=(9, 5)), start_layer=start)
        ref = Q.vit_graphcam(sd64, res.tokens, cfg[3], start_layer=start, prefix="transformer.")
        assert rel(res.cluster_cam, ref["cluster_cam"]) <= TOL64
    with pytest.raises(ValueError):
        graphcam.class_maps(model, make_batch("ref", sizes=(9, 5)), start_layer=3)


# ------------------------------------------------------------------------------------------------ the rules at their edges
def test_safe_divide_edges():
    from wsi_hgnn_amd.gtn import graphcam
    for sd in (graphcam.sd, Q.sd):
        for dtype in (torch.float64, torch.float32):
            a = torch.tensor([3.0, -2.0, 0.0, 5.0, 1.0], dtype=dtype)
            b = torch.tensor([0.0, 0.0, 0.0, -1e-9, 2.0], dtype=dtype)
            out = sd(a, b)
            assert out.dtype == dtype and torch.equal(out[:3], torch.zeros(3, dtype=dtype))              # exact zeros, not 3 / 1e-9
            assert float(out[3]) == float(a[3] / torch.tensor(1e-9, dtype=dtype))                         # b + 1e-9 == 0: the denominator 1e-9
            assert float(out[4]) == float(a[4] / (b[4] + 1e-9))


def test_a_zero_token_row_gets_zero_relevance():
    from wsi_hgnn_amd.gtn import graphcam
    X, W, R = Q.linear_case(2, 3, 5, 8, 12, seed=5, signed=True)
    X[1, 3] = 0
    for lin in (graphcam._lin, Q.lin):
        out = lin(X.double(), W.double(), R.double())
        assert torch.equal(out[1, :, 3], torch.zeros(3, 8, dtype=torch.float64)) and float(out[1, :, 2].abs().min()) > 0
    X, r1, r2, A, B = Q.residual_case(2, 3, 5, 8, seed=6)
    a, b = graphcam._residual(X.double(), r1.double(), r2.double(), A.double(), B.double())
    ra, rb = Q.residual(X.double(), r1.double(), r2.double(), A.double(), B.double())
    assert rel(a, ra) <= 1e-12 and rel(b, rb) <= 1e-12
    planted = (A + B) == 0
    assert planted.any() and float(a[planted.unsqueeze(1).expand_as(a)].abs().max()) == 0                 # A = -B: sd(., 0) = 0


def test_linear_rule_matches_the_reference_form():
    """``lin`` against layers.Linear.relprop written with autograd as the reference does (alpha = 1)."""
    X, W, R = (t.double() for t in Q.linear_case(1, 1, 6, 8, 12, seed=7, signed=True))
    x1, x2 = X.clamp(min=0).requires_grad_(True), X.clamp(max=0).requires_grad_(True)
    Z1, Z2 = x1 @ W.clamp(min=0).t(), x2 @ W.clamp(max=0).t()
    S = Q.sd(R[:, 0], Z1 + Z2).detach()
    want = x1 * torch.autograd.grad(Z1, x1, S)[0] + x2 * torch.autograd.grad(Z2, x2, S)[0]
    assert rel(Q.lin(X, W, R)[:, 0], want.detach()) <= 1e-12


# ------------------------------------------------------------------------------------------------ the interface
def test_refused_methods_and_heads(fix):
    from wsi_hgnn_amd import gtn
    from wsi_hgnn_amd.gtn import graphcam
    cfg = dict((t, c) for t, c, _ in Q.fixture_shapes(fix))["small"]
    model = make_classifier(fix, "small", cfg, torch.float32)
    for method in ("full", "grad", "last_layer", "last_layer_attn", "second_layer"):
        with pytest.raises(NotImplementedError, match=method):
            graphcam.class_maps(model, make_batch(), method=method)
    with pytest.raises(ValueError):
        graphcam.class_maps(model, make_batch(), method="nonsense")
    with pytest.raises(NotImplementedError, match="alpha"):
        graphcam.class_maps(model, make_batch(), alpha=0.5)
    with pytest.raises(ValueError):
        graphcam.class_maps(model, make_batch(), classes=[3])
    vt = gtn.VisionTransformer(num_classes=3, embed_dim=32, depth=1, num_heads=4, mlp_head=True, kernels=False)
    with pytest.raises(NotImplementedError, match="mlp_head"):
        graphcam.token_maps(vt, torch.randn(1, 5, 32))
    with pytest.raises(NotImplementedError, match="mlp_head"):
        vt.forward_saving(torch.randn(1, 5, 32))


def test_the_model_is_left_as_it_was(fix):
    from wsi_hgnn_amd import gtn
    from wsi_hgnn_amd.gtn import graphcam
    cfg = dict((t, c) for t, c, _ in Q.fixture_shapes(fix))["small"]
    n, E, depth, H, C = cfg
    model = make_classifier(fix, "small", cfg, torch.float32)
    plain = gtn.Classifier(C, in_feats=IN_FEATS, embed_dim=E, node_cluster_num=n - 1, depth=depth, num_heads=H, kernels=False)
    keys = list(model.state_dict().keys())
    assert keys == list(plain.state_dict().keys())
    assert [k for k in keys if k.startswith("transformer.")] == ["transformer." + k for k in Q.fixture_state(fix, "small")]   # the reference's own keys
    state = {k: v.clone() for k, v in model.state_dict().items()}
    batch = make_batch()
    model.eval()
    with torch.no_grad():
        before = model.logits(batch)[0]
    for training in (True, False):
        model.train(training)
        graphcam.class_maps(model, batch)
        assert model.training is training
        assert all(p.grad is None for p in model.parameters())
        assert list(model.state_dict().keys()) == keys and all(torch.equal(v, state[k]) for k, v in model.state_dict().items())
    model.eval()
    with torch.no_grad():
        assert torch.equal(model.logits(batch)[0], before)
    # forward_saving computes forward's logits
    model.eval()
    tokens = graphcam.class_maps(model, batch).tokens
    with torch.no_grad():
        logits, saved, x0 = model.transformer.forward_saving(tokens)
        assert torch.equal(logits, model.transformer(tokens))
    assert len(saved) == depth and set(saved[0]) == {"x_in", "norm1_out", "qkv", "lse", "attn_concat", "proj_out", "x_mid", "norm2_out", "gelu_out", "mlp_out"}
    assert x0.shape == (len(SIZES), E) and saved[0]["lse"].shape == (len(SIZES), H, n)


def test_save_reference_files_round_trip(fix, tmp_path):
    from wsi_hgnn_amd.gtn import graphcam
    cfg = dict((t, c) for t, c, _ in Q.fixture_shapes(fix))["small"]
    model = make_classifier(fix, "small", cfg, torch.float32)
    res = graphcam.class_maps(model, make_batch())
    g, a, b = 1, SIZES[0], SIZES[0] + SIZES[1]
    graphcam.save_reference_files(res, g, str(tmp_path / "graphcam"))
    load = lambda name: torch.load(str(tmp_path / "graphcam" / name))
    assert torch.equal(load("s_matrix_ori.pt"), res.pool_logits[a:b])
    assert torch.equal(load("s_matrix.pt"), res.assign[a:b].argmax(1)) and load("s_matrix.pt").shape == (SIZES[1],)
    assert load("prob.pt").shape == (1, 3) and torch.equal(load("prob.pt"), torch.softmax(res.prob[g:g + 1], -1))    # the reference's double softmax
    for c in range(3):
        assert load(f"cam_{c}.pt").shape == (1, cfg[0] - 1) and torch.equal(load(f"cam_{c}.pt"), res.cluster_cam[g:g + 1, c])
    # what src/vis_graphcam.py:71-92 computes from those files is the slide's node map
    m = torch.softmax(load("s_matrix_ori.pt"), 1) @ load("cam_2.pt").transpose(1, 0)
    assert rel(m[:, 0], res.node_cam[a:b, 2]) <= 1e-5
    with pytest.raises(IndexError):
        graphcam.save_reference_files(res, 3, str(tmp_path / "graphcam"))


def test_a_constant_map_has_heat_zero(fix):
    """A slide of one row has min == max: the reference divides 0 by 0, the package defines the heat as 0."""
    from wsi_hgnn_amd.gtn import graphcam
    cfg = dict((t, c) for t, c, _ in Q.fixture_shapes(fix))["small"]
    model = make_classifier(fix, "small", cfg, torch.float32)
    res = graphcam.class_maps(model, make_batch(sizes=(1, 6)))
    assert torch.equal(res.node_heat[0], torch.zeros(3)) and torch.isfinite(res.node_heat).all() and float(res.node_heat[1:].max()) > 0
    _, _, heat = Q.node_maps(res.pool_logits.double(), (1, 6), res.cluster_cam.double(), res.prob.double())
    assert float((res.node_heat.double() - heat).abs().max()) <= 1e-3


def test_kernel_cases_are_within_the_float32_condition():
    """The signed (cancelling) inputs of the GPU kernel tests: their float32 CPU error e32' stays below 1e-2 at the fixed seeds."""
    for name, fn, inputs in Q.signed_cases():
        e = Q.rel_err_f32(fn, *inputs)
        print(f"{name}: e32' {e:.3e}")
        assert e <= 1e-2, name
