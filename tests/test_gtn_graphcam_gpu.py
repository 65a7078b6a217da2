"""GraphCAM of the GTNMIL baseline on the GPU: ``gtn.graphcam.class_maps`` over the relevance kernels against the float64 restatement
(tests/graphcam_cases.py) fed the same pooled tokens, against its own tensor-operation form on the device, without a host synchronisation, and
leaving training untouched.  The model carries the transformer weights recorded from the reference (tests/golden/gtn/reference_graphcam.npz) at
both recorded shapes; the batch is graphcam_cases.model_batch: 3 slides of 40 / 129 / 7 rows.

Bound: max(1e-4, 4 E32) x the largest float64 entry of each (slide, class) tensor, E32 the largest float32 error of the reference's own code
recorded for the shape.  The factor 4 covers another order of summation, which moves the near-zero denominator that dominates; a slip in a
formula (a missing / 2, a scaled q k^T, a sum over the batch instead of the slide) moves a map by 10 % and more."""
import pytest
import torch

import graphcam_cases as Q

pytestmark = pytest.mark.gpu

DEV = "cuda"
SIZES = Q.MODEL_SIZES
RATIOS = {}


@pytest.fixture(scope="module")
def fix():
    return Q.load_fixture()


@pytest.fixture(scope="module", params=["small", "ref"])
def shape(request, fix):
    return request.param, dict((t, c) for t, c, _ in Q.fixture_shapes(fix))[request.param]


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for k, v in sorted(RATIOS.items()):
        print(f"\nlargest e_gpu / E32, {k}: {v:.3e}", end="")
    print()


def make_model(fix, tag, cfg, kernels=True):
    from wsi_hgnn_amd import gtn
    n, E, depth, H, C = cfg
    m = gtn.Classifier(C, in_feats=Q.MODEL_IN_FEATS, embed_dim=E, node_cluster_num=n - 1, depth=depth, num_heads=H, kernels=kernels)
    m.load_state_dict(Q.model_state(fix, tag))
    return m.to(DEV)


def make_batch(tag, sizes=SIZES):
    from wsi_hgnn_amd import gtn
    x, row, col, w, sizes = Q.model_batch(tag, sizes)
    return gtn.GraphBatch(x.to(DEV), row.to(DEV), col.to(DEV), w.to(DEV), sizes)


def _note(tag, what, errs, e32):
    for k, v in errs.items():
        key = f"{tag} {what} {k}"
        RATIOS[key] = max(RATIOS.get(key, 0.0), v / e32)


@pytest.mark.parametrize("method", Q.METHODS)
def test_class_maps_against_float64(fix, shape, method):
    from wsi_hgnn_amd.gtn import graphcam
    tag, cfg = shape
    n, E, depth, H, C = cfg
    model = make_model(fix, tag, cfg)
    assert graphcam.kernels_cover(model.transformer, n)
    res = graphcam.class_maps(model, make_batch(tag), method=method, keep_layer_maps=True)
    sd64 = {k: v.double().cpu() for k, v in model.state_dict().items() if v.dtype.is_floating_point}
    ref = Q.vit_graphcam(sd64, res.tokens.double().cpu(), H, method=method, prefix="transformer.")
    e32 = Q.fixture_e32(fix, tag)
    bound = max(1e-4, 4 * e32)
    errs = Q.field_errors(res.cluster_cam.cpu(), [m.cpu() for m in res.layer_maps], ref, len(SIZES), C)
    _, node_cam, node_heat = Q.node_maps(res.pool_logits.double().cpu(), SIZES, ref["cluster_cam"], ref["prob"])
    rel = lambda a, b: float((a.double().cpu() - b).abs().max()) / float(b.abs().max())
    errs["node_cam"], errs["node_heat"] = rel(res.node_cam, node_cam), rel(res.node_heat, node_heat)
    print(f"{tag} {method}: " + ", ".join(f"{k} {v:.3e}" for k, v in errs.items()) + f"; E32 {e32:.3e}, bound {bound:.3e}")
    _note(tag, "against float64,", errs, e32)
    assert all(torch.isfinite(t).all() for t in (res.cluster_cam, res.node_cam, res.node_heat))
    assert float((res.prob.double().cpu() - ref["prob"]).abs().max()) <= 1e-5
    assert max(errs.values()) <= bound, errs


@pytest.mark.parametrize("method", Q.METHODS)
def test_kernels_against_tensor_operations(fix, shape, method):
    from wsi_hgnn_amd.gtn import graphcam
    tag, cfg = shape
    model = make_model(fix, tag, cfg)
    a = graphcam.class_maps(model, make_batch(tag), method=method, keep_layer_maps=True, kernels=True)
    b = graphcam.class_maps(model, make_batch(tag), method=method, keep_layer_maps=True, kernels=False)
    e32 = Q.fixture_e32(fix, tag)
    ref = dict(cluster_cam=b.cluster_cam.double().cpu(), layer_maps=[m.double().cpu() for m in b.layer_maps])
    errs = Q.field_errors(a.cluster_cam.cpu(), [m.cpu() for m in a.layer_maps], ref, len(SIZES), cfg[4])
    errs["node_cam"] = float((a.node_cam - b.node_cam).abs().max()) / float(b.node_cam.abs().max())
    errs["node_heat"] = float((a.node_heat - b.node_heat).abs().max()) / float(b.node_heat.abs().max())
    print(f"{tag} {method} kernels vs tensors: " + ", ".join(f"{k} {v:.3e}" for k, v in errs.items()))
    _note(tag, "against tensor operations,", errs, e32)
    assert max(errs.values()) <= max(1e-4, 4 * e32), errs


def test_identical_calls_give_identical_bits_and_classes_select(fix):
    from wsi_hgnn_amd.gtn import graphcam
    cfg = dict((t, c) for t, c, _ in Q.fixture_shapes(fix))["ref"]
    model, batch = make_model(fix, "ref", cfg), make_batch("ref")
    a, b = graphcam.class_maps(model, batch), graphcam.class_maps(model, batch)
    assert torch.equal(a.cluster_cam, b.cluster_cam) and torch.equal(a.node_heat, b.node_heat)
    one = graphcam.class_maps(model, batch, classes=[1])
    assert torch.equal(one.cluster_cam[:, 0], a.cluster_cam[:, 1])
    alone = graphcam.class_maps(model, make_batch("ref", SIZES[:1]))
    assert float((alone.cluster_cam[0] - a.cluster_cam[0]).abs().max()) <= max(1e-4, 4 * Q.fixture_e32(fix, "ref")) * float(a.cluster_cam[0].abs().max())


def test_class_maps_reads_nothing_back(fix):
    """Every launch of ``class_maps`` queues without a synchronising call (the per-class ``autograd.grad`` included)."""
    from wsi_hgnn_amd.gtn import graphcam
    cfg = dict((t, c) for t, c, _ in Q.fixture_shapes(fix))["ref"]
    model, batch = make_model(fix, "ref", cfg), make_batch("ref")
    first = graphcam.class_maps(model, batch)                      # (first use: code objects, the batch's plan and segment tables)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for method in Q.METHODS:
            res = graphcam.class_maps(model, batch, method=method, keep_layer_maps=True)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert res.cluster_cam.is_cuda and res.node_heat.is_cuda and res.prob.is_cuda and torch.isfinite(first.cluster_cam).all()


def test_training_is_untouched_by_a_class_maps_call(fix):
    from wsi_hgnn_amd import gtn, optim
    from wsi_hgnn_amd.gtn import graphcam
    cfg = dict((t, c) for t, c, _ in Q.fixture_shapes(fix))["small"]
    labels = torch.tensor([0, 2, 1], device=DEV)
    losses = []
    for explain in (False, True):
        model, batch = make_model(fix, "small", cfg), make_batch("small")
        model.train()
        opt = optim.Adam(model.parameters(), lr=1e-3)
        step = []
        for _ in range(2):
            if explain:
                graphcam.class_maps(model, batch)
                assert model.training
            step.append(gtn.train_one_step(model, batch, labels, opt))
        losses.append(torch.stack(step))
    assert torch.equal(losses[0], losses[1]), losses
