"""The GTNMIL model on the GPU: gtn.VisionTransformer against the fixture recorded from the reference's own transformer, gtn.Classifier against
the float64 restatement (tests/gtn_cases.py) in train and eval mode, the kernel path against the tensor-operation path, and a few training
steps.  Tolerance (tests/test_mil_kernels_gpu.py's norm): error <= 1e-4 x the largest float64 entry of each tensor."""
import os

import numpy as np
import pytest
import torch

import gtn_cases as C
from mil_cases import Ratios

pytestmark = pytest.mark.gpu

DEV = "cuda"
TOL = 1e-4
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R = Ratios(TOL)
SMALL = dict(n_class=3, in_feats=48, embed_dim=32, node_cluster_num=10, depth=2, num_heads=4)
WIDE = dict(n_class=3, in_feats=1024, embed_dim=64, node_cluster_num=100, depth=3, num_heads=8)


@pytest.fixture(scope="module", autouse=True)
def _report_ratios():
    yield
    R.report()


def _batch(slides, dev=DEV):
    from wsi_hgnn_amd import gtn
    off = np.concatenate([[0], np.cumsum([s[0].shape[0] for s in slides])])
    w = None if slides[0][3] is None else torch.cat([s[3] for s in slides]).to(dev)
    return gtn.GraphBatch(torch.cat([s[0] for s in slides]).to(dev), torch.cat([s[1] + int(o) for s, o in zip(slides, off)]).to(dev),
                          torch.cat([s[2] + int(o) for s, o in zip(slides, off)]).to(dev), w, [s[0].shape[0] for s in slides])


def _model(cfg, base, **kw):
    from wsi_hgnn_amd import gtn
    m = gtn.Classifier(cfg["n_class"], cfg["in_feats"], cfg["embed_dim"], cfg["node_cluster_num"], cfg["depth"], cfg["num_heads"], **kw)
    m.load_state_dict(base, strict=True)
    return m.to(DEV)


def test_transformer_against_the_reference_fixture():
    from wsi_hgnn_amd import gtn
    f = np.load(os.path.join(ROOT, "tests", "golden", "gtn", "reference_vit.npz"))
    n_class, E, depth, heads = (int(v) for v in f["config"])
    for fused in (True, False):
        m = gtn.VisionTransformer(num_classes=n_class, embed_dim=E, depth=depth, num_heads=heads, fused_attention=fused)
        m.load_state_dict({k: torch.from_numpy(f["sd." + k]) for k in m.state_dict()}, strict=True)
        m = m.to(DEV)
        x = torch.from_numpy(f["x"]).to(DEV).requires_grad_(True)
        out = m(x)
        (out * torch.from_numpy(f["w"]).to(DEV, torch.float32)).sum().backward()
        case = f"fixture fused={fused}"
        R.check(out, torch.from_numpy(f["logits"]), "vit logits", case)
        R.check(x.grad, torch.from_numpy(f["g.x"]), "vit g_x", case)
        for k, p in m.named_parameters():
            R.check(p.grad, torch.from_numpy(f["g." + k]), "vit g_param", f"{case} {k}")


def _against_cases(cfg, sizes, train, seed):
    slides = C.slides_case(sizes, cfg["in_feats"], seed=seed)
    labels = torch.tensor([(2 * i + 1) % cfg["n_class"] for i in range(len(sizes))])
    base = C.classifier_state(cfg["n_class"], cfg["in_feats"], cfg["embed_dim"], cfg["node_cluster_num"], cfg["depth"], cfg["num_heads"], seed=seed + 1)
    sd = C.as_float64_leaves(base)
    ref = C.classifier_forward(sd, slides, labels, cfg["num_heads"], train=train)
    ref["loss"].backward()
    m = _model(cfg, base)
    m.train(train)
    pred, lab, loss, probs = m(_batch(slides), labels.to(DEV))
    loss.backward()
    case = f"{'train' if train else 'eval'} E={cfg['embed_dim']}"
    R.check(loss, ref["loss"], "loss", case)
    R.check(probs, ref["probs"], "probs", case)
    assert torch.equal(pred.cpu(), ref["logits"].argmax(1))
    for k, p in m.named_parameters():
        R.check(p.grad, sd[k].grad, "g_param", f"{case} {k}")
    rm, rv = m.state_dict()["conv1.bn_layer.running_mean"], m.state_dict()["conv1.bn_layer.running_var"]
    if train:
        R.check(rm, 0.9 * sd["conv1.bn_layer.running_mean"] + 0.1 * ref["bn_mean"], "running_mean", case)
        R.check(rv, 0.9 * sd["conv1.bn_layer.running_var"] + 0.1 * ref["bn_var"], "running_var", case)
        assert int(m.state_dict()["conv1.bn_layer.num_batches_tracked"]) == 1
    else:
        assert torch.equal(rm.cpu(), base["conv1.bn_layer.running_mean"]) and torch.equal(rv.cpu(), base["conv1.bn_layer.running_var"])


@pytest.mark.parametrize("train", [True, False])
def test_classifier_against_float64(train):
    _against_cases(SMALL, (1, 40, 129), train, seed=21)


def test_classifier_at_the_reference_widths():
    _against_cases(WIDE, (40, 129), True, seed=31)


@pytest.mark.parametrize("train", [True, False])
def test_kernel_path_equals_the_tensor_operation_path(train):
    slides = C.slides_case((1, 40, 129), SMALL["in_feats"], seed=41)
    labels = torch.tensor([0, 2, 1], device=DEV)
    base = C.classifier_state(3, SMALL["in_feats"], 32, 10, 2, 4, seed=42)
    res = {}
    for kernels in (True, False):
        m = _model(SMALL, base, kernels=kernels)
        m.train(train)
        _, _, loss, probs = m(_batch(slides), labels)
        loss.backward()
        res[kernels] = (loss.detach(), probs.detach(), {k: p.grad for k, p in m.named_parameters()}, m.state_dict())
    case = "kernels vs tensors " + ("train" if train else "eval")
    R.check(res[True][0], res[False][0], "loss", case)
    R.check(res[True][1], res[False][1], "probs", case)
    for k in res[True][2]:
        R.check(res[True][2][k], res[False][2][k], "g_param", f"{case} {k}")
    for k in ("conv1.bn_layer.running_mean", "conv1.bn_layer.running_var"):
        R.check(res[True][3][k], res[False][3][k], k.split(".")[-1], case)


def test_a_graph_batch_gives_what_the_packed_batch_gives():
    import wsi_hgnn_amd as W
    from wsi_hgnn_amd import gtn, synthetic
    graphs = [synthetic.homogeneous_graph(n, SMALL["in_feats"], out_edges=3, seed=50 + n) for n in (40, 129)]
    g = W.batch(graphs).to(DEV)
    base = C.classifier_state(3, 48, 32, 10, 2, 4, seed=52)
    m = _model(SMALL, base).eval()
    labels = torch.tensor([1, 2], device=DEV)
    u, v = g.edges()
    gb = gtn.GraphBatch(g.ndata["feat"], v, u, None, [40, 129])
    with torch.no_grad():
        a, b = m(g, labels), m(gb, labels)
    assert torch.equal(a[2], b[2]) and torch.equal(a[3], b[3])


def test_training_lowers_the_loss():
    from wsi_hgnn_amd import gtn, optim
    slides = C.slides_case((40, 129, 64), SMALL["in_feats"], seed=61)
    labels = torch.tensor([0, 1, 2], device=DEV)
    torch.manual_seed(62)
    m = gtn.Classifier(**SMALL).to(DEV)
    opt = optim.Adam(m.parameters(), lr=1e-3)
    batch = _batch(slides)
    losses = [float(gtn.train_one_step(m, batch, labels, opt)) for _ in range(6)]
    assert all(np.isfinite(losses)) and losses[5] < losses[0], losses
