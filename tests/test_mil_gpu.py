"""ABMIL and DSMIL on the GPU (default fp32 GEMM mode): against the fixture recorded from the reference's own modules
(tests/golden/mil/reference_mil.npz) as one batch of three bags and as three single-bag calls, against the float64 restatement of
tests/mil_cases.py on a batch with empty bags in the middle and at the end, and the behaviour of a training step.  Tolerance
(tests/test_gat_gpu.py's norm): error <= 1e-4 x the largest float64 entry of each tensor."""
import copy
import os

import numpy as np
import pytest
import torch

import mil_cases as MC

pytestmark = pytest.mark.gpu

DEV = "cuda"
TOL = 1e-4
HERE = os.path.dirname(os.path.abspath(__file__))
R = MC.Ratios(TOL)
DS_OUT = ("classes", "pred", "A", "B")
DS_FN = ("classes", "pred", "B")           # the outputs the functionals weigh: A is returned detached (the reference's objective never differentiates it)


@pytest.fixture(scope="module", autouse=True)
def _report_ratios():
    yield
    R.report()


@pytest.fixture(scope="module")
def fix():
    return dict(np.load(os.path.join(HERE, "golden", "mil", "reference_mil.npz")))


def _sd(fix, model):
    return {k[len(model) + 4:]: torch.as_tensor(v) for k, v in fix.items() if k.startswith(model + ".sd.")}


def _make(model, K, C):
    from wsi_hgnn_amd.mil import abmil, dsmil
    if model == "dsmil":
        return dsmil.MILNet(dsmil.FCLayer(K, C), dsmil.BClassifier(K, C, dropout_v=0.0))
    return abmil.BClassifier(K, C)


def _outputs(model, m, x, bags):
    out = m(x, bags)
    return dict(zip(DS_OUT, out)) if model == "dsmil" else {"Y": out}


def _check_grads(m, ref_grads, case, zero_bound=None):
    """``ref_grads``: name -> float64 gradient.  ABMIL's attention.2.bias has a gradient of ZERO in exact arithmetic: it is the sum over all
    rows of the score gradients, and a softmax ignores a shift of its scores, so every bag's score gradients sum to 0.  Float64 leaves
    1e-17 there; 1e-4 of the tensor's own largest entry would be no bound at all.  It is held to ``zero_bound`` instead: the tolerance the
    kernel test puts on one bag's sum of score gradients (1e-4 x the largest float64 score gradient), once per non-empty bag."""
    largest = max(float(g.abs().max()) for g in ref_grads.values())
    for k, p in m.named_parameters():
        ref = ref_grads[k]
        assert p.grad is not None, k
        if float(ref.abs().max()) <= 1e-12 * largest:
            assert k == "attention.2.bias" and zero_bound is not None, k
            print(f"{case} g_{k}: {float(p.grad.abs().max()):.3e} against a bound of {zero_bound:.3e}")
            assert float(p.grad.abs().max()) <= zero_bound, f"{case} g_{k}"
        else:
            R.check(p.grad, ref, "g_" + k, case)


def _zero_bound(score_grads):
    """See ``_check_grads``: (non-empty bags) x 1e-4 x the largest float64 score gradient."""
    return len(score_grads) * TOL * max(float(a.grad.abs().max()) for a in score_grads)


@pytest.mark.parametrize("split", ["one_batch", "single_bags"])
@pytest.mark.parametrize("model", ["abmil", "dsmil"])
def test_reference_fixture(fix, model, split):
    from wsi_hgnn_amd import mil
    sizes = [int(n) for n in fix["sizes"]]
    off = MC.offsets(sizes)
    m = _make(model, MC.FIXTURE_K, MC.FIXTURE_C)
    m.load_state_dict(_sd(fix, model), strict=True)
    m.to(DEV)
    x = torch.as_tensor(fix["x"]).to(DEV).requires_grad_(True)
    names = DS_OUT if model == "dsmil" else ("Y",)
    fn = DS_FN if model == "dsmil" else ("Y",)
    w = {k: torch.as_tensor(fix[f"{model}.w_{k}"]).to(DEV, torch.float32) for k in fn}
    if split == "one_batch":
        outs = _outputs(model, m, x, mil.bag_plan(sizes, DEV))
        sum((outs[k] * w[k]).sum() for k in fn).backward()
    else:
        parts = []
        for s, (a, b) in enumerate(zip(off[:-1], off[1:])):
            o = _outputs(model, m, x[a:b], None)                       # the reference's call: one bag, no plan
            rows = {"Y": slice(s, s + 1), "pred": slice(s, s + 1), "B": slice(s, s + 1), "classes": slice(a, b), "A": slice(a, b)}
            sum((o[k] * w[k][rows[k]]).sum() for k in fn).backward()
            parts.append(o)
        outs = {k: torch.cat([p[k] for p in parts], 0) for k in names}
    for k in names:
        R.check(outs[k], torch.as_tensor(fix[f"{model}.{k}"]), k, f"{model} fixture {split}")
    R.check(x.grad, torch.as_tensor(fix[f"{model}.g.x"]), "g_x", f"{model} fixture {split}")
    zero_bound = None
    if model == "abmil":            # the score gradients of the same functional, from the restatement tests/test_mil.py holds against this fixture
        kept = []
        y64 = MC.abmil_forward(MC.to64({k: v.numpy() for k, v in _sd(fix, model).items()}), torch.as_tensor(fix["x"], dtype=torch.float64), sizes, kept)
        (y64 * torch.as_tensor(fix["abmil.w_Y"])).sum().backward()
        zero_bound = _zero_bound(kept)
    _check_grads(m, {k: torch.as_tensor(fix[f"{model}.g.{k}"]) for k, _ in m.named_parameters()}, f"{model} fixture {split}", zero_bound)


def _seeded(model, K, C, seed):
    torch.manual_seed(seed)
    m = _make(model, K, C)
    if model == "abmil":                        # a freshly initialised ABMIL attention is nearly flat: sharpen it so that the softmax matters
        with torch.no_grad():                   # (DSMIL's is peaked as initialised: a critical instance's score of itself dominates its bag)
            m.attention[2].weight.mul_(6.0)
    return m


@pytest.mark.parametrize("C", MC.MODEL_CS)
@pytest.mark.parametrize("model", ["abmil", "dsmil"])
def test_batch_with_empty_bags_against_float64(model, C):
    from wsi_hgnn_amd import mil
    sizes, K = MC.MODEL_SIZES, MC.MODEL_K
    n, S = sum(sizes), len(sizes)
    m = _seeded(model, K, C, 100 + C)
    g = torch.Generator().manual_seed(200 + C)
    x = torch.randn(n, K, generator=g)
    shapes = {"Y": (S, C), "classes": (n, C), "pred": (S, C), "A": (n, C), "B": (S, C, K)}
    names = DS_OUT if model == "dsmil" else ("Y",)
    fn = DS_FN if model == "dsmil" else ("Y",)
    w = {k: torch.randn(shapes[k], generator=g) for k in fn}
    sd64 = MC.to64({k: v.detach().numpy() for k, v in m.state_dict().items()})
    x64 = x.double().requires_grad_(True)
    kept = []
    ref = MC.dsmil_forward(sd64, x64, sizes) if model == "dsmil" else (MC.abmil_forward(sd64, x64, sizes, kept),)
    ref = dict(zip(names, ref))
    sum((ref[k] * w[k].double()).sum() for k in fn).backward()
    m.to(DEV)
    xd = x.to(DEV).requires_grad_(True)
    outs = _outputs(model, m, xd, mil.bag_plan(sizes, DEV))
    sum((outs[k] * w[k].to(DEV)).sum() for k in fn).backward()
    assert not outs.get("A", xd.detach()).requires_grad
    case = f"{model} C={C} empty bags"
    for k in names:
        R.check(outs[k], ref[k], k, case)
    R.check(xd.grad, x64.grad, "g_x", case)
    _check_grads(m, {k: sd64[k].grad for k, _ in m.named_parameters()}, case, _zero_bound(kept) if kept else None)
    bias = (m.b_classifier.fcc.bias if model == "dsmil" else m.classifier[0].bias).detach()
    pred = outs["pred" if model == "dsmil" else "Y"]
    for s, cnt in enumerate(sizes):
        if cnt == 0:
            assert torch.equal(pred[s], bias)                       # an empty bag: nothing pooled, the last layer's bias alone
    # the objective against the per-bag statement of the reference's
    labels = [0, 1, C, 0, 1][:S]                                      # one label past the last class: the all-zero target row
    labels = [min(l, 1) for l in labels] if C == 1 else labels
    loss = mil.bag_loss(m(xd.detach(), mil.bag_plan(sizes, DEV)), labels, C, model, mil.bag_plan(sizes, DEV))
    want = MC.dsmil_loss((ref["classes"], ref["pred"]), labels, C, sizes) if model == "dsmil" else MC.abmil_loss(ref["Y"], labels, C, sizes)
    R.check(loss.view(1), want.detach().view(1), "loss", case)


def _step_twice(model, m, x, bags, labels):
    """Two training steps from the same state: (parameters after, loss) of each."""
    from wsi_hgnn_amd import mil
    start = copy.deepcopy(m.state_dict())
    res = []
    for _ in range(2):
        m.load_state_dict(start)
        opt = torch.optim.Adam(m.parameters(), lr=1e-3, betas=(0.5, 0.9))
        loss = mil.train_one_step(m, opt, x, bags, labels)
        res.append(({k: v.detach().clone() for k, v in m.named_parameters()}, loss.clone()))
    return start, res


@pytest.mark.parametrize("model", ["abmil", "dsmil"])
def test_train_one_step_moves_every_live_parameter_and_repeats_bit_for_bit(model):
    from wsi_hgnn_amd import mil
    sizes, K, C = MC.MODEL_SIZES, MC.MODEL_K, 2
    m = _seeded(model, K, C, 7).to(DEV)
    x = torch.randn(sum(sizes), K, generator=torch.Generator().manual_seed(8)).to(DEV)
    start, (a, b) = _step_twice(model, m, x, mil.bag_plan(sizes, DEV), [0, 1, 1, 2, 0])
    assert torch.isfinite(a[1]) and torch.equal(a[1], b[1])
    for k in a[0]:
        assert torch.equal(a[0][k], b[0][k]), k
        if k != "attention.2.bias":               # its gradient is zero in exact arithmetic (a softmax ignores a shift): not a live parameter
            assert not torch.equal(a[0][k], start[k]), f"{k} did not move"


def test_a_row_critical_for_two_classes_keeps_the_step_reproducible():
    from wsi_hgnn_amd import mil
    from wsi_hgnn_amd.mil import dsmil
    sizes, K, C = (300, 1, 129), MC.MODEL_K, 2
    m = _seeded("dsmil", K, C, 17)
    with torch.no_grad():                         # class 1's instance score = class 0's + 0.5: the same row tops both columns of every bag
        m.i_classifier.fc[0].weight[1] = m.i_classifier.fc[0].weight[0]
        m.i_classifier.fc[0].bias[1] = m.i_classifier.fc[0].bias[0] + 0.5
    m.to(DEV)
    x = torch.randn(sum(sizes), K, generator=torch.Generator().manual_seed(18)).to(DEV)
    rp = mil.bag_plan(sizes, DEV)
    onehot = dsmil.critical_onehot(m.i_classifier(x)[1], rp)
    assert onehot.sum(0).tolist() == [3.0, 3.0] and int((onehot.sum(1) == 2).sum()) == 3      # three rows, each critical for both classes
    start, (a, b) = _step_twice("dsmil", m, x, rp, [0, 1, 1])
    assert torch.equal(a[1], b[1])
    for k in a[0]:
        assert torch.equal(a[0][k], b[0][k]), k
        assert not torch.equal(a[0][k], start[k]), f"{k} did not move"


@pytest.mark.parametrize("model", ["abmil", "dsmil"])
def test_graph_batch_input_equals_tensor_and_plan_input(model):
    import wsi_hgnn_amd as W
    from wsi_hgnn_amd import mil
    sizes, K, C = (40, 1, 131), 32, 3
    m = _seeded(model, K, C, 27).to(DEV)
    x = torch.randn(sum(sizes), K, generator=torch.Generator().manual_seed(28))
    off = MC.offsets(sizes)
    graphs = []
    for a, b in zip(off[:-1], off[1:]):
        src = torch.arange(b - a, dtype=torch.int64)
        graphs.append(W.HeteroGraph.homogeneous(b - a, src, src.flip(0), feat=x[a:b].clone()))
    g = W.batch(graphs).to(DEV)
    with torch.no_grad():
        from_graph = _outputs(model, m, g, None)
        from_rows = _outputs(model, m, x.to(DEV), mil.bag_plan(sizes, DEV))
    for k in from_rows:
        assert torch.equal(from_graph[k], from_rows[k]), k
