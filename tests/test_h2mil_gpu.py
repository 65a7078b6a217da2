"""The H2MIL model on the GPU: ``kernels=True`` against the float64 restatement of tests/h2mil_cases.py on the three margin-condition slides of
about 60, 150 and 400 nodes (clusters, node types, trees and edge sets exactly; probabilities, loss and every parameter gradient within
1e-4 x the largest float64 entry), with dropout 0 and in ``eval()`` with dropout 0.3; ``kernels=True`` against ``kernels=False``; a few training
steps on a two-slide toy problem; the RAConv fixture recorded from the reference's own code."""
import os

import numpy as np
import pytest
import torch

import h2mil_cases as C
from mil_cases import Ratios

pytestmark = pytest.mark.gpu

DEV = "cuda"
TOL = 1e-4
R = Ratios(TOL)
LABELS = torch.tensor([0, 2, 1])
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "h2mil")


@pytest.fixture(scope="module", autouse=True)
def _report_ratios():
    yield
    R.report()


@pytest.fixture(scope="module")
def reference():
    """(slides, float64 state, the restatement's probabilities / pools / loss / gradients) - computed once, shared, never changed."""
    state = {k: v.detach() for k, v in C.make_model(kernels=False, dtype=torch.float64).state_dict().items()}
    slides = C.model_slides(state)
    return (slides, state) + C.reference_run(slides, state, LABELS)


def _model(state, kernels, drop=0.0):
    m = C.make_model(kernels=kernels, drop_out_ratio=drop)
    m.load_state_dict({k: v.float() for k, v in state.items()})
    return m.to(DEV)


def _check_discrete(outs, pools, what):
    for b, po in enumerate(pools):
        for layer in (0, 1):
            r = po[layer]
            assert torch.equal(outs[1][layer][b].cpu(), r["cluster"]), f"{what}: cluster {layer + 1} of slide {b}"
            assert torch.equal(outs[2][layer][b].cpu(), r["node_type"]), f"{what}: node types {layer + 1} of slide {b}"
            assert torch.equal(outs[4][layer][b].cpu(), r["tree"]), f"{what}: tree {layer + 1} of slide {b}"
            assert torch.equal(outs[6][layer][b].cpu(), r["edge_index"]), f"{what}: edges {layer + 1} of slide {b}"
            R.check(outs[3][layer][b], r["fitness"], "fitness", f"{what} pool {layer + 1} slide {b}")
            R.check(outs[5][layer][b], r["x_y_index"], "x_y_index", f"{what} pool {layer + 1} slide {b}")


def test_model_with_kernels_equals_the_restatement(reference):
    from wsi_hgnn_amd import h2mil
    slides, state, probs, pools, loss, grads = reference
    batch = h2mil.from_slides(slides).to(DEV)
    m = _model(state, True).train()                                  # dropout 0: train mode computes what eval does
    outs = m(batch)
    got_loss = h2mil.loss_fn(outs[0], LABELS.to(DEV))
    got_loss.backward()
    _check_discrete(outs, pools, "train, dropout 0")
    R.check(outs[0], probs, "probabilities", "train, dropout 0")
    R.check(got_loss, loss, "loss", "train, dropout 0")
    for k, p in m.named_parameters():
        if k.startswith(("pool_1.", "pool_2.")):
            assert p.grad is None, k
        else:
            R.check(p.grad, grads[k], "g." + k, "train, dropout 0")
    assert m.pool_1.readbacks == 1 and m.pool_2.readbacks == 1           # one small copy per pooling layer and forward
    m3 = _model(state, True, drop=0.3).eval()
    outs3 = m3(batch)
    _check_discrete(outs3, pools, "eval, dropout 0.3")
    R.check(outs3[0], probs, "probabilities", "eval, dropout 0.3")
    assert torch.equal(outs3[0], outs[0].detach()), "eval under dropout 0.3 computes what dropout 0 computes"


def test_kernels_and_tensor_operations_agree_on_the_gpu(reference):
    from wsi_hgnn_amd import h2mil
    slides, state, probs, pools, loss, grads = reference
    batch = h2mil.from_slides(slides).to(DEV)
    mk, mt = _model(state, True), _model(state, False)
    ok, ot = mk(batch), mt(batch)
    h2mil.loss_fn(ok[0], LABELS.to(DEV)).backward()
    h2mil.loss_fn(ot[0], LABELS.to(DEV)).backward()
    _check_discrete(ot, pools, "tensor operations")
    R.check(ok[0], ot[0].double(), "probabilities, kernels against tensor operations")
    R.check(ot[0], probs, "probabilities, tensor operations")
    for (k, p), (_, q) in zip(mk.named_parameters(), mt.named_parameters()):
        if p.grad is not None:
            R.check(q.grad, grads[k], "tensor operations g." + k)
            assert float((p.grad.double() - q.grad.double()).abs().max()) <= 2 * TOL * float(grads[k].abs().max()), k
    for t in (1, 2, 4, 6):
        for layer in (0, 1):
            assert all(torch.equal(a, b) for a, b in zip(ok[t][layer], ot[t][layer]))


@pytest.mark.parametrize("mpool", ("global_max_pool", "global_att_pool"))
def test_the_other_readouts_with_kernels(mpool):
    """The two smaller shapes, drawn under THIS model's weights until the margin condition holds."""
    from wsi_hgnn_amd import h2mil
    state = {k: v.detach() for k, v in C.make_model(kernels=False, dtype=torch.float64, mpool=mpool, seed=11).state_dict().items()}
    slides = C.model_slides(state, mpool=mpool, shapes=C.MODEL_SHAPES[:2])
    probs, pools, _, _ = C.reference_run(slides, state, LABELS[:2], mpool=mpool)
    m = C.make_model(kernels=True, mpool=mpool, seed=11).to(DEV)
    outs = m(h2mil.from_slides(slides).to(DEV))
    _check_discrete(outs, pools, mpool)
    R.check(outs[0], probs, "probabilities", mpool)


def test_train_one_step_lowers_the_loss():
    from wsi_hgnn_amd import h2mil
    torch.manual_seed(3)
    m = h2mil.H2MIL(12, 0, 8, 2, drop_out_ratio=0.0).to(DEV)
    a, b = C.tree_slide(1, 6, (2, 4), feat=12), C.tree_slide(2, 6, (2, 4), feat=12)
    b["x"] = b["x"] + 1.5
    batch, labels = h2mil.from_slides([a, b]).to(DEV), torch.tensor([0, 1], device=DEV)
    opt = torch.optim.Adam(m.parameters(), lr=1e-2)
    losses = [float(h2mil.train_one_step(m, batch, labels, opt)) for _ in range(8)]
    assert all(np.isfinite(losses)) and losses[-1] < losses[0], losses
    assert all(torch.isfinite(p).all() for p in m.parameters())


def test_raconv_fixture_on_the_gpu():
    from wsi_hgnn_amd import h2mil
    fix = dict(np.load(os.path.join(GOLD, "reference_raconv.npz")))
    cin, cout = fix["config"].tolist()
    m = h2mil.RAConv(cin, cout)
    m.load_state_dict({k: torch.from_numpy(fix["sd." + k]) for k in fix["keys"].tolist()})
    m = m.to(DEV)
    x = torch.from_numpy(fix["x"]).to(DEV).requires_grad_(True)
    ei, nt = torch.from_numpy(fix["edge_index"]).to(DEV), torch.from_numpy(fix["node_type"]).to(DEV)
    out = m(x, ei, nt)
    out.backward(torch.from_numpy(fix["w"]).float().to(DEV))
    R.check(out, torch.from_numpy(fix["out"]), "out", "fixture")
    R.check(x.grad, torch.from_numpy(fix["g.x"]), "g.x", "fixture")
    for k, p in m.named_parameters():
        R.check(p.grad, torch.from_numpy(fix["g." + k]), "g." + k, "fixture")
