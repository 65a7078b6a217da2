"""The MIL baselines without a GPU: the float64 restatement of tests/mil_cases.py against the fixture recorded from the reference's own
modules (tests/golden/mil/reference_mil.npz), the module surface (parameter order, state_dict keys and shapes, strict loading), the new
exports and their argument errors, the target rule of the objective, and bag plans from sizes and from a graph batch."""
import ctypes
import os

import numpy as np
import pytest
import torch

import mil_cases as MC

HERE = os.path.dirname(os.path.abspath(__file__))
SYMBOLS = ("wsi_bag_softmax_pool_fwd", "wsi_bag_softmax_pool_bwd", "wsi_bag_scores_fwd", "wsi_bag_scores_bwd")


@pytest.fixture(scope="module")
def fix():
    return dict(np.load(os.path.join(HERE, "golden", "mil", "reference_mil.npz")))


def _sd(fix, model):
    return {k[len(model) + 4:]: v for k, v in fix.items() if k.startswith(model + ".sd.")}


def _check(got, want, bound, what):
    want = torch.as_tensor(want, dtype=torch.float64)
    err = float((got.detach() - want).abs().max())
    assert err <= bound * float(want.abs().max()), f"{what}: {err:.3e} over {float(want.abs().max()):.3e}"


def test_restatement_reproduces_the_reference_abmil(fix):
    sd = MC.to64(_sd(fix, "abmil"))
    x = torch.as_tensor(fix["x"], dtype=torch.float64).requires_grad_(True)
    Y = MC.abmil_forward(sd, x, fix["sizes"])
    _check(Y, fix["abmil.Y"], 1e-6, "Y")
    (Y * torch.as_tensor(fix["abmil.w_Y"])).sum().backward()
    _check(x.grad, fix["abmil.g.x"], 1e-5, "g_x")
    largest = max(float(np.abs(fix["abmil.g." + k]).max()) for k in sd)
    for k, p in sd.items():
        want = fix["abmil.g." + k]
        if float(np.abs(want).max()) <= 1e-12 * largest:      # attention.2.bias: a softmax ignores a shift of its scores, the gradient is 0
            assert float(p.grad.abs().max()) <= 1e-12 * largest, k
        else:
            _check(p.grad, want, 1e-5, "g_" + k)


def test_restatement_reproduces_the_reference_dsmil(fix):
    sd = MC.to64(_sd(fix, "dsmil"))
    x = torch.as_tensor(fix["x"], dtype=torch.float64).requires_grad_(True)
    outs = dict(zip(("classes", "pred", "A", "B"), MC.dsmil_forward(sd, x, fix["sizes"])))
    for k, v in outs.items():
        _check(v, fix["dsmil." + k], 1e-6, k)
    sum((v * torch.as_tensor(fix["dsmil.w_" + k])).sum() for k, v in outs.items() if k != "A").backward()     # (A: returned detached)
    _check(x.grad, fix["dsmil.g.x"], 1e-5, "g_x")
    for k, p in sd.items():
        _check(p.grad, fix["dsmil.g." + k], 1e-5, "g_" + k)


def test_restatement_handles_empty_bags():
    torch.manual_seed(3)
    from wsi_hgnn_amd.mil import dsmil
    m = dsmil.MILNet(dsmil.FCLayer(8, 2), dsmil.BClassifier(8, 2)).double()
    sd = dict(m.state_dict())
    x = torch.randn(5, 8, dtype=torch.float64)
    classes, pred, A, B = MC.dsmil_forward(sd, x, (3, 0, 2, 0))
    assert classes.shape == (5, 2) and A.shape == (5, 2) and B.shape == (4, 2, 8) and pred.shape == (4, 2)
    assert torch.equal(pred[1], sd["b_classifier.fcc.bias"]) and torch.equal(pred[3], sd["b_classifier.fcc.bias"]) and not B[1].any()
    out, lse, p = MC.softmax_pool(torch.randn(5, 2, dtype=torch.float64), x, (3, 0, 2, 0))
    assert not out[1].any() and not lse[3].any() and torch.allclose(p[:3].sum(0), torch.ones(2, dtype=torch.float64))


@pytest.mark.parametrize("model", ["abmil", "abmil_", "dsmil"])
def test_module_surface_matches_the_reference(fix, model):
    from wsi_hgnn_amd.mil import abmil, dsmil
    K, C = MC.FIXTURE_K, MC.FIXTURE_C
    if model == "dsmil":
        m = dsmil.MILNet(dsmil.FCLayer(K, C), dsmil.BClassifier(K, C, dropout_v=0.0))
    else:
        m = (abmil.BClassifier if model == "abmil" else abmil.BClassifier_)(K, C)
    name = model.rstrip("_")
    sd = _sd(fix, name)
    assert [k for k, _ in m.named_parameters()] == list(fix[name + ".order"])
    own = m.state_dict()
    assert list(own) == list(sd)
    assert {k: tuple(v.shape) for k, v in own.items()} == {k: tuple(v.shape) for k, v in sd.items()}
    m.load_state_dict({k: torch.as_tensor(v) for k, v in sd.items()}, strict=True)
    assert all(torch.equal(v, torch.as_tensor(sd[k])) for k, v in m.state_dict().items())
    if model == "dsmil":
        assert isinstance(m.b_classifier.v[0], torch.nn.Dropout) and tuple(m.b_classifier.fcc.weight.shape) == (C, C, K)
        assert dsmil.score_scale() == 1.0 / float(torch.sqrt(torch.tensor(128, dtype=torch.float32)))


def test_library_exports_the_bag_kernels():
    from wsi_hgnn_amd import _native as N
    lib = N.load()
    for s in SYMBOLS:
        assert s in N.EXPORTS and getattr(lib, s) is not None
        assert all(a in (ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_float) for a in N.EXPORTS[s][1]), s
    assert lib.wsi_abi_version() == 26


def test_bag_kernels_reject_bad_arguments_without_a_gpu():
    """Arguments are checked on the host before any launch: with values that must be rejected no kernel runs and no GPU is needed."""
    from wsi_hgnn_amd import _native as N
    lib = N.load()
    err = lambda: lib.wsi_last_error().decode()
    EINVAL, ENOSYS = -22, -38
    P = 4096                                   # a non-null address that is never dereferenced: every call below is rejected first
    fwd = lambda sc=P, C=3, val=P, D=16, cr=P, nch=2, sg=P, ns=2, part=P, out=P, lse=P: lib.wsi_bag_softmax_pool_fwd(
        sc, max(C, 1), C, 1.0, val, max(D, 1), D, cr, nch, sg, ns, part, out, lse, None, None)
    assert fwd(C=0) == EINVAL and "bad argument" in err()
    assert fwd(D=0) == EINVAL and "bad argument" in err()
    assert fwd(nch=-1) == EINVAL and fwd(ns=-1) == EINVAL
    assert fwd(C=9) == ENOSYS and "at most 8" in err()
    for null in ("sc", "val", "cr", "sg", "part", "out", "lse"):
        assert fwd(**{null: None}) == EINVAL and "null pointer" in err(), null
    assert lib.wsi_bag_softmax_pool_fwd(P, 2, 3, 1.0, P, 16, 16, P, 2, P, 2, P, P, P, P, None) == EINVAL       # lds < C
    bwd = lambda go=P, out=P, sc=P, C=3, stats=P, val=P, D=16, cr=P, cs=P, nch=2, ns=2, delta=P, gs=P, gv=P: lib.wsi_bag_softmax_pool_bwd(
        go, out, sc, max(C, 1), C, 1.0, stats, val, max(D, 1), D, cr, cs, nch, ns, delta, gs, max(C, 1), gv, max(D, 1), None)
    assert bwd(C=0) == EINVAL and bwd(D=0) == EINVAL and "bad argument" in err()
    assert bwd(C=9) == ENOSYS
    for null in ("go", "sc", "stats", "val", "cr", "cs"):
        assert bwd(**{null: None}) == EINVAL and "null pointer" in err(), null
    assert bwd(out=None) == EINVAL and bwd(delta=None) == EINVAL            # needed for g_scores ...
    assert bwd(gs=None, gv=None) == 0                                       # ... nothing asked for: nothing to do
    sf = lambda x=P, D=128, t=P, C=3, cr=P, cs=P, nch=2, sc=P: lib.wsi_bag_scores_fwd(x, max(D, 1), D, t, C, cr, cs, nch, sc, max(C, 1), None)
    assert sf(C=0) == EINVAL and sf(D=0) == EINVAL and sf(C=9) == ENOSYS
    for null in ("x", "t", "cr", "cs", "sc"):
        assert sf(**{null: None}) == EINVAL and "null pointer" in err(), null
    sb = lambda w=P, t=P, w2=None, t2=None, C=3, D=128, cr=P, cs=P, nch=2, gx=P: lib.wsi_bag_scores_bwd(
        w, max(C, 1), t, w2, max(C, 1), t2, C, D, cr, cs, nch, gx, max(D, 1), None)
    assert sb(C=0) == EINVAL and sb(D=0) == EINVAL and sb(C=9) == ENOSYS
    for null in ("w", "t", "cr", "cs", "gx"):
        assert sb(**{null: None}) == EINVAL and "null pointer" in err(), null
    assert sb(w2=P) == EINVAL and sb(t2=P) == EINVAL                        # the second term needs both of its factors


def test_ops_refuse_cpu_tensors():
    from wsi_hgnn_amd import ops
    from wsi_hgnn_amd.mil import bag_plan
    rp = bag_plan([3, 2], "cpu")
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.bag_softmax_pool(torch.zeros(5, 2), torch.zeros(5, 4), rp)
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.bag_scores(torch.zeros(5, 4), torch.zeros(5, 2), rp)
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.bag_attention(torch.zeros(5, 2), torch.zeros(2, 2), rp)


def test_bag_loss_target_rule():
    from wsi_hgnn_amd import mil
    t = mil.bag_targets([0, 2, 3, 1], 3)
    assert t.tolist() == [[1, 0, 0], [0, 0, 1], [0, 0, 0], [0, 1, 0]]            # a label past the last class: the all-zero row
    assert mil.bag_targets([0.0, 1.0, 0.25], 1).tolist() == [[0.0], [1.0], [0.25]]
    for labels, C in (([0, 2, 3, 1], 3), ([1, 0, 1, 0], 1)):
        assert torch.equal(mil.bag_targets(labels, C), torch.stack([MC.target_row(l, C) for l in labels]))
    torch.manual_seed(5)
    pred = torch.randn(4, 3, dtype=torch.float64)
    got = mil.bag_loss(pred, [0, 2, 3, 1], 3, "abmil")
    assert abs(float(got) - float(MC.abmil_loss(pred, [0, 2, 3, 1], 3, (5, 1, 2, 9)))) < 1e-12
    one = mil.bag_loss((None, pred[:1], None, None), [2], 3, "abmil")           # one bag: the reference's loss
    ref = torch.nn.BCEWithLogitsLoss()(pred[:1].view(1, -1), torch.tensor([[0.0, 0.0, 1.0]], dtype=torch.float64))
    assert abs(float(one) - float(ref)) < 1e-12
    with pytest.raises(ValueError):
        mil.bag_loss(pred, [0, 1], 3, "abmil")
    with pytest.raises(ValueError):
        mil.bag_loss(pred, [0, 2, 3, 1], 3, "dsmil")


def test_bag_plan_from_sizes_and_from_a_graph_batch_agree():
    import wsi_hgnn_amd as W
    from wsi_hgnn_amd import mil
    sizes = [5, 1, 300, 129]
    graphs = []
    for i, n in enumerate(sizes):
        src = torch.arange(n, dtype=torch.int64)
        graphs.append(W.HeteroGraph.homogeneous(n, src, src.flip(0), feat=torch.full((n, 4), float(i))))
    g = W.batch(graphs)
    a, b = mil.bag_plan(sizes, "cpu"), mil.bag_plan(g, "cpu")
    assert a.ranges == b.ranges == [(0, 5), (5, 6), (6, 306), (306, 435)]
    for name in ("chunk_row", "chunk_seg", "seg_chunk"):
        assert torch.equal(getattr(a, name), getattr(b, name)), name
    assert a.num_segs == 4 and a.num_rows == 435 and a.num_chunks == 1 + 1 + 3 + 2
    assert torch.equal(a.row_segment(), b.row_segment())
    c = mil.bag_plan(torch.tensor([3, 0, 2]), "cpu", chunk=2)
    assert c.ranges == [(0, 3), (3, 3), (3, 5)] and c.num_chunks == 3 and c.has_empty()
    h, rp = mil.rows_and_plan(g, None)
    assert h.shape == (435, 4) and rp.ranges == a.ranges and mil.rows_and_plan(g, None)[1] is rp
    with pytest.raises(ValueError):
        mil.bag_plan([3, -1], "cpu")
    with pytest.raises(ValueError):
        mil.rows_and_plan(torch.zeros(4, 2), a)
