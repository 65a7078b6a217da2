"""``models.GIN`` on the GPU against the float64 restatement of tests/gin_cases.py: logits, loss, every parameter gradient (eps and the
BatchNorm affine terms included) and the running statistics after the step, in train and eval mode, over a batch of three graphs of 1, 37 and
200 nodes; the projection-first rule both ways; one model under every GEMM arithmetic; counter-based dropout replayed from
``ops.dropout_keep_mask``; ``trainer.train_one_step`` and ``io.evaluate``; the logits of the reference's own ``GIN.forward``
(tests/golden/gin/reference_gin.npz).

The side of every ReLU's kink is decided in fp32: the reference replays the GPU's decisions (the sign of every BatchNorm output, which is
what each ReLU of the model sees), and every entry where the GPU's side differs from float64's must have a float64 pre-activation within the
tolerance of zero - the only place where the two may legitimately differ.  Tolerance: 1e-4 of the largest float64 entry of each tensor.
The exception are the gradients that are exactly zero by construction - the bias of a Linear in front of a train-mode BatchNorm (its mean is
subtracted again) and the bias of an attention gate (a softmax does not see a shift): their float64 value is 1e-17 of rounding noise, so
1e-4 of it says nothing; they are held to 1e-4 of the largest column sum of the magnitudes of the terms that cancel
(gin_cases.cancelling_bounds), the scale of the sum's own rounding error."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import gin_cases as C

pytestmark = pytest.mark.gpu

DEV = "cuda"
TOL = C.TOL
SIZES = (1, 37, 200)
LABELS = torch.tensor([0, 2, 1])
# (num_layers, num_mlp_layers, neighbour reducer, readout, learn_eps, input_dim, hidden_dim): every value of every setting occurs, input_dim
# above hidden_dim (projection first under sum / mean) and not above
SETTINGS = [(2, 2, "mean", "att", True, 48, 16), (2, 1, "sum", "sum", True, 48, 16), (3, 2, "max", "mean", True, 12, 16),
            (3, 1, "mean", "max", False, 12, 16), (3, 2, "sum", "att", False, 16, 16), (2, 2, "max", "sum", True, 48, 16)]
IDS = ["L{}-mlp{}-{}-{}-eps{}-{}to{}".format(*s) for s in SETTINGS]


def _close(got, ref, what, bound=None):
    """``bound``: the absolute bound of an exactly-cancelling gradient (gin_cases.cancelling_bounds) in place of 1e-4 of the largest entry."""
    ref = ref.detach().to(torch.float64).cpu()
    got = got.detach().to(torch.float64).cpu()
    bound = TOL * max(float(ref.abs().max()), 1e-30) if bound is None else bound
    err = float((got - ref).abs().max())
    print(f"{what}: error / bound {err / bound:.3e}")
    assert err <= bound, f"{what}: max error {err:.3e} > {bound:.3e}"


def _graphs(in_dim, seed=5):
    """Three graphs: one node with a self loop; 37 and 200 nodes with random edges (duplicates, self loops, nodes without in-edges)."""
    from wsi_hgnn_amd.graph import HeteroGraph
    gen = torch.Generator().manual_seed(seed)
    out = []
    for n in SIZES:
        if n == 1:
            src, dst = torch.tensor([0]), torch.tensor([0])
        else:
            src = torch.randint(0, n, (5 * n,), generator=gen)
            dst = torch.randint(n // 8, n, (5 * n,), generator=gen)          # the first eighth has no in-edge
            src, dst = torch.cat([src, src[:n // 2], torch.arange(0, n, 3)]), torch.cat([dst, dst[:n // 2], torch.arange(0, n, 3)])
        g = HeteroGraph.homogeneous(n, src, dst)
        g.ndata["feat"] = torch.randn(n, in_dim, generator=gen)
        out.append(g)
    return out


def _batch(in_dim):
    import wsi_hgnn_amd as W
    g = W.batch(_graphs(in_dim)).to(DEV)
    from wsi_hgnn_amd.models.GCN import homo_plan
    hp = homo_plan(g)
    csr = {"n": hp.num_nodes, "rowptr": hp.rowptr.cpu().long(), "src": hp.src.cpu().long()}
    return g, csr, torch.tensor(SIZES)


def _model(setting, dropout=0.0, seed=21):
    from wsi_hgnn_amd.models import GIN
    L, mlp, neigh, pool, learn, din, hid = setting
    torch.manual_seed(seed)
    m = GIN(din, hid, 3, L, mlp, dropout, pool, neigh, learn)
    gen = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():                                             # statistics, affine terms and eps away from their initial values
        for k, v in m.state_dict().items():
            if k.endswith("running_mean") or ("bn" in k or "batch_norms" in k) and k.endswith(".bias"):
                v.copy_(0.3 * torch.randn(v.shape, generator=gen))
            elif k.endswith("running_var") or ("bn" in k or "batch_norms" in k) and k.endswith(".weight"):
                v.copy_(0.5 + torch.rand(v.shape, generator=gen))
            elif k.endswith(".eps"):
                v.fill_(0.3)
    return m.to(DEV)


def _record_relu_sides(m):
    """The sign of every BatchNorm output in call order: each feeds one ReLU."""
    from wsi_hgnn_amd.models.GIN import BatchNorm1d
    sides, hooks = [], []
    for mod in m.modules():
        if isinstance(mod, BatchNorm1d):
            hooks.append(mod.register_forward_hook(lambda _m, _i, out: sides.append((out.detach() > 0).double().cpu())))
    return sides, hooks


def _state64(m, grad=True):
    out = {}
    for k, v in m.state_dict().items():
        t = v.detach().cpu().double() if v.is_floating_point() else v.detach().cpu().clone()
        out[k] = t.requires_grad_(True) if (grad and k in dict(m.named_parameters())) else t
    return out


def _check_kinks(pre, sides, what):
    differing = 0
    for i, (z, s) in enumerate(zip(pre, sides)):
        bad = (z.detach() > 0).double() != s
        differing += int(bad.sum())
        if bad.any():
            assert float(z.detach()[bad].abs().max()) <= TOL * float(z.detach().abs().max()), f"{what}: ReLU {i} differs away from its kink"
    print(f"{what}: {differing} ReLU sides differ from float64's")


def _parity(setting, train, gemm=None):
    L, mlp, neigh, pool, learn, din, hid = setting
    g, csr, bnn = _batch(din)
    m = _model(setting)
    m.train(train)
    state = _state64(m)
    sides, hooks = _record_relu_sides(m)
    logits = m(g)
    loss = F.cross_entropy(logits, LABELS.to(DEV))
    loss.backward()
    torch.cuda.synchronize()
    for h in hooks:
        h.remove()
    x = g.ndata["feat"].cpu().double()
    taps = {}
    rlogits, buffers, pre = C.model_ref(state, x, csr, bnn, L, mlp, neigh, pool, train, masks=sides, taps=taps)
    rloss = F.cross_entropy(rlogits, LABELS)
    rloss.backward()
    bounds = C.cancelling_bounds(taps)
    what = f"{'train' if train else 'eval'}"
    assert len(pre) == len(sides) == (L - 1) * mlp
    _check_kinks(pre, sides, what)
    _close(logits, rlogits, "logits")
    assert abs(float(loss) - float(rloss)) <= TOL * max(abs(float(rloss)), 1e-30)
    dead = set(m.dead_parameter_names())
    for k, p in m.named_parameters():
        if k in dead:
            assert p.grad is None and state[k].grad is None, k
        else:
            _close(p.grad, state[k].grad, f"d loss / d {k}", bounds.get(k))
    after = m.state_dict()
    for k, v in buffers.items():
        if k.endswith("num_batches_tracked"):
            assert int(after[k]) == int(v) == (1 if train else 0), k
        else:
            _close(after[k], v, k)
    return m, g, bounds


@pytest.mark.parametrize("train", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("setting", SETTINGS, ids=IDS)
def test_model_parity(setting, train):
    m, _, _ = _parity(setting, train)
    first_projects = setting[2] in ("sum", "mean") and setting[5] > setting[6]
    assert m.layers[0].project_first() is first_projects


def test_model_parity_under_every_gemm_arithmetic(gemm_mode):
    _parity(SETTINGS[0], True)


@pytest.mark.parametrize("setting", [SETTINGS[0], SETTINGS[1]], ids=IDS[:2])
def test_projection_first_and_aggregate_first_agree(setting):
    from wsi_hgnn_amd import ops
    g, _, _ = _batch(setting[5])
    bounds = _parity(setting, True)[2]                                # (the exactly-cancelling gradients: two runs agree within their bound)
    res = {}
    for on in (False, True):
        ops.set_gin_project_first(on)
        try:
            m = _model(setting).train()
            assert m.layers[0].project_first() is on
            logits = m(g)
            F.cross_entropy(logits, LABELS.to(DEV)).backward()
            res[on] = (logits.detach(), {k: p.grad for k, p in m.named_parameters() if p.grad is not None}, {k: v.clone() for k, v in m.state_dict().items()})
        finally:
            ops.set_gin_project_first(True)
    _close(res[True][0], res[False][0], "logits")
    for k, v in res[False][1].items():
        _close(res[True][1][k], v, f"d loss / d {k}", bounds.get(k))
    for k, v in res[False][2].items():
        if v.is_floating_point():
            _close(res[True][2][k], v, k)


def test_dropout_under_a_seed_base_is_the_counter_based_draw():
    from wsi_hgnn_amd import ops
    setting = (3, 2, "mean", "sum", True, 12, 16)
    g, csr, bnn = _batch(12)
    m = _model(setting, dropout=0.5).train()
    state = _state64(m, grad=False)
    base = torch.tensor([12345], dtype=torch.int32, device=DEV)
    sides, hooks = _record_relu_sides(m)
    torch.manual_seed(77)
    with ops.dropout_seed_base(base):
        logits = m(g)
    torch.cuda.synchronize()
    for h in hooks:
        h.remove()
    torch.manual_seed(77)
    drop = ops.CounterDropout(0.5, ops.next_dropout_seed(), base)
    keep = ops.dropout_keep_mask(drop, sum(SIZES), 16).double() * drop.scale
    assert 0.3 < float((keep > 0).double().mean()) < 0.7
    rlogits, _, pre = C.model_ref(state, g.ndata["feat"].cpu().double(), csr, bnn, 3, 2, "mean", "sum", True, masks=sides, drops=[keep])
    _check_kinks(pre, sides, "dropout")
    _close(logits, rlogits, "logits")
    m.eval()
    with ops.dropout_seed_base(base):
        assert torch.equal(m(g), m(g))                                # eval mode: no draw


def test_train_one_step_and_evaluate_take_a_gin():
    from wsi_hgnn_amd import graph as G, io as wio, synthetic, trainer
    from wsi_hgnn_amd.data import GraphBatchLoader
    from wsi_hgnn_amd.models import from_config
    slides = [G.to_homogeneous(synthetic.hetero_graph(60 + 10 * i, 24, seed=i)) for i in range(4)]
    labels = [0, 1, 1, 0]
    torch.manual_seed(1)
    m = from_config({"name": "GIN", "in_dim": 24, "hidden_dim": 16, "out_dim": 2, "num_layers": 2, "num_mlp_layers": 2, "feat_drop": 0.2,
                     "graph_pooling_type": "att", "neighbor_pooling_type": "mean"}).to(DEV)
    opt = torch.optim.Adam(m.parameters(), lr=5e-4, weight_decay=1e-4)
    before = m.layers[0].eps.detach().clone()
    losses = []
    for batch, y in GraphBatchLoader(slides, labels, 2, DEV, shuffle=False):
        losses.append(trainer.train_one_step(m, opt, torch.nn.CrossEntropyLoss(), batch, y, DEV)[0])
    assert len(losses) == 2 and all(np.isfinite(l) for l in losses)
    assert not torch.equal(m.layers[0].eps.detach(), before)          # eps is learned
    assert int(m.layers[0].apply_func.bn.num_batches_tracked) == 2
    res = wio.evaluate(m, GraphBatchLoader(slides, labels, 2, DEV, shuffle=False))
    assert np.isfinite(res["loss"]) and 0.0 <= res["accuracy"] <= 1.0
    assert m.training


def test_reference_logits_on_the_gpu():
    """The logits of the reference's own GIN.forward (float64, DGL stand-ins) from the fixture's state, in eval and train mode."""
    import wsi_hgnn_amd as W
    from wsi_hgnn_amd.models import GIN
    npz = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gin", "reference_gin.npz"))
    src, dst, bnn = (torch.from_numpy(npz[k]).long() for k in ("src", "dst", "batch_num_nodes"))
    graphs, off = [], 0
    for n in bnn.tolist():
        keep = (dst >= off) & (dst < off + n)
        g = W.graph.HeteroGraph.homogeneous(n, src[keep] - off, dst[keep] - off)
        g.ndata["feat"] = torch.from_numpy(npz["x"][off:off + n]).float()
        graphs.append(g)
        off += n
    batch = W.batch(graphs).to(DEV)
    for i, s in enumerate(npz["settings"].tolist()):
        neigh, pool, mlp, learn = s.split("|")
        m = GIN(12, 8, 3, 2, int(mlp), 0.0, pool, neigh, learn == "True")
        m.load_state_dict({k.split("/", 2)[2]: torch.from_numpy(npz[k]) for k in npz.files if k.startswith(f"{i}/state/")}, strict=True)
        m = m.to(DEV)
        m.eval()
        _close(m(batch), torch.from_numpy(npz[f"{i}/logits_eval"]), f"{s} eval logits")
        m.train()
        _close(m(batch), torch.from_numpy(npz[f"{i}/logits_train"]), f"{s} train logits")
        for k in npz.files:
            if k.startswith(f"{i}/after/") and not k.endswith("num_batches_tracked"):
                _close(m.state_dict()[k.split("/", 2)[2]], torch.from_numpy(npz[k]), k)
