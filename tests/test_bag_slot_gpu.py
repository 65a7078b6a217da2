"""ABMIL and DSMIL stepped on bag slots on the GPU: a slot's loss, predictions and parameter gradients against the float64 restatement of
tests/mil_cases.py on the UNPADDED batch (rows dropped by the tensor formulation; tolerance of tests/test_mil_gpu.py: error <= 1e-4 x the
largest float64 entry of each tensor), and ``CapturedBagStep``: loss trajectory and final parameters bit-equal to an eager twin that steps on
slot tables of its own - without and with patch dropout, across an ``lr`` change with ``recapture()``, for a ReMix mixed bag - and what it
refuses."""
import copy

import numpy as np
import pytest
import torch

import bag_slot_cases as BC
import mil_cases as MC

pytestmark = pytest.mark.gpu

DEV = "cuda"
TOL = 1e-4
K = 64
R = MC.Ratios(TOL)
MODELS = (("dsmil", 2), ("abmil", 1))


@pytest.fixture(scope="module", autouse=True)
def _report_ratios():
    yield
    R.report()


def _make(model, C, seed):
    from wsi_hgnn_amd.mil import abmil, dsmil
    torch.manual_seed(seed)
    if model == "dsmil":
        return dsmil.MILNet(dsmil.FCLayer(K, C), dsmil.BClassifier(K, C, dropout_v=0.0))
    m = abmil.BClassifier(K, C)
    with torch.no_grad():                       # (a freshly initialised ABMIL attention is nearly flat: sharpen it so that the softmax matters)
        m.attention[2].weight.mul_(6.0)
    return m


def _adam(m):
    from wsi_hgnn_amd import optim
    return optim.Adam(m.parameters(), lr=2e-4, betas=(0.5, 0.9), weight_decay=5e-3, capturable=True)


@pytest.mark.parametrize("p", [0.0, 0.25])
@pytest.mark.parametrize("model,C", MODELS)
def test_slot_against_the_unpadded_batch_in_float64(model, C, p):
    from wsi_hgnn_amd import mil
    sizes, labels = (300, 0, 129), (1, 0, 1)                    # an empty real bag in the middle, an unused bag, the filler
    m = _make(model, C, 300 + C).to(DEV)
    slot = mil.BagSlot(K, sum(sizes) + 140, BC.BAG_CAP, num_classes=C, device=DEV, dropout_patch=p)
    bags = BC.make_bags(sizes, K, 70, DEV)
    draws = BC.draws_for(sizes, 3)
    slot.load(bags, labels, draws)
    outputs = m(slot.rows, slot.plan)
    pred = outputs[1] if model == "dsmil" else outputs
    loss = mil.bag_loss(outputs, None, C, model, slot.plan, weights=slot.weights, targets=slot.targets)
    loss.backward()
    # float64 on the unpadded batch
    rows, new_sizes, _ = mil.dropout_patches_tensor(torch.cat([t.cpu() for t in bags]), sizes, p, draws)
    sd = MC.to64({k: v.detach().cpu().numpy() for k, v in m.state_dict().items()})
    x64 = rows.to(torch.float64)
    case = f"{model} slot p={p}"
    zero_bound = None
    if model == "dsmil":
        out64 = MC.dsmil_forward(sd, x64, new_sizes)
        loss64, pred64 = MC.dsmil_loss(out64, labels, C, new_sizes), out64[1]
    else:
        kept = []
        pred64 = MC.abmil_forward(sd, x64, new_sizes, kept)
        loss64 = MC.abmil_loss(pred64, labels, C, new_sizes)
    loss64.backward()
    if model == "abmil":                        # (tests/test_mil_gpu.py::_check_grads: attention.2.bias has an exactly zero gradient)
        zero_bound = len(kept) * TOL * max(float(a.grad.abs().max()) for a in kept)
    R.check(loss.view(1), loss64.view(1), "loss", case)
    R.check(pred[:len(sizes)], pred64, "pred", case)
    largest = max(float(g.grad.abs().max()) for g in sd.values())
    for k, prm in m.named_parameters():
        ref = sd[k].grad
        assert prm.grad is not None, k
        if float(ref.abs().max()) <= 1e-12 * largest:
            assert k == "attention.2.bias" and zero_bound is not None, k
            print(f"{case} g_{k}: {float(prm.grad.abs().max()):.3e} against a bound of {zero_bound:.3e}")
            assert float(prm.grad.abs().max()) <= zero_bound, f"{case} g_{k}"
        else:
            R.check(prm.grad, ref, "g_" + k, case)


class _Twin:
    """What ``CapturedBagStep`` does, eagerly, on slots of its own: the same loads, ``mil.slot_step`` where it replays."""

    def __init__(self, m, opt, slots, warmup_batches):
        from wsi_hgnn_amd import mil
        self.m, self.opt, self.mil = m, opt, mil
        order = sorted(range(len(slots)), key=lambda i: slots[i].row_cap)
        self.slots = [slots[i] for i in order]
        m.train()
        for i, slot in zip(order, self.slots):
            slot.load(*warmup_batches[i])
            mil.slot_step(m, opt, slot)

    def step(self, bags, labels):
        mil = self.mil
        sizes = [int(t.shape[0]) for t in bags]
        slot = next((s for s in self.slots if s.fits(sizes)), None)
        if slot is not None:
            slot.load(bags, labels)
            return mil.slot_step(self.m, self.opt, slot)[0]
        big = self.slots[-1]
        x, plan = mil.dropout_patches(torch.cat(list(bags)), sizes, big.dropout_patch, big.take_draws(len(bags)) if big.dropout_patch > 0 else None)
        return mil.train_one_step(self.m, self.opt, x, plan, labels)


def _slots(C, p):
    from wsi_hgnn_amd import mil
    return [mil.BagSlot(K, 700, 2, num_classes=C, device=DEV, dropout_patch=p, seed=4),          # (given largest first: the step sorts them)
            mil.BagSlot(K, 200, 2, num_classes=C, device=DEV, dropout_patch=p, seed=4)]


def _batches(seed):
    """Six batches for the slots of ``_slots`` (the third fits the small one), then one that fits neither."""
    sizes = [(300, 129), (650,), (127, 2), (0, 400), (699,), (201,), (500, 300)]
    labels = [(1, 0), (0,), (1, 1), (0, 1), (1,), (0,), (1, 0)]
    return [(BC.make_bags(s, K, seed + i, DEV), list(l)) for i, (s, l) in enumerate(zip(sizes, labels))]


def _pair(model, C, p):
    from wsi_hgnn_amd import mil
    m = _make(model, C, 500 + C).to(DEV)
    twin_m = copy.deepcopy(m)
    opt, twin_opt = _adam(m), _adam(twin_m)
    warm = [(BC.make_bags((600,), K, 90, DEV), [1]), (BC.make_bags((150,), K, 91, DEV), [0])]
    cap = mil.CapturedBagStep(m, opt, _slots(C, p), warmup=1, warmup_batches=warm)
    twin = _Twin(twin_m, twin_opt, _slots(C, p), warm)
    return m, opt, cap, twin_m, twin_opt, twin


def _same_state(m, twin_m, opt, twin_opt):
    for (k, a), (_, b) in zip(m.state_dict().items(), twin_m.state_dict().items()):
        assert torch.equal(a, b), k
    for pa, pb in zip(m.parameters(), twin_m.parameters()):
        for key in ("exp_avg", "exp_avg_sq", "step"):
            assert torch.equal(torch.as_tensor(opt.state[pa][key]), torch.as_tensor(twin_opt.state[pb][key])), key


@pytest.mark.parametrize("p", [0.0, 0.25])
@pytest.mark.parametrize("model,C", MODELS)
def test_captured_trajectory_equals_the_eager_twin(model, C, p):
    m, opt, cap, twin_m, twin_opt, twin = _pair(model, C, p)
    assert [s.row_cap for s in cap.slots] == [200, 700] and cap.steps_taken == 2
    losses = []
    for i, (bags, labels) in enumerate(_batches(100)):
        loss, pred = cap.step(bags, labels)
        assert pred.shape == (len(bags), C)
        want = twin.step(bags, labels)
        assert torch.equal(loss, want), (i, float(loss), float(want))
        losses.append(float(loss))
    assert cap.replays == 6 and cap.eager_steps == 1 and cap.steps_taken == 9
    assert len(set(losses)) == len(losses) and all(np.isfinite(losses))
    _same_state(m, twin_m, opt, twin_opt)


def test_recapture_follows_an_lr_change():
    m, opt, cap, twin_m, twin_opt, twin = _pair("dsmil", 2, 0.0)
    batches = _batches(200)
    for bags, labels in batches[:2]:
        assert torch.equal(cap.step(bags, labels)[0], twin.step(bags, labels))
    before = {k: v.clone() for k, v in m.state_dict().items()}
    for o in (opt, twin_opt):
        for group in o.param_groups:
            group["lr"] = 5e-5
    cap.recapture()
    for k, v in m.state_dict().items():
        assert torch.equal(v, before[k]), k                     # recording takes no step
    for bags, labels in batches[2:6]:
        assert torch.equal(cap.step(bags, labels)[0], twin.step(bags, labels))
    _same_state(m, twin_m, opt, twin_opt)
    assert cap.replays == 6 and cap.eager_steps == 0


def test_remix_mixed_bags_step_through_a_slot():
    from wsi_hgnn_amd import mil
    from wsi_hgnn_amd.mil import remix
    S, Kp, V = 6, 8, 4
    g = torch.Generator().manual_seed(8)
    bank = remix.PrototypeBank(torch.randn(S, Kp, K, generator=g).to(DEV), (0.25 * torch.randn(S, Kp, V, K, generator=g)).to(DEV), [0, 1, 0, 1, 1, 0])
    m = _make("abmil", 1, 77).to(DEV)
    twin_m = copy.deepcopy(m)
    opt, twin_opt = _adam(m), _adam(twin_m)
    rng = np.random.RandomState(3)
    draws = [[remix.draw_mix(rng, bank.labels, idx, Kp, "joint", 0.5, V) for idx in pair] for pair in ((0, 3), (4, 1), (2, 5))]
    mixed = []
    for ds in draws:
        rows, sizes = remix.mix(bank, ds)
        mixed.append((torch.split(rows, sizes), [int(bank.labels[d.idx]) for d in ds]))
    slot_args = dict(feats=K, row_cap=2 * 4 * Kp + 1, bag_cap=2, num_classes=1, device=DEV)
    cap = mil.CapturedBagStep(m, opt, mil.BagSlot(**slot_args), warmup_batches=[mixed[0]])
    twin = _Twin(twin_m, twin_opt, [mil.BagSlot(**slot_args)], [mixed[0]])
    for bags, labels in mixed[1:]:
        loss, pred = cap.step(bags, labels)
        assert torch.equal(loss, twin.step(bags, labels)) and pred.shape == (2, 1)
    assert cap.replays == 2 and cap.eager_steps == 0
    _same_state(m, twin_m, opt, twin_opt)


def test_refusals():
    from wsi_hgnn_amd import mil, optim
    from wsi_hgnn_amd.mil import dsmil
    slot = mil.BagSlot(K, 100, 1, num_classes=2, device=DEV)
    m = _make("dsmil", 2, 1).to(DEV)
    with pytest.raises(ValueError, match="no batch to warm up"):
        mil.CapturedBagStep(m, _adam(m), slot)
    slot.load(BC.make_bags((50,), K, 1, DEV), [1])
    with pytest.raises(RuntimeError, match="capturable"):
        mil.CapturedBagStep(m, optim.Adam(m.parameters(), lr=1e-3), slot)
    with pytest.raises(RuntimeError, match="capturable"):
        mil.CapturedBagStep(m, torch.optim.Adam(m.parameters(), lr=1e-3), slot)
    dropping = dsmil.MILNet(dsmil.FCLayer(K, 2), dsmil.BClassifier(K, 2, dropout_v=0.2)).to(DEV)
    with pytest.raises(RuntimeError, match="Dropout"):
        mil.CapturedBagStep(dropping, _adam(dropping), slot)
    with pytest.raises(RuntimeError, match="GPU"):
        mil.CapturedBagStep(m, _adam(m), mil.BagSlot(K, 100, 1, device="cpu"))
    with pytest.raises(RuntimeError, match="not supported"):
        lin = torch.nn.Linear(K, 2).to(DEV)
        mil.CapturedBagStep(lin, _adam(lin), slot)
    with pytest.raises(ValueError, match="no slot"):
        mil.CapturedBagStep(m, _adam(m), [])
