"""The learning rate as a device word on the GPU.  The contract is bit-equality with the float rate: a step whose word holds the
double ``v`` leaves every bit - parameters, state tensors, step words - that the same step with ``lr = v`` leaves (tests/test_optim_gpu.py ties
the float path to ``torch.optim``, so no tolerance enters here).  All five kernel instances, vector and scalar path, more tensors than one
launch holds, gated tensors, a step recorded into a hipGraph, and the captured classes under ``torch.optim.lr_scheduler.CosineAnnealingLR``
without anything being recorded again - also across a ``load_state_dict``."""
import copy

import pytest
import torch

import bag_slot_cases as BC
import gtn_slot_cases as GS
import slot_cases as C

pytestmark = pytest.mark.gpu

DEV = "cuda"
RATES = (1e-2, 3.3e-3, 0.0, 7e-4)
RULES = {
    "sgd": ("SGD", dict()),
    "sgd_momentum": ("SGD", dict(momentum=0.9, nesterov=True)),
    "adagrad": ("Adagrad", dict(lr_decay=5e-3, weight_decay=5e-3, capturable=True)),
    "adadelta": ("Adadelta", dict()),
    "adam": ("Adam", dict(betas=(0.5, 0.9), weight_decay=5e-3, capturable=True)),          # the reference's MIL setting
}
SIZES = (1, 5, 4095, 4096, 4097, 0)            # around one workgroup's 4096 elements; a zero-element tensor takes no slot of the table


def _params(sizes, seed, unaligned=True):
    g = torch.Generator().manual_seed(seed)
    ps = [torch.randn(n, generator=g).to(DEV).requires_grad_() for n in sizes]
    if unaligned:                               # 4097 elements starting one element into their storage: no 16-byte alignment, the scalar path
        ps.append(torch.randn(4098, generator=g).to(DEV)[1:].detach().requires_grad_())
        assert ps[-1].data_ptr() % 16 == 4 and ps[-1].is_contiguous()
    return ps


def _twins(rule, sizes, seed=5, unaligned=True):
    """(parameters, optimizer with a word, the word), (parameters, optimizer with a float)."""
    from wsi_hgnn_amd import optim as O
    name, kw = RULES[rule]
    pa, pb = _params(sizes, seed, unaligned), _params(sizes, seed, unaligned)
    word = O.lr_word(RATES[0], DEV)
    return (pa, getattr(O, name)(pa, lr=word, **kw), word), (pb, getattr(O, name)(pb, lr=RATES[0], **kw))


def _set_grads(pa, pb, seed):
    g = torch.Generator().manual_seed(seed)
    for a, b in zip(pa, pb):
        grad = torch.randn(a.shape, generator=g).to(DEV)
        a.grad, b.grad = grad.clone(), grad.clone()


def _assert_same(pa, oa, pb, ob, what=""):
    for i, (a, b) in enumerate(zip(pa, pb)):
        assert torch.equal(a, b), (what, i, "p")
        sa, sb = oa.state.get(a, {}), ob.state.get(b, {})
        assert sa.keys() == sb.keys(), (what, i)
        for k in sa:
            assert torch.equal(torch.as_tensor(sa[k]), torch.as_tensor(sb[k])), (what, i, k)


@pytest.mark.parametrize("rule", list(RULES))
def test_a_word_steps_as_the_float_rate_bit_for_bit(rule):
    (pa, oa, word), (pb, ob) = _twins(rule, SIZES)
    for step, v in enumerate(RATES):
        _set_grads(pa, pb, 100 + step)
        word.fill_(v)
        for group in ob.param_groups:
            group["lr"] = v
        before = [p.detach().clone() for p in pa]
        moments = {k: t.clone() for k, t in oa.state.get(pa[3], {}).items() if k != "step"}
        oa.step()
        ob.step()
        _assert_same(pa, oa, pb, ob, (rule, step))
        moved = [not torch.equal(p, q) for p, q in zip(pa, before) if p.numel() > 1]
        if v == 0.0:
            assert not any(moved), (rule, "a rate of 0.0 moves no parameter")
            assert step > 0 and all(not torch.equal(oa.state[pa[3]][k], t) for k, t in moments.items()), (rule, "the moments move at rate 0.0")
        else:
            assert all(moved), (rule, step)
    assert oa.param_groups[0]["lr"] is word
    if "step" in oa._state_keys(oa.param_groups[0]):
        assert all(float(oa.state[p]["step"]) == len(RATES) for p in pa)


@pytest.mark.parametrize("rule", list(RULES))
def test_more_tensors_than_one_launch_holds(rule):
    sizes = [1 + (37 * i) % 300 for i in range(97)] + [4097, 0, 8193]          # 100 tensors, 99 non-empty: two launches of at most 88
    (pa, oa, word), (pb, ob) = _twins(rule, sizes, seed=6, unaligned=False)
    for step, v in enumerate(RATES[:3]):
        _set_grads(pa, pb, 200 + step)
        word.fill_(v)
        ob.param_groups[0]["lr"] = v
        oa.step()
        ob.step()
        _assert_same(pa, oa, pb, ob, (rule, step))


@pytest.mark.parametrize("rule", list(RULES))
def test_gate_and_word_together(rule):
    (pa, oa, word), (pb, ob) = _twins(rule, (5, 4097, 4096, 300), seed=7)
    table = torch.ones(2, device=DEV)
    for params, opt in ((pa, oa), (pb, ob)):
        opt.gate([params[1], params[4]], table, 0)             # an aligned and the unaligned tensor behind gate word 0
        opt.gate([params[2]], table, 1)
    _set_grads(pa, pb, 300)
    oa.step()
    ob.step()                                                   # every gate open: the state exists now
    _assert_same(pa, oa, pb, ob, (rule, "open"))
    table[0] = 0.0
    kept = [(pa[i].detach().clone(), {k: torch.as_tensor(v).clone() for k, v in oa.state.get(pa[i], {}).items()}) for i in (1, 4)]
    for step, v in enumerate(RATES[1:3] + RATES[:1]):
        _set_grads(pa, pb, 301 + step)
        word.fill_(v)
        ob.param_groups[0]["lr"] = v
        oa.step()
        ob.step()
        _assert_same(pa, oa, pb, ob, (rule, step))
        for i, (p0, st0) in zip((1, 4), kept):                  # gate word 0.0: p, the states and the step word bit for bit as they were
            assert torch.equal(pa[i], p0), (rule, step, i)
            for k, t in st0.items():
                assert torch.equal(torch.as_tensor(oa.state[pa[i]][k]), t), (rule, step, i, k)
    assert float(word) == RATES[0]
    if "step" in oa._state_keys(oa.param_groups[0]):
        assert [float(oa.state[pa[i]]["step"]) for i in range(5)] == [4.0, 1.0, 4.0, 4.0, 1.0]


@pytest.mark.parametrize("rule", list(RULES))
def test_a_recorded_step_follows_every_fill_of_the_word(rule):
    """The step itself recorded under capture_error_mode="thread_local" - any read-back of the word would raise there - and replayed three times
    with a fill_ before each, against an eager float twin."""
    (pa, oa, word), (pb, ob) = _twins(rule, (5, 4097, 4096), seed=8)
    _set_grads(pa, pb, 400)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        oa.step()                                               # (state, ticket words and the descriptor table exist before the capture)
    torch.cuda.current_stream().wait_stream(side)
    ob.step()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, capture_error_mode="thread_local"):
        oa.step()
    _assert_same(pa, oa, pb, ob, (rule, "recording takes no step"))
    for step, v in enumerate(RATES[1:]):
        g = torch.Generator().manual_seed(401 + step)
        for a, b in zip(pa, pb):
            grad = torch.randn(a.shape, generator=g).to(DEV)
            a.grad.copy_(grad)                                  # (the graph holds the gradients' pointers)
            b.grad = grad
        word.fill_(v)
        graph.replay()
        ob.param_groups[0]["lr"] = v
        ob.step()
        _assert_same(pa, oa, pb, ob, (rule, step))


# ---- the captured classes under torch's CosineAnnealingLR ------------------------------------------------------------------------------

def _cosine(opt):
    return torch.optim.lr_scheduler.CosineAnnealingLR(opt, T_max=4, eta_min=5e-6)


def _follow(word, twin_opt) -> float:
    """The eager twin's float rate set to float(word)."""
    v = float(word)
    for group in twin_opt.param_groups:
        group["lr"] = v
    return v


def _same_model_and_adam(m, twin_m, opt, twin_opt):
    for (k, a), (_, b) in zip(m.state_dict().items(), twin_m.state_dict().items()):
        assert torch.equal(a, b), k
    _assert_same(list(m.parameters()), opt, list(twin_m.parameters()), twin_opt)          # (a parameter no loss reaches has no state on either side)
    assert sum("exp_avg" in opt.state.get(p, {}) for p in m.parameters()) >= 4


def _run_scheduled(step_cap, step_twin, batches, cap, opt, twin_opt, word):
    """``batches`` through the captured side and the eager twin, the scheduler stepped after every two steps; the rates that were in force."""
    graphs = list(cap.graphs)
    sched = _cosine(opt)
    rates = [_follow(word, twin_opt)]
    for i, batch in enumerate(batches):
        a, b = step_cap(batch), step_twin(batch)
        assert torch.equal(a, b), (i, float(a), float(b))
        if i % 2 == 1:
            sched.step()
            rates.append(_follow(word, twin_opt))
    assert len(cap.graphs) == len(graphs) and all(a is b for a, b in zip(cap.graphs, graphs))       # nothing was recorded again
    assert opt.param_groups[0]["lr"] is word
    assert len(set(rates)) == len(rates) and all(5e-6 <= r <= rates[0] for r in rates), rates
    return rates


# GTNMIL: the configuration of tests/test_gtn_slot_gpu.py
GTN_SIZES = (40, 55, 129, 100, 60, 150, 30, 139)
GTN_BATCHES = (([0, 1], [1, 0]), ([2, 3], [2, 2]), ([4], [0]), ([5, 0], [1, 2]), ([6, 7], [0, 1]), ([1, 6], [2, 0]))        # the fourth fits no slot
GTN_WARM = (([2], [1]), ([0], [0]))


def _gtn_slots(gtn, ss):
    cap = 2 * max(ss.entries)
    return [gtn.GraphSlot(GS.SMALL["in_feats"], 2, 140, cap, device=DEV), gtn.GraphSlot(GS.SMALL["in_feats"], 2, 60, cap, device=DEV)]


def test_captured_gtn_step_follows_a_torch_scheduler_without_recapture():
    from wsi_hgnn_amd import gtn, optim
    ss = gtn.SlideSet(GS.shuffled_slides(GTN_SIZES, GS.SMALL["in_feats"], 300, [i % 2 == 0 for i in range(len(GTN_SIZES))]), device=DEV)
    m = GS.build_model(gtn, GS.SMALL, GS.model_case((2,), (True,), seed=400)[2], DEV)
    twin_m = copy.deepcopy(m)
    word = optim.lr_word(1e-3, DEV)
    opt = optim.Adam(m.parameters(), lr=word, weight_decay=5e-4, capturable=True)
    twin_opt = optim.Adam(twin_m.parameters(), lr=1e-3, weight_decay=5e-4, capturable=True)
    cap = gtn.CapturedGraphStep(m, opt, _gtn_slots(gtn, ss), warmup=1, warmup_batches=[(ss, *w) for w in GTN_WARM])
    slots = _gtn_slots(gtn, ss)
    order = sorted(range(2), key=lambda i: slots[i].num_rows)
    for i in order:                                             # the twin: the same loads on slots of its own, gtn.slot_step where the class replays
        gtn.slot_step(twin_m, twin_opt, slots[i].load(ss, *GTN_WARM[i]))
    slots = [slots[i] for i in order]

    def twin_step(batch):
        idxs, labels = batch
        sizes, entries = [ss.sizes[i] for i in idxs], [ss.entries[i] for i in idxs]
        slot = next((s for s in slots if s.fits(sizes, entries)), None)
        if slot is not None:
            return gtn.slot_step(twin_m, twin_opt, slot.load(ss, idxs, labels))[0]
        return gtn.train_one_step(twin_m, ss.batch(idxs), torch.tensor(labels, device=DEV), twin_opt)

    rates = _run_scheduled(lambda b: cap.step(ss, *b)[0], twin_step, GTN_BATCHES, cap, opt, twin_opt, word)
    assert len(rates) == 4 and cap.replays == 5 and cap.eager_steps == 1
    _same_model_and_adam(m, twin_m, opt, twin_opt)


# DSMIL: the configuration of tests/test_bag_slot_gpu.py
K = 64


def _dsmil(seed):
    from wsi_hgnn_amd.mil import dsmil
    torch.manual_seed(seed)
    return dsmil.MILNet(dsmil.FCLayer(K, 2), dsmil.BClassifier(K, 2, dropout_v=0.0)).to(DEV)


def _bag_slots(mil):
    return [mil.BagSlot(K, 700, 2, num_classes=2, device=DEV, dropout_patch=0.0, seed=4), mil.BagSlot(K, 200, 2, num_classes=2, device=DEV, dropout_patch=0.0, seed=4)]


def _bag_batches(seed):
    sizes = [(300, 129), (650,), (127, 2), (0, 400), (699,), (201,), (500, 300)]          # the third fits the small slot, the last fits neither
    labels = [(1, 0), (0,), (1, 1), (0, 1), (1,), (0,), (1, 0)]
    return [(BC.make_bags(s, K, seed + i, DEV), list(l)) for i, (s, l) in enumerate(zip(sizes, labels))]


def _bag_pair():
    from wsi_hgnn_amd import mil, optim
    m = _dsmil(502)
    twin_m = copy.deepcopy(m)
    word = optim.lr_word(2e-4, DEV)
    adam = dict(betas=(0.5, 0.9), weight_decay=5e-3, capturable=True)
    opt, twin_opt = optim.Adam(m.parameters(), lr=word, **adam), optim.Adam(twin_m.parameters(), lr=2e-4, **adam)
    warm = [(BC.make_bags((600,), K, 90, DEV), [1]), (BC.make_bags((150,), K, 91, DEV), [0])]
    cap = mil.CapturedBagStep(m, opt, _bag_slots(mil), warmup=1, warmup_batches=warm)
    slots = _bag_slots(mil)
    order = sorted(range(2), key=lambda i: slots[i].row_cap)
    twin_m.train()
    for i in order:
        slots[i].load(*warm[i])
        mil.slot_step(twin_m, twin_opt, slots[i])
    slots = [slots[i] for i in order]

    def twin_step(batch):
        bags, labels = batch
        sizes = [int(t.shape[0]) for t in bags]
        slot = next((s for s in slots if s.fits(sizes)), None)
        if slot is not None:
            slot.load(bags, labels)
            return mil.slot_step(twin_m, twin_opt, slot)[0]
        x, plan = mil.dropout_patches(torch.cat(list(bags)), sizes, 0.0, None)
        return mil.train_one_step(twin_m, twin_opt, x, plan, labels)

    return m, opt, word, cap, twin_m, twin_opt, twin_step


def test_captured_bag_step_follows_a_torch_scheduler_without_recapture():
    m, opt, word, cap, twin_m, twin_opt, twin_step = _bag_pair()
    rates = _run_scheduled(lambda b: cap.step(*b)[0], twin_step, _bag_batches(200), cap, opt, twin_opt, word)
    assert len(rates) == 4 and cap.replays == 6 and cap.eager_steps == 1
    _same_model_and_adam(m, twin_m, opt, twin_opt)


def test_captured_slot_step_over_heatnet4_follows_a_torch_scheduler():
    """trainer.CapturedSlotStep has no recapture(): a word is the only way it follows a schedule.  The smallest slot of tests/slot_cases.py."""
    from wsi_hgnn_amd import models, optim
    from wsi_hgnn_amd.data import BatchSlot
    from wsi_hgnn_amd.trainer import CapturedSlotStep
    ld = C.loader(torch.device("cuda:0"))
    lf = torch.nn.CrossEntropyLoss()

    def make(lr):
        torch.manual_seed(3)
        m = models.HEATNet4(C.IN_DIM, 64, 2, 2, 4, C.ND, 0.0, "mean").to("cuda:0").eval()
        return m, optim.Adam(m.parameters(), lr=lr, weight_decay=5e-3, capturable=True)

    word = optim.lr_word(1e-3, "cuda:0")
    m, opt = make(word)
    twin_m, twin_opt = make(1e-3)
    cap = CapturedSlotStep(m, opt, lf, BatchSlot(ld, C.SMALL), warmup=1, warmup_batches=[[4]])
    slot = BatchSlot(ld, C.SMALL)

    def twin_step(idxs):
        slot.load(idxs)
        twin_opt.zero_grad(set_to_none=True)
        loss = lf(twin_m(slot.graph), slot.labels)
        loss.backward()
        twin_opt.step()
        return loss.detach()

    twin_step([4])                                              # the warm-up step
    rates = _run_scheduled(lambda idxs: cap.step(idxs)[0], twin_step, C.SMALL_CASES + C.SMALL_CASES, cap, opt, twin_opt, word)
    assert len(rates) == 4 and cap.replays == 6 and cap.eager_steps == 0
    _same_model_and_adam(m, twin_m, opt, twin_opt)


def test_a_checkpoint_loaded_under_a_capture_is_what_the_next_replay_steps_from():
    m, opt, word, cap, twin_m, twin_opt, twin_step = _bag_pair()
    batches = _bag_batches(300)[:6]
    graphs, ptr = list(cap.graphs), word.data_ptr()
    sched = _cosine(opt)
    _follow(word, twin_opt)
    assert torch.equal(cap.step(*batches[0])[0], twin_step(batches[0]))
    ckpt = copy.deepcopy(twin_opt.state_dict())                 # a FLOAT optimizer's checkpoint: moments and counts after three steps ...
    assert type(ckpt["param_groups"][0]["lr"]) is float
    ckpt["param_groups"][0]["lr"] = 7.5e-5                       # ... and a rate neither side holds
    for b in batches[1:3]:
        assert torch.equal(cap.step(*b)[0], twin_step(b))
    sched.step()
    assert float(word) != 7.5e-5 and _follow(word, twin_opt) != 2e-4
    opt.load_state_dict(copy.deepcopy(ckpt))
    twin_opt.load_state_dict(copy.deepcopy(ckpt))
    assert opt.param_groups[0]["lr"] is word and word.data_ptr() == ptr and float(word) == 7.5e-5
    assert type(twin_opt.param_groups[0]["lr"]) is float and twin_opt.param_groups[0]["lr"] == 7.5e-5
    assert isinstance(opt.param_groups[0]["initial_lr"], torch.Tensor) and opt.param_groups[0]["initial_lr"].data_ptr() != ptr
    assert all(float(opt.state[p]["step"]) == 3.0 for p in m.parameters())
    for b in batches[3:]:
        assert torch.equal(cap.step(*b)[0], twin_step(b))
    assert all(a is b for a, b in zip(cap.graphs, graphs)) and cap.replays == 6 and cap.eager_steps == 0
    _same_model_and_adam(m, twin_m, opt, twin_opt)
