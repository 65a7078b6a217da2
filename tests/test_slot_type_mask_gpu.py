"""Batch slots with a device-side presence table on the GPU: the presence kernel (csrc/segment_table.hip) against the tensor
route bit for bit; the masked heads of HEATNet2 / HEATNet4 / HGT on a batch that lacks a node type against the loader's unpadded batch by the
project's 1e-4 rule; the optimizer gate of csrc/optim.hip under every rule; trainer.CapturedSlotStep / CapturedSlotEval over ``type_mask``
slots against eager twins.  Fixture: tests/type_mask_cases.py, exact fp32 GEMMs."""
import copy

import pytest
import torch

import type_mask_cases as M

pytestmark = pytest.mark.gpu


def _dev():
    return torch.device("cuda", torch.cuda.current_device())


@pytest.fixture(scope="module")
def ld():
    from wsi_hgnn_amd import ops
    ops.set_gemm_precision("fp32")
    return M.loader(_dev())


@pytest.fixture(scope="module")
def ald():
    return M.loader(_dev(), augment=True)


# ------------------------------------------------------------------------------------------------ 1. the presence kernel
def test_presence_kernel_equals_the_tensor_route_bit_for_bit(ld, ald):
    """Plain, augmented and quota fills of a GPU slot and of a CPU slot side by side, a poison value in the GPU table before every fill, a
    present batch behind an absent one in every series: the same 32-bit words."""
    from wsi_hgnn_amd.data import BatchSlot
    emptying, sparing = M.found_draws()
    cld, cald = M.loader("cpu"), M.loader("cpu", augment=True)

    def quota(i):
        qn, qe = M.stored_quota(cald, i)
        return [0 if (i, t) == (M.THREE, M.RARE) else q for t, q in enumerate(qn)], qe

    plain = [(idxs, None) for idxs, _ in M.PLAIN + [M.PLAIN[1], M.PLAIN[0]]]
    aug = [([M.THREE], [emptying]), ([M.THREE], [sparing]), ([M.THREE, M.TYPELESS], [emptying, 5]), ([M.THREE, 1], [emptying, 5]),
           ([M.TYPELESS], [9]), ([0, 1], [1, 2])]
    quo = [([M.THREE], [sparing]), ([M.THREE, 5], [sparing, 3]), ([M.THREE, M.TYPELESS], [sparing, 3]), ([0, 1], [1, 2])]
    seen = set()
    for g, c, series in ((BatchSlot(ld, M.BIG, type_mask=True), BatchSlot(cld, M.BIG, type_mask=True), plain),
                         (BatchSlot(ald, M.BIG, type_mask=True), BatchSlot(cald, M.BIG, type_mask=True), aug),
                         (BatchSlot(ald, M.BIG, quota=quota, type_mask=True), BatchSlot(cald, M.BIG, quota=quota, type_mask=True), quo)):
        for idxs, draws in series:
            g.type_present.fill_(float("nan"))
            g.load(idxs, draws)
            c.load(idxs, draws)
            assert torch.equal(g.type_present.cpu().view(torch.int32), c.type_present.view(torch.int32)), (idxs, draws, g.type_present.tolist())
            assert torch.equal(g.bufs["seg_nonempty"].cpu().view(torch.int32), c.bufs["seg_nonempty"].view(torch.int32)), (idxs, draws)
            seen.add(tuple(c.type_present.tolist()))
        assert g.type_present.tolist() == [1.0, 1.0, 1.0]              # every series ends on a present batch behind an absent one
    assert seen == {(1.0, 1.0, 1.0), (1.0, 1.0, 0.0)}


def test_presence_entry_point_reads_the_real_slides_only():
    """The C entry point by hand: T = 70 (more node types than a wave has lanes), the filler column set everywhere, b_cap = 0 and bad arguments."""
    from wsi_hgnn_amd import _native as N
    lib, dev = N.load(), _dev()
    T, graphs, b_cap = 70, 4, 3
    gen = torch.Generator().manual_seed(2)
    ne = (torch.rand(T, graphs, generator=gen) < 0.2).to(torch.float32)
    ne[:, b_cap:] = 1.0                                                # the filler holds every type
    ne[5], ne[69, 2] = 0.0, 1.0
    ne[5, b_cap:] = 1.0
    table = ne.reshape(-1).to(dev)
    out = torch.full((T + 1,), -7.0, device=dev)
    N.check(lib.wsi_type_present(N.ptr(table), T, graphs, b_cap, N.ptr(out), N.stream()), "wsi_type_present")
    want = (ne[:, :b_cap] != 0).any(dim=1).to(torch.float32)
    assert torch.equal(out[:T].cpu(), want) and out[T].item() == -7.0 and want[5] == 0.0 and want[69] == 1.0 and 0 < want.sum() < T
    N.check(lib.wsi_type_present(N.ptr(table), T, graphs, 0, N.ptr(out), N.stream()), "wsi_type_present")
    assert out[:T].abs().sum().item() == 0.0 and out[T].item() == -7.0
    for args in ((0, graphs, b_cap), (T, graphs, graphs + 1), (T, graphs, -1)):
        assert lib.wsi_type_present(N.ptr(table), *args, N.ptr(out), N.stream()) == N.WSI_EINVAL
    assert lib.wsi_type_present(N.ptr(table), T, graphs, b_cap, None, N.stream()) == N.WSI_EINVAL


# ------------------------------------------------------------------------------------------------ 2. forward and backward
def _model(ld, name, hidden=64, drop=0.0, train=False):
    from wsi_hgnn_amd import models
    torch.manual_seed(3)
    if name == "HGT":
        ed = {tuple(r): i for i, r in enumerate(ld.items[0].rels)}
        m = models.HGT(M.ND, ed, M.IN_DIM, hidden, 2, 2, 4, use_norm=True, graph_pooling_type="mean")
    else:
        m = getattr(models, name)(M.IN_DIM, hidden, 2, 2, 4, M.ND, drop, "mean")
    m = m.to(_dev())
    return m.train() if train else m.eval()


def _run(m, graph, labels, rows):
    lf = torch.nn.CrossEntropyLoss()
    m.zero_grad(set_to_none=True)
    logits = m(graph)
    loss = lf(logits, labels)
    loss.backward()
    return logits.detach()[:rows].clone(), loss.item(), {k: (None if p.grad is None else p.grad.clone()) for k, p in m.named_parameters()}


def _close(tag, a, b):
    """The project's 1e-4 rule: logits and loss within 1e-4, every gradient within 1e-4 of its tensor's largest entry."""
    (la, lossa, ga), (lb, lossb, gb) = a, b
    print(tag, "logits", (la - lb).abs().max().item(), "loss", abs(lossa - lossb))
    assert (la - lb).abs().max().item() <= 1e-4 and abs(lossa - lossb) <= 1e-4, tag
    for k in ga:
        if ga[k] is None:
            continue
        err, top = (ga[k] - gb[k]).abs().max().item(), ga[k].abs().max().item()
        print(tag, k, err, top)
        assert err <= 1e-4 * top, (tag, k, err, top)


@pytest.mark.parametrize("name", ["HEATNet2", "HEATNet4", "HGT"])
@pytest.mark.parametrize("idxs", [[M.TYPELESS], [M.TYPELESS, 6]])
def test_masked_heads_on_a_batch_without_a_type_match_the_unpadded_batch(ld, name, idxs):
    """Logits of the real slides, loss and every gradient on the slot graph against the same model on the loader's unpadded batch.  A
    parameter is without a gradient on the unpadded side exactly when ``type_gated_parameters()[2]`` names it, and there the padded side
    holds exact zeros."""
    from wsi_hgnn_amd.data import BatchSlot
    m = _model(ld, name)
    slot = BatchSlot(ld, M.BIG, per_relation_src=(name == "HGT"), type_mask=True).load(idxs)
    assert slot.type_present.tolist() == [1.0, 1.0, 0.0]
    G, y, _ = ld._assemble(idxs, 0)
    ref, got = _run(m, G, y, len(idxs)), _run(m, slot.graph, slot.labels, len(idxs))
    dead = set(m.dead_parameter_names())
    names = {id(p): k for k, p in m.named_parameters()}
    gated = [{names[id(p)] for p in ps} for ps in m.type_gated_parameters()]
    assert len(gated) == 3
    none_unpadded = {k for k, g in ref[2].items() if g is None} - dead
    print(name, "gradient None on the unpadded batch:", sorted(none_unpadded))
    assert none_unpadded == gated[M.RARE], (sorted(none_unpadded), sorted(gated[M.RARE]))
    assert {k for k, g in got[2].items() if g is None} == dead
    for k in gated[M.RARE]:
        assert got[2][k].abs().max().item() == 0.0, k
    _close((name, idxs), ref, got)


@pytest.mark.parametrize("name", ["HEATNet2", "HEATNet4", "HGT"])
def test_a_present_type_gives_the_default_slot_bits(ld, name):
    """Multiplying by 1.0 is exact: logits, loss and every gradient of a batch in which every type is present, ``type_mask`` slot against the
    default slot."""
    from wsi_hgnn_amd.data import BatchSlot
    m = _model(ld, name)
    for idxs in ([0, 1], [M.THREE], [M.HUB, 5]):
        a = BatchSlot(ld, M.BIG, per_relation_src=(name == "HGT"), type_mask=True).load(idxs)
        b = BatchSlot(ld, M.BIG, per_relation_src=(name == "HGT")).load(idxs)
        assert a.type_present.tolist() == [1.0, 1.0, 1.0]
        (la, lossa, ga), (lb, lossb, gb) = _run(m, a.graph, a.labels, 3), _run(m, b.graph, b.labels, 3)
        assert torch.equal(la, lb) and lossa == lossb, idxs
        for k in ga:
            assert (ga[k] is None and gb[k] is None) or torch.equal(ga[k], gb[k]), (idxs, k)


def test_heatnet4_without_normalised_blocks_masks_sum_and_columns(ld):
    """The ``normalize_attn=False`` path: ``hg`` sums the present types only and the absent type's columns are exact zeros."""
    from wsi_hgnn_amd.data import BatchSlot
    m = _model(ld, "HEATNet4")
    for t in "012":
        m.attn[t].normalize_attn = False
    idxs = [M.TYPELESS]
    slot = BatchSlot(ld, M.BIG, type_mask=True).load(idxs)
    G, y, _ = ld._assemble(idxs, 0)
    ref, got = _run(m, G, y, 1), _run(m, slot.graph, slot.labels, 1)
    names = {id(p): k for k, p in m.named_parameters()}
    gated = {names[id(p)] for p in m.type_gated_parameters()[M.RARE]}
    assert {k for k, g in ref[2].items() if g is None} - set(m.dead_parameter_names()) == gated == {"attn.2.op.weight"}
    assert got[2]["attn.2.op.weight"].abs().max().item() == 0.0
    _close(("HEATNet4 sigmoid blocks", idxs), ref, got)


# ------------------------------------------------------------------------------------------------ 3. the optimizer gate
SIZES = [1, 7, 1024, 1025, 0]
BOUND = {0: 0, 2: 1, 4: 0}                    # tensor -> word of the gate table; tensors 1 and 3 have no gate

RULES = {"sgd": lambda O, ps: O.SGD(ps, lr=0.1, weight_decay=0.01),
         "sgd_momentum": lambda O, ps: O.SGD(ps, lr=0.1, momentum=0.9, weight_decay=0.01, nesterov=True),
         "adagrad": lambda O, ps: O.Adagrad(ps, lr=0.1, lr_decay=0.1, weight_decay=0.01, capturable=True),
         "adadelta": lambda O, ps: O.Adadelta(ps, lr=1.0, weight_decay=0.01),
         "adam": lambda O, ps: O.Adam(ps, lr=0.1, weight_decay=0.01, capturable=True)}


def _snapshot(opt, params):
    out = []
    for p in params:
        st = opt.state.get(p, {})
        out.append([p.detach().clone()] + [v.clone() for _, v in sorted(st.items()) if isinstance(v, torch.Tensor)])
    return out


@pytest.mark.parametrize("rule", sorted(RULES))
def test_gated_launch_leaves_closed_tensors_alone_and_steps_the_others_as_ever(rule):
    """Five tensors (1, 7, 1024, 1025 and 0 elements), three bound to two gate words, two unbound.  Step 1 with every gate open creates the
    state; step 2 closes word 0 (tensors 0 and 4), step 3 flips the words ON THE SAME descriptor table (tensor 2 closed).  A closed tensor's
    p, state tensors and step word are torch.equal to their values before, the ticket words stay zero, and every other tensor is
    torch.equal to an ungated twin that starts the step from the same state."""
    from wsi_hgnn_amd import optim as O
    dev = _dev()
    gen = torch.Generator().manual_seed(11)
    params = [torch.nn.Parameter(torch.randn(n, generator=gen).to(dev)) for n in SIZES]
    opt = RULES[rule](O, params)
    table = torch.ones(2, device=dev)
    for i, w in BOUND.items():
        opt.gate([params[i]], table, w)
    cached = None
    for step, words in enumerate(([1.0, 1.0], [0.0, 1.0], [3.0, 0.0])):
        table.copy_(torch.tensor(words))
        closed = {i for i, w in BOUND.items() if words[w] == 0.0}
        grads = [torch.randn(n, generator=gen).to(dev) for n in SIZES]
        twin_params = [torch.nn.Parameter(p.detach().clone()) for p in params]
        twin = RULES[rule](O, twin_params)
        if step:
            twin.load_state_dict(copy.deepcopy(opt.state_dict()))
        for p, q, g in zip(params, twin_params, grads):
            p.grad, q.grad = g.clone(), g.clone()
        before = _snapshot(opt, params)
        opt.step()
        twin.step()
        torch.cuda.synchronize()
        after, want = _snapshot(opt, params), _snapshot(twin, twin_params)
        for i in range(len(SIZES)):
            if i in closed and step:
                assert len(after[i]) == len(before[i]) and all(torch.equal(a, b) for a, b in zip(after[i], before[i])), (rule, step, i)
                if SIZES[i]:
                    assert not torch.equal(want[i][0], before[i][0]), (rule, step, i)        # (the twin did move it: the comparison says something)
            else:
                assert len(after[i]) == len(want[i]) and all(torch.equal(a, b) for a, b in zip(after[i], want[i])), (rule, step, i)
        tickets = opt.__dict__.get("_wsi_tickets", {}).get(dev)
        assert tickets is None or int(tickets.abs().sum()) == 0, (rule, step)
        tables = opt.__dict__.get("_wsi_tables", {}).get(0)           # (the first step's table goes with the ticket index it creates)
        assert step < 2 or (tables is not None and tables is cached), "the descriptor table was rebuilt between the closed steps"
        cached = tables
    if rule not in ("sgd", "sgd_momentum"):                          # the closed steps were not counted: tensors 0 and 4 once, tensor 2 once
        assert [float(opt.state[p]["step"]) for p in params] == [2.0, 3.0, 2.0, 3.0, 2.0]
    opt.gate(params, None)                                            # unbound: the plain entry point again, every tensor stepped
    for p in params:
        p.grad = torch.ones_like(p)
    opt.step()
    if rule not in ("sgd", "sgd_momentum"):
        assert [float(opt.state[p]["step"]) for p in params] == [3.0, 4.0, 3.0, 4.0, 3.0]


def test_gated_entry_point_checks_its_arguments():
    from wsi_hgnn_amd import _native as N
    import ctypes
    lib, dev = N.load(), _dev()
    p, g, s0, s1 = (torch.zeros(8, device=dev) for _ in range(4))
    arr = (N.OptimTensor * 1)()
    arr[0].p, arr[0].g, arr[0].s0, arr[0].s1, arr[0].n = p.data_ptr(), g.data_ptr(), s0.data_ptr(), s1.data_ptr(), 8
    h = N.OptimHyper()
    h.lr, h.beta1, h.beta2, h.eps, h.host_step = 0.1, 0.9, 0.999, 1e-8, 1.0
    table = torch.zeros(2, device=dev)
    call = lambda rule, idx, tab, n: lib.wsi_optim_step_gated(rule, ctypes.cast(arr, ctypes.c_void_p), 1, ctypes.addressof(h),
                                                              ctypes.cast((ctypes.c_int32 * 1)(idx), ctypes.c_void_p), tab, n, N.stream())
    assert call(N.WSI_OPTIM_ADAM, 3, N.ptr(table), 2) == N.WSI_EINVAL            # index outside the table
    assert call(N.WSI_OPTIM_ADAM, 1, None, 2) == N.WSI_EINVAL                    # gated without a table
    assert call(N.WSI_OPTIM_ADAM, 1, N.ptr(table), 256) == N.WSI_EINVAL          # more words than an index byte reaches
    assert call(N.WSI_OPTIM_ADAM, 1, N.ptr(table), 2) == N.WSI_EINVAL            # a rule that reads t, gated, with a host count
    assert b"host count" in lib.wsi_last_error()
    assert call(N.WSI_OPTIM_SGD, 1, N.ptr(table), 2) == 0                        # SGD reads no count; the gate is closed: nothing moves
    g.fill_(1.0)
    assert call(N.WSI_OPTIM_SGD, 1, N.ptr(table), 2) == 0
    torch.cuda.synchronize()
    assert p.abs().sum().item() == 0.0
    assert call(N.WSI_OPTIM_SGD, 0, None, 0) == 0                                # no gate at all: wsi_optim_step
    torch.cuda.synchronize()
    assert torch.equal(p, torch.full_like(p, -0.1))


# ------------------------------------------------------------------------------------------------ 4. the trajectory
SEQUENCE = [[0, 1], [M.TYPELESS], [M.HUB, 5], [M.TYPELESS, 6], [1, M.THREE], M.NO_FIT]      # [TYPELESS]: the small slot; NO_FIT: eagerly
WARM = [[M.HUB, 5], [5]]                                                                    # big slot, small slot


def _adam(m):
    from wsi_hgnn_amd import optim
    return optim.Adam(m.parameters(), lr=1e-3, weight_decay=5e-3, capturable=True)


def _gated_state(m, o):
    """The parameters gated on the rare type, their moments and their step words."""
    out = []
    for p in m.type_gated_parameters()[M.RARE]:
        st = o.state[p]
        out += [p.detach().clone(), st["exp_avg"].clone(), st["exp_avg_sq"].clone(), st["step"].clone()]
    return out


def _padded_twin(ld, m, o, sequence, base):
    """Eager steps on the slots' own graphs with the same presence table and the same gates, in CapturedSlotStep's order (small slot first)."""
    from wsi_hgnn_amd import ops
    from wsi_hgnn_amd.data import BatchSlot
    lf = torch.nn.CrossEntropyLoss()
    big = BatchSlot(ld, M.BIG, type_mask=True)
    small = BatchSlot(ld, M.SMALL, type_mask=big.type_present)
    for t, ps in enumerate(m.type_gated_parameters()):
        o.gate(ps, big.type_present, t)
    losses = []

    def one(G, y):
        o.zero_grad(set_to_none=True)
        with ops.dropout_seed_base(base):
            l = lf(m(G), y)
            l.backward()
        o.step()
        if base is not None:
            ops.advance_dropout_seed_base(base)
        return l.item()

    for slot, idxs in ((small, WARM[1]), (big, WARM[0])):
        slot.load(idxs)
        one(slot.graph, slot.labels)
    for idxs in sequence:
        slot = small if small.fits(idxs) else (big if big.fits(idxs) else None)
        if slot is None:
            big.type_present.fill_(1.0)
            G, y, _ = ld._assemble(idxs, 0)
            losses.append(one(G, y))
        else:
            slot.load(idxs)
            losses.append(one(slot.graph, slot.labels))
    return losses


def _unpadded_twin(ld, m, o, sequence):
    """Eager steps on the loader's unpadded batches: an absent head has no gradient and the optimizer leaves it alone by itself."""
    lf = torch.nn.CrossEntropyLoss()
    losses = []
    for idxs in [WARM[1], WARM[0]] + list(sequence):
        G, y, _ = ld._assemble(idxs, 0)
        o.zero_grad(set_to_none=True)
        l = lf(m(G), y)
        l.backward()
        o.step()
        losses.append(l.item())
    return losses[2:]


@pytest.mark.parametrize("drop", [0.2, 0.0])
def test_captured_trajectory_over_batches_that_lack_a_type(ld, monkeypatch, drop):
    """CapturedSlotStep over two ``type_mask`` slots, HEATNet4, capturable Adam: ordinary batches, the type-less batch twice (once per slot)
    and one batch that fits no slot.  The losses and the final state equal, bit for bit, those of eager steps on the slots' own graphs under
    the same gates; the gated parameters, their moments and their step words are untouched across each type-less step and trail the other
    step words by exactly two at the end; the eager fallback leaves the shared table all ones.

    With feat_drop 0.2 (train mode) the counter-based dropout mask is a function of the ROW of the node table, and a slot's rows are not the
    unpadded batch's (the filler sits between the node types): the two draw different masks, so the comparison with the unpadded twin - every
    loss within 1e-4 - is made at feat_drop 0.0, where nothing else differs.  (Parameters are not compared there: Adam turns a gradient
    element of the size of the 1e-4 rule's own noise into a step of +-lr.)"""
    from wsi_hgnn_amd import ops
    from wsi_hgnn_amd.data import BatchSlot
    from wsi_hgnn_amd.trainer import CapturedSlotStep
    lf = torch.nn.CrossEntropyLoss()
    calls = {"n": 0}

    def seeds():                                   # the host seeds of a step: the same two values at every step (what a capture freezes them to)
        calls["n"] += 1
        return 1000 + (calls["n"] % 2)

    monkeypatch.setattr(ops, "next_dropout_seed", seeds)
    train = drop > 0
    m2 = _model(ld, "HEATNet4", 128, drop, train)
    o2 = _adam(m2)
    slots = [BatchSlot(ld, M.BIG, type_mask=True), BatchSlot(ld, M.SMALL, type_mask=True)]
    step = CapturedSlotStep(m2, o2, lf, slots, warmup=1, warmup_batches=WARM)
    assert all(s.type_present is step.type_table for s in step.slots) and step.type_table is slots[0].type_present
    first = None if step.seed_base is None else int(step.seed_base.item()) - 2 * ops.SEED_STRIDE
    got, typeless = [], 0
    for idxs in SEQUENCE:
        before = _gated_state(m2, o2)
        loss, logits = step.step(idxs)
        assert logits.shape == (len(idxs), 2)
        got.append(loss.item())
        if all(ld.items[i].num_nodes[M.RARE] == 0 for i in idxs):
            typeless += 1
            assert step.type_table.tolist() == [1.0, 1.0, 0.0]
            after = _gated_state(m2, o2)
            assert len(before) == 12 and all(torch.equal(a, b) for a, b in zip(before, after)), idxs
        else:
            assert step.type_table.tolist() == [1.0, 1.0, 1.0], idxs
            assert not torch.equal(before[0], _gated_state(m2, o2)[0]), idxs
    assert typeless == 2 and step.replays == 5 and step.eager_steps == 1 and step.slot_for([M.TYPELESS]) == 0 and step.slot_for(M.NO_FIT) is None
    names = {id(p): k for k, p in m2.named_parameters()}
    gated = {names[id(p)] for p in m2.type_gated_parameters()[M.RARE]}
    counts = {k: float(o2.state[p]["step"]) for k, p in m2.named_parameters() if p in o2.state}
    assert {k for k, v in counts.items() if v == 6.0} == gated and {v for k, v in counts.items() if k not in gated} == {8.0}, counts

    m1 = _model(ld, "HEATNet4", 128, drop, train)
    base = None if first is None else torch.tensor([((first + (1 << 31)) % (1 << 32)) - (1 << 31)], dtype=torch.int32, device=_dev())
    eager = _padded_twin(ld, m1, _adam(m1), SEQUENCE, base)
    assert got == eager, (got, eager)
    for (k, a), (_, b) in zip(m1.state_dict().items(), m2.state_dict().items()):
        assert torch.equal(a, b), k
    if not train:
        m3 = _model(ld, "HEATNet4", 128, drop, train)
        free = _unpadded_twin(ld, m3, _adam(m3), SEQUENCE)
        print("captured", got, "unpadded", free)
        assert max(abs(a - b) for a, b in zip(got, free)) <= 1e-4, (got, free)


# ------------------------------------------------------------------------------------------------ 5. augmented slots
@pytest.mark.parametrize("which", ["emptying", "sparing"])
def test_captured_step_on_the_emptying_and_the_sparing_draw(which):
    """One replayed step over the three-node slide under the draw that empties its type 2 and under one that does not: bit-equal to the eager
    step on the slot's own graph under the same gates, and within the 1e-4 rule of an eager step on the unpadded augmented slide."""
    from wsi_hgnn_amd import graph as G
    from wsi_hgnn_amd.data import BatchSlot
    from wsi_hgnn_amd.trainer import CapturedSlotStep
    lf = torch.nn.CrossEntropyLoss()
    draw = M.found_draws()[0 if which == "emptying" else 1]
    idxs, warm = [M.THREE], [[0, 1]]
    ald = M.loader(_dev(), augment=True)                              # (fresh loaders: the warm-up draws follow the loaders' batch counters)
    m2 = _model(ald, "HEATNet4")
    o2 = _adam(m2)
    slot = BatchSlot(ald, M.BIG, type_mask=True)
    step = CapturedSlotStep(m2, o2, lf, slot, warmup=1, warmup_batches=warm)       # (the warm-up draws advance the loader's counter: the twin's too)
    slot.load(idxs, [draw])
    step.graphs[0].replay()
    loss, logits = step.outputs[0]
    want = 0.0 if which == "emptying" else 1.0
    assert slot.type_present.tolist() == [1.0, 1.0, want] and (slot.counts()[0][0][M.RARE] == 0) == (which == "emptying")

    ld2 = M.loader(_dev(), augment=True)
    m1 = _model(ald, "HEATNet4")
    o1 = _adam(m1)
    twin = BatchSlot(ld2, M.BIG, type_mask=True)
    for t, ps in enumerate(m1.type_gated_parameters()):
        o1.gate(ps, twin.type_present, t)
    for batch, draws in ((warm[0], None), (idxs, [draw])):
        twin.load(batch, draws)
        o1.zero_grad(set_to_none=True)
        l1 = lf(m1(twin.graph), twin.labels)
        l1.backward()
        o1.step()
    assert loss.item() == l1.item()
    for (k, a), (_, b) in zip(m1.state_dict().items(), m2.state_dict().items()):
        assert torch.equal(a, b), k
    steps = {float(o2.state[p]["step"]) for p in m2.type_gated_parameters()[M.RARE]}
    assert steps == ({1.0} if which == "emptying" else {2.0})

    m3 = _model(ald, "HEATNet4")
    unpadded = G.batch([g.to(_dev()) for g in M.unpadded_augmented(M.loader("cpu", augment=True), idxs, [draw])])
    y = torch.tensor([M.LABELS[i] for i in idxs], device=_dev())
    assert unpadded.num_nodes("2") == slot.counts()[0][0][M.RARE]
    slot.load(idxs, [draw])
    _close((which, draw), _run(m3, unpadded, y, 1), _run(m3, slot.graph, slot.labels, 1))


# ------------------------------------------------------------------------------------------------ 6. evaluation
@pytest.mark.parametrize("name", ["HEATNet4", "HGT"])
def test_captured_eval_of_batches_that_lack_a_type(ld, name):
    """CapturedSlotEval over ``type_mask`` slots: the logits of the type-less batches against the eval-mode forward io.evaluate runs on the
    loader's unpadded batches, within 1e-4; the epoch's loss against io.evaluate's over the same batches."""
    from wsi_hgnn_amd import io as wio
    from wsi_hgnn_amd.data import BatchSlot, GraphBatchLoader
    from wsi_hgnn_amd.trainer import CapturedSlotEval
    m = _model(ld, name)
    hgt = name == "HGT"
    ev = CapturedSlotEval(m, [BatchSlot(ld, M.BIG, per_relation_src=hgt, type_mask=True), BatchSlot(ld, M.SMALL, per_relation_src=hgt, type_mask=True)])
    assert all(s.type_present is ev.type_table for s in ev.slots)
    batches = [[0, 1], [M.TYPELESS, 6], [M.TYPELESS], [M.HUB, 5], [M.THREE]]
    with torch.no_grad():
        for idxs in batches:
            got = ev.run(idxs).clone()
            G, y, _ = ld._assemble(idxs, 0)
            with wio.eval_mode(m):
                want = m(G)
            assert (got - want).abs().max().item() <= 1e-4, (idxs, (got - want).abs().max().item())
    assert ev.replays == len(batches) and ev.eager_runs == 0
    batches = batches[:2] + batches[3:]                               # every slide once: the metrics hold one row per slide of the loader
    order = [i for b in batches for i in b]
    sub = GraphBatchLoader([M.slides()[i] for i in order], [M.LABELS[i] for i in order], 1, _dev(), shuffle=False, resident=True)
    res, ref = ev.evaluate(batches), wio.evaluate(m, sub)
    assert res["n"] == len(order) and abs(res["loss"] - ref["loss"]) <= 1e-4 and abs(res["accuracy"] - ref["accuracy"]) < 1e-6
