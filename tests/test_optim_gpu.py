"""The one-launch optimizers (wsi_hgnn_amd.optim.SGD / Adagrad / Adadelta / Adam, the count on the host or on the device;
csrc/optim.hip::optim_step_kernel) against the installed ``torch.optim`` classes on the same device in fp32.

Tolerance: the project's own from test_adam_step_matches_torch_adam - after every step ``|x - y|_max <= 2e-6 * max(1, |y|_max)`` on the parameters,
``1e-6`` relative (to the tensor's largest magnitude, floored at 1) on the state tensors at the end.  Both sides do the same handful of fp32
operations per element; they differ by where a product is fused into an add, i.e. by an ulp (6e-8 relative) per operation."""
import copy
import ctypes
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

SHAPES = [(512, 1024), (513,), (7, 3), (1,), (4096 * 3 + 5,), (64, 64)]
STEPS = 6


def _dev():
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def _inputs():
    """Start values and the gradients of every step, drawn once and never written: the shapes of the Adam test (odd sizes: the scalar tail; more than
    one workgroup; one element) plus a 70-element parameter that is a view 4 bytes into its buffer (no 16-byte lane accesses); gradients scaled
    10^(i - 2); parameter 2 has no gradient at odd steps (its own step count)."""
    gen = torch.Generator(device="cpu").manual_seed(9)
    start = [torch.randn(s, generator=gen).to(_dev()) for s in SHAPES] + [torch.randn(70, generator=gen).to(_dev())]
    grads = []
    for it in range(STEPS + 1):                                 # (one more: the continued run from the exchanged state)
        row = []
        for i, x in enumerate(start):
            if i == 2 and it % 2 == 1:
                row.append(None)
            else:
                row.append((torch.randn(x.shape, generator=gen) * (10.0 ** (i - 2) if i < len(SHAPES) else 1.0)).to(_dev()))
        grads.append(row)
    return start, grads


def _params():
    start, _ = _inputs()
    ps = [x.clone().requires_grad_() for x in start[:-1]]
    base = torch.zeros(71, device=_dev())
    base[1:].copy_(start[-1])
    view = base[1:].detach().requires_grad_()                   # a leaf that IS the view: data_ptr() % 16 == 4
    assert view.data_ptr() % 16 == 4 and view.is_leaf and view.is_contiguous()
    return ps + [view]


def _set_grads(ps, it):
    _, grads = _inputs()
    for p, g in zip(ps, grads[it]):
        p.grad = None if g is None else g.clone()


def _close(x, y, rel, what):
    err, bound = (x - y).abs().max().item(), rel * max(1.0, y.abs().max().item())
    assert err <= bound, (what, err, bound)
    return err


def _states_close(a, b, mine, ref):
    for p, q in zip(mine, ref):
        sa, sb = a.state.get(p, {}), b.state.get(q, {})
        assert sa.keys() == sb.keys()
        for f in sb:
            if f == "step":
                assert float(sa[f]) == float(sb[f]), f
            else:
                _close(sa[f], sb[f], 1e-6, f)


RULES = {
    "sgd": ("SGD", dict(lr=1e-2, weight_decay=5e-3)),
    "sgd-momentum": ("SGD", dict(lr=1e-2, weight_decay=5e-3, momentum=0.9)),
    "sgd-dampening": ("SGD", dict(lr=1e-2, weight_decay=5e-3, momentum=0.9, dampening=0.1)),
    "sgd-nesterov": ("SGD", dict(lr=1e-2, weight_decay=5e-3, momentum=0.9, nesterov=True)),
    "adagrad": ("Adagrad", dict(lr=1e-2, lr_decay=5e-3, weight_decay=5e-3)),
    "adagrad-initial": ("Adagrad", dict(lr=1e-2, lr_decay=5e-3, weight_decay=5e-3, initial_accumulator_value=0.1)),
    "adadelta-lr1": ("Adadelta", dict(lr=1.0, weight_decay=5e-3)),
    "adadelta": ("Adadelta", dict(lr=5e-3, weight_decay=5e-3)),
    "adam": ("Adam", dict(lr=1e-2, weight_decay=5e-3)),
}


@pytest.mark.parametrize("rule", sorted(RULES))
def test_rule_matches_torch_optim(rule):
    """6 steps of each rule against torch.optim's class of the same name; then the state_dicts change sides and one more step still agrees."""
    from wsi_hgnn_amd import optim as O
    name, kw = RULES[rule]
    mine, ref = _params(), _params()
    a, b = getattr(O, name)(mine, **kw), getattr(torch.optim, name)(ref, **kw)
    worst = 0.0
    for it in range(STEPS):
        _set_grads(mine, it)
        _set_grads(ref, it)
        a.step()
        b.step()
        for i, (x, y) in enumerate(zip(mine, ref)):
            worst = max(worst, _close(x, y, 2e-6, (rule, it, i)))
    print(f"{rule}: largest parameter difference to torch.optim.{name} over {STEPS} steps {worst:.3e}")
    _states_close(a, b, mine, ref)
    sa, sb = copy.deepcopy(a.state_dict()), copy.deepcopy(b.state_dict())
    assert sa["state"].keys() == sb["state"].keys()
    for k in sb["state"]:
        assert sa["state"][k].keys() == sb["state"][k].keys()
    # a checkpoint written by one is read by the other, which goes on from it
    mine2 = [x.detach().clone().requires_grad_() for x in mine]
    ref2 = [x.detach().clone().requires_grad_() for x in ref]
    a2, b2 = getattr(O, name)(mine2, **kw), getattr(torch.optim, name)(ref2, **kw)
    a2.load_state_dict(sb)
    b2.load_state_dict(sa)
    _set_grads(mine2, STEPS)
    _set_grads(ref2, STEPS)
    a2.step()
    b2.step()
    for i, (x, y) in enumerate(zip(mine2, ref2)):
        _close(x, y, 2e-6, (rule, "continued", i))
    _states_close(a2, b2, mine2, ref2)


@pytest.mark.parametrize("rule", ["sgd-momentum", "sgd", "adagrad", "adadelta-lr1", "adam"])
def test_more_tensors_than_the_table_holds_with_empty_ones_and_version_counters(rule):
    """300 tensors (the kernel's table holds 88: four launches) with zero-element tensors among them - the launch loop advances by what a table
    consumed - against torch.optim; every version counter of p and of every state tensor moves at every step."""
    from wsi_hgnn_amd import optim as O
    name, kw = RULES[rule] if rule != "adam" else ("Adam", dict(lr=1e-2, weight_decay=5e-3, capturable=True))
    gen = torch.Generator(device="cpu").manual_seed(4)
    sizes = [0 if i in (3, 17, 40, 130) else 5 + 7 * (i % 90) for i in range(300)]
    ps = [torch.randn(n, generator=gen).to(_dev()) for n in sizes]
    mine = [p.clone().requires_grad_() for p in ps]
    ref = [p.clone().requires_grad_() for p in ps]
    a, b = getattr(O, name)(mine, **kw), getattr(torch.optim, name)(ref, **kw)
    for it in range(3):
        for x, y in zip(mine, ref):
            g = torch.randn(x.shape, generator=gen).to(_dev())
            x.grad, y.grad = g.clone(), g.clone()
        states = [t for x in mine for t in a.state.get(x, {}).values() if torch.is_tensor(t)]        # (what exists: the first step creates most of it)
        assert it == 0 or rule == "sgd" or len(states) >= 300
        before = [t._version for t in mine + states]
        a.step()
        b.step()
        assert all(t._version > v for t, v in zip(mine + states, before)), it
        for i, (x, y) in enumerate(zip(mine, ref)):
            if x.numel():
                _close(x, y, 2e-6, (rule, it, i))
    if rule == "adam":
        assert all(float(a.state[x]["step"]) == 3.0 for x in mine)       # the empty ones too, as torch counts them
        assert int(a._wsi_tickets[_dev()].abs().sum()) == 0


@pytest.mark.parametrize("name,kw", [("Adam", dict(lr=1e-2, weight_decay=5e-3)), ("Adagrad", dict(lr=1e-2, lr_decay=5e-3, weight_decay=5e-3))])
def test_device_step_count_matches_the_host_count(name, kw):
    """capturable=True (state["step"] a 0-dim fp32 device word the kernel reads and advances) against capturable=False (a host count) of the same class:
    same tolerance as against torch; the word counts the steps each parameter took; the ticket words are zero after every step; a tensor of four
    workgroups and a tensor of one element both advance by exactly one per step."""
    from wsi_hgnn_amd import optim as O
    mine, ref = _params(), _params()
    a, b = getattr(O, name)(mine, capturable=True, **kw), getattr(O, name)(ref, capturable=False, **kw)
    assert a.param_groups[0]["capturable"] and not b.param_groups[0]["capturable"]
    identical = True
    taken = [0] * len(mine)
    for it in range(STEPS):
        _set_grads(mine, it)
        _set_grads(ref, it)
        a.step()
        b.step()
        for i, (x, y) in enumerate(zip(mine, ref)):
            taken[i] += x.grad is not None
            _close(x, y, 2e-6, (name, it, i))
            identical = identical and torch.equal(x, y)
            st = a.state[x]["step"]
            assert torch.is_tensor(st) and st.is_cuda and st.dtype == torch.float32 and st.dim() == 0
            assert float(st) == taken[i] == float(b.state[y]["step"]), (it, i)
        assert int(a._wsi_tickets[_dev()].abs().sum()) == 0, it
    assert taken[2] == STEPS // 2 and taken[4] == STEPS and mine[4].numel() > 3 * 4096 and mine[3].numel() == 1
    print(f"{name}: capturable=True and capturable=False bit-identical over {STEPS} steps: {identical}")
    _states_close(a, b, mine, ref)
    if name == "Adam":                                          # and against torch's own capturable Adam, whose state it can load
        c = torch.optim.Adam([x.detach().clone().requires_grad_() for x in mine], capturable=True, **kw)
        c.load_state_dict(copy.deepcopy(a.state_dict()))
        assert all(torch.is_tensor(s["step"]) and s["step"].is_cuda for s in c.state.values())


def test_adam_entry_point_is_the_shared_path():
    """lib.wsi_adam_step (the drop-in entry point; this test is its only Python caller) against optim.Adam(capturable=False) on clones: both run
    the same kernel instance with host-computed factors from the same doubles, so p, exp_avg and exp_avg_sq are EQUAL after every step.  Its own
    argument checks return WSI_EINVAL and leave every tensor as it was - a bad tensor 99 of 100 included (checked before the first launch)."""
    from wsi_hgnn_amd import optim as O, _native as N
    lib = N.load()
    kw = dict(lr=1e-2, betas=(0.9, 0.999), eps=1e-8, weight_decay=5e-3)
    ref = _params()
    b = O.Adam(ref, capturable=False, **kw)
    mine = _params()
    ms, vs = [torch.zeros_like(p) for p in mine], [torch.zeros_like(p) for p in mine]

    def call(arr, count, step=1, beta1=kw["betas"][0]):
        return lib.wsi_adam_step(ctypes.cast(arr, ctypes.c_void_p) if arr is not None else None, count, kw["lr"], beta1, kw["betas"][1],
                                 kw["eps"], kw["weight_decay"], step, N.stream())

    def table(idx):
        arr = (N.AdamTensor * len(idx))()
        for k, i in enumerate(idx):
            arr[k].p, arr[k].g, arr[k].m, arr[k].v, arr[k].n = mine[i].data_ptr(), mine[i].grad.data_ptr(), ms[i].data_ptr(), vs[i].data_ptr(), mine[i].numel()
        return arr

    taken = [0] * len(mine)
    for it in range(3):
        _set_grads(mine, it)
        _set_grads(ref, it)
        by_t = {}
        for i, p in enumerate(mine):
            if p.grad is not None:
                taken[i] += 1
                by_t.setdefault(taken[i], []).append(i)
        for t, idx in by_t.items():
            assert call(table(idx), len(idx), step=t) == N.WSI_OK
        b.step()
        for i, (x, y) in enumerate(zip(mine, ref)):
            assert torch.equal(x, y), (it, i)
            assert torch.equal(ms[i], b.state[y]["exp_avg"]) and torch.equal(vs[i], b.state[y]["exp_avg_sq"]), (it, i)
            assert b.state[y]["step"] == taken[i]
    # refused calls: WSI_EINVAL, nothing written
    _set_grads(mine, 0)
    idx = list(range(len(mine)))
    copies = [[t.detach().clone() for t in ts] for ts in (mine, ms, vs)]
    hundred = table([k % len(mine) for k in range(100)])       # (the same tensors over and over: more entries than the kernel's table of 88 holds)
    hundred[99].g, hundred[99].n = None, 5                     # a null gradient on a non-empty tensor, behind a full first table
    for rc in (call(table(idx), len(idx), step=0), call(table(idx), len(idx), beta1=1.0), call(None, 2), call(hundred, 100)):
        assert rc == N.WSI_EINVAL
    torch.cuda.synchronize()
    for ts, cs in zip((mine, ms, vs), copies):
        for i, (x, c) in enumerate(zip(ts, cs)):
            assert torch.equal(x, c), i


@pytest.mark.parametrize("which", ["adam", "sgd"])
def test_captured_step_replays_the_packages_own_optimizers(which, monkeypatch):
    """trainer.CapturedStep with optim.Adam(capturable=True) and with optim.SGD(momentum=0.9): the optimizer is ONE kernel node of the hipGraph;
    replays walk the eager trajectory of the same optimizer class bit for bit (the bound of test_captured_step_replays_the_eager_trajectory),
    and Adam's device step word counts warm-up steps plus replays."""
    import wsi_hgnn_amd as W
    from wsi_hgnn_amd import models, synthetic, graph as graph_mod, optim as O
    from wsi_hgnn_amd.trainer import CapturedStep
    monkeypatch.setattr(graph_mod, "HEAVY_DEGREE", 8)             # hub kernels (side stream fork / join) inside the capture
    nd = {"0": 0, "1": 1, "2": 2}
    G = W.batch([synthetic.hetero_graph(300 + 50 * i, 48, seed=70 + i, dst_mode="hub") for i in range(2)]).to(_dev())
    y = torch.tensor([1, 0], device=_dev())
    lf = torch.nn.CrossEntropyLoss()

    def make():
        torch.manual_seed(3)
        m = models.HEATNet2(48, 64, 2, 2, 4, nd, 0.0, "mean").to(_dev())
        if which == "adam":
            return m, O.Adam(m.parameters(), lr=1e-3, weight_decay=5e-3, capturable=True)
        return m, O.SGD(m.parameters(), lr=1e-2, weight_decay=5e-3, momentum=0.9)

    m1, o1 = make()
    eager = []
    for _ in range(8):
        o1.zero_grad(set_to_none=True)
        l = lf(m1(G), y)
        l.backward()
        o1.step()
        eager.append(l.item())
    m2, o2 = make()
    for _ in range(2):                                          # stepped eagerly before, as in the test this one follows
        o2.zero_grad(set_to_none=True)
        l = lf(m2(G), y)
        l.backward()
        o2.step()
    del l
    step = CapturedStep(m2, o2, lf, G, y, warmup=1)
    got = [step().item() for _ in range(5)]
    assert got == eager[3:], (got, eager[3:])
    for (k, a), (_, b) in zip(m1.state_dict().items(), m2.state_dict().items()):
        assert torch.equal(a, b), k
    if which == "adam":
        words = [float(s["step"]) for s in o2.state.values()]
        assert words and all(w == 2 + 1 + 5 for w in words), words          # 2 eager steps, 1 warm-up step, 5 replays
        assert int(o2._wsi_tickets[_dev()].abs().sum()) == 0
        with pytest.raises(RuntimeError, match="capturable"):
            CapturedStep(m2, O.Adam(m2.parameters(), lr=1e-3), lf, G, y)    # host-side step count: refused


def test_sgd_step_refreshes_the_packed_weights():
    """ops.repack_weights is wired behind SGD.step as behind Adam.step: under scaled-fp16 projections the step packs the updated weights (one launch
    per op), the next forward reads those planes (hits, no pack of its own), and gives the same bits as a forward that packs afresh."""
    from wsi_hgnn_amd import models, synthetic, ops, optim as O
    G, y = synthetic.hetero_batch(2, 600, 64, rank=0, dst_mode="uniform")
    G, y = G.to(_dev()), y.to(_dev())
    try:
        ops.set_gemm_precision("fp16x3")
        ops.invalidate_packed_weights()
        torch.manual_seed(611)
        m = models.HEATNet4(64, 128, 2, 2, 4, {"0": 0, "1": 1, "2": 2}, 0.0, "max").to(_dev())
        opt = O.SGD(m.parameters(), lr=1e-2, momentum=0.9)
        for _ in range(2):
            opt.zero_grad(set_to_none=True)
            torch.nn.functional.cross_entropy(m(G), y).backward()
            packs = ops._PACKED["packs"]
            opt.step()
            behind = ops._PACKED["packs"] - packs
        assert behind >= 1                                       # the step packed
        hits, packs = ops._PACKED["hits"], ops._PACKED["packs"]
        with_cache = m(G).detach().clone()
        assert ops._PACKED["hits"] > hits and ops._PACKED["packs"] == packs      # the forward read what the step packed
        ops.invalidate_packed_weights()
        afresh = m(G).detach()
        assert torch.equal(with_cache, afresh)
    finally:
        ops.invalidate_packed_weights()
        ops.set_gemm_precision("fp32")
