"""CPU-side checks of the learning rate as a device word: ``wsi_optim_step_lr`` is declared and exported and its argument
checks return before any HIP call (a fake device address is never touched), the constructors' refusals, ``optim.lr_word``,
``parser.parse_optimizer(..., device_lr=True)`` on the reference's recorded branches, and ``load_state_dict`` both ways on CPU tensors."""
import copy
import ctypes
import json
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -22
P = 1 << 40                 # a fake device address, 8-byte aligned: every call below returns before touching it


def _lib():
    import __graft_entry__
    __graft_entry__.build()
    from wsi_hgnn_amd import _native
    return _native.load(), _native


def _hyper(N, **kw):
    h = N.OptimHyper(lr=1e-2, weight_decay=0.0, momentum=0.0, dampening=0.0, nesterov=0.0, lr_decay=0.0, eps=1e-8, rho=0.9,
                     beta1=0.9, beta2=0.999, host_step=1.0)
    for k, v in kw.items():
        setattr(h, k, v)
    return h


def _table(N, n_tensors=1, **kw):
    arr = (N.OptimTensor * n_tensors)()
    for a in arr:
        a.p, a.g, a.s0, a.s1, a.step, a.ticket, a.n, a.flags = P, P, P, P, P, P, 100, 0
        for k, v in kw.items():
            setattr(a, k, v)
    return arr


def _call(lib, rule, arr, count, h, word, gidx=None, gtable=None, glen=0):
    return lib.wsi_optim_step_lr(rule, ctypes.cast(arr, ctypes.c_void_p) if arr is not None else None, count, ctypes.addressof(h),
                                 ctypes.cast(gidx, ctypes.c_void_p) if gidx is not None else None, gtable, glen, word, None)


def test_the_symbol_is_declared_and_exported():
    lib, N = _lib()
    header = open(os.path.join(ROOT, "include", "wsi_hgnn.h")).read()
    assert re.search(r"\bint\s+wsi_optim_step_lr\s*\(", header)
    res, args = N.EXPORTS["wsi_optim_step_lr"]
    assert res is ctypes.c_int and len(args) == 9 and args[0] is ctypes.c_int32 and args[6] is ctypes.c_int32 and args[7] is ctypes.c_void_p
    assert lib.wsi_optim_step_lr is not None                       # (bound by load(); a missing symbol raises there)
    assert "wsi_optim_step_gated" in N.EXPORTS and "wsi_optim_step" in N.EXPORTS and N.WSI_ABI_VERSION == 26


def test_argument_checks_of_the_entry_point():
    lib, N = _lib()
    err = lambda: lib.wsi_last_error().decode()
    h = _hyper(N)
    for rule in (N.WSI_OPTIM_SGD, N.WSI_OPTIM_ADAGRAD, N.WSI_OPTIM_ADADELTA, N.WSI_OPTIM_ADAM):
        for off in (1, 2, 4, 7):                                   # the word is one double: 8-byte aligned
            assert _call(lib, rule, _table(N), 1, h, P + off) == EINVAL and "aligned" in err(), (rule, off)
    # a rule that reads the count takes a word with a step word per tensor only: the host, which takes a host count's factors, cannot read it
    for rule in (N.WSI_OPTIM_ADAGRAD, N.WSI_OPTIM_ADAM):
        assert _call(lib, rule, _table(N, step=None, ticket=None), 1, h, P) == EINVAL and "no step word" in err()
        arr = _table(N, 3)
        arr[2].step = None
        assert _call(lib, rule, arr, 3, h, P) == EINVAL and "tensor 2" in err()
    # the gate arguments are checked as wsi_optim_step_gated checks them
    one, two = (ctypes.c_int32 * 1)(2), (ctypes.c_int32 * 1)(-1)
    for word in (None, P):
        assert _call(lib, N.WSI_OPTIM_SGD, _table(N), 1, h, word, one, P, 1) == EINVAL and "gate index" in err()
        assert _call(lib, N.WSI_OPTIM_SGD, _table(N), 1, h, word, two, P, 1) == EINVAL and "gate index" in err()
        assert _call(lib, N.WSI_OPTIM_SGD, _table(N), 1, h, word, (ctypes.c_int32 * 1)(1), None, 1) == EINVAL and "null gate table" in err()
        assert _call(lib, N.WSI_OPTIM_SGD, _table(N), 1, h, word, None, None, 256) == EINVAL and "gate_len" in err()
        assert lib.wsi_optim_step_gated(N.WSI_OPTIM_SGD, ctypes.cast(_table(N), ctypes.c_void_p), 1, ctypes.addressof(h),
                                        ctypes.cast(one, ctypes.c_void_p), P, 1, None) == EINVAL and "gate index" in err()
    # what wsi_optim_step refuses stays refused
    assert _call(lib, 4, _table(N), 1, h, P) == EINVAL and "unknown rule" in err()
    assert _call(lib, N.WSI_OPTIM_ADAM, _table(N, s1=None), 1, h, P) == EINVAL and "null pointer" in err()
    assert _call(lib, N.WSI_OPTIM_SGD, _table(N), 1, _hyper(N, weight_decay=-1.0), P) == EINVAL and "hyper-parameter" in err()


@pytest.mark.parametrize("bad", [float("nan"), float("inf"), -1.0])
def test_hyper_lr_is_ignored_beside_a_word_and_checked_without_one(bad):
    lib, N = _lib()
    h = _hyper(N, lr=bad)
    for rule in (N.WSI_OPTIM_SGD, N.WSI_OPTIM_ADAGRAD, N.WSI_OPTIM_ADADELTA, N.WSI_OPTIM_ADAM):
        assert _call(lib, rule, None, 0, h, None) == EINVAL and "hyper-parameter" in lib.wsi_last_error().decode()
        assert _call(lib, rule, None, 0, h, P) == 0                # accepted: the checks pass and there is nothing to launch
        empty = _table(N, 3, n=0, p=None, g=None, s0=None, s1=None)
        assert _call(lib, rule, empty, 3, h, P) == 0               # zero-element tensors only: no launch, no HIP call


def test_count_zero_is_ok():
    lib, N = _lib()
    h = _hyper(N)
    for word in (None, P):
        assert _call(lib, N.WSI_OPTIM_ADAM, None, 0, h, word) == 0
        assert _call(lib, N.WSI_OPTIM_SGD, _table(N), 0, h, word) == 0


def test_lr_word_and_constructor_refusals():
    from wsi_hgnn_amd import optim as O
    w = O.lr_word(3e-4)
    assert isinstance(w, torch.Tensor) and w.dtype == torch.float64 and w.numel() == 1 and w.device.type == "cpu"
    assert w.item() == 3e-4                                        # a Python float is held exactly
    assert O.lr_word(1, "cpu").item() == 1.0
    p = lambda: [torch.zeros(3, requires_grad=True)]
    for cls, kw in ((O.SGD, {}), (O.Adagrad, dict(capturable=True)), (O.Adadelta, {}), (O.Adam, dict(capturable=True))):
        opt = cls(p(), lr=w, **kw)
        assert all(g["lr"] is w for g in opt.param_groups)         # the very tensor: a scheduler's fill_ is what the launch reads
        with pytest.raises(ValueError, match="lr_word"):
            cls(p(), lr=torch.tensor(1e-3), **kw)                  # float32
        with pytest.raises(ValueError, match="lr_word"):
            cls(p(), lr=torch.tensor([1e-3, 1e-3], dtype=torch.float64), **kw)
        with pytest.raises(ValueError, match="lr_word"):
            cls(p(), lr=torch.tensor(1, dtype=torch.int64), **kw)
        cls(p(), lr=torch.full((1, 1), -1.0, dtype=torch.float64), **kw)       # one element of any shape; its VALUE is never read back
    for cls in (O.Adam, O.Adagrad):
        with pytest.raises(ValueError, match="capturable=True"):
            cls(p(), lr=w)
        with pytest.raises(ValueError, match="capturable=True"):
            cls(p(), lr=w, capturable=False)
        with pytest.raises(ValueError, match="invalid hyper-parameter"):
            cls(p(), lr=-1.0)                                      # a float is checked as ever


def test_the_word_must_live_with_the_parameters():
    """Checked where the parameters' device is known: require_capturable before a capture (the first step's own check needs a GPU)."""
    from wsi_hgnn_amd import capture, optim as O
    opt = O.Adam([torch.zeros(3, requires_grad=True)], lr=O.lr_word(1e-3), capturable=True)
    capture.require_capturable("test", opt)
    opt.param_groups[0]["lr"] = torch.tensor(1e-3)                 # rebound to a float32 tensor since
    with pytest.raises(RuntimeError, match="lr_word"):
        capture.require_capturable("test", opt)
    opt.param_groups[0]["lr"] = O.lr_word(1e-3, "meta")
    with pytest.raises(RuntimeError, match="lr_word"):
        capture.require_capturable("test", opt)
    # torch.optim's own: a tensor lr as torch accepts it
    capture.require_capturable("test", torch.optim.Adam([torch.zeros(3, requires_grad=True)], lr=torch.tensor(1e-3), capturable=True))
    with pytest.raises(RuntimeError, match="capturable"):
        capture.require_capturable("test", O.Adam([torch.zeros(3, requires_grad=True)], lr=1e-3))


_SURFACE = json.load(open(os.path.join(ROOT, "tests", "golden", "reference_surface.json")))


@pytest.mark.parametrize("rec", _SURFACE["parse_optimizer"], ids=lambda r: r["opt_method"])
def test_parse_optimizer_device_lr(rec):
    from wsi_hgnn_amd import optim as O
    from wsi_hgnn_amd.parser import parse_optimizer
    model = torch.nn.Linear(4, 3)
    cfg = {"opt_method": rec["opt_method"], "lr": rec["lr"], "weight_decay": rec["weight_decay"]}
    opt = parse_optimizer(cfg, model, native=True, device_lr=True)
    assert type(opt) is getattr(O, rec["class"])
    assert [id(p) for p in opt.param_groups[0]["params"]] == [id(p) for p in model.parameters()]
    lr = opt.param_groups[0]["lr"]
    assert isinstance(lr, torch.Tensor) and lr.dtype == torch.float64 and lr.numel() == 1 and lr.device == model.weight.device
    assert lr.item() == rec["defaults"]["lr"] == rec["lr"]
    assert opt.param_groups[0]["capturable"] is True               # Adam and Adagrad: built capturable; SGD and Adadelta always are
    for k in ("weight_decay", "lr_decay", "eps", "rho", "momentum", "dampening", "nesterov", "initial_accumulator_value"):
        if k in rec["defaults"]:
            assert opt.defaults[k] == rec["defaults"][k], k
    if "betas" in rec["defaults"]:
        assert list(opt.defaults["betas"]) == rec["defaults"]["betas"]
    with pytest.raises(ValueError, match="native=True"):
        parse_optimizer(cfg, model, device_lr=True)
    with pytest.raises(ValueError, match="native=True"):
        parse_optimizer(cfg, model, native=False, device_lr=True)
    # the defaults build exactly what they built
    plain = parse_optimizer(cfg, model, native=True)
    assert type(plain) is type(opt) and plain.param_groups[0]["lr"] == rec["lr"] and isinstance(plain.param_groups[0]["lr"], float)
    assert plain.param_groups[0]["capturable"] is (rec["class"] in ("SGD", "Adadelta"))
    assert type(parse_optimizer(cfg, model)) is getattr(torch.optim, rec["class"])


def _with_state(cls, kw, lr):
    torch.manual_seed(1)
    ps = [torch.randn(5, 3, requires_grad=True), torch.randn(7, requires_grad=True)]
    opt = cls(ps, lr=lr, **kw)
    group = opt.param_groups[0]
    for p in ps:
        if opt._state_keys(group):
            opt._ensure_state(p, group, opt.state[p])
            for k in opt._state_keys(group):
                if k != "step":
                    opt.state[p][k].normal_()
    return ps, opt


@pytest.mark.parametrize("name,kw", [("SGD", dict(momentum=0.9)), ("Adagrad", dict(capturable=True)), ("Adadelta", {}), ("Adam", dict(capturable=True))])
def test_load_state_dict_keeps_the_word_and_a_float_stays_a_float(name, kw):
    from wsi_hgnn_amd import optim as O
    cls = getattr(O, name)
    word = O.lr_word(1e-2)
    _, a = _with_state(cls, kw, word)
    _, b = _with_state(cls, kw, 3e-3)                              # a float optimizer
    _, c = _with_state(cls, kw, O.lr_word(7e-4))                   # another word optimizer
    sched = torch.optim.lr_scheduler.CosineAnnealingLR(c, T_max=4, eta_min=5e-6)        # adds initial_lr: a tensor of its own
    assert isinstance(c.param_groups[0]["initial_lr"], torch.Tensor) and c.param_groups[0]["initial_lr"] is not c.param_groups[0]["lr"]
    ptr, states = word.data_ptr(), [v for p in a.param_groups[0]["params"] for v in a.state[p].values() if isinstance(v, torch.Tensor)]
    # a float checkpoint into the word optimizer
    a.load_state_dict(copy.deepcopy(b.state_dict()))
    assert a.param_groups[0]["lr"] is word and word.data_ptr() == ptr and word.item() == 3e-3
    assert a.param_groups[0]["capturable"] is True
    # a tensor checkpoint (torch saves a tensor lr as a tensor) into the word optimizer, initial_lr with it
    sd = copy.deepcopy(c.state_dict())
    assert isinstance(sd["param_groups"][0]["lr"], torch.Tensor)   # state_dict() stays torch's layout
    a.load_state_dict(sd)
    g = a.param_groups[0]
    assert g["lr"] is word and word.data_ptr() == ptr and word.item() == 7e-4
    assert isinstance(g["initial_lr"], torch.Tensor) and g["initial_lr"].dtype == torch.float64 and g["initial_lr"].item() == 7e-4
    assert g["initial_lr"] is not word and g["initial_lr"].data_ptr() != ptr and g["initial_lr"] is not sd["param_groups"][0]["initial_lr"]
    kept = g["initial_lr"]
    a.load_state_dict(copy.deepcopy(b.state_dict()))              # (no initial_lr in this checkpoint: the scheduler's tensor stays)
    assert a.param_groups[0]["initial_lr"] is kept and word.item() == 3e-3
    # the state tensors this object steps are kept too and hold the loaded values (a recorded step reads and writes them)
    for (pa, pc) in zip(a.param_groups[0]["params"], c.param_groups[0]["params"]):
        a.load_state_dict(copy.deepcopy(c.state_dict()))
        for k, v in c.state[pc].items():
            assert torch.equal(torch.as_tensor(a.state[pa][k]), torch.as_tensor(v)), k
    assert all(any(v is w for w in states) for p in a.param_groups[0]["params"] for v in a.state[p].values() if isinstance(v, torch.Tensor))
    # a tensor checkpoint into the float optimizer: a float, initial_lr too
    b.load_state_dict(copy.deepcopy(c.state_dict()))
    g = b.param_groups[0]
    assert type(g["lr"]) is float and g["lr"] == 7e-4 and type(g["initial_lr"]) is float and g["initial_lr"] == 7e-4
    # torch's own optimizer reads a word checkpoint back (CPU: not capturable there)
    if name != "SGD":
        sd = copy.deepcopy(a.state_dict())
        sd["param_groups"][0]["capturable"] = False
        t = getattr(torch.optim, name)([torch.zeros(5, 3, requires_grad=True), torch.zeros(7, requires_grad=True)])
        t.load_state_dict(sd)
        assert float(t.param_groups[0]["lr"]) == float(word)
    del sched
