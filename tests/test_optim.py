"""CPU-side checks of the one-launch optimizers (wsi_hgnn_amd.optim: SGD, Adagrad, Adadelta, Adam with a device count): the argument checks of
``wsi_optim_step`` (every one before the first HIP call: no GPU needed), ``parser.parse_optimizer(..., native=True)`` against the calls the
reference makes (tests/golden/reference_surface.json), the refusals, and the ``state_dict`` layout against ``torch.optim``'s."""
import copy
import ctypes
import json
import os

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -22
# a fake device address: every call below must fail its argument check before touching it
P = 1 << 40


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


def _call(lib, rule, arr, count, h):
    return lib.wsi_optim_step(rule, ctypes.cast(arr, ctypes.c_void_p) if arr is not None else None, count,
                              ctypes.addressof(h) if h is not None else None, None)


def test_optim_step_rejects_bad_rule_table_and_sizes():
    lib, N = _lib()
    err = lambda: lib.wsi_last_error().decode()
    h = _hyper(N)
    assert _call(lib, 4, _table(N), 1, h) == EINVAL and "unknown rule" in err()
    assert _call(lib, -1, _table(N), 1, h) == EINVAL and "unknown rule" in err()
    assert _call(lib, N.WSI_OPTIM_SGD, None, 1, h) == EINVAL and "null tensor table" in err()
    assert _call(lib, N.WSI_OPTIM_SGD, _table(N), -1, h) == EINVAL and "negative" in err()
    assert _call(lib, N.WSI_OPTIM_SGD, _table(N), 1, None) == EINVAL and "hyper" in err()
    assert _call(lib, N.WSI_OPTIM_SGD, _table(N, n=-5), 1, h) == EINVAL and "negative size" in err()
    # a bad tensor anywhere in the table fails the call before the first launch (tensor 199 lies behind two full tables)
    arr = _table(N, 200)
    arr[199].p = None
    assert _call(lib, N.WSI_OPTIM_SGD, arr, 200, h) == EINVAL and "tensor 199" in err()
    # nothing to do: no tensors, or only zero-element ones (which need no pointers)
    assert _call(lib, N.WSI_OPTIM_SGD, None, 0, h) == 0
    assert _call(lib, N.WSI_OPTIM_ADAM, _table(N, 3, n=0, p=None, g=None, s0=None, s1=None, step=None, ticket=None), 3, h) == 0


@pytest.mark.parametrize("rule,needs", [("SGD", ()), ("SGD_MOMENTUM", ("s0",)), ("ADAGRAD", ("s0",)), ("ADADELTA", ("s0", "s1")), ("ADAM", ("s0", "s1"))])
def test_optim_step_rejects_null_pointers_the_rule_needs(rule, needs):
    lib, N = _lib()
    err = lambda: lib.wsi_last_error().decode()
    h = _hyper(N, momentum=0.9 if rule == "SGD_MOMENTUM" else 0.0)
    code = getattr(N, "WSI_OPTIM_" + rule.replace("_MOMENTUM", ""))
    for f in ("p", "g") + needs:
        assert _call(lib, code, _table(N, **{f: None}), 1, h) == EINVAL and "null pointer" in err(), f
    assert _call(lib, code, _table(N, ticket=None), 1, h) == EINVAL and "without a ticket" in err()
    if rule in ("ADAGRAD", "ADAM"):                # the rules that read the count: no device word and no host count
        assert _call(lib, code, _table(N, step=None, ticket=None), 1, _hyper(N, host_step=0.0)) == EINVAL and "host_step" in err()


@pytest.mark.parametrize("rule,bad", [
    ("SGD", dict(lr=-1.0)), ("SGD", dict(weight_decay=-1e-3)), ("SGD", dict(momentum=-0.1)), ("SGD", dict(lr=float("nan"))),
    ("SGD", dict(nesterov=1.0)), ("SGD", dict(nesterov=1.0, momentum=0.9, dampening=0.1)), ("SGD", dict(nesterov=0.5, momentum=0.9)),
    ("ADAGRAD", dict(lr_decay=-1.0)), ("ADAGRAD", dict(eps=-1.0)), ("ADAGRAD", dict(lr=float("inf"))),
    ("ADADELTA", dict(rho=1.5)), ("ADADELTA", dict(rho=-0.1)), ("ADADELTA", dict(eps=-1e-6)), ("ADADELTA", dict(rho=float("nan"))),
    ("ADAM", dict(beta1=1.0)), ("ADAM", dict(beta2=-0.1)), ("ADAM", dict(beta2=1.0)), ("ADAM", dict(eps=-1.0)), ("ADAM", dict(weight_decay=-1.0)),
])
def test_optim_step_rejects_hyper_parameters_out_of_range(rule, bad):
    lib, N = _lib()
    assert _call(lib, getattr(N, "WSI_OPTIM_" + rule), _table(N), 1, _hyper(N, **bad)) == EINVAL
    assert "hyper-parameter" in lib.wsi_last_error().decode()


_SURFACE = json.load(open(os.path.join(ROOT, "tests", "golden", "reference_surface.json")))


@pytest.mark.parametrize("rec", _SURFACE["parse_optimizer"], ids=lambda r: r["opt_method"])
def test_parse_optimizer_native_builds_the_packages_classes(rec):
    """The calls the reference's parse_optimizer makes on its own branches (recorded in the golden surface): ``native=True`` builds the package's
    class of the same name with the recorded lr / weight_decay / lr_decay; the default still builds torch.optim's."""
    from wsi_hgnn_amd import optim as O
    from wsi_hgnn_amd.parser import parse_optimizer
    model = torch.nn.Linear(4, 3)
    cfg = {"opt_method": rec["opt_method"], "lr": rec["lr"], "weight_decay": rec["weight_decay"]}
    opt = parse_optimizer(cfg, model, native=True)
    assert type(opt) is getattr(O, rec["class"])
    assert [id(p) for p in opt.param_groups[0]["params"]] == [id(p) for p in model.parameters()]
    for k in ("lr", "weight_decay", "lr_decay", "eps", "rho", "momentum", "dampening", "nesterov", "initial_accumulator_value"):
        if k in rec["defaults"]:
            assert opt.defaults[k] == rec["defaults"][k], k
    if "betas" in rec["defaults"]:
        assert list(opt.defaults["betas"]) == rec["defaults"]["betas"]
    ref = parse_optimizer(cfg, model)
    assert type(ref) is getattr(torch.optim, rec["class"]) and type(parse_optimizer(cfg, model, native=False)) is type(ref)


def _all(params, **kw):
    from wsi_hgnn_amd import optim as O
    return [(O.SGD, torch.optim.SGD, dict(lr=1e-2, momentum=0.9)), (O.SGD, torch.optim.SGD, dict(lr=1e-2)),
            (O.Adagrad, torch.optim.Adagrad, dict(lr=1e-2, lr_decay=5e-3, initial_accumulator_value=0.1)),
            (O.Adadelta, torch.optim.Adadelta, dict()), (O.Adam, torch.optim.Adam, dict(lr=1e-2))]


def test_constructor_arguments_and_defaults_match_torch():
    import inspect
    from wsi_hgnn_amd import optim as O
    for name, args in (("SGD", ("lr", "momentum", "dampening", "weight_decay", "nesterov")),
                       ("Adagrad", ("lr", "lr_decay", "weight_decay", "initial_accumulator_value", "eps")),
                       ("Adadelta", ("lr", "rho", "eps", "weight_decay")), ("Adam", ("lr", "betas", "eps", "weight_decay"))):
        ours = inspect.signature(getattr(O, name).__init__).parameters
        theirs = inspect.signature(getattr(torch.optim, name).__init__).parameters
        assert [k for k in ours if k in args] == [k for k in theirs if k in args], name         # same order
        for a in args:
            assert ours[a].default == theirs[a].default and ours[a].kind == theirs[a].kind, (name, a)
    assert inspect.signature(O.Adam.__init__).parameters["capturable"].default is False
    assert inspect.signature(O.Adagrad.__init__).parameters["capturable"].default is False


def test_refusals():
    from wsi_hgnn_amd import optim as O
    for cls in (O.SGD, O.Adagrad, O.Adadelta, O.Adam):
        cpu_p = torch.zeros(3, requires_grad=True)
        cpu_p.grad = torch.ones(3)
        with pytest.raises(RuntimeError, match="GPU only"):
            cls([cpu_p]).step()                                      # no CPU path
        for kw in ("maximize", "foreach", "differentiable"):
            with pytest.raises(ValueError, match=kw):
                cls([cpu_p], **{kw: True})
    for cls in (O.SGD, O.Adagrad, O.Adam):
        with pytest.raises(ValueError, match="fused"):
            cls([torch.zeros(3, requires_grad=True)], fused=True)
    with pytest.raises(ValueError, match="amsgrad"):
        O.Adam([torch.zeros(3, requires_grad=True)], amsgrad=True)
    with pytest.raises(ValueError):
        O.SGD([torch.zeros(3, requires_grad=True)], nesterov=True)   # torch's rule: needs momentum and zero dampening
    with pytest.raises(ValueError):
        O.Adagrad([torch.zeros(3, requires_grad=True)], lr=-1.0)
    for cls in (O.SGD, O.Adadelta):                                  # no count is read: CapturedStep takes them as they are
        assert all(g["capturable"] for g in cls([torch.zeros(3, requires_grad=True)]).param_groups)
    assert not O.Adam([torch.zeros(3, requires_grad=True)]).param_groups[0]["capturable"]
    assert O.Adam([torch.zeros(3, requires_grad=True)], capturable=True).param_groups[0]["capturable"]


@pytest.mark.parametrize("which,capturable", [(0, None), (1, None), (2, False), (2, True), (3, None), (4, False), (4, True)])
def test_state_dict_layout_is_torchs_and_loads_both_ways(which, capturable):
    """State created by the package's own initialiser has torch's keys; a state_dict of either loads into the other.  (torch steps on the CPU here;
    ours cannot, its state is created by the code path step() uses.)"""
    torch.manual_seed(0)
    ps = [torch.randn(5, 3, requires_grad=True), torch.randn(7, requires_grad=True)]
    qs = [p.detach().clone().requires_grad_() for p in ps]
    ours_cls, torch_cls, kw = _all(ps)[which]
    a = ours_cls(ps, **kw) if capturable is None else ours_cls(ps, capturable=capturable, **kw)      # (SGD and Adadelta have one form)
    b = torch_cls(qs, **kw)
    for q in qs:
        q.grad = torch.randn_like(q)
    b.step()
    b.step()
    group = a.param_groups[0]
    for p in ps:
        if a._state_keys(group):
            a._ensure_state(p, group, a.state[p])
    sa, sb = a.state_dict(), copy.deepcopy(b.state_dict())       # (a checkpoint: its tensors are nobody's live state)
    assert sa["state"].keys() == sb["state"].keys()
    for k in sb["state"]:
        assert sa["state"][k].keys() == sb["state"][k].keys(), k
        for f, v in sb["state"][k].items():
            if f != "step" and v is not None:
                assert sa["state"][k][f].shape == v.shape and sa["state"][k][f].dtype == v.dtype
    if ours_cls.__name__ == "Adagrad":
        assert all(float(s["sum"].min()) == float(s["sum"].max()) == pytest.approx(0.1) for s in sa["state"].values())
    if "step" in a._state_keys(group):
        steps = [s["step"] for s in a.state.values()]
        assert all((torch.is_tensor(s) and s.dtype == torch.float32 and s.dim() == 0) if group["capturable"] else s == 0 for s in steps)
    # torch's checkpoint into ours: the tensors arrive, the count in THIS object's form, the object's capturable choice survives
    a.load_state_dict(sb)
    assert a.param_groups[0]["capturable"] == group["capturable"]
    for p, q in zip(ps, qs):
        for f, v in b.state[q].items():
            if f == "step":
                assert float(a.state[p]["step"]) == 2.0
                assert torch.is_tensor(a.state[p]["step"]) == bool(group["capturable"])
            else:
                assert (a.state[p][f] is None and v is None) or torch.equal(a.state[p][f], v)
    # ... and ours into torch's, which then steps on from it exactly as the optimizer that wrote the checkpoint
    qs2 = [q.detach().clone().requires_grad_() for q in qs]
    for q, q2 in zip(qs, qs2):
        q2.grad = q.grad.clone()
    b2 = torch_cls(qs2, **kw)
    sd = copy.deepcopy(a.state_dict())
    sd["param_groups"][0]["capturable"] = False                    # (on the CPU, where this test runs, torch has no capturable form)
    b2.load_state_dict(sd)
    b2.step()
    b.step()
    for q, q2 in zip(qs, qs2):
        assert torch.equal(q, q2)
        for f, v in b.state[q].items():
            assert (v is None and b2.state[q2][f] is None) or float((b2.state[q2][f].cpu() - v).abs().max()) == 0.0, f
    assert a.state_dict()["param_groups"][0].keys() >= sb["param_groups"][0].keys()          # torch's group keys, so torch reads them back
    assert not any(k.startswith("_wsi") for k in a.state_dict()["param_groups"][0])
