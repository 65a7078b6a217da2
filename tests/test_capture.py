"""The host-side pieces of the capture protocol (wsi_hgnn_amd.capture): the optimizer and dropout checks, slot selection and the evaluation
context.  Nothing here touches a GPU; what the captured classes record and replay is held by their own GPU suites."""
import pytest
import torch
from torch import nn

from wsi_hgnn_amd import capture, optim as O


def _params():
    return [nn.Parameter(torch.zeros(3)), nn.Parameter(torch.zeros(2, 2))]


def test_require_capturable_refuses_a_host_step_count():
    with pytest.raises(RuntimeError, match="^Who: the optimizer must be capturable.*its step count has to live on the device"):
        capture.require_capturable("Who", torch.optim.SGD(_params(), lr=0.1))
    a, b = _params()
    mixed = torch.optim.Adam([{"params": [a], "capturable": True}, {"params": [b]}], lr=0.1)
    assert [g["capturable"] for g in mixed.param_groups] == [True, False]
    with pytest.raises(RuntimeError, match="capturable"):
        capture.require_capturable("Who", mixed)
    with pytest.raises(RuntimeError, match="capturable"):
        capture.require_capturable("Who", O.Adam(_params(), lr=0.1))


@pytest.mark.parametrize("make", [lambda p: O.SGD(p, lr=0.1, momentum=0.9), lambda p: O.Adadelta(p), lambda p: O.Adam(p, lr=0.1, capturable=True),
                                  lambda p: torch.optim.Adam(p, lr=0.1, capturable=True)], ids=["SGD", "Adadelta", "Adam", "torch.Adam"])
def test_require_capturable_accepts_a_device_step_count(make):
    assert capture.require_capturable("Who", make(_params())) is None


class _Counter(nn.Module):
    """Stands for a layer whose dropout is drawn counter-based (HEATLayer, HGTLayer)."""

    def __init__(self, p, counter_dropout=None):
        super().__init__()
        self.drop = nn.Dropout(p)
        if counter_dropout is not None:
            self.counter_dropout = counter_dropout


def test_dropout_check_refuses_a_host_generator_draw():
    model = nn.Sequential(nn.Linear(4, 4), nn.Dropout(0.2))
    with pytest.raises(RuntimeError, match="^Who: the model holds a torch.nn.Dropout with p > 0 in train mode"):
        capture.counter_dropout_only("Who", model)
    assert model.training                                      # (the check changes nothing)
    assert capture.counter_dropout_only("Who", model.eval()) is False
    assert capture.counter_dropout_only("Who", nn.Sequential(nn.Linear(4, 4), nn.Dropout(0.0))) is False
    assert capture.counter_dropout_only("Who", nn.Linear(4, 4), (_Counter,)) is False


def test_dropout_check_reports_that_a_seed_word_is_needed():
    model = nn.Sequential(_Counter(0.2), nn.Linear(4, 4), _Counter(0.5, counter_dropout=True))
    assert capture.counter_dropout_only("Who", model, (_Counter,)) is True
    assert capture.counter_dropout_only("Who", model, (nn.Linear, _Counter)) is True
    assert capture.counter_dropout_only("Who", model.eval(), (_Counter,)) is False
    # a layer of a declared type that draws from the host generator after all, and an owner of no declared type
    for bad in (nn.Sequential(_Counter(0.2), _Counter(0.2, counter_dropout=False)), nn.Sequential(_Counter(0.2), nn.Dropout(0.1))):
        with pytest.raises(RuntimeError, match="^Who: the model draws dropout masks outside the HEAT layers' counter-based draw"):
            capture.counter_dropout_only("Who", bad, (_Counter,))
    with pytest.raises(RuntimeError, match="Dropout"):
        capture.counter_dropout_only("Who", model.train())      # no type declared: refused as any other dropout


def test_new_seed_word_is_one_int32_word():
    torch.manual_seed(0)
    a, b = capture.new_seed_word("cpu"), capture.new_seed_word("cpu")
    assert a.dtype == torch.int32 and tuple(a.shape) == (1,) and int(a) != int(b)


def test_trainable_params_releases_gradients_and_skips_frozen_parameters():
    a, b = _params()
    c = nn.Parameter(torch.zeros(1), requires_grad=False)
    a.grad = torch.ones_like(a)
    opt = torch.optim.SGD([{"params": [a, c]}, {"params": [b]}], lr=0.1)
    got = capture.trainable_params(opt)
    assert len(got) == 2 and got[0] is a and got[1] is b and a.grad is None


def test_grad_step_is_backward_then_step():
    def run(step):
        torch.manual_seed(1)
        lin, unused = nn.Linear(3, 2), nn.Parameter(torch.ones(2))
        opt = torch.optim.SGD(list(lin.parameters()) + [unused], lr=0.5, momentum=0.9)
        x = torch.arange(6.0).reshape(2, 3)
        return [step(opt, lin, x) for _ in range(3)], [p.detach().clone() for p in lin.parameters()], unused

    def plain(opt, lin, x):
        opt.zero_grad(set_to_none=True)
        y = lin(x)
        loss = y.square().mean()
        loss.backward()
        opt.step()
        return loss.detach(), y.detach()

    def shared(opt, lin, x):
        def compute():
            y = lin(x)
            return y.square().mean(), y
        out = capture.grad_step(opt, capture.trainable_params(opt), compute)
        assert isinstance(out, tuple) and not out[0].requires_grad and not out[1].requires_grad
        return out

    (outs_a, params_a, _), (outs_b, params_b, unused) = run(plain), run(shared)
    assert all(torch.equal(u, v) for a, b in zip(outs_a, outs_b) for u, v in zip(a, b))
    assert all(torch.equal(u, v) for u, v in zip(params_a, params_b))
    assert unused.grad is None and torch.equal(unused.detach(), torch.ones(2))       # the loss does not reach it: not stepped
    lin = nn.Linear(3, 1)
    opt = torch.optim.SGD(lin.parameters(), lr=0.1)
    loss = capture.grad_step(opt, capture.trainable_params(opt), lambda: lin(torch.ones(1, 3)).sum())
    assert isinstance(loss, torch.Tensor) and loss.dim() == 0 and not loss.requires_grad


class _Slot:
    def __init__(self, cap):
        self.cap, self.asked = cap, []

    def fits(self, sizes, entries=None):
        self.asked.append((sizes, entries))
        return sum(sizes) <= self.cap and (entries is None or sum(entries) <= 2 * self.cap)


def test_first_fit_takes_the_first_slot_in_the_given_order():
    slots = [_Slot(4), _Slot(8), _Slot(8), _Slot(2)]
    assert capture.first_fit(slots, [1, 2]) == 0
    assert capture.first_fit(slots, [5]) == 1                  # (not the later slot of the same size, nor a sorted order of its own)
    assert slots[2].asked == [] and slots[3].asked == []
    assert capture.first_fit(slots, [9]) is None
    assert capture.first_fit([], [1]) is None
    assert capture.first_fit(slots, [3], [9]) == 1             # the two-argument description: sizes, entries
    assert slots[0].asked[-1] == ([3], [9])
    assert capture.first_fit(slots, [3], [17]) is None


def test_smallest_first_keeps_the_warm_up_batches_with_their_slots():
    a, b, c = _Slot(8), _Slot(2), _Slot(8)
    slots, batches = capture.smallest_first([a, b, c], lambda s: s.cap, ["a", "b", "c"])
    assert slots == [b, a, c] and batches == ["b", "a", "c"]   # (stable: equal slots keep their order)
    assert capture.smallest_first([a, b], lambda s: s.cap) == ([b, a], None)


class _Loaded:
    def __init__(self, num_real=0):
        self.num_real, self.got = num_real, None

    def load(self, *batch):
        self.got = batch


def test_load_warm_up_batch():
    slot = _Loaded()
    capture.load_warm_up_batch("Who", 1, slot, [("x",), ("bags", "labels")])
    assert slot.got == ("bags", "labels")
    capture.load_warm_up_batch("Who", 0, _Loaded(num_real=2), None)
    with pytest.raises(ValueError, match="^Who: slot 3 holds no batch to warm up on"):
        capture.load_warm_up_batch("Who", 3, _Loaded(), None)


def test_eval_mode_restores_the_training_flag():
    model = nn.Sequential(nn.Linear(2, 2), nn.Dropout(0.5))
    with capture.eval_mode(model):
        assert not model.training and not model[1].training and not torch.is_grad_enabled()
        assert not model(torch.ones(1, 2)).requires_grad
    assert model.training and model[1].training and torch.is_grad_enabled()
    with pytest.raises(KeyError):
        with capture.eval_mode(model):
            raise KeyError("inside")
    assert model.training and torch.is_grad_enabled()
    model.eval()
    with capture.eval_mode(model):
        assert not model.training
    assert not model.training
