"""The capture protocol: what every class that records a step or a forward into a hipGraph and replays it over new data goes through
(``trainer.CapturedStep`` / ``CapturedSlotStep`` / ``CapturedSlotEval``, ``mil.CapturedBagStep`` / ``CapturedBagEval``,
``gtn.CapturedGraphStep``).  The classes hold what is particular to them - the models they accept, how a batch is described to
``fits`` / ``load``, the recorded body, the eager fallback - and build on the functions here, in this order:

  1. ``require_capturable``: the optimizer keeps its step count on the device.  A host count would be frozen into the graph.
  2. ``counter_dropout_only``: train-mode dropout must be drawn as a function of (host seed + a DEVICE word, row, column) -
     ``ops.CounterDropout``.  The capture freezes the host seeds; the recorded step itself advances the word (``new_seed_word``), so every
     replay drops other entries, forward and backward of one replay the same ones.  A module that draws a mask tensor from a host-seeded
     generator state cannot be replayed: every replay would drop the same entries.
  3. ``trainable_params``: the parameters the step differentiates, after ``zero_grad(set_to_none=True)``.  A model that has been stepped
     before keeps its AccumulateGrad nodes bound to the stream of that step for as long as ANYTHING keeps its last autograd graph alive; such
     a node makes the capture synchronise with the default stream, which is invalid and, on this ROCm, a segfault in capture_end rather than
     an error.  What a class can release it does: the gradients.  What it cannot: tensors of an earlier step the CALLER still holds (a
     previous loss or logits) - they are dropped before a captured class is built (PyTorch's general rule for captures).  For the same reason
     the step body (``grad_step``) takes its gradients from ``torch.autograd.grad`` and assigns them, it never calls ``backward``.
  4. ``warm_up``: the body runs eagerly on a fresh side stream, which forks from and joins the current stream, so that plans, caches and
     allocator pools settle before the capture.  For a training class these runs ARE optimisation steps: they count in ``steps_taken``, and
     the loader's batch counter and the dropout word advance with them.
  5. ``torch.cuda.synchronize``: every other stream has joined before a capture starts.
  6. ``record``: the body is recorded - not executed - under ``capture_error_mode="thread_local"``.  The captures of one class share one
     memory pool: the ``pool()`` of the first graph is handed to the next.  A failure is raised as a RuntimeError that says what to do
     instead.
  7. Per batch, ``first_fit`` takes the smallest slot that fits (the slots are kept sorted, smallest first); the class fills it, replays its
     graph and returns the recorded outputs cut to the real items.  A batch no slot fits runs the same body eagerly, through the ordinary
     assembly.
  8. The learning rate.  A FLOAT ``lr`` is a host value and is frozen into a capture; the classes with a ``recapture()`` record their graphs
     again, without stepping, after it changes.  A tensor ``lr`` - ``optim.lr_word(value, device)``, a float64 device word - is
     read by every replay when it runs: change it with ``fill_`` and the next replay steps at the new rate, nothing is recorded again.
     ``torch.optim.lr_scheduler.*`` work on it unchanged: they ``fill_`` a tensor ``lr`` in place, and with one their arithmetic ends in one
     ``.item()`` per scheduler step, outside any capture.  Never REBIND ``group["lr"]`` under a captured class: the graph holds the word's
     pointer.  The other hyper-parameters stay host values.

``eval_mode`` is what the evaluation classes and the eager evaluators record and run under.
"""
from __future__ import annotations

import contextlib
from typing import Callable, Sequence

import torch


def require_capturable(who: str, optimizer: torch.optim.Optimizer) -> None:
    """Every parameter group of ``optimizer`` carries ``capturable=True`` (``optim.SGD`` and ``optim.Adadelta`` read no count and set it).  A
    tensor ``lr`` of the package's own optimizers is a float64 word on the device of the group's parameters (their constructors and first
    step check the same; a group rebound since is caught here, before it is recorded); ``torch.optim``'s optimizers take a tensor ``lr`` as
    torch accepts it."""
    from . import optim
    for group in optimizer.param_groups:
        if not group.get("capturable", False):
            raise RuntimeError(f"{who}: the optimizer must be capturable (wsi_hgnn_amd.optim.Adam(..., capturable=True)): "
                               "its step count has to live on the device, a host count would be frozen into the graph")
        lr = group.get("lr")
        if isinstance(lr, torch.Tensor) and isinstance(optimizer, optim._OneLaunch):
            if lr.dtype != torch.float64 or lr.numel() != 1 or any(p.device != lr.device for p in group["params"]):
                raise RuntimeError(f"{who}: a tensor lr is a float64 one-element tensor on the parameters' device "
                                   "(wsi_hgnn_amd.optim.lr_word(value, device)): the recorded step reads it there")


def counter_dropout_only(who: str, model: torch.nn.Module, counter_based: Sequence[type] = ()) -> bool:
    """True when ``model`` draws dropout (train mode, a ``torch.nn.Dropout`` with p > 0) and every module that owns one is of a
    ``counter_based`` type - one that draws counter-based under ``ops.dropout_seed_base``, unless it says otherwise with
    ``counter_dropout = False``: the caller then needs a device seed word (``new_seed_word``).  False when nothing is dropped.  Any other
    owner: RuntimeError."""
    live = lambda m: isinstance(m, torch.nn.Dropout) and m.p > 0.0
    if not (model.training and any(live(m) for m in model.modules())):
        return False
    if not counter_based:
        raise RuntimeError(f"{who}: the model holds a torch.nn.Dropout with p > 0 in train mode; its generator state is a host value a capture "
                           "would freeze - every replay would drop the same entries.  Step such a model eagerly")
    owners = [m for m in model.modules() if any(live(c) for c in m.children())]
    if not all(isinstance(m, tuple(counter_based)) and getattr(m, "counter_dropout", True) for m in owners):
        raise RuntimeError(f"{who}: the model draws dropout masks outside the HEAT layers' counter-based draw (train mode, p > 0); their "
                           "generator state is a host value a capture would freeze - every replay would drop the same entries.  Step such a "
                           "model eagerly")
    return True


def new_seed_word(device) -> torch.Tensor:
    """A one-element int32 tensor on ``device`` holding a random word: what ``ops.dropout_seed_base`` takes and the recorded step advances."""
    return torch.empty((), dtype=torch.int64).random_(-(1 << 31), 1 << 31).to(torch.int32).reshape(1).to(device)


def trainable_params(optimizer: torch.optim.Optimizer) -> list:
    """Release every gradient (see the module's note on AccumulateGrad nodes) and list the parameters a step differentiates."""
    optimizer.zero_grad(set_to_none=True)
    return [p for group in optimizer.param_groups for p in group["params"] if p.requires_grad]


def grad_step(optimizer: torch.optim.Optimizer, params, compute: Callable):
    """One optimisation step that can be recorded: ``compute()`` returns the loss, or a tuple of the loss and further tensors; the gradients
    are those of ``loss.backward()`` (a parameter the loss does not reach: None).  Returns what ``compute`` returned, detached."""
    optimizer.zero_grad(set_to_none=True)
    out = compute()
    grads = torch.autograd.grad(out[0] if isinstance(out, tuple) else out, params, allow_unused=True)
    for p, g in zip(params, grads):
        p.grad = g
    optimizer.step()
    return tuple(t.detach() for t in out) if isinstance(out, tuple) else out.detach()


def smallest_first(slots, size: Callable, warmup_batches=None):
    """(``slots`` sorted by ``size(slot)``, ``warmup_batches`` - one per slot, or None - in the same order): what ``first_fit`` tries in turn."""
    order = sorted(range(len(slots)), key=lambda i: size(slots[i]))
    return [slots[i] for i in order], None if warmup_batches is None else [warmup_batches[i] for i in order]


def load_warm_up_batch(who: str, i: int, slot, warmup_batches) -> None:
    """Slot ``i`` warms up on ``slot.load(*warmup_batches[i])``, or (None) on the batch the caller has loaded into it."""
    if warmup_batches is not None:
        slot.load(*warmup_batches[i])
    elif slot.num_real == 0:
        raise ValueError(f"{who}: slot {i} holds no batch to warm up on - load one, or pass warmup_batches")


def warm_up(device, n: int, fn: Callable) -> None:
    """``max(1, n)`` calls of ``fn`` on a fresh side stream that forks from and joins ``device``'s current stream."""
    side = torch.cuda.Stream(device=device)
    side.wait_stream(torch.cuda.current_stream(device))
    with torch.cuda.stream(side):
        for _ in range(max(1, n)):
            fn()
    torch.cuda.current_stream(device).wait_stream(side)


def step_failure(output: str) -> str:
    """The ``failure_hint`` of a training step whose caller may still hold ``output`` of an earlier eager step."""
    return ("the step could not be captured into a hipGraph (is a tensor of an earlier eager step's autograd graph - a previous loss or "
            f"{output} - still alive in the caller?); run the step eagerly instead")


def record(who: str, fn: Callable, pool, failure_hint: str):
    """(graph, what ``fn`` returned) with ``fn`` recorded on the current stream into a new graph that allocates from ``pool`` (None: a pool
    of its own; ``graph.pool()`` for the next capture).  The one place of the package that captures.  The caller has warmed ``fn`` up and
    synchronised the device.  A failure: RuntimeError ``who: failure_hint``."""
    graph = torch.cuda.CUDAGraph()
    try:
        # thread_local: only what THIS thread does during the capture can invalidate it (another thread's allocation or sync must not), and an
        # illegal call here surfaces as a Python error at that call instead of a broken capture found at capture_end.  (What does not surface:
        # a stale AccumulateGrad node - a segfault in capture_end; see the module's note 3.)
        with torch.cuda.graph(graph, pool=pool, capture_error_mode="thread_local"):
            out = fn()
    except Exception as exc:
        raise RuntimeError(f"{who}: {failure_hint}") from exc
    return graph, out


def first_fit(slots, *batch):
    """Index of the first slot of ``slots`` (sorted smallest first) with ``slot.fits(*batch)``, or None."""
    for i, slot in enumerate(slots):
        if slot.fits(*batch):
            return i
    return None


@contextlib.contextmanager
def eval_mode(model: torch.nn.Module):
    """``model.eval()`` under ``torch.no_grad()``; the model's training flag is what it was on exit, also after an exception."""
    was_training = model.training
    model.eval()
    try:
        with torch.no_grad():
            yield
    finally:
        model.train(was_training)
