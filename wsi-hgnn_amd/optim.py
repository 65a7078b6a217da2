"""The optimizer step of the reference's trainer on the GPU in ONE launch.

``parser.parse_optimizer`` (parser.py:15-46) builds ``torch.optim.Adam(model.parameters(), lr, weight_decay)`` (:33-38), :class:`Adagrad`
(``lr_decay = weight_decay``, :23), :class:`Adadelta`, and :class:`SGD` for anything else; ``trainer/train_gnn.py:72`` calls ``optimizer.step()``
after ``loss.backward()``.  The four classes here are those optimizers with torch's arithmetic (Adam: L2 penalty added to the gradient,
bias-corrected moments, ``amsgrad=False``), torch's constructor arguments and torch's ``state_dict`` layout (``step`` / ``exp_avg`` /
``exp_avg_sq``; ``momentum_buffer``; ``sum`` / ``step``; ``step`` / ``square_avg`` / ``acc_delta`` - checkpoints move between the two), each
stepping every parameter of a group through ``wsi_optim_step`` (csrc/optim.hip): one kernel template over the rule, one launch over all tensors -
for Adam 28 bytes of HBM traffic per element, where torch's fused path takes two launches at half the bandwidth on this model's 54 tensors.
GPU only - there is no CPU path.

Adam and Adagrad read the step count.  By default ``state["step"]`` is a Python int, as a checkpoint of torch's holds it, and the step's factors
are taken on the host.  ``capturable=True`` keeps it as a 0-dim fp32 device word, torch's capturable layout, which the kernel itself reads and
advances: that is what ``trainer.CapturedStep`` needs to replay the step from a hipGraph.  SGD and Adadelta never read a count, so their groups
always carry ``capturable=True``.

The learning rate may be a device word too: ``lr`` a float64 one-element tensor on the parameters' device, what
:func:`lr_word` returns and what ``torch.optim`` itself accepts as a tensor ``lr``.  The launch then goes through ``wsi_optim_step_lr`` and the
kernel reads the rate when it RUNS: no step reads the tensor back, and a step recorded into a hipGraph follows every later ``fill_`` of the word -
which is how ``torch.optim.lr_scheduler.*`` change a tensor ``lr``.  So under a captured class the rate is changed with ``fill_`` (or by a torch
scheduler) and ``group["lr"]`` is NEVER rebound: the capture holds the word's pointer.  An eager step follows a rebound ``group["lr"]`` at the
next step (the cached descriptor table is keyed on the word's ``data_ptr``).  With the double ``v`` in the word a step gives the bits of the
same step with the float ``lr = v``.  Adam and Adagrad take a word under ``capturable=True`` only: a host count has its factors taken on the
host, which cannot see the word (torch draws the same line).  All groups that were given the same tensor share one rate.
"""
from __future__ import annotations

import ctypes
from typing import Iterable

import torch

from . import _native as N


def _refuse(name: str, **unsupported) -> None:
    """torch.optim's keywords that select another algorithm or another implementation: accepted at their defaults, refused otherwise."""
    for k, v in unsupported.items():
        if v:
            raise ValueError(f"wsi_hgnn_amd.optim.{name} has one implementation (one HIP launch) and one algorithm: {k}={v!r} is not supported")


def lr_word(value: float, device=None) -> torch.Tensor:
    """A learning rate the kernels read on the device: a 0-dim float64 tensor on ``device`` holding ``value`` (float64, so that a Python float
    a scheduler ``fill_``s in is held exactly).  Pass it as ``lr=`` to the optimizers of this module."""
    return torch.full((), float(value), dtype=torch.float64, device=device)


def _check_lr(name: str, lr, reads_count: bool = False, capturable: bool = True) -> None:
    """The constructors' check of ``lr``: a float is >= 0; a tensor is a device word (never read back here - torch checks no tensor lr either)."""
    if isinstance(lr, torch.Tensor):
        if lr.dtype != torch.float64 or lr.numel() != 1:
            raise ValueError(f"{name}: a tensor lr is a float64 tensor of exactly one element on the parameters' device (got {lr.dtype}, "
                             f"{lr.numel()} elements): make one with wsi_hgnn_amd.optim.lr_word(value, device)")
        if reads_count and not capturable:
            raise ValueError(f"{name}: a tensor lr needs capturable=True - this rule's factors depend on the step count, and with a count kept on "
                             "the host they are taken on the host, where the word cannot be read without a synchronisation")
    elif lr < 0.0:
        raise ValueError(f"{name}: invalid hyper-parameter")


def _host_lr(group: dict) -> float:
    """``hyper->lr``: the float rate, or 0.0 beside a word (wsi_optim_step_lr ignores it) - a tensor is never read back."""
    lr = group["lr"]
    return 0.0 if isinstance(lr, torch.Tensor) else float(lr)


def _load_into(kept: torch.Tensor, value) -> torch.Tensor:
    """``kept`` holding ``value`` (a number or a one-element tensor): the object and its ``data_ptr`` stay, which a capture depends on."""
    if isinstance(value, torch.Tensor):
        kept.copy_(value.detach().reshape(kept.shape))
    else:
        kept.fill_(float(value))
    return kept


def _check_param(name: str, p: torch.Tensor) -> None:
    if not p.is_cuda or p.dtype != torch.float32 or not p.is_contiguous():
        raise RuntimeError(f"wsi_hgnn_amd.optim.{name} steps contiguous fp32 parameters on the GPU only (no CPU path)")
    if p.grad.is_sparse:
        raise RuntimeError(f"wsi_hgnn_amd.optim.{name} does not take sparse gradients")


class _OneLaunch(torch.optim.Optimizer):
    """What the optimizers that step through ``wsi_optim_step`` share: the per-group descriptor table, the ticket words, the step contract."""

    RULE = None                 # N.WSI_OPTIM_*
    STATE = ()                  # state tensors in the order of wsi_optim_tensor_t's s0, s1
    READS_COUNT = False         # the rule's arithmetic depends on the step count (Adagrad's clr, Adam's bias corrections)

    def _new_state(self, p: torch.Tensor, group: dict) -> dict:
        """Create ``self.state[p]`` in torch's layout for this rule and return it."""
        st = self.state[p]
        if "step" in self._state_keys(group):
            st["step"] = torch.zeros((), dtype=torch.float32, device=p.device) if group["capturable"] else 0
        for k in self.STATE:
            st[k] = torch.zeros_like(p, memory_format=torch.contiguous_format)
        self.__dict__.pop("_wsi_tables", None)                    # (a cached table holds the pointers of the state it was built over)
        return st

    def _state_keys(self, group: dict):
        return ("step",) + tuple(self.STATE)

    def _ensure_state(self, p: torch.Tensor, group: dict, st: dict) -> int:
        """State of a parameter about to be stepped; returns its wsi_optim_tensor_t flags."""
        if len(st) == 0:
            self._new_state(p, group)
        return 0

    def _hyper(self, group: dict, h) -> None:
        raise NotImplementedError

    def _tickets(self, device: torch.device) -> torch.Tensor:
        # one int32 word per parameter, zero between launches (the workgroups of a tensor count themselves through it); on the optimizer, not in
        # `state`: state_dict() stays torch's
        bufs = self.__dict__.setdefault("_wsi_tickets", {})
        buf = bufs.get(device)
        if buf is None:
            n = sum(len(g["params"]) for g in self.param_groups)
            buf = bufs[device] = torch.zeros(max(n, 1), dtype=torch.int32, device=device)
        return buf

    def _ticket_index(self) -> dict:
        idx = self.__dict__.get("_wsi_ticket_index")
        n = sum(len(g["params"]) for g in self.param_groups)
        if idx is None or len(idx) != n:
            idx = self.__dict__["_wsi_ticket_index"] = {id(p): i for i, p in enumerate(p for g in self.param_groups for p in g["params"])}
            self.__dict__.pop("_wsi_tickets", None)               # (a parameter group was added: larger buffers,
            self.__dict__.pop("_wsi_tables", None)                #  and tables that point into the old ones go)
        return idx

    def gate(self, params, table, index: int = 0) -> None:
        """Bind ``params`` to the gate word ``table[index]`` (``table``: a float32 1-d tensor of at most 255 words on the parameters' device;
        DESIGN 3.29): the launch reads the word ON THE DEVICE and leaves a parameter whose word is 0.0 alone - ``p``, its state tensors and
        its ``step`` word stay bit for bit as they were, what torch does to a parameter whose gradient is ``None`` - and steps it as ever
        when the word is anything else.  That is how a captured step, which differentiates a fixed parameter list, skips the head of a node
        type the batch lacks (``trainer.CapturedSlotStep`` over ``BatchSlot(type_mask=True)``).  All gated parameters of one optimizer
        share one table.  ``gate(params, None)`` unbinds.  Adam and Adagrad read the count: a host count advances whether the kernel stepped
        the tensor or not, so they take a gate under ``capturable=True`` only."""
        params = list(params)
        gates = self.__dict__.setdefault("_wsi_gates", {})
        self.__dict__.pop("_wsi_tables", None)                    # (a cached descriptor table holds the gate indices it was built with)
        if table is None:
            for p in params:
                gates.pop(id(p), None)
            return
        name = type(self).__name__
        group_of = {id(p): g for g in self.param_groups for p in g["params"]}
        for p in params:
            if id(p) not in group_of:
                raise ValueError(f"{name}.gate: a parameter this optimizer does not step")
            if self.READS_COUNT and not group_of[id(p)]["capturable"]:
                raise RuntimeError(f"{name}.gate needs capturable=True: this rule reads the step count, and a count kept on the host advances "
                                   "whether the kernel stepped the tensor or not - the gate is read on the device only")
        if (not isinstance(table, torch.Tensor) or table.dtype != torch.float32 or table.dim() != 1 or not table.is_cuda
                or not table.is_contiguous() or not 1 <= table.numel() <= 255):
            raise ValueError(f"{name}.gate: the table is a contiguous float32 1-d tensor of 1 to 255 words on the GPU")
        if not 0 <= int(index) < table.numel():
            raise ValueError(f"{name}.gate: index {index} outside the table's {table.numel()} words")
        if any(p.device != table.device for p in params):
            raise ValueError(f"{name}.gate: the table and the parameters live on different devices")
        rebound = {id(p) for p in params}
        if any(t.data_ptr() != table.data_ptr() for k, (t, _) in gates.items() if k not in rebound):
            raise ValueError(f"{name}.gate: all gated parameters of one optimizer share one table (one launch reads one)")
        for p in params:
            gates[id(p)] = (table, int(index))

    def load_state_dict(self, state_dict) -> None:
        # torch replaces the groups by the saved ones and keeps a saved count as it finds it: where the count lives is this OBJECT'S choice
        # (a checkpoint written by torch.optim, host counts, loads into a capturable optimizer and the other way round)
        # So is whether the rate is a word: an optimizer built with one keeps THAT tensor (a capture holds its pointer) and fills it with the
        # loaded value, float or tensor; one built with a float takes float(value).  `initial_lr`, which schedulers add, likewise - a tensor
        # of its own on the device, never an alias of lr.
        capturable = [g["capturable"] for g in self.param_groups]
        # The state tensors this object already steps are kept as well where the loaded ones have their shape, dtype and device, and take the
        # loaded values: a recorded step reads and writes THEM, so a checkpoint loaded under a captured class is what its next replay sees.
        rates = [(g["lr"], g.get("initial_lr")) for g in self.param_groups]
        kept = {p: dict(self.state[p]) for g in self.param_groups for p in g["params"] if p in self.state}
        super().load_state_dict(state_dict)
        for group, cap, (lr, initial) in zip(self.param_groups, capturable, rates):
            group["capturable"] = cap
            if isinstance(lr, torch.Tensor):
                group["lr"] = _load_into(lr, group["lr"])
                if "initial_lr" in group:
                    group["initial_lr"] = _load_into(initial if isinstance(initial, torch.Tensor) else torch.empty_like(lr), group["initial_lr"])
                elif isinstance(initial, torch.Tensor):
                    group["initial_lr"] = initial
            else:
                group["lr"] = float(group["lr"])
                if isinstance(group.get("initial_lr"), torch.Tensor):
                    group["initial_lr"] = float(group["initial_lr"])
            for p in group["params"]:
                st = self.state.get(p)
                if not st:
                    continue
                old = kept.get(p, {})
                if "step" in st:
                    if cap:
                        word = old.get("step")
                        if isinstance(word, torch.Tensor) and word.dtype == torch.float32 and word.dim() == 0 and word.device == p.device:
                            st["step"] = _load_into(word, st["step"])
                        else:
                            st["step"] = torch.as_tensor(float(st["step"]), dtype=torch.float32).reshape(()).to(p.device)
                    else:
                        st["step"] = int(st["step"])
                for k, new in st.items():
                    was = old.get(k)
                    if (k != "step" and isinstance(new, torch.Tensor) and isinstance(was, torch.Tensor) and was is not new
                            and (was.shape, was.dtype, was.device, was.is_contiguous()) == (new.shape, new.dtype, new.device, True)):
                        st[k] = was.copy_(new)
        self.__dict__.pop("_wsi_tables", None)

    def _step_group(self, lib, gi: int, group: dict) -> None:
        name = type(self).__name__
        cap = group["capturable"]
        host_counts = self.READS_COUNT and not cap
        word = group["lr"] if isinstance(group["lr"], torch.Tensor) else None
        if word is not None and host_counts:
            raise ValueError(f"{name}: a tensor lr needs capturable=True (the host takes this rule's factors for a host count, and cannot read the word)")
        keys = self._state_keys(group)
        by_step = {}
        for p in group["params"]:
            if p.grad is None:
                continue
            _check_param(name, p)
            st = self.state[p] if keys else {}                  # (SGD without momentum keeps no state, and like torch leaves no empty entry)
            flags = self._ensure_state(p, group, st)
            t = 0
            # the count is a plain Python number (a state loaded from torch.optim brings a tensor: converted once; torch converts back when it
            # loads ours).  One host-tensor update per parameter and step, as torch keeps them, was the one thing in this loop that touched the
            # CPU tensor machinery - and with it, once in ~30 steps, an 80 ms stall of the whole process on a CPU-quota'd box.
            if host_counts:
                t = int(st["step"]) + 1
                st["step"] = t
            g = p.grad if p.grad.is_contiguous() else p.grad.contiguous()
            by_step.setdefault(t, []).append((p, g, st, flags))
        if not by_step:
            return
        tables = self.__dict__.setdefault("_wsi_tables", {})      # (on the optimizer, not in param_groups: state_dict() stays plain data)
        index = self._ticket_index()
        has_step = "step" in keys and not host_counts
        hyper = self.__dict__.get("_wsi_hyper")
        if hyper is None:
            hyper = self.__dict__["_wsi_hyper"] = N.OptimHyper()
        self._hyper(group, hyper)
        for t, items in by_step.items():                        # (one launch when every parameter has been stepped equally often, or counts on the device)
            # the descriptor table is kept between steps and only the pointers that move are refreshed: the parameter's and the gradient's.  The
            # state tensors, step words included, are replaced by _new_state and load_state_dict only, and both drop the table
            key = (tuple(id(p) for p, _, _, _ in items), None if word is None else word.data_ptr())        # (a rebound group["lr"] is followed)
            cached = tables.get(gi)
            if cached is None or cached[0] != key:
                if word is not None:                            # (the constructor's check again: the group's lr may have been rebound since)
                    _check_lr(name, word)
                    if word.device != items[0][0].device:
                        raise ValueError(f"{name}: the lr tensor lives on {word.device}, the parameters on {items[0][0].device}: make it with "
                                         "wsi_hgnn_amd.optim.lr_word(value, device)")
                arr = (N.OptimTensor * len(items))()
                tick = self._tickets(items[0][0].device)
                written, empty = [], []                        # every tensor the launch writes; the step words of zero-element tensors
                gates = self.__dict__.get("_wsi_gates") or {}
                gidx, gtable = (ctypes.c_int32 * len(items))(), None          # per tensor 0 or the 1-based word of the gate table (gate())
                for k, (a, (p, _, st, _)) in enumerate(zip(arr, items)):
                    bound = gates.get(id(p))
                    if bound is not None:
                        gtable, gidx[k] = bound[0], bound[1] + 1
                    a.n = p.numel()
                    written.append(p)
                    for field, k in zip(("s0", "s1"), self.STATE):
                        setattr(a, field, st[k].data_ptr())
                        written.append(st[k])
                    if has_step:
                        if p.device != tick.device:
                            tick = self._tickets(p.device)
                        a.step, a.ticket = st["step"].data_ptr(), tick.data_ptr() + 4 * index[id(p)]
                        written.append(st["step"])
                        if a.n == 0:
                            empty.append((st["step"], None if bound is None else bound[0][bound[1]]))
                cached = tables[gi] = (key, arr, ctypes.cast(arr, ctypes.c_void_p), written, empty, gidx, gtable)
            _, arr, arr_p, written, empty, gidx, gtable = cached
            for a, (p, g, _, flags) in zip(arr, items):
                a.p, a.g, a.flags = p.data_ptr(), g.data_ptr(), flags
            for count, gate in empty:                             # (no workgroup of the launch covers a zero-element tensor; torch counts its steps too -
                count += 1 if gate is None else (gate != 0).to(torch.float32)      # those of a gated one where its gate word says so, on the device)
            hyper.host_step = float(t)
            if word is not None:                                 # the rate is read by the launch, on the device: no read-back, nothing a capture freezes
                N.check(lib.wsi_optim_step_lr(self.RULE, arr_p, len(items), ctypes.addressof(hyper),
                                              None if gtable is None else ctypes.cast(gidx, ctypes.c_void_p), N.ptr(gtable),
                                              0 if gtable is None else gtable.numel(), word.data_ptr(), N.stream()), "wsi_optim_step_lr")
            elif gtable is None:
                N.check(lib.wsi_optim_step(self.RULE, arr_p, len(items), ctypes.addressof(hyper), N.stream()), "wsi_optim_step")
            else:
                N.check(lib.wsi_optim_step_gated(self.RULE, arr_p, len(items), ctypes.addressof(hyper), ctypes.cast(gidx, ctypes.c_void_p),
                                                 N.ptr(gtable), gtable.numel(), N.stream()), "wsi_optim_step_gated")
            # the kernel wrote through raw pointers: move the version counters as torch.optim's in-place ops would, so that autograd's "modified
            # by an inplace operation" check and every version-keyed fact about these tensors (ops._annotate) see the step
            torch.autograd.graph.increment_version(written)

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        lib = N.load()
        from . import ops
        ops._background_recover()       # a backward pass that raised never joined its side stream: order this step behind it (no-op otherwise)
        for gi, group in enumerate(self.param_groups):
            self._step_group(lib, gi, group)
        ops.repack_weights()            # the packed fp16 planes of the weights the projections read (ops._PACKED): all of them in one launch per op
        return loss


class SGD(_OneLaunch):
    """``torch.optim.SGD`` (the fall-through of parser.py:15-46) in one launch; momentum, dampening, nesterov and weight decay as torch's."""
    RULE = N.WSI_OPTIM_SGD

    def __init__(self, params: Iterable, lr: float = 1e-3, momentum: float = 0, dampening: float = 0, weight_decay: float = 0,
                 nesterov: bool = False, *, maximize: bool = False, foreach=None, differentiable: bool = False, fused=None):
        _refuse("SGD", maximize=maximize, foreach=foreach, differentiable=differentiable, fused=fused)
        _check_lr("SGD", lr)
        if momentum < 0.0 or weight_decay < 0.0:
            raise ValueError("SGD: invalid hyper-parameter")
        if nesterov and (momentum <= 0 or dampening != 0):
            raise ValueError("Nesterov momentum requires a momentum and zero dampening")
        super().__init__(params, dict(lr=lr, momentum=momentum, dampening=dampening, weight_decay=weight_decay, nesterov=nesterov,
                                      capturable=True,       # (no count is read: nothing a capture could freeze)
                                      maximize=False, foreach=None, differentiable=False, fused=None))      # (torch's group keys: checkpoints move both ways)

    def _state_keys(self, group):
        return ("momentum_buffer",) if group["momentum"] != 0 else ()

    def gate(self, params, table, index: int = 0) -> None:
        # a gated tensor's FIRST step may be one the gate skips: its buffer then starts at zero, and the step that does run computes
        # momentum * 0 + (1 - dampening) * g - torch's first step (buf = g) exactly when dampening is 0
        params = list(params)
        if table is not None:
            group_of = {id(p): g for g in self.param_groups for p in g["params"]}
            if any(id(p) in group_of and group_of[id(p)]["momentum"] != 0 and group_of[id(p)]["dampening"] != 0 for p in params):
                raise ValueError("SGD.gate: with momentum, a gate needs dampening = 0 (a tensor whose first step the gate skips starts from a zero "
                                 "buffer, which equals torch's first step only then)")
        super().gate(params, table, index)

    def _new_state(self, p, group):
        st = self.state[p]
        gated = id(p) in (self.__dict__.get("_wsi_gates") or {})
        # written, not read, by the first step - unless a gate skips that step: zeros then (see gate)
        st["momentum_buffer"] = (torch.zeros_like if gated else torch.empty_like)(p, memory_format=torch.contiguous_format)
        self.__dict__.pop("_wsi_tables", None)
        return st

    def _ensure_state(self, p, group, st):
        if group["momentum"] == 0:
            return 0                                             # (no state at all, as torch)
        if st.get("momentum_buffer") is None:
            self._new_state(p, group)
            return N.WSI_OPTIM_FIRST
        return 0

    def _step_group(self, lib, gi, group):
        self.STATE = self._state_keys(group)
        super()._step_group(lib, gi, group)

    def _hyper(self, group, h):
        h.lr, h.weight_decay, h.momentum = _host_lr(group), float(group["weight_decay"]), float(group["momentum"])
        h.dampening, h.nesterov = float(group["dampening"]), float(bool(group["nesterov"]))


class Adagrad(_OneLaunch):
    """``torch.optim.Adagrad`` (parser.py:20-24; the reference passes ``lr_decay = weight_decay``) in one launch."""
    RULE = N.WSI_OPTIM_ADAGRAD
    STATE = ("sum",)
    READS_COUNT = True

    def __init__(self, params: Iterable, lr: float = 1e-2, lr_decay: float = 0, weight_decay: float = 0, initial_accumulator_value: float = 0,
                 eps: float = 1e-10, foreach=None, *, maximize: bool = False, differentiable: bool = False, fused=None, capturable: bool = False):
        _refuse("Adagrad", maximize=maximize, foreach=foreach, differentiable=differentiable, fused=fused)
        _check_lr("Adagrad", lr, True, bool(capturable))
        if lr_decay < 0.0 or weight_decay < 0.0 or initial_accumulator_value < 0.0 or eps < 0.0:
            raise ValueError("Adagrad: invalid hyper-parameter")
        super().__init__(params, dict(lr=lr, lr_decay=lr_decay, eps=eps, weight_decay=weight_decay,
                                      initial_accumulator_value=initial_accumulator_value, capturable=bool(capturable),
                                      foreach=None, maximize=False, differentiable=False, fused=None))
        for group in self.param_groups:                          # torch.optim.Adagrad creates its state in the constructor
            for p in group["params"]:
                self._new_state(p, group)

    def _new_state(self, p, group):
        st = super()._new_state(p, group)
        if group["initial_accumulator_value"]:
            st["sum"].fill_(float(group["initial_accumulator_value"]))
        return st

    def _hyper(self, group, h):
        h.lr, h.weight_decay, h.lr_decay, h.eps = _host_lr(group), float(group["weight_decay"]), float(group["lr_decay"]), float(group["eps"])


class Adadelta(_OneLaunch):
    """``torch.optim.Adadelta`` (parser.py:25-30) in one launch; ``state["step"]`` is a device word the kernel advances (the rule never reads it)."""
    RULE = N.WSI_OPTIM_ADADELTA
    STATE = ("square_avg", "acc_delta")

    def __init__(self, params: Iterable, lr: float = 1.0, rho: float = 0.9, eps: float = 1e-6, weight_decay: float = 0, foreach=None, *,
                 capturable: bool = True, maximize: bool = False, differentiable: bool = False):
        _refuse("Adadelta", maximize=maximize, foreach=foreach, differentiable=differentiable)
        if not capturable:
            raise ValueError("Adadelta: the count is kept on the device and the rule never reads it - there is no non-capturable form")
        _check_lr("Adadelta", lr)
        if not (0.0 <= rho <= 1.0) or eps < 0.0 or weight_decay < 0.0:
            raise ValueError("Adadelta: invalid hyper-parameter")
        super().__init__(params, dict(lr=lr, rho=rho, eps=eps, weight_decay=weight_decay, capturable=True,      # (always: no count is read)
                                      maximize=False, foreach=None, differentiable=False))

    def _hyper(self, group, h):
        h.lr, h.weight_decay, h.rho, h.eps = _host_lr(group), float(group["weight_decay"]), float(group["rho"]), float(group["eps"])


class Adam(_OneLaunch):
    """``torch.optim.Adam`` (parser.py:33-38, the reference's default) in one launch; the count a Python int, or a device word under ``capturable=True``."""
    RULE = N.WSI_OPTIM_ADAM
    STATE = ("exp_avg", "exp_avg_sq")
    READS_COUNT = True

    def __init__(self, params: Iterable, lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-8, weight_decay: float = 0.0,
                 amsgrad: bool = False, *, foreach=None, maximize: bool = False, capturable: bool = False, differentiable: bool = False,
                 fused=None, decoupled_weight_decay: bool = False):
        _refuse("Adam", amsgrad=amsgrad, foreach=foreach, maximize=maximize, differentiable=differentiable, fused=fused,
                decoupled_weight_decay=decoupled_weight_decay)
        _check_lr("Adam", lr, True, bool(capturable))
        if eps < 0.0 or weight_decay < 0.0 or not (0.0 <= betas[0] < 1.0) or not (0.0 <= betas[1] < 1.0):
            raise ValueError("Adam: invalid hyper-parameter")
        super().__init__(params, dict(lr=lr, betas=tuple(betas), eps=eps, weight_decay=weight_decay, capturable=bool(capturable),
                                      amsgrad=False, maximize=False, foreach=None, differentiable=False, fused=None, decoupled_weight_decay=False))

    def _hyper(self, group, h):
        h.lr, h.weight_decay, h.eps = _host_lr(group), float(group["weight_decay"]), float(group["eps"])
        h.beta1, h.beta2 = float(group["betas"][0]), float(group["betas"][1])
