"""Patch dropout on the device, bags in padded slots of fixed shape, and a captured training step replayed over them.

The reference trains ABMIL / DSMIL on ONE bag per step (``train_tcga_k-fold.py:54-88``), optionally after ``dropout_patches`` (lines 90-96); at
that size a step is a few dozen small launches and the host takes longer to issue them than the GPU to run them.  ``BagSlot`` holds a batch of
bags in static device tables of one shape - the real bags, empty bags up to ``bag_cap``, and a filler bag of zero rows that takes what is left -
so that ``CapturedBagStep`` records the step once per slot (a hipGraph, ``capture.py``) and replays it over new bags: per step one descriptor
upload, the fill kernels, one replay.  The patch dropout is drawn inside the fill (``csrc/bag_slot.hip``); the draw contract is in
``include/wsi_hgnn.h`` and ``dropout_patches_tensor`` restates it with tensor operations.
"""
from __future__ import annotations

import array
import struct
from typing import List, Optional, Sequence, Tuple

import torch

from .. import _native as N
from .. import capture, ops
from . import abmil, dsmil
from .bags import bag_plan

_M32 = 0xffffffff
_GOLDEN = 0x9E3779B1
_SECOND = 0x85EBCA6B


def patch_counts(n: int, p: float) -> Tuple[int, int]:
    """(k, m) of the reference's ``dropout_patches`` (train_tcga_k-fold.py:90-96) for a bag of ``n`` rows at rate ``p``: it keeps
    ``k = int(n * (1 - p))`` rows and appends ``m = int(n * p)`` of them again - these float expressions, which do not floor as exact
    arithmetic would (n = 100, p = 0.29: 71 and 28).  ``m > k`` raises ValueError as numpy's choice without replacement does."""
    n = int(n)
    if n < 0 or not 0.0 <= p <= 1.0:
        raise ValueError("patch_counts: n >= 0 and 0 <= p <= 1")
    k, m = int(n * (1 - p)), int(n * p)
    if m > k:
        raise ValueError(f"patch_counts: cannot repeat {m} of {k} kept rows (n = {n}, p = {p}): a larger sample than the population")
    return k, m


def _fmix32_tensor(h: torch.Tensor) -> torch.Tensor:
    """``ops._fmix32`` on an int64 tensor of 32-bit values."""
    h = h ^ (h >> 16)
    h = (h * 0x85EBCA6B) & _M32
    h = h ^ (h >> 13)
    h = (h * 0xC2B2AE35) & _M32
    return h ^ (h >> 16)


def patch_keys(rows: torch.Tensor, draw: int, second: bool, key_bits: int = 32) -> torch.Tensor:
    """int64 keys of the int64 row numbers ``rows`` under the draw word ``draw``: key1 (``second=False``) or key2 of the draw contract."""
    s = ops._fmix32((int(draw) ^ _SECOND) & _M32 if second else int(draw) & _M32)
    return _fmix32_tensor((rows * _GOLDEN + s) & _M32) & ((1 << key_bits) - 1)


def _sizes(bags) -> List[int]:
    if isinstance(bags, ops.ReducePlan):
        if bags.first_row != 0:
            raise ValueError("dropout_patches: the bag plan must start at row 0")
        return [b - a for a, b in bags.ranges]
    return [int(c) for c in (bags.tolist() if isinstance(bags, torch.Tensor) else bags)]


def _check_bits(key_bits: int) -> None:
    if not 1 <= int(key_bits) <= 32:
        raise ValueError("key_bits is between 1 and 32")


def dropout_patches_tensor(x: torch.Tensor, sizes: Sequence[int], p: float, draws: Sequence[int], key_bits: int = 32):
    """(rows, new_sizes, sel): the patch dropout of the draw contract with integer tensor operations and stable sorts, on x's device (CPU or
    GPU).  ``x`` [N, L] holds the bags one after the other, ``sizes`` their row counts, ``draws`` one 32-bit word per bag.  Per bag the kept
    rows are the k rows with the smallest (key1, row) in ascending row order, then the m kept rows with the smallest (key2, row) in ascending
    row order; ``sel`` (int32) is the source row - within its bag - of every output row."""
    _check_bits(key_bits)
    sizes = [int(n) for n in sizes]
    if len(draws) != len(sizes) or sum(sizes) != x.shape[0]:
        raise ValueError("dropout_patches_tensor: sizes, draws and rows disagree")
    dev = x.device
    sels, new_sizes, glob, off = [], [], [], 0
    for n, d in zip(sizes, draws):
        k, m = patch_counts(n, p)
        i = torch.arange(n, dtype=torch.int64, device=dev)
        kept = torch.sort(torch.argsort(patch_keys(i, d, False, key_bits), stable=True)[:k]).values
        pads = torch.sort(kept[torch.argsort(patch_keys(kept, d, True, key_bits), stable=True)[:m]]).values
        s = torch.cat([kept, pads])
        sels.append(s)
        glob.append(s + off)
        new_sizes.append(k + m)
        off += n
    sel = torch.cat(sels) if sels else torch.zeros(0, dtype=torch.int64, device=dev)
    rows = x.index_select(0, torch.cat(glob)) if glob else x[:0]
    return rows, new_sizes, sel.to(torch.int32)


def _default_draws(seed: int, counter: int, count: int) -> List[int]:
    from ..data import augment_draw
    return [augment_draw(seed, counter, b) for b in range(count)]


def dropout_patches(x: torch.Tensor, bags, p: float, draws: Optional[Sequence[int]] = None, seed: int = 0, kernels: Optional[bool] = None):
    """(rows, plan): the reference's ``dropout_patches`` for every bag of a batch at once.  ``x`` [N, L] fp32, ``bags`` the batch's ``bag_plan``
    (or the bags' row counts); ``draws``: one 32-bit word per bag (None: ``data.augment_draw(seed, 0, bag)``).  The new plan is
    ``bag_plan`` of sizes the host knows (``patch_counts``), so nothing is read back.  On the GPU a selection launch and a row-gather launch
    whatever the number of bags (``kernels=False``: the tensor formulation); ``p == 0`` returns its inputs."""
    sizes = _sizes(bags)
    if p == 0:
        return x, (bags if isinstance(bags, ops.ReducePlan) else bag_plan(sizes, x.device))
    if draws is None:
        draws = _default_draws(seed, 0, len(sizes))
    if len(draws) != len(sizes) or sum(sizes) != x.shape[0]:
        raise ValueError("dropout_patches: sizes, draws and rows disagree")
    use = x.is_cuda if kernels is None else bool(kernels)
    if not use:
        rows, new_sizes, _ = dropout_patches_tensor(x.to(torch.float32), sizes, p, draws)
        return rows, bag_plan(new_sizes, x.device)
    counts = [patch_counts(n, p) for n in sizes]
    x = x.to(torch.float32)
    if x.dim() != 2 or (x.shape[0] > 0 and x.shape[1] > 1 and x.stride(1) != 1):
        x = x.reshape(x.shape[0], -1).contiguous()
    off, sources = 0, []
    for n in sizes:
        sources.append(x[off:off + n])
        off += n
    rows, _ = ops.bag_dropout_rows(sources, counts, draws)
    return rows, bag_plan([k + m for k, m in counts], x.device)


def _float_bits(xs: Sequence[float]) -> List[int]:
    return list(struct.unpack(f"<{len(xs)}i", struct.pack(f"<{len(xs)}f", *xs)))


class BagSlot:
    """A batch of bags of FIXED shape: static device tables that ``load`` rewrites for every batch that fits, so that a step captured over them
    (``CapturedBagStep``) replays over new bags.

    ``rows`` [row_cap, feats] fp32: the real bags one after the other, then the filler's rows (zero).  ``plan``: an ``ops.ReducePlan`` with
    ``bag_cap + 1`` segments - the real bags, empty bags up to ``bag_cap``, and the filler, which takes every row the real bags leave (at least
    one) - padded to the slot's chunk capacity with empty chunks that no segment owns (as ``graph.SlotBatch`` pads the readout plan); its
    counts, inverse counts, non-empty flags and row -> segment table are filled too.  ``targets`` [bag_cap + 1, C]: ``bag_targets`` of the
    labels, zero for unused bags and the filler.  ``weights`` [bag_cap + 1, 1]: 1 / (number of real non-empty bags) for each of those, else 0,
    so that ``bag_loss(..., weights=, targets=)`` is the batch's loss with no host value in it.

    ``dropout_patch > 0``: every ``load`` takes the reference's ``dropout_patches`` of every bag inside the fill (the draw of
    ``dropout_patches``; ``draws=None`` takes ``data.augment_draw(seed, counter, bag)`` with the slot's running load counter).  Capacities are
    those of the undropped bags: dropping never adds rows.

    On the GPU a ``load`` is one upload (per bag the source pointer, row stride, n, k, m, destination row and draw, then the host-built small
    tables) and a fixed number of launches (``wsi_bag_dropout_select`` when the slot drops, ``wsi_bag_slot_fill``): no read-back, no
    allocation inside the library, no shape changes.  The fill writes behind PyTorch's version counters.  On the CPU the same
    tables come from tensor operations (``dropout_patches_tensor``): what the tests hold the kernels against."""

    def __init__(self, feats: int, row_cap: int, bag_cap: int = 1, num_classes: int = 2, device="cuda", chunk: int = 128,
                 dropout_patch: float = 0.0, seed: int = 0):
        if feats < 1 or row_cap < 2 or bag_cap < 1 or num_classes < 1 or chunk < 1:
            raise ValueError("BagSlot: feats >= 1, row_cap >= 2, bag_cap >= 1, num_classes >= 1, chunk >= 1")
        if not 0.0 <= dropout_patch <= 0.5:
            raise ValueError("BagSlot: dropout_patch is between 0 and 0.5 (beyond, the reference repeats more rows than it keeps)")
        self.feats, self.row_cap, self.bag_cap, self.num_classes, self.chunk = int(feats), int(row_cap), int(bag_cap), int(num_classes), int(chunk)
        self.dropout_patch, self.seed, self.counter = float(dropout_patch), int(seed), 0
        self.device = torch.device(device)
        S = self.num_segs = self.bag_cap + 1
        # chunks of any batch that fits: sum of ceil(n_s / chunk) over S segments of row_cap rows in all
        self.chunk_cap = self.row_cap // self.chunk + S
        dev, C = self.device, self.num_classes
        self.rows = torch.zeros((self.row_cap, self.feats), dtype=torch.float32, device=dev)
        self.row_seg = torch.zeros(self.row_cap, dtype=torch.int32, device=dev)
        self.sel = torch.zeros(self.row_cap, dtype=torch.int32, device=dev) if self.dropout_patch > 0 else None
        # the small tables: ONE int32 buffer (floats as their bits), the attributes are views into it
        o, parts = 0, {}
        for name, words in (("chunk_row", self.chunk_cap + 1), ("chunk_seg", self.chunk_cap), ("seg_chunk", S + 1), ("counts", S),
                            ("inv_counts", S), ("nonempty", S), ("targets", S * C), ("weights", S)):
            parts[name] = (o, o + words)
            o += words
        self._parts, self.small = parts, torch.zeros(o, dtype=torch.int32, device=dev)
        view = lambda name: self.small[parts[name][0]:parts[name][1]]
        fview = lambda name: view(name).view(torch.float32)
        p = self.plan = ops.ReducePlan()
        p.device, p.num_segs, p.num_chunks, p.num_rows, p.first_row = dev, S, self.chunk_cap, self.row_cap, 0
        p.chunk_row, p.chunk_seg, p.seg_chunk = view("chunk_row"), view("chunk_seg"), view("seg_chunk")
        p._counts, p._inv_counts, p._nonempty = fview("counts").view(-1, 1), fview("inv_counts").view(-1, 1), fview("nonempty").view(-1, 1)
        p._row_seg = self.row_seg
        self.targets = fview("targets").view(S, C)
        self.weights = fview("weights").view(S, 1)
        self.num_real, self.sizes = 0, []
        self._desc = None

    # ---------------------------------------------------------------- host arithmetic
    def _chunks(self, sizes: Sequence[int]) -> int:
        return sum((n + self.chunk - 1) // self.chunk for n in sizes)

    def fits(self, sizes: Sequence[int]) -> bool:
        """``sizes``: the (undropped) row counts of a batch's bags.  True when the bags, their rows plus one row for the filler, and the
        chunks of bags and filler all fit."""
        sizes = [int(n) for n in sizes]
        if not 1 <= len(sizes) <= self.bag_cap or any(n < 0 for n in sizes):
            return False
        left = self.row_cap - sum(sizes)
        return left >= 1 and self._chunks(sizes) + self._chunks([left]) <= self.chunk_cap

    def take_draws(self, count: int) -> List[int]:
        """The draw words of the next batch of ``count`` bags; advances the slot's load counter."""
        draws = _default_draws(self.seed, self.counter, count)
        self.counter += 1
        return draws

    def tables(self, new_sizes: Sequence[int], labels) -> List[int]:
        """The int32 words of the small tables for a batch whose bags have ``new_sizes`` rows (after dropping) and labels ``labels``."""
        S, C, B = self.num_segs, self.num_classes, len(new_sizes)
        real = sum(new_sizes)
        seg_sizes = list(new_sizes) + [0] * (self.bag_cap - B) + [self.row_cap - real]
        chunk_row, chunk_seg, seg_chunk, ranges, r = [], [], [0], [], 0
        for s, n in enumerate(seg_sizes):
            ranges.append((r, r + n))
            end = r + n
            while r < end:
                chunk_row.append(r)
                chunk_seg.append(s)
                r = min(end, r + self.chunk)
            seg_chunk.append(len(chunk_row))
        pad = self.chunk_cap - len(chunk_seg)
        if pad < 0:
            raise ValueError("BagSlot: chunk capacity exceeded")
        chunk_row += [self.row_cap] * (pad + 1)
        chunk_seg += [S - 1] * pad
        labels = [float(v) for v in (labels.tolist() if isinstance(labels, torch.Tensor) else labels)]
        if len(labels) != B:
            raise ValueError(f"BagSlot: {B} bags but {len(labels)} labels")
        targets = [0.0] * (S * C)
        for b, v in enumerate(labels):
            if C == 1:
                targets[b] = v
            elif 0 <= int(v) < C:
                targets[b * C + int(v)] = 1.0
        live = sum(1 for n in new_sizes if n > 0)
        weights = [1.0 / live if n > 0 else 0.0 for n in new_sizes] + [0.0] * (S - B)
        self.plan.ranges = ranges
        self.plan._seg_of = {}
        return (chunk_row + chunk_seg + seg_chunk
                + _float_bits([float(n) for n in seg_sizes] + [1.0 / n if n > 0 else 0.0 for n in seg_sizes] + [1.0 if n > 0 else 0.0 for n in seg_sizes]
                              + targets + weights))

    # ---------------------------------------------------------------- the fill
    def load(self, bags: Sequence[torch.Tensor], labels, draws: Optional[Sequence[int]] = None) -> "BagSlot":
        """Write the batch ``bags`` (tensors [n_i, feats] fp32 on the slot's device; views with a row stride of their own are fine) with host
        labels ``labels`` into the slot's tables, on the current stream.  Raises ValueError when the batch does not fit."""
        bags = list(bags)
        sizes = [int(t.shape[0]) for t in bags]
        if not self.fits(sizes):
            raise ValueError("the batch does not fit the slot")
        if self.dropout_patch > 0:
            if draws is None:
                draws = self.take_draws(len(bags))
            counts = [patch_counts(n, self.dropout_patch) for n in sizes]
        else:
            draws, counts = [0] * len(bags), [(n, 0) for n in sizes]
        if len(draws) != len(bags):
            raise ValueError("BagSlot.load: one draw per bag")
        new_sizes = [k + m for k, m in counts]
        small = self.tables(new_sizes, labels)
        self.num_real, self.sizes = len(bags), new_sizes
        if self.device.type != "cuda":
            self._load_tensor(bags, sizes, draws, small)
            return self
        N.require_cuda(*bags)
        words, _ = ops.bag_descriptors(bags, counts, draws, self.feats)
        nb = len(words)
        host = torch.cat([torch.frombuffer(array.array("q", words), dtype=torch.int64).view(torch.int32), torch.tensor(small, dtype=torch.int32)])
        desc = ops.host_to_device(host, torch.int32, self.device)
        lib, st = N.load(), N.stream()
        if self.sel is not None:
            N.check(lib.wsi_bag_dropout_select(N.ptr(desc), len(bags), 32, N.ptr(self.sel), self.row_cap, st), "wsi_bag_dropout_select")
        N.check(lib.wsi_bag_slot_fill(N.ptr(desc), len(bags), N.ptr(self.sel), N.ptr(self.rows), self.feats, self.feats, self.row_cap,
                                      N.ptr(self.row_seg), self.num_segs - 1, N.ptr(desc, nb * 8), N.ptr(self.small), len(small), st),
                "wsi_bag_slot_fill")
        self._desc = desc            # (stream-ordered: the table must outlive the launches; the next load replaces it behind them)
        return self

    def _load_tensor(self, bags, sizes, draws, small) -> None:
        with torch.no_grad():
            x = torch.cat([t.to(torch.float32) for t in bags]) if bags else self.rows[:0]
            rows, new_sizes, _ = dropout_patches_tensor(x, sizes, self.dropout_patch, draws)
            real = rows.shape[0]
            self.rows.zero_()
            self.rows[:real] = rows
            seg = torch.repeat_interleave(torch.arange(len(new_sizes), dtype=torch.int32), torch.tensor(new_sizes, dtype=torch.int64))
            self.row_seg.fill_(self.num_segs - 1)
            self.row_seg[:real] = seg.to(self.row_seg.device)
            self.small.copy_(torch.tensor(small, dtype=torch.int32))


def check_bag_slots(who: str, milnet, slots):
    """What a capture over bag slots needs (``CapturedBagStep``, ``CapturedBagEval``): ABMIL or DSMIL, slots on one GPU.  Returns (slots as a
    list, their device)."""
    slots = [slots] if isinstance(slots, BagSlot) else list(slots)
    if not slots:
        raise ValueError(f"{who}: no slot")
    if not isinstance(milnet, (dsmil.MILNet, abmil.BClassifier)):
        raise RuntimeError(f"{who}: {type(milnet).__name__} is not supported - abmil.BClassifier / BClassifier_ or dsmil.MILNet")
    dev = slots[0].device
    if dev.type != "cuda" or any(s.device != dev for s in slots):
        raise RuntimeError(f"{who}: the slots must live on one GPU")
    return slots, dev


def slot_step(milnet, optimizer, slot: BagSlot, params=None):
    """One training step on the batch a slot holds - the body of ``train_one_step`` with the slot's device-side targets and weights, gradients
    from ``torch.autograd.grad``: nothing in it is a host value of the batch, so it can be recorded.  Returns (loss, predictions
    [bag_cap + 1, C]), detached."""
    from . import bag_loss

    def compute():
        outputs = milnet(slot.rows, slot.plan)
        pred = outputs[1] if isinstance(outputs, (tuple, list)) else outputs
        model = "dsmil" if isinstance(milnet, dsmil.MILNet) else "abmil"
        return bag_loss(outputs, None, pred.shape[-1], model, slot.plan, weights=slot.weights, targets=slot.targets), pred
    return capture.grad_step(optimizer, capture.trainable_params(optimizer) if params is None else params, compute)


class CapturedBagStep:
    """One captured ABMIL / DSMIL training step per ``BagSlot``, replayed over new bags every step: the regime the reference trains in (one bag
    per step, ``train_tcga_k-fold.py:54-88``; ReMix's reduced bags), where the host takes longer to issue the step's launches than the GPU to
    run them.  Protocol: ``capture.py``; EVERY slot takes its ``warmup`` (1) optimisation steps (on ``warmup_batches[i] = (bags, labels)`` for
    slot i; None: on what the caller has loaded into the slot) before the first capture, and a ``torch.nn.Dropout`` with p > 0 in train mode
    is refused: these models draw no counter-based dropout.

    ``step(bags, labels)`` loads the smallest slot (fewest rows) that fits and replays; a batch no slot fits runs eagerly through
    ``mil.train_one_step`` - after ``mil.dropout_patches`` if the slots drop - and is counted in ``eager_steps``.  The reference steps a
    ``CosineAnnealingLR`` every epoch.  A FLOAT ``lr`` is a host value frozen into a capture: ``recapture()`` records the graphs again,
    without stepping, after it changes.  A word - ``optim.Adam(..., lr=optim.lr_word(2e-4, device), capturable=True)`` - is read by every
    replay: ``torch.optim.lr_scheduler.*`` work on it unchanged (they ``fill_`` a tensor ``lr``; their arithmetic ends in one ``.item()`` per
    scheduler step, outside any capture) and nothing is recorded again.  Never rebind ``group["lr"]`` here (``capture.py``, point 8).

    ReMix needs nothing more - a slot loads from any device tensor::

        rows, sizes = remix.mix(bank, draws)
        loss, pred = captured.step(torch.split(rows, sizes), [bank.labels[d.idx] for d in draws])
    """

    def __init__(self, milnet: torch.nn.Module, optimizer: torch.optim.Optimizer, slots, warmup: int = 1, warmup_batches=None):
        slots, dev = check_bag_slots("CapturedBagStep", milnet, slots)
        if len({(s.feats, s.num_classes, s.dropout_patch) for s in slots}) != 1:
            raise ValueError("CapturedBagStep: the slots must agree on feats, num_classes and dropout_patch")
        capture.require_capturable("CapturedBagStep", optimizer)
        milnet.train()
        capture.counter_dropout_only("CapturedBagStep", milnet)
        self.milnet, self.optimizer = milnet, optimizer
        self.slots, warmup_batches = capture.smallest_first(slots, lambda s: s.row_cap, warmup_batches)
        self.params = capture.trainable_params(optimizer)
        self.steps_taken, self.replays, self.eager_steps = 0, 0, 0
        for i, slot in enumerate(self.slots):
            capture.load_warm_up_batch("CapturedBagStep", i, slot, warmup_batches)
            capture.warm_up(dev, warmup, lambda: slot_step(self.milnet, self.optimizer, slot, self.params))
            self.steps_taken += max(1, warmup)
        self.graphs, self.outputs = [], []
        self.recapture()

    def recapture(self) -> None:
        """Record every slot's graph again (no step is taken): after a change of a host-side hyper-parameter such as ``lr``."""
        self.graphs, self.outputs = [], []
        torch.cuda.synchronize(self.slots[0].device)
        for slot in self.slots:
            cg, out = capture.record("CapturedBagStep", lambda: slot_step(self.milnet, self.optimizer, slot, self.params),
                                     self.graphs[-1].pool() if self.graphs else None, capture.step_failure("prediction"))
            self.graphs.append(cg)
            self.outputs.append(out)

    def slot_for(self, sizes: Sequence[int]):
        """Index of the smallest slot the batch fits, or None."""
        return capture.first_fit(self.slots, sizes)

    def step(self, bags: Sequence[torch.Tensor], labels):
        """One optimisation step on the bags ``bags`` (device tensors [n_i, feats]) with host labels ``labels``.  Returns ``(loss,
        predictions[:len(bags)])`` as device tensors; those of a replayed step are overwritten by the next replay of the same slot."""
        bags = list(bags)
        i = self.slot_for([int(t.shape[0]) for t in bags])
        self.steps_taken += 1
        if i is None:
            self.eager_steps += 1
            return self._eager(bags, labels)
        slot = self.slots[i]
        slot.load(bags, labels)
        self.graphs[i].replay()
        self.replays += 1
        loss, pred = self.outputs[i]
        return loss, pred[:slot.num_real]

    def _eager(self, bags, labels):
        """A batch no slot fits: ``mil.train_one_step`` on the unpadded batch (dropped with the largest slot's next draws if the slots drop)."""
        from . import train_one_step
        big = self.slots[-1]
        x = torch.cat([t.to(torch.float32) for t in bags])
        x, plan = dropout_patches(x, [int(t.shape[0]) for t in bags], big.dropout_patch,
                                  big.take_draws(len(bags)) if big.dropout_patch > 0 else None)
        seen = []
        hook = self.milnet.register_forward_hook(lambda _m, _i, out: seen.append(out))
        try:
            loss = train_one_step(self.milnet, self.optimizer, x, plan, labels)
        finally:
            hook.remove()
        out = seen[-1]
        return loss, (out[1] if isinstance(out, (tuple, list)) else out).detach()
