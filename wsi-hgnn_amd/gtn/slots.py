"""GTNMIL slides in padded slots of fixed shape, and a captured training step replayed over them.

A GTNMIL step on a packed batch is bound by the host: some 45 small GEMM launches through ctypes, an ``ops.EdgeCSR`` (two sorts, two cumsums)
per batch, per-slide row ranges baked into the grouped GEMMs.  ``GraphSlot`` holds a batch in static device tables of ONE shape - ``cells``
cells of ``cell_rows`` rows, slide i at the head of cell i, every other row dead - so that ``CapturedGraphStep`` records the step once per slot
(a hipGraph, ``capture.py``) and replays it over new slides: per step one descriptor upload, the two fill launches (``csrc/graph_slot.hip``), one
replay.  ``SlideSet`` keeps the data set resident with every slide's LOCAL CSR / CSC tables built once; the block-diagonal adjacency of a
batch is those tables one after the other, rebased by the fill.
"""
from __future__ import annotations

import array
import ctypes
from typing import List, Optional, Sequence

import torch

from .. import _native as N
from .. import capture, ops
from .batch import GraphBatch

_DESC = 16              # int64 words per slide descriptor (include/wsi_hgnn.h, wsi_graph_slot_fill)


class SlideSet:
    """The resident data set: per slide ``x`` [n, F] fp32 on ``device`` and the slide's local ``ops.EdgeCSR`` (CSR by row, CSC by column,
    weights attached if it has any), built ONCE.  ``items``: one ``(x, row, col, weight or None)`` with local indices per slide, or one
    single-slide ``GraphBatch`` (``gtn.from_grid`` output) per slide.  The original entries are kept for ``batch`` - the packed ``GraphBatch``
    of a few slides, what a step that fits no slot runs on."""

    def __init__(self, items, device="cuda"):
        self.device = torch.device(device)
        self.x, self.ec, self.entries_coo, self.sizes, self.entries = [], [], [], [], []
        for item in items:
            if isinstance(item, GraphBatch):
                if item.num_graphs != 1:
                    raise ValueError("SlideSet: one slide per item (a GraphBatch of one slide)")
                item = (item.x, item.row, item.col, item.weight)
            x, row, col, w = item
            if x.dim() != 2 or x.shape[0] < 1:
                raise ValueError("SlideSet: a slide is x [n >= 1, F] with its entries (row, col, weight)")
            x = x.detach().to(self.device, torch.float32).contiguous()
            row, col = row.to(self.device, torch.int64), col.to(self.device, torch.int64)
            w = None if w is None else w.detach().to(self.device, torch.float32)
            n = int(x.shape[0])
            if row.numel() and (int(row.min()) < 0 or int(col.min()) < 0 or int(row.max()) >= n or int(col.max()) >= n):
                raise ValueError("SlideSet: an entry outside its slide (row and col are local: 0 <= index < n)")
            self.x.append(x)
            self.ec.append(ops.EdgeCSR(row, col, n).with_weights(w))
            self.entries_coo.append((row, col, w))
            self.sizes.append(n)
            self.entries.append(int(row.numel()))
        if not self.x:
            raise ValueError("SlideSet: no slide")
        if len({t.shape[1] for t in self.x}) != 1:
            raise ValueError("SlideSet: the slides disagree on the feature width")
        self.feats = int(self.x[0].shape[1])
        # the pointer words of every slide's descriptor, once: [x, x_stride, rowptr, src, edge_w, colptr, csc_dst, edge_w_csc, rows, entries]
        self._words = [(x.data_ptr(), x.stride(0), ec.rowptr.data_ptr(), ec.src.data_ptr(), 0 if ec.edge_w is None else ec.edge_w.data_ptr(),
                        ec.colptr.data_ptr(), ec.csc_dst.data_ptr(), 0 if ec.edge_w_csc is None else ec.edge_w_csc.data_ptr(), n, e)
                       for x, ec, n, e in zip(self.x, self.ec, self.sizes, self.entries)]

    def __len__(self) -> int:
        return len(self.x)

    def batch(self, idxs: Sequence[int]) -> GraphBatch:
        """The packed ``GraphBatch`` of the slides ``idxs`` (weights of 1 for an unweighted slide next to a weighted one)."""
        idxs = list(idxs)
        rows, cols, off = [], [], 0
        weighted = any(self.entries_coo[i][2] is not None for i in idxs)
        ws = []
        for i in idxs:
            r, c, w = self.entries_coo[i]
            rows.append(r + off)
            cols.append(c + off)
            if weighted:
                ws.append(torch.ones(r.shape[0], dtype=torch.float32, device=self.device) if w is None else w)
            off += self.sizes[i]
        return GraphBatch(torch.cat([self.x[i] for i in idxs]), torch.cat(rows), torch.cat(cols), torch.cat(ws) if weighted else None,
                          [self.sizes[i] for i in idxs])


class GraphSlot:
    """A batch of at most ``cells`` slides of FIXED shape.  Cell g owns the rows ``[g * cell_rows, (g + 1) * cell_rows)``; a slide's rows
    come first in its cell, the rest of the cell is dead, a cell without a slide is all dead.  Static tables, allocated once, rewritten by
    ``load``: ``x`` [cells * cell_rows, feats] (zero in dead rows), ``live`` [rows] and ``cell_live`` [cells] fp32 0 / 1, ``inv_cells`` (one
    word: 1 / slides), ``live_rows`` (one word: the live rows as fp32), ``labels`` int64 [cells] (-100 in unused cells) and the tables of an
    ``ops.EdgeCSR`` over all rows (``ec``: ``rowptr``, ``src``, ``edge_w``, ``colptr``, ``csc_dst``, ``edge_w_csc``; entry arrays of length
    ``entry_cap``, weights always present, a dead row an empty range in both directions).  ``rp``: an ``ops.ReducePlan`` over the cells, built
    once.  Everything that reads the adjacency walks ``rowptr`` / ``colptr`` (``wsi_spmm_sum`` is sized by rows, ``wsi_mincut_fwd`` / ``_bwd`` by
    the plan's chunks), so the entries behind the batch's last one are never referenced and are not rewritten.

    The model takes a slot where it takes a ``GraphBatch`` (``num_graphs = cells``): BatchNorm becomes ``ops.masked_batch_norm``, the pooling
    losses masked means, the labels the slot's.  On the GPU a ``load`` is one upload and two launches (``wsi_graph_slot_fill``): no read-back,
    no allocation inside the library, writes behind PyTorch's version counters.  On the CPU the same tables come from tensor
    operations: what the tests hold the kernels against, bit for bit."""

    is_slot = True

    def __init__(self, feats: int, cells: int, cell_rows: int, entry_cap: int, device="cuda"):
        if feats < 1 or cells < 1 or cell_rows < 1 or entry_cap < 0 or cells * cell_rows < 2 or cells * cell_rows >= 2 ** 31 - 1 or entry_cap >= 2 ** 31:
            raise ValueError("GraphSlot: feats >= 1, cells >= 1, cell_rows >= 1, at least 2 rows, entry_cap >= 0, all below 2^31")
        self.feats, self.cells, self.cell_rows, self.entry_cap = int(feats), int(cells), int(cell_rows), int(entry_cap)
        self.device = dev = torch.device(device)
        R = self.num_rows = self.cells * self.cell_rows
        self.x = torch.zeros((R, self.feats), dtype=torch.float32, device=dev)
        self.live = torch.zeros(R, dtype=torch.float32, device=dev)
        self.cell_live = torch.zeros(self.cells, dtype=torch.float32, device=dev)
        self.scalars = torch.zeros(2, dtype=torch.float32, device=dev)
        self.inv_cells, self.live_rows = self.scalars[0:1], self.scalars[1:2]
        self.labels = torch.full((self.cells,), -100, dtype=torch.int64, device=dev)
        ec = self.ec = object.__new__(ops.EdgeCSR)
        ec.num_nodes, ec.num_edges = R, self.entry_cap
        ec.rowptr = torch.zeros(R + 1, dtype=torch.int32, device=dev)
        ec.colptr = torch.zeros(R + 1, dtype=torch.int32, device=dev)
        ec.src = torch.zeros(max(self.entry_cap, 1), dtype=torch.int32, device=dev)
        ec.csc_dst = torch.zeros(max(self.entry_cap, 1), dtype=torch.int32, device=dev)
        ec.edge_w = torch.ones(max(self.entry_cap, 1), dtype=torch.float32, device=dev)
        ec.edge_w_csc = torch.ones(max(self.entry_cap, 1), dtype=torch.float32, device=dev)
        ec.perm = ec.csc_eid = ec.in_norm = ec.out_norm = None
        self.rp = ops.ReducePlan.from_ranges([(g * self.cell_rows, (g + 1) * self.cell_rows) for g in range(self.cells)], dev)
        self.sizes = [self.cell_rows] * self.cells             # (the tensor-operation path: every cell is a "slide" of cell_rows rows)
        self.num_real, self.real_sizes, self.num_entries = 0, [], 0
        self._seg = self._coo = self._desc = None

    # ---------------------------------------------------------------- what the model reads of a batch
    @property
    def num_graphs(self) -> int:
        return self.cells

    def segment(self) -> torch.Tensor:
        if self._seg is None:
            self._seg = torch.arange(self.cells, device=self.device).repeat_interleave(self.cell_rows)
        return self._seg

    def _entries(self):
        """(row, col, weight) of the loaded batch's entries in CSR order: the ``kernels=False`` path (it counts rowptr's ranges, which reads
        back on a GPU; the kernel path never comes here)."""
        if self._coo is None:
            E = self.num_entries
            counts = (self.ec.rowptr[1:] - self.ec.rowptr[:-1]).to(torch.int64)
            row = torch.arange(self.num_rows, device=self.device).repeat_interleave(counts)
            self._coo = (row, self.ec.src[:E].to(torch.int64), self.ec.edge_w[:E])
        return self._coo

    row = property(lambda self: self._entries()[0])
    col = property(lambda self: self._entries()[1])
    weight = property(lambda self: self._entries()[2])

    # ---------------------------------------------------------------- host arithmetic
    def fits(self, sizes: Sequence[int], entries: Sequence[int]) -> bool:
        """``sizes`` / ``entries``: rows and adjacency entries of a batch's slides.  True when there are at most ``cells`` slides, each of 1 to
        ``cell_rows`` rows, at most ``entry_cap`` entries in all - and at least 2 rows in all (BatchNorm refuses one value per channel)."""
        sizes, entries = [int(n) for n in sizes], [int(e) for e in entries]
        if not 1 <= len(sizes) <= self.cells or len(entries) != len(sizes):
            return False
        if any(not 1 <= n <= self.cell_rows for n in sizes) or any(e < 0 for e in entries):
            return False
        return sum(entries) <= self.entry_cap and sum(sizes) >= 2

    # ---------------------------------------------------------------- the fill
    def load(self, slides: SlideSet, idxs: Sequence[int], labels) -> "GraphSlot":
        """Write the slides ``idxs`` of ``slides`` with host labels ``labels`` into the slot's tables, on the current stream.  Raises
        ValueError when the batch does not fit (``fits``; fewer than 2 live rows included: the device cannot raise)."""
        idxs = [int(i) for i in idxs]
        labels = [int(v) for v in (labels.tolist() if isinstance(labels, torch.Tensor) else labels)]
        if len(labels) != len(idxs):
            raise ValueError(f"GraphSlot.load: {len(idxs)} slides but {len(labels)} labels")
        if slides.feats != self.feats or slides.device != self.device:
            raise ValueError("GraphSlot.load: the slide set and the slot disagree on feats or device")
        sizes, entries = [slides.sizes[i] for i in idxs], [slides.entries[i] for i in idxs]
        if not self.fits(sizes, entries):
            raise ValueError(f"the batch does not fit the slot ({len(sizes)} slides of {sizes} rows and {entries} entries; {self.cells} cells of "
                             f"{self.cell_rows} rows, {self.entry_cap} entries, at least 2 rows in all)")
        total, B = sum(entries), len(idxs)
        self.num_real, self.real_sizes, self.num_entries, self._coo = B, sizes, total, None
        if self.device.type != "cuda":
            self._load_tensor(slides, idxs, labels, sizes, entries)
            return self
        words, e0 = [], 0
        for i, lab, e in zip(idxs, labels, entries):
            words += slides._words[i]
            words += (e0, lab, 0, 0, 0, 0)
            e0 += e
        desc = ops.host_to_device(torch.frombuffer(array.array("q", words), dtype=torch.int64), torch.int64, self.device)
        ec = self.ec
        N.check(N.load().wsi_graph_slot_fill(N.ptr(desc), B, self.cells, self.cell_rows, self.feats, self.entry_cap, total,
                                             ctypes.c_float(1.0 / B), ctypes.c_float(float(sum(sizes))), N.ptr(self.x), N.ptr(self.live),
                                             N.ptr(self.cell_live), N.ptr(self.scalars), N.ptr(self.labels), N.ptr(ec.rowptr), N.ptr(ec.src),
                                             N.ptr(ec.edge_w), N.ptr(ec.colptr), N.ptr(ec.csc_dst), N.ptr(ec.edge_w_csc), N.stream()),
                "wsi_graph_slot_fill")
        self._desc = desc            # (stream-ordered: the table must outlive the launches; the next load replaces it behind them)
        return self

    def _load_tensor(self, slides: SlideSet, idxs, labels, sizes, entries) -> None:
        """The fill with tensor operations (the CPU path; the statement the kernels are tested against)."""
        ec, R, dev = self.ec, self.cell_rows, self.device
        with torch.no_grad():
            self.x.zero_()
            self.live.zero_()
            self.cell_live.zero_()
            self.labels.fill_(-100)
            e0 = 0
            for g, (i, n, e) in enumerate(zip(idxs, sizes, entries)):
                loc, a = slides.ec[i], g * R
                self.x[a:a + n] = slides.x[i]
                self.live[a:a + n] = 1.0
                ec.rowptr[a:a + n] = loc.rowptr[:n] + e0
                ec.colptr[a:a + n] = loc.colptr[:n] + e0
                ec.rowptr[a + n:a + R] = e0 + e                # dead rows: an empty range at the running entry offset
                ec.colptr[a + n:a + R] = e0 + e
                ec.src[e0:e0 + e] = loc.src + a
                ec.csc_dst[e0:e0 + e] = loc.csc_dst + a
                ec.edge_w[e0:e0 + e] = 1.0 if loc.edge_w is None else loc.edge_w
                ec.edge_w_csc[e0:e0 + e] = 1.0 if loc.edge_w_csc is None else loc.edge_w_csc
                e0 += e
            B = len(idxs)
            ec.rowptr[B * R:] = e0
            ec.colptr[B * R:] = e0
            self.cell_live[:B] = 1.0
            self.labels[:B] = torch.tensor(labels, dtype=torch.int64, device=dev)
            self.scalars.copy_(torch.tensor([ctypes.c_float(1.0 / B).value, float(sum(sizes))], dtype=torch.float32))


def slot_step(model, optimizer, slot: GraphSlot, params=None):
    """One training step on the batch a slot holds - the body of ``gtn.train_one_step`` with the slot's device-side labels and masks, gradients
    from ``torch.autograd.grad``: nothing in it is a host value of the batch, so it can be recorded.  Returns (loss, softmax [cells, n_class]),
    detached."""
    model.train()
    return capture.grad_step(optimizer, capture.trainable_params(optimizer) if params is None else params, lambda: model(slot, None)[2:])


class CapturedGraphStep:
    """One captured GTNMIL training step per ``GraphSlot``, replayed over new slides every step.  Protocol: ``capture.py``; EVERY slot takes
    its ``warmup`` (1) optimisation steps (on ``warmup_batches[i] = (slides, idxs, labels)`` for slot i; None: on what the caller has loaded
    into the slot) before the first capture, and a ``torch.nn.Dropout`` with p > 0 in train mode is refused.  Under a capture the
    projections keep their weight gradients on the capturing stream and the statistics stream is not used (``ops`` checks the capture
    itself), as for the other captured steps; no queue setting is touched.

    ``step(slides, idxs, labels)`` loads the smallest slot (fewest rows) that fits and replays; a batch no slot fits runs eagerly through
    ``gtn.train_one_step`` on ``slides.batch(idxs)`` and is counted in ``eager_steps``.  The reference steps a ``CosineAnnealingLR`` every epoch
    (``main_kfold*.py:118-157``).  A FLOAT ``lr`` is a host value frozen into a capture: ``recapture()`` records the graphs again, without
    stepping, after it changes.  A word - ``optim.Adam(..., lr=optim.lr_word(1e-3, device), capturable=True)`` - is read by every replay:
    ``torch.optim.lr_scheduler.*`` work on it unchanged (they ``fill_`` a tensor ``lr``; their arithmetic ends in one ``.item()`` per
    scheduler step, outside any capture) and nothing is recorded again.  Never rebind ``group["lr"]`` here (``capture.py``, point 8)."""

    def __init__(self, model: torch.nn.Module, optimizer: torch.optim.Optimizer, slots, warmup: int = 1, warmup_batches=None):
        from .GraphTransformer import Classifier
        slots = [slots] if isinstance(slots, GraphSlot) else list(slots)
        if not slots:
            raise ValueError("CapturedGraphStep: no slot")
        if not isinstance(model, Classifier) or not model.kernels:
            raise RuntimeError(f"CapturedGraphStep: {type(model).__name__} is not supported - gtn.Classifier on its kernel path")
        dev = slots[0].device
        if dev.type != "cuda" or any(s.device != dev for s in slots):
            raise RuntimeError("CapturedGraphStep: the slots must live on one GPU")
        if len({(s.feats, s.cells) for s in slots}) != 1:
            raise ValueError("CapturedGraphStep: the slots must agree on feats and cells")
        capture.require_capturable("CapturedGraphStep", optimizer)
        model.train()
        capture.counter_dropout_only("CapturedGraphStep", model)
        self.model, self.optimizer = model, optimizer
        self.slots, warmup_batches = capture.smallest_first(slots, lambda s: s.num_rows, warmup_batches)
        self.params = capture.trainable_params(optimizer)
        self.steps_taken, self.replays, self.eager_steps = 0, 0, 0
        for i, slot in enumerate(self.slots):
            capture.load_warm_up_batch("CapturedGraphStep", i, slot, warmup_batches)
            capture.warm_up(dev, warmup, lambda: slot_step(self.model, self.optimizer, slot, self.params))
            self.steps_taken += max(1, warmup)
        self.graphs, self.outputs = [], []
        self.recapture()

    def recapture(self) -> None:
        """Record every slot's graph again (no step is taken): after a change of a host-side hyper-parameter such as ``lr``."""
        self.graphs, self.outputs = [], []
        torch.cuda.synchronize(self.slots[0].device)
        for slot in self.slots:
            cg, out = capture.record("CapturedGraphStep", lambda: slot_step(self.model, self.optimizer, slot, self.params),
                                     self.graphs[-1].pool() if self.graphs else None, capture.step_failure("softmax"))
            self.graphs.append(cg)
            self.outputs.append(out)

    def slot_for(self, sizes: Sequence[int], entries: Sequence[int]):
        """Index of the smallest slot the batch fits, or None."""
        return capture.first_fit(self.slots, sizes, entries)

    def step(self, slides: SlideSet, idxs: Sequence[int], labels):
        """One optimisation step on the slides ``idxs`` of ``slides`` with host labels ``labels``.  Returns ``(loss, softmax[:len(idxs)])`` as
        device tensors; those of a replayed step are overwritten by the next replay of the same slot."""
        idxs = [int(i) for i in idxs]
        i = self.slot_for([slides.sizes[j] for j in idxs], [slides.entries[j] for j in idxs])
        self.steps_taken += 1
        if i is None:
            self.eager_steps += 1
            return self._eager(slides, idxs, labels)
        slot = self.slots[i]
        slot.load(slides, idxs, labels)
        self.graphs[i].replay()
        self.replays += 1
        loss, probs = self.outputs[i]
        return loss, probs[:slot.num_real]

    def _eager(self, slides: SlideSet, idxs: List[int], labels):
        """A batch no slot fits: ``gtn.train_one_step`` on the packed batch."""
        from .GraphTransformer import train_one_step
        labels = [int(v) for v in (labels.tolist() if isinstance(labels, torch.Tensor) else labels)]
        lab = ops.host_to_device(labels, torch.int64, slides.device)
        seen = []
        hook = self.model.register_forward_hook(lambda _m, _i, out: seen.append(out))
        try:
            loss = train_one_step(self.model, slides.batch(idxs), lab, self.optimizer)
        finally:
            hook.remove()
        return loss, seen[-1][3].detach()
