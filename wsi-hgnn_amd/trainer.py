"""The caller of the hot path: one optimisation step, mirroring ``GNNTrainer.train_one_step``
(trainer/train_gnn.py:55-79) on the MI355X path.

Differences from the reference, all on the caller side of the same semantics:
  * a tuple/list of heterogeneous graphs is block-diagonally batched and run as ONE forward (the reference loops
    ``[self.gnn(g) for g in graphs]`` and concatenates, :59-62) — identical logits, one set of launches;
  * with ``torch.distributed`` initialised, gradients are averaged over ranks with one flat RCCL all-reduce
    (``dist.GradBucket``) between ``backward`` and ``optimizer.step``;
  * loss / accuracy stay on the device unless ``sync=True`` (the reference's ``.item()`` / ``.cpu().numpy()`` at :73-79
    force a host sync every step).
The training loop, datasets, checkpointing and evaluators around it are out of scope.
"""
from __future__ import annotations

from typing import Optional, Sequence, Union

import torch
import torch.nn.functional as F

from . import capture
from .dist import GradBucket
from .graph import HeteroGraph, batch as batch_graphs


def acc(pred: torch.Tensor, label: torch.Tensor) -> torch.Tensor:
    """utils.py ``acc``: fraction of argmax hits (kept on the device)."""
    return (pred.argmax(dim=1) == label).to(torch.float32).mean()


def apply_loss(loss_fcn, pred: torch.Tensor, label: torch.Tensor) -> torch.Tensor:
    """``loss_fcn(pred, label)``; the reference's classification loss - ``nn.CrossEntropyLoss()`` with its defaults, parser.py:182-183 - on GPU logits
    runs as ONE launch forward and one backward (``ops.cross_entropy``: the same arithmetic) instead of torch's four kernels and two fills."""
    if (type(loss_fcn) is torch.nn.CrossEntropyLoss and loss_fcn.weight is None and loss_fcn.reduction == "mean" and loss_fcn.ignore_index == -100
            and loss_fcn.label_smoothing == 0.0 and pred.is_cuda and pred.dim() == 2 and pred.dtype == torch.float32 and label.dtype == torch.int64
            and label.dim() == 1 and pred.numel() <= 65536):
        from . import ops
        return ops.cross_entropy(pred, label)
    return loss_fcn(pred, label)


def train_one_step(gnn: torch.nn.Module, optimizer: torch.optim.Optimizer, loss_fcn, graphs: Union[HeteroGraph, Sequence[HeteroGraph]],
                   label: torch.Tensor, device, bucket: Optional[GradBucket] = None, sync: bool = True):
    """trainer/train_gnn.py:55-79.  Returns (loss, accuracy, pred, prob, label) — python float / numpy arrays when
    ``sync`` (as the reference), device tensors otherwise."""
    optimizer.zero_grad(set_to_none=True)                           # :56 (every parameter, inside or outside a bucket)
    label = label.to(device)                                        # :57
    if isinstance(graphs, (tuple, list)):                           # :59-62 heterogeneous graphs arrive as a tuple
        gs = [x.to(device) for x in graphs]
        same = all(x.ntypes == gs[0].ntypes and x.canonical_etypes == gs[0].canonical_etypes for x in gs[1:])
        if same:                                                    # one block-diagonal batch, one forward
            pred = gnn(batch_graphs(gs) if len(gs) > 1 else gs[0])
        else:                                                       # dgl.to_heterogeneous keeps only the relations that occur, so
            pred = torch.cat([gnn(x) for x in gs])                  # slides may differ in schema: per-graph forward as :61
    else:
        pred = gnn(graphs.to(device))                               # :64-65
    prob = F.softmax(pred, dim=1)                                   # :67
    loss = apply_loss(loss_fcn, pred, label)                        # :68
    if bucket is not None:
        bucket.arm()                                                # data parallel: reduce pieces of the gradient while backward runs
    loss.backward()                                                 # :70
    if bucket is not None:
        if bucket.world_size() > 1:
            bucket.check_outside(p for grp in optimizer.param_groups for p in grp["params"])
        bucket.all_reduce_mean()
    optimizer.step()                                                # :71
    accuracy = acc(pred, label)                                     # :73
    if not sync:
        return loss.detach(), accuracy, pred.detach().argmax(dim=1), prob.detach(), label
    bad = getattr(loss, "_wsi_bad_label", None)                      # ops.cross_entropy: a label outside [0, C) other than ignore_index
    if bad is not None and int(bad.item()):
        raise RuntimeError("train_one_step: a label lies outside [0, num_classes) (torch.nn.CrossEntropyLoss would trip its device assert)")
    return (loss.item(), float(accuracy.item()), pred.detach().cpu().numpy().argmax(axis=1),                # :75-79
            prob.detach().cpu().numpy(), label.detach().cpu().numpy())


def _seeded_step(optimizer, params, seed_base, compute):
    """``capture.grad_step`` with every dropout draw of forward and backward taken under the device word ``seed_base`` (None: no dropout),
    which the step then advances - part of the recorded step: the next replay draws other masks."""
    from . import ops
    with ops.dropout_seed_base(seed_base):
        out = capture.grad_step(optimizer, params, compute)
    if seed_base is not None:
        ops.advance_dropout_seed_base(seed_base)
    return out


class CapturedStep:
    """One training step (forward + loss + backward + optimizer) on a RESIDENT batch, captured once into a hipGraph and replayed.

    The reference trains slide by slide (``trainer/train_gnn.py:48-79``): the same few hundred graphs every epoch, each a step whose ~100 kernel
    launches the host takes longer to issue than the GPU to run (one 5k-node BRCA-shaped graph under HEATNet2: 1.80 ms eager, 0.83 ms replayed -
    ``tools/graph_capture_probe.py``).  Everything the step launches goes to the capturing stream - the library keeps no stream or state of its
    own, never allocates or synchronises (``include/wsi_hgnn.h``), and the hub kernels' side stream forks from and joins that stream with events -
    so the whole step records as one graph.  What the capture bakes in: the graph's kernel plan and every shape, i.e. one ``CapturedStep`` per
    resident batch (captures may share a memory ``pool``).  Protocol: ``capture.py`` - a capturable optimizer
    (``wsi_hgnn_amd.optim.Adam(..., capturable=True)``: the whole optimizer step is then ONE node of the graph; ``optim.SGD`` and
    ``optim.Adadelta`` read no count and are taken as they are; ``torch.optim``'s capturable optimizers work too), train-mode dropout only as
    the HEAT layers' counter-based draw, ``warmup`` (3) eager steps that ARE optimisation steps.  A model stepped eagerly before is fine - as
    long as the caller holds no tensor of those steps' autograd graphs any more (a previous loss, logits).  At the benchmark's size the step
    is GPU-bound and replay changes nothing (6.87 vs 6.93 ms).

    >>> step = CapturedStep(model, wsi_hgnn_amd.optim.Adam(model.parameters(), lr=1e-4, capturable=True), torch.nn.CrossEntropyLoss(), G, labels)
    >>> for _ in range(epochs): loss = step()          # a device tensor, overwritten by the next replay
    """

    def __init__(self, gnn: torch.nn.Module, optimizer: torch.optim.Optimizer, loss_fcn, graph: HeteroGraph, label: torch.Tensor,
                 warmup: int = 3, pool=None):
        from .models.heat_layer import HEATLayer
        if not label.is_cuda:
            raise RuntimeError("CapturedStep: the batch and its labels must be resident on the GPU")
        capture.require_capturable("CapturedStep", optimizer)
        self.seed_base = capture.new_seed_word(label.device) if capture.counter_dropout_only("CapturedStep", gnn, (HEATLayer,)) else None
        self.gnn, self.optimizer, self.loss_fcn, self.graph, self.label = gnn, optimizer, loss_fcn, graph, label
        self.params = capture.trainable_params(optimizer)
        self.cuda_graph = None
        capture.warm_up(label.device, warmup, self._eager)
        torch.cuda.synchronize(label.device)
        self.cuda_graph, self.loss = capture.record("CapturedStep", self._eager, pool, capture.step_failure("logits"))
        self.steps_taken = max(1, warmup)                  # (the capture records the step without executing it)

    def _eager(self) -> torch.Tensor:
        return _seeded_step(self.optimizer, self.params, self.seed_base, lambda: self.loss_fcn(self.gnn(self.graph), self.label))

    def __call__(self) -> torch.Tensor:
        self.cuda_graph.replay()
        self.steps_taken += 1
        return self.loss

    def pool(self):
        """The memory pool of this capture, for further ``CapturedStep(..., pool=...)`` over other resident batches."""
        return self.cuda_graph.pool()


def _check_slots(who: str, verb: str, gnn: torch.nn.Module, slots):
    """What a capture over batch slots needs of the model and the slots (``CapturedSlotStep``, ``CapturedSlotEval``): a HEAT trunk, HGT over
    slots that carry the per-relation-source plan, or GCN / GIN over homogeneous slots (one node type, one relation: the slot then keeps
    GraphConv's degree norms and, for GIN's BatchNorms, the live rows and their count current), with any readout ('att' runs from the slot's device tables, ``ops.attention_readout``); slots on the
    GPU fed by one loader.  Returns (slots as a list, their loader, its device)."""
    from .data import BatchSlot
    from .models.heat_net import HEATTrunk
    slots = [slots] if isinstance(slots, BatchSlot) else list(slots)
    if not slots:
        raise ValueError(f"{who}: no slot")
    if len({bool(getattr(s, "type_mask", False)) for s in slots}) > 1:
        raise ValueError(f"{who}: slots with and without type_mask are mixed - the slots of one capture share one presence table (DESIGN 3.29): "
                         "build all of them with BatchSlot(..., type_mask=True), or none")
    from .models.GCN import GCN
    from .models.GIN import GIN
    from .models.HGT import HGT
    from .pooling import GlobalAttentionPooling
    if type(gnn) is GIN:
        # GIN's BatchNorms take their statistics over the live rows the slot derives on the device behind every fill
        if not all(getattr(s, "live_rows", None) is not None for s in slots):
            raise RuntimeError(f"{who}: GIN needs homogeneous slots - a loader of graph.to_homogeneous slides (one node type, one relation) - "
                               f"or {verb} it eagerly")
        if any(s.type_mask for s in slots):
            raise ValueError(f"{who}: type_mask tells the heads of a heterogeneous model which node types a batch holds; GIN has one")
    elif type(gnn) is GCN:
        if not all(s.degree_norms is not None for s in slots):
            raise RuntimeError(f"{who}: GCN needs homogeneous slots - a loader of graph.to_homogeneous slides (one node type, one relation) - "
                               f"or {verb} it eagerly")
        if any(s.type_mask for s in slots):
            raise ValueError(f"{who}: type_mask tells the heads of a heterogeneous model which node types a batch holds; GCN has one")
    elif type(gnn) is HGT:
        # HGT's attention runs on the per-relation-source plan, which a slot re-derives on the device behind every fill - when it
        # was built with the tables for it
        if not all(getattr(s, "per_relation_src", False) for s in slots):
            raise RuntimeError(f"{who}: HGT needs slots that carry the per-relation-source plan - build every slot with "
                               f"BatchSlot(loader, capacity, per_relation_src=True) - or {verb} it eagerly")
    elif not isinstance(gnn, HEATTrunk):
        raise RuntimeError(f"{who}: {type(gnn).__name__} is not supported - HEATNet2 / HEATNet4, HGT over slots built with "
                           f"per_relation_src=True and GCN / GIN over homogeneous slots (HGT + ASAP and HeteroRGCN rebuild host-side structure per "
                           f"batch); {verb} it eagerly")
    if type(gnn) not in (GCN, GIN) and isinstance(gnn.pools[0], GlobalAttentionPooling) and gnn.pools[0].gate_nn.in_features != gnn.n_hid:
        # (the reference sizes pools[0]'s gate for in_dim and applies it to hidden_dim-wide node states, models/HEATNet4.py:182-187 and :219)
        raise RuntimeError(f"{who}: the attention readout's first gate reads {gnn.pools[0].gate_nn.in_features} columns but the node states it "
                           f"pools have {gnn.n_hid}: 'att' needs in_dim == hidden_dim; use a sum / mean / max readout")
    loader = slots[0].loader
    if any(s.loader is not loader for s in slots):
        raise ValueError(f"{who}: all slots must be fed by one loader")
    if loader.device.type != "cuda":
        raise RuntimeError(f"{who}: the slots must live on the GPU")
    return slots, loader, loader.device


def two_live_rows(slot, idxs: Sequence[int]) -> bool:
    """Will the batch ``idxs`` (one that fits) leave ``slot`` at least two live rows, which a train-mode BatchNorm over them needs (GIN; the
    device cannot raise)?  Plain slot: the stored node count n >= 2.  Augmented slot that drops nodes with probability p: fewer than two of n
    survive with probability p^n + n (1 - p) p^(n - 1), which must stay at or under 2 ** -32, the bound ``BatchSlot.fits`` holds its own
    rule to (n >= 38 at p = 0.5).  Quota slot: the node quotas must also sum to 2 or more."""
    n = sum(sum(slot.loader.items[i].num_nodes) for i in idxs)
    if n < 2:
        return False
    spec = slot.spec
    if spec is not None and spec.node_thr > 0:
        p = spec.node_thr / 65536.0
        if p ** n + n * (1.0 - p) * p ** (n - 1) > 2.0 ** -32:
            return False
    if slot.quota is not None and sum(sum(slot.quota_of(i)[0]) for i in idxs) < 2:
        return False
    return True


def _share_type_table(slots):
    """Slots built with ``type_mask``: rebind all of them to ONE presence table, the first slot's, and return it (else None).  Before any
    warm-up or capture: a recorded step reads the table its slot graph carried when it was recorded."""
    if not slots[0].type_mask:
        return None
    table = slots[0].type_present
    for s in slots[1:]:
        s.share_type_table(table)
    return table


def _gate_by_type(who: str, gnn: torch.nn.Module, optimizer, table: torch.Tensor) -> None:
    """``optimizer.gate(gnn.type_gated_parameters()[t], table, t)`` for every node type t: the parameters an eager step on a
    batch without the type leaves without a gradient are stepped only when ``table[t]`` says the type is there."""
    from . import optim as _optim
    if not isinstance(optimizer, _optim._OneLaunch):
        raise RuntimeError(f"{who}: slots with type_mask need a wsi_hgnn_amd.optim optimizer (Adam / Adagrad with capturable=True, SGD, Adadelta): "
                           f"a captured step hands the head of an absent node type exact zero gradients where the eager step hands it None, and "
                           f"{type(optimizer).__module__}.{type(optimizer).__name__} cannot skip a tensor on a device-side word - "
                           "wsi_hgnn_amd.optim's one-launch step can (optimizer.gate)")
    stepped = {id(p) for g in optimizer.param_groups for p in g["params"]}
    gated = [[p for p in params if id(p) in stepped] for params in gnn.type_gated_parameters()]
    optimizer.gate([p for params in gated for p in params], None)          # (an earlier capture's table: one optimizer reads one)
    for t, params in enumerate(gated):
        if params:
            optimizer.gate(params, table, t)


def _first_slide(who: str, i: int, slot, also=None):
    """The default warm-up batch of slot ``i``: the first slide of the data set that fits it alone (and passes ``also(slot, [j])``)."""
    first = next(([j] for j in sorted(slot.members) if slot.fits([j]) and (also is None or also(slot, [j]))), None)
    if first is None:
        raise ValueError(f"{who}: no slide of the data set fits slot {i}")
    return first


class CapturedSlotStep:
    """One captured training step per batch SLOT (``data.BatchSlot``), replayed over NEW slides every step: the regime the reference trains in
    (one or two slides per step, ``trainer/train_gnn.py:48-79``), where the host takes longer to issue the step's launches than the GPU to run them.
    ``CapturedStep`` bakes a resident batch into its graph; a slot's tables have one shape for every batch that fits, so one capture serves them
    all.  Per step the host uploads one descriptor table, launches one fill kernel into the slot's static tables and replays.

    ``slots``: one ``BatchSlot`` or several of different capacity over the same loader (small slides then do not pay for the largest);
    ``step(idxs)`` takes the smallest slot (fewest node rows) that fits.  A batch no slot fits runs eagerly through the loader's ordinary
    assembly.  Protocol: ``capture.py``; slot by slot the ``warmup`` (1) optimisation steps run on ``warmup_batches[i]`` (default: the slot's
    first fitting batch of one slide) and the slot is captured before the next one warms up; train-mode dropout may be the HEAT and the HGT
    layers' counter-based draw, GCN's or GIN's inter-layer one (all slots advance ONE device word).  HEATNet2 / HEATNet4, HGT over
    slots built with ``per_relation_src=True`` (the slot re-derives HGT's plan on the device behind every fill), and GCN / GIN
    over homogeneous slots, with a sum / mean / max readout or the attention readout ('att': one pass over the slot's
    readout tables); HGT + ASAP and HeteroRGCN rebuild host-side structure - those are refused.

    GIN in train mode: its BatchNorms run over the slot's live rows, counted on the device, and need two of them - the device cannot raise,
    so ``slot_for`` sends a batch that might leave fewer to the eager route (``two_live_rows``).

    Slots over a loader with a slot-compatible ``transform=`` (``data.slot_augment_spec``) are AUGMENTED: every ``step`` fills its slot with a fresh
    draw taken on the device (no read-back) in front of the replay, a batch no slot fits goes through ``loader._augmented``, and either way the
    loader's batch counter advances exactly once per step - under one seed the trajectory follows the eager loader's draws.

    ``metrics``: a ``metrics.EpochMetrics`` on the slots' device; the recorded step and the eager one then end with
    ``metrics.update(logits, labels)`` - the reference's per-epoch training metrics (``train_gnn.py:73-79,104-108``) with no read-back per step
    (the warm-up steps count too: ``metrics.reset()`` where the epoch starts).  ``None``: the recorded step is exactly what it was.

    Slots built with ``type_mask=True`` (all of them or none) also take batches that lack a node type, and augmented ones
    batches a draw can empty of one: the slots are rebound to ONE presence table (the first slot's), every fill re-derives it on the device,
    the heads multiply by it, and ``optimizer.gate(gnn.type_gated_parameters()[t], table, t)`` keeps the parameters that an eager step would
    leave without a gradient - weights, moments and step counts - exactly as they were.  This needs a ``wsi_hgnn_amd.optim`` optimizer
    (torch's capturable ones cannot skip a tensor and are refused); the eager fallback sets the table to ones before it steps."""

    def __init__(self, gnn: torch.nn.Module, optimizer: torch.optim.Optimizer, loss_fcn, slots, warmup: int = 1, warmup_batches=None, metrics=None):
        self.slots, self.loader, dev = _check_slots("CapturedSlotStep", "step", gnn, slots)
        if metrics is not None and metrics.device != dev:
            raise RuntimeError(f"CapturedSlotStep: metrics= must live on the slots' device ({dev})")
        self.metrics = metrics
        from .models.heat_layer import HEATLayer
        from .models.HGT import HGTLayer
        from .models.GCN import GCN
        from .models.GIN import GIN
        capture.require_capturable("CapturedSlotStep", optimizer)
        # slots with a presence table: one table for all of them, and the optimizer gated on it
        self.type_table = _share_type_table(self.slots)
        if self.type_table is not None:
            _gate_by_type("CapturedSlotStep", gnn, optimizer, self.type_table)
        # (an HGTLayer, and GCN's and GIN's inter-layer dropout, draw counter-based whenever a seed base is active, which it is throughout this
        # class's steps)
        self.seed_base = capture.new_seed_word(dev) if capture.counter_dropout_only("CapturedSlotStep", gnn, (HEATLayer, HGTLayer, GCN, GIN)) else None
        self.two_rows = type(gnn) is GIN
        self.gnn, self.optimizer, self.loss_fcn = gnn, optimizer, loss_fcn
        self.slots, warmup_batches = capture.smallest_first(self.slots, lambda s: s.layout.N, warmup_batches)
        self.params = capture.trainable_params(optimizer)
        self.steps_taken, self.replays, self.eager_steps = 0, 0, 0
        self.graphs, self.outputs = [], []
        for i, slot in enumerate(self.slots):
            slot.load(list(warmup_batches[i]) if warmup_batches is not None else
                      _first_slide("CapturedSlotStep", i, slot, two_live_rows if self.two_rows and gnn.training else None))
            body = lambda: self._eager(slot.graph, slot.labels)
            capture.warm_up(dev, warmup, body)
            self.steps_taken += max(1, warmup)
            torch.cuda.synchronize(dev)
            cg, out = capture.record("CapturedSlotStep", body, self.graphs[-1].pool() if self.graphs else None, capture.step_failure("logits"))
            self.graphs.append(cg)
            self.outputs.append(out)

    def _eager(self, graph: HeteroGraph, label: torch.Tensor):
        def compute():
            pred = self.gnn(graph)
            return self.loss_fcn(pred, label), pred
        loss, pred = _seeded_step(self.optimizer, self.params, self.seed_base, compute)
        if self.metrics is not None:
            self.metrics.update(pred, label)
        return loss, pred

    def slot_for(self, idxs: Sequence[int]):
        """Index of the smallest slot the batch fits, or None.  GIN in train mode: of the slots that leave its BatchNorms two live rows
        (``two_live_rows``)."""
        if self.two_rows and self.gnn.training:
            idxs = list(idxs)
            return next((i for i, slot in enumerate(self.slots) if slot.fits(idxs) and two_live_rows(slot, idxs)), None)
        return capture.first_fit(self.slots, idxs)

    def overflows(self) -> int:
        """Fills, over all slots, in which a survivor quota bound and the batch was truncated (``BatchSlot.overflows``; 0 for slots without
        quotas).  A read-back per slot: once per epoch, not per step."""
        return sum(slot.overflows() for slot in self.slots)

    def step(self, idxs: Sequence[int]):
        """One optimisation step on the loader's slides ``idxs``.  Returns ``(loss, logits[:len(idxs)])`` as device tensors; those of a replayed
        step are overwritten by the next replay of the same slot."""
        idxs = list(idxs)
        i = self.slot_for(idxs)
        self.steps_taken += 1
        if i is None:                                          # fits no slot: the loader's ordinary batch, stepped eagerly
            if self.loader.transform is not None:              # (augmented: the general route; it advances the loader's batch counter as a fill does)
                G, labels = self.loader._augmented(idxs)
            else:
                G, labels, ready = self.loader._assemble(idxs, 0)
                if ready is not None:
                    torch.cuda.current_stream(self.loader.device).wait_event(ready)
            self.eager_steps += 1
            if self.type_table is not None:                    # the loader's unpadded batch: the model reads no table and an absent head has no
                self.type_table.fill_(1.0)                     # gradient of its own - every gate open
            return self._eager(G, labels)
        slot = self.slots[i]
        slot.load(idxs)
        self.graphs[i].replay()
        self.replays += 1
        loss, pred = self.outputs[i]
        return loss, pred[:slot.num_real]


class CapturedSlotEval:
    """The forward of an evaluation pass captured once per batch SLOT and replayed over the data set: what the reference does after every epoch,
    one slide at a time (``trainer/train_gnn.py:110-115``, ``evaluator/eval_homo_graph.py:61-95``) - the same host-bound regime as its training
    step.  Each slot's graph records ``pred = gnn(slot.graph); metrics.update(pred, slot.labels)`` in eval mode under ``no_grad``; ``evaluate``
    fills and replays batch after batch and reads the epoch's numbers back ONCE (``metrics.EpochMetrics.compute``).  The filler and the empty
    graphs of a slot are labelled -100 and are not counted.  Protocol: ``capture.py``, slot by slot as ``CapturedSlotStep``.

    The recorded forward reads the LIVE parameters: under a stream capture every projection packs its own weights (``ops.repack_weights``), the
    statistics stream is not used, and the eval-mode forward keeps no other table that depends on a parameter - an optimizer step between two
    ``evaluate`` calls changes the result as it must.  A training capture (``CapturedSlotStep``) lives beside this one on slots and a memory
    pool of its own.

    Slots built with ``type_mask=True`` (all or none) are rebound to one presence table and also take batches that lack a node
    type; nothing else changes.

    Refused: what ``CapturedSlotStep`` refuses (HGT on slots without the per-relation plan, slots off the GPU or over several loaders), and slots over a loader
    with ``transform=`` - evaluation sees the stored slides (the reference augments ``type_ == "train"`` only, data.py:116-117).
    ``metrics=None`` builds an ``EpochMetrics`` for ``len(loader.items)`` rows."""

    def __init__(self, gnn: torch.nn.Module, slots, metrics=None, warmup: int = 1):
        self.slots, self.loader, dev = _check_slots("CapturedSlotEval", "evaluate", gnn, slots)
        if self.loader.transform is not None:
            raise RuntimeError("CapturedSlotEval: the slots' loader has a transform=; evaluation sees the stored slides - build the slots over a "
                               "loader without one")
        self.gnn = gnn
        self.slots = sorted(self.slots, key=lambda s: s.layout.N)                      # smallest first: what run() tries in turn
        self.type_table = _share_type_table(self.slots)                                # (slots with type_mask: one presence table)
        self.replays, self.eager_runs = 0, 0
        self.graphs, self.outputs = [], []
        with capture.eval_mode(gnn):
            firsts = [_first_slide("CapturedSlotEval", i, slot) for i, slot in enumerate(self.slots)]
            if metrics is None:
                from .metrics import EpochMetrics
                slot = self.slots[0].load(firsts[0])
                metrics = EpochMetrics(gnn(slot.graph).shape[1], len(self.loader.items), dev)
            elif metrics.device != dev:
                raise RuntimeError(f"CapturedSlotEval: metrics= must live on the slots' device ({dev})")
            self.metrics = metrics
            for slot, first in zip(self.slots, firsts):
                slot.load(first)
                body = lambda: self._eager(slot.graph, slot.labels)
                capture.warm_up(dev, warmup, body)
                torch.cuda.synchronize(dev)
                cg, out = capture.record("CapturedSlotEval", body, self.graphs[-1].pool() if self.graphs else None,
                                         "the forward could not be captured into a hipGraph; evaluate eagerly (io.evaluate) instead")
                self.graphs.append(cg)
                self.outputs.append(out)
            metrics.reset()                                        # (the warm-up forwards counted their rows)

    def _eager(self, graph: HeteroGraph, label: torch.Tensor) -> torch.Tensor:
        pred = self.gnn(graph)
        self.metrics.update(pred, label)
        return pred

    def slot_for(self, idxs: Sequence[int]):
        """Index of the smallest slot the batch fits, or None."""
        return capture.first_fit(self.slots, idxs)

    def run(self, idxs: Sequence[int]) -> torch.Tensor:
        """The logits ``[len(idxs), C]`` of the loader's slides ``idxs`` (a device tensor; those of a replay are overwritten by the next replay of
        the same slot), their rows appended to ``metrics``.  A batch no slot fits runs eagerly through the loader's ordinary assembly."""
        idxs = list(idxs)
        i = self.slot_for(idxs)
        if i is None:
            with capture.eval_mode(self.gnn):
                G, labels, ready = self.loader._assemble(idxs, 0)
                if ready is not None:
                    torch.cuda.current_stream(self.loader.device).wait_event(ready)
                self.eager_runs += 1
                return self._eager(G, labels)
        slot = self.slots[i]
        slot.load(idxs)
        self.graphs[i].replay()
        self.replays += 1
        return self.outputs[i][:slot.num_real]

    def batches(self):
        """The default batches of ``evaluate``: every schema bucket's slides in stored order, ``loader.batch_size`` at a time."""
        bs = self.loader.batch_size
        return [ix[k:k + bs] for ix in self.loader.buckets.values() for k in range(0, len(ix), bs)]

    def evaluate(self, batches=None, average: str = "binary"):
        """``metrics.reset()``, every batch through ``run``, ``metrics.compute(average)``: the keys of ``io.evaluate`` plus ``"n"``.  One read-back."""
        self.metrics.reset()
        for idxs in (self.batches() if batches is None else batches):
            self.run(idxs)
        return self.metrics.compute(average)
