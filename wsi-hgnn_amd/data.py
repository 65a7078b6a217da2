"""Batched graph loader — the MI355X replacement for the reference's ``GraphDataLoader`` use
(trainer/train_gnn.py:48-53: ``batch_size``, ``shuffle=True``, ``drop_last=False``) and for the per-step
``g.to(device)`` of trainer/train_gnn.py:60,64.

The reference moves every graph host->device inside the step (a 10k-node WSI graph is 41 MB of 1024-d features) and
runs one forward per graph.  Sized for 288 GB of HBM3E instead:

* ``resident=True`` (default when the data set fits in half of the free HBM — a 1000-slide TCGA cohort is ~41 GB):
  every graph's features and packed edge arrays are uploaded ONCE; a batch is assembled by device-to-device copies
  straight into the kernels' type-major ``[N, F]`` layout (no PCIe traffic in the step at all);
* ``resident=False``: features stay in pinned host memory and a side HIP stream copies each (graph, node type) block
  into its slice of one of two alternating device buffers while the previous step computes (events order buffer reuse).

Either way the CSR/CSC kernel plan of the batch is assembled on the device from per-graph, per-node-type PIECES of each
graph's own plan (``graph.PlanPieces``, built once per stored graph): the batch layout is type-major and block-diagonal,
so the plan of a batch is a concatenation of pieces plus offset additions — ~45 small launches, **no sort**, no host
sync — and the returned ``HeteroGraph`` carries the plan, the CSR-ordered ``sim`` and the already-concatenated feature
table, so the model does no further preprocessing.
``transform=`` (``transforms.Compose`` ...) augments every slide drawn for a batch on the loader's device, as the reference's TRAINING data set
does each time a graph is loaded (data.py:16-23,116-117); such batches take the general route (``graph.batch``, then the model's ``plan()``)
because the stored pieces describe the unaugmented slide.  Evaluation loaders take no transform: the reference augments ``type_ == "train"`` only.
Dataset parsing (DGL pickles, labels from TCGA barcodes — data.py:67-123) stays out of scope; graphs arrive as
``HeteroGraph`` objects (see INTEGRATION.md for the one-off DGL conversion).
"""
from __future__ import annotations

from collections import OrderedDict
from typing import Iterator, List, Optional, Sequence, Tuple

import torch

from . import graph as _graph_mod
from .graph import HeteroGraph, PlanHeader, PlanPieces, _resolve_device, assemble_plan, host_to_device


def augment_draw(seed: int, counter: int, slide: int) -> int:
    """The 32-bit draw of slide number ``slide`` in batch number ``counter`` (running over the loader's life) of a loader seeded with ``seed``."""
    from .ops import _fmix32
    return _fmix32(_fmix32(_fmix32(int(seed)) + int(counter) * 0x9E3779B1) + int(slide) * 0x85EBCA6B)


class StoredGraph:
    """One WSI graph in loader form: per-type features + the per-node-type pieces of its own kernel plan."""

    def __init__(self, g: HeteroGraph, label: int, device: torch.device, resident: bool):
        self.ntypes = g.ntypes
        self.rels = g.canonical_etypes
        self.num_nodes = [g.num_nodes(t) for t in self.ntypes]
        self.label = int(label)
        # the graph's own kernel plan, cut into per-node-type pieces (device-resident, ~2 MB per 10k-node graph)
        edges = OrderedDict((r, tuple(x.to(device) for x in g.edges(r))) for r in self.rels)
        # (a graph without the ``sim`` edge field - graph.to_homogeneous output, which GraphConv reads no edge field of - stores zeros)
        sims = {r: (g._eframes[r]["sim"].to(device=device, dtype=torch.float32) if "sim" in g._eframes[r]
                    else torch.zeros(edges[r][0].numel(), dtype=torch.float32, device=device)) for r in self.rels}
        topo = HeteroGraph.from_coo(OrderedDict(zip(self.ntypes, self.num_nodes)), edges, sim=sims)
        self.edges, self.sims = edges, sims      # per-relation COO (local ids): the batch's COO is an offset-concat of these, built
        plan = topo.plan()                       # only if something asks for it (HeteroGraph._edges)
        self.num_edges = plan.num_edges
        pos = None
        if all("_pos" in g.nodes[t].data for t in self.ntypes) and _graph_mod.LOCALITY:   # graph.apply_locality_order was applied to this slide (same switch as graph._build_plan)
            pos = torch.cat([g.nodes[t].data["_pos"].reshape(-1) for t in self.ntypes])
        self.pieces = PlanPieces(PlanHeader(self.ntypes, self.rels, self.num_nodes), plan, topo.cat_edata_csr("sim"), pos)
        self.max_in_degree = self.pieces.max_in_degree
        feats = [g.nodes[t].data["feat"].to(torch.float32).contiguous() for t in self.ntypes]
        if resident:
            place = lambda x: x.to(device)
        elif device.type == "cuda":
            place = lambda x: x.pin_memory()
        else:
            place = lambda x: x
        self.feat = [place(f) for f in feats]
        self.bytes = sum(f.numel() * 4 for f in feats)
        self._feat_scale: List[Optional[torch.Tensor]] = [None] * len(feats)

    def feat_scale(self, t: int) -> torch.Tensor:
        """Row scales (absmax bits, ops.row_absmax) of the resident features of node type ``t``: taken once per stored graph."""
        if self._feat_scale[t] is None:
            from . import ops
            self._feat_scale[t] = ops.row_absmax(self.feat[t]) if self.feat[t].shape[0] else torch.empty((0, 1), dtype=torch.int32, device=self.feat[t].device)
        return self._feat_scale[t]


def _batch_coo(its: Sequence[StoredGraph], ntypes, rels):
    """Per-relation COO and ``sim`` of the block-diagonal batch of ``its`` (what ``graph.batch`` would hold): every stored
    graph's local ids shifted by the number of same-type nodes of the graphs before it.  Needed only by consumers that
    re-derive structure from the edges (HGT's per-relation-source plan, ``to_homogeneous``, ``batch``, ``save_graph``);
    the HEAT path runs on the assembled plan and never calls this."""
    tindex = {t: i for i, t in enumerate(ntypes)}
    off = [[0] * len(ntypes)]
    for it in its:
        off.append([a + b for a, b in zip(off[-1], it.num_nodes)])
    edges, efields = OrderedDict(), {}
    for r in rels:
        si, di = tindex[r[0]], tindex[r[2]]
        edges[r] = (torch.cat([it.edges[r][0] + off[b][si] for b, it in enumerate(its)]),
                    torch.cat([it.edges[r][1] + off[b][di] for b, it in enumerate(its)]))
        efields[r] = {"sim": torch.cat([it.sims[r] for it in its])}
    return edges, efields


class GraphBatchLoader:
    """Iterates over (batched HeteroGraph on ``device``, labels on ``device``)."""

    def __init__(self, graphs: Sequence[HeteroGraph], labels: Sequence[int], batch_size: int, device,
                 shuffle: bool = True, drop_last: bool = False, seed: int = 611, resident: Optional[bool] = None, passes: int = 1,
                 assemble_on_side_stream: bool = False, transform=None):
        """``transform``: a callable ``(HeteroGraph, draw=seed) -> HeteroGraph`` (``transforms.reference_train_transform()``) applied to every
        slide each time it is drawn, on ``device`` (pinned-host data sets: after the transfer), with the draw ``augment_draw(seed, running batch
        counter, slide index)``: two loaders with one seed yield identical batches, successive passes different ones.  ``None`` (default, and what an
        evaluation loader passes): the stored slides, through the assembled-plan path."""
        if len(graphs) != len(labels):
            raise ValueError("graphs and labels differ in length")
        if len(graphs) == 0:
            raise ValueError("empty data set")
        self.device = _resolve_device(device)          # 'cuda' -> 'cuda:<current>': devices compare by value downstream
        total = sum(g.num_nodes(t) * g.nodes[t].data["feat"].shape[1] * 4 for g in graphs for t in g.ntypes)
        if resident is None:
            free = torch.cuda.mem_get_info(self.device)[0] if self.device.type == "cuda" else 0
            resident = total < 0.5 * free
        self.resident = bool(resident)
        self.items = [StoredGraph(g, y, self.device, self.resident) for g, y in zip(graphs, labels)]
        # Slides may differ in schema (dgl.to_heterogeneous keeps only the relations that occur, and an ABSENT relation is not
        # an EMPTY one: the cross-relation mean's denominator differs), and only same-schema graphs can be batched
        # block-diagonally: every batch is drawn from one schema bucket (the reference runs such graphs one by one,
        # trainer/train_gnn.py:59-62, which is the batch-size-1 case of the same thing).
        self.buckets = OrderedDict()
        for i, it in enumerate(self.items):
            self.buckets.setdefault((tuple(it.ntypes), tuple(it.rels)), []).append(i)
        self.batch_size, self.shuffle, self.drop_last = int(batch_size), shuffle, drop_last
        # one iterator = ``passes`` (re-shuffled) passes over the data set: the prefetch crosses the boundary between them.  (The first batch of an
        # iterator has nothing in front of it to hide its transfer behind; with a handful of batches per pass - bench.py --pcie: two - that start-up
        # cost is paid every other step.)
        self.passes = max(1, int(passes))
        self.gen = torch.Generator().manual_seed(seed)
        self.transform, self.seed, self._batches_drawn = transform, int(seed), 0
        self.in_dim = self.items[0].feat[0].shape[1]
        # pinned-host mode: the transfers travel on ops' "work" side stream - idle while this loader feeds steps (it blocks the side streams then,
        # __iter__) - rather than on one more stream of its own: a fourth hardware queue in use stretches the step (ops._SIDE_STREAMS)
        self.copy_stream = None
        if not self.resident:
            from . import ops
            self.copy_stream = ops.side_stream(self.device, "work")
        # device-resident data set: the NEXT batch (feature concatenation + kernel plan, ~50 small kernels and one 328 MB copy) is put together
        # in line on the caller's stream, behind the step just enqueued.  ``assemble_on_side_stream=True`` moves it to a side stream; measured in round 4
        # (bench.py --pcie, hbm_resident, same box) that is the SLOWER choice - 7.86 vs 7.52 ms per step: the side stream has to start behind the
        # caller's stream anyway (the stored graphs' tensors may have work pending there), so nothing overlaps and the hand-over costs - and beside
        # the background weight gradients (ops._gemm_tn_background, a second side stream) it doubled the step (14.1 ms); with it the loader
        # therefore keeps those launches in order
        self.side_stream = (torch.cuda.Stream(device=self.device)
                            if self.resident and self.device.type == "cuda" and assemble_on_side_stream else None)
        if self.side_stream is not None:
            from . import ops
            ops.block_background_weight_gradients(True, who="loader")
        self._bufs: List[Optional[torch.Tensor]] = [None, None]
        self._free_evt: List[Optional[torch.cuda.Event]] = [None, None]

    def __len__(self) -> int:
        bs = self.batch_size
        return self.passes * sum(len(ix) // bs if self.drop_last else (len(ix) + bs - 1) // bs for ix in self.buckets.values())

    # ------------------------------------------------------------------ batch assembly
    def _assemble(self, idxs: List[int], slot: int):
        its = [self.items[i] for i in idxs]
        ntypes, rels = its[0].ntypes, its[0].rels
        B, T = len(its), len(ntypes)
        dev = self.device
        counts = [[it.num_nodes[t] for it in its] for t in range(T)]
        hd = PlanHeader(ntypes, rels, [sum(c) for c in counts])
        n = hd.N
        # ---- features -> type-major [N, F] buffer
        ready = None
        if self.resident and self.side_stream is not None:
            main = torch.cuda.current_stream(dev)
            # the stored graphs' tensors may still have work pending on the caller's stream (graphs handed over already on the
            # device are kept as they are; first-use scale scans): the side stream starts behind it
            self.side_stream.wait_stream(main)
            with torch.cuda.stream(self.side_stream):
                feat = torch.empty((n, self.in_dim), dtype=torch.float32, device=dev)
                self._copy_features(feat, its, hd)
                scales = self._cat_feature_scales(its, hd, n, dev)
                plan, sim = assemble_plan(hd, [it.pieces for it in its], dev, counts)
                labels = host_to_device([it.label for it in its], torch.int64, dev)
                ready = torch.cuda.Event()
                ready.record(self.side_stream)
            # allocated under the side stream, consumed on the caller's: the caching allocator must not hand this memory to the next
            # side-stream assembly while the caller's kernels still read it
            for t_ in [feat, sim, labels, scales] + [v for v in vars(plan).values() if isinstance(v, torch.Tensor)]:
                if t_ is not None and t_.is_cuda:
                    t_.record_stream(main)
        elif self.resident:
            feat = torch.empty((n, self.in_dim), dtype=torch.float32, device=dev)
            self._copy_features(feat, its, hd)
            scales = self._cat_feature_scales(its, hd, n, dev)
            plan, sim = assemble_plan(hd, [it.pieces for it in its], dev, counts)
            labels = host_to_device([it.label for it in its], torch.int64, dev)
        else:
            with torch.cuda.stream(self.copy_stream):
                if self._free_evt[slot] is not None:
                    self.copy_stream.wait_event(self._free_evt[slot])    # the step that read this buffer has finished
                buf = self._bufs[slot]
                if buf is None or buf.shape[0] < n:
                    buf = self._bufs[slot] = torch.empty((int(n * 1.1) + 1, self.in_dim), dtype=torch.float32, device=dev)
                feat = buf[:n]
                self._copy_features(feat, its, hd)
                # ---- kernel plan of the batch from the stored pieces (no sort, no sync), on the copy stream as well
                plan, sim = assemble_plan(hd, [it.pieces for it in its], dev, counts)
                labels = host_to_device([it.label for it in its], torch.int64, dev)
                ready = torch.cuda.Event()
                ready.record(self.copy_stream)
            scales = None
            main = torch.cuda.current_stream(dev)
            for t_ in [sim, labels] + [v for v in vars(plan).values() if isinstance(v, torch.Tensor)]:
                if t_ is not None and t_.is_cuda:
                    t_.record_stream(main)       # (the feature buffers are persistent and guarded by events instead)
        # ---- the graph object the models consume
        nn_ = OrderedDict((t, hd.counts[i]) for i, t in enumerate(ntypes))
        G = HeteroGraph._from_plan(nn_, rels, {t: torch.tensor(counts[i], dtype=torch.int64) for i, t in enumerate(ntypes)},
                                   plan, lambda: _batch_coo(its, ntypes, rels))
        parts = []
        for i, t in enumerate(ntypes):
            v = feat[hd.type_off[i]:hd.type_off[i + 1]]
            G._nframes[t]["feat"] = v
            parts.append(v)
        sig = tuple((p.data_ptr(), tuple(p.shape), p.dtype, p._version) for p in parts)
        cache = G.__dict__.setdefault("_cat_cache", {})
        cache["feat"] = (sig, feat)                       # the type-major table already IS the concatenation
        cache[("e", "sim")] = ((), sim)                   # CSR-ordered; valid while the per-relation fields are untouched
        if scales is not None:                            # fp16x3 / auto: the input projection finds the features' row scales ready
            from . import ops
            ops.attach_row_scales(feat, scales)
        return G, labels, ready

    def _cat_feature_scales(self, its, hd, n, dev) -> Optional[torch.Tensor]:
        """Resident data set under a scaled GEMM arithmetic: the row scales of the batch's feature table, concatenated from the
        stored graphs' own (each scanned once, at its first use) in the table's type-major order."""
        from . import ops
        if dev.type != "cuda" or not ops.scaled_gemm_mode():
            return None
        scales = torch.empty((n, 1), dtype=torch.int32, device=dev)
        for t in range(len(hd.ntypes)):
            a, b = hd.type_off[t], hd.type_off[t + 1]
            if b > a:
                torch.cat([it.feat_scale(t) for it in its], dim=0, out=scales[a:b])
        return scales

    def _copy_features(self, feat, its, hd) -> None:
        if self.resident:
            # device-resident data set: one concatenation KERNEL per node type.  (Per-block ``copy_`` calls are D2D
            # hipMemcpyAsync's that the runtime sometimes routes through the slow SDMA engine: sporadic 50 ms stalls.)
            for t in range(len(hd.ntypes)):
                a, b = hd.type_off[t], hd.type_off[t + 1]
                if b > a:
                    torch.cat([it.feat[t] for it in its], dim=0, out=feat[a:b])
            return
        for t in range(len(hd.ntypes)):
            row = hd.type_off[t]
            for it in its:
                k = it.num_nodes[t]
                if k:
                    feat[row:row + k].copy_(it.feat[t], non_blocking=True)
                row += k

    def _augmented(self, idxs: List[int]):
        """A batch of augmented slides: every slide as a single graph on the device, ``transform`` with its own draw, then the general route -
        ``graph.batch``; the model builds the plan (``HeteroGraph.plan``).  The stored pieces describe the unaugmented slide and are not used."""
        dev = self.device
        counter, self._batches_drawn = self._batches_drawn, self._batches_drawn + 1
        gs = []
        for i in idxs:
            it = self.items[i]
            feats = it.feat if self.resident else [f.to(dev, non_blocking=True) for f in it.feat]
            g = HeteroGraph.from_coo(OrderedDict(zip(it.ntypes, it.num_nodes)), it.edges, feat=dict(zip(it.ntypes, feats)), sim=it.sims)
            gs.append(self.transform(g, draw=augment_draw(self.seed, counter, i)))
        return _graph_mod.batch(gs), host_to_device([self.items[i].label for i in idxs], torch.int64, dev)

    def __iter__(self) -> Iterator[Tuple[HeteroGraph, torch.Tensor]]:
        batches = []
        for _ in range(self.passes):
            one = []
            for ix in self.buckets.values():
                order = [ix[j] for j in torch.randperm(len(ix), generator=self.gen).tolist()] if self.shuffle else list(ix)
                bb = [order[i:i + self.batch_size] for i in range(0, len(order), self.batch_size)]
                if self.drop_last and bb and len(bb[-1]) < self.batch_size:
                    bb.pop()
                one += bb
            if self.shuffle and len(self.buckets) > 1:
                one = [one[j] for j in torch.randperm(len(one), generator=self.gen).tolist()]
            batches += one
        if not batches:
            return
        if self.transform is not None:
            for idxs in batches:
                yield self._augmented(idxs)
            return
        # pinned-host mode: while this iterator feeds steps, every launch of those steps stays on the caller's stream (ops.block_side_streams: beside
        # H2D transfers a second compute stream stretches the step from 6.7 to 10 ms; the transfer bounds it at ~6 ms either way)
        pinned = not self.resident and self.device.type == "cuda"
        who = f"loader-{id(self)}"
        if pinned:
            from . import ops
            ops.block_side_streams(True, who)
        try:
            slot = 0
            nxt = self._assemble(batches[0], slot)
            for bi in range(len(batches)):
                G, labels, ready = nxt
                used = slot
                # pinned-host mode: the NEXT batch is put together BEFORE this one is handed over - its H2D copies are then already queued on the
                # copy stream (behind the event of the step that last read that buffer) when the consumer enqueues its step, and run beside that
                # step on the GPU whether or not the host is running ahead of it.  A device-resident data set assembles in line on the caller's
                # stream: there the next batch's ~50 assembly kernels and feature concatenation go BEHIND the step just enqueued (after the yield),
                # not in front of it
                if not self.resident and bi + 1 < len(batches):
                    slot ^= 1
                    nxt = self._assemble(batches[bi + 1], slot)
                cur = torch.cuda.current_stream(self.device) if self.device.type == "cuda" else None
                if ready is not None:
                    cur.wait_event(ready)
                yield G, labels
                if self.resident and bi + 1 < len(batches):
                    slot ^= 1
                    nxt = self._assemble(batches[bi + 1], slot)
                if not self.resident:
                    evt = torch.cuda.Event()
                    evt.record(cur)                               # the consumer has enqueued its step on `cur`: the buffer is free behind it
                    self._free_evt[used] = evt
        finally:
            if pinned:
                ops.block_side_streams(False, who)


def slot_augment_spec(transform):
    """The ``graph.AugmentSpec`` of a slot-compatible pipeline: a ``transforms.Compose`` whose members are DropNode, DropEdge, NodeShuffle and
    FeatMask, each kind at most once, in any order (the set one ``ops.augment_graph`` call fuses), FeatMask naming at most the node field
    ``"feat"`` and no edge field.  Anything else raises RuntimeError."""
    from . import transforms as _tr
    refuse = lambda why: RuntimeError(f"BatchSlot: the loader's transform is not slot-compatible ({why}); a slot draws the augmentation on the device for "
                                      "a Compose of at most one each of DropNode, DropEdge, NodeShuffle and FeatMask(node_feat_names=['feat']) - step "
                                      "other pipelines eagerly")
    if not isinstance(transform, _tr.Compose):
        raise refuse("not a transforms.Compose")
    found = {}
    for k, t in enumerate(transform.transforms):
        if not isinstance(t, _tr.BaseTransform) or type(t) not in (_tr.DropNode, _tr.DropEdge, _tr.NodeShuffle, _tr.FeatMask):
            raise refuse(f"member {k} is not one of the four transforms")
        if t.kind in found:
            raise refuse(f"{type(t).__name__} occurs twice")
        if isinstance(t, _tr.FeatMask):
            if t.edge_feat_names:
                raise refuse("FeatMask over an edge field")
            if list(t.node_feat_names or []) not in ([], ["feat"]):
                raise refuse("FeatMask over a node field other than 'feat'")
            found[t.kind] = (k, t.threshold) if t.node_feat_names else None
        else:
            found[t.kind] = (k, getattr(t, "threshold", 0))
    return _graph_mod.AugmentSpec(**{k: v for k, v in found.items() if v is not None})


QUOTA_DELTA = 2.0 ** -32           # per table: the probability that the "bound" quota binds (the constant of BatchSlot.fits' type-present rule)


def slot_quota_bound(it: StoredGraph, spec):
    """``(qn[t], qe[j])``: survivor quotas of a stored slide under the pipeline ``spec`` that a draw exceeds with probability at most 2 ** -32
    per table.  With p_n, p_e the quantised probabilities (threshold / 65536; 0 for an absent stage) and lam = ln(2 ** 32) / 2:

        qn[t] = min(n_t, ceil(n_t (1 - p_n) + sqrt(lam n_t)))                                   (Hoeffding; n_t without DropNode)
        mu_j  = (E_j - loops_j) (1 - p_n) ** 2 (1 - p_e) + loops_j (1 - p_n) (1 - p_e)
        qe[j] = min(E_j, ceil(mu_j + sqrt(lam (sum_v c_v ** 2 + E_j))))                         (bounded differences)

    c_v: edges of relation j incident to node v, a self-loop counted once - what one node draw can move the count by; every edge draw (by index
    or by rank) moves it by at most 1.  Cached on the stored slide per (p_n, p_e); one device -> host copy per slide."""
    import math
    key = (spec.node_thr if spec.drop_node is not None else None, spec.edge_thr if spec.drop_edge is not None else None)
    cache = it.__dict__.setdefault("_quota_bound", {})
    if key in cache:
        return cache[key]
    lam = math.log(1.0 / QUOTA_DELTA) / 2.0
    pn = spec.node_thr / 65536.0 if spec.drop_node is not None else 0.0
    pe = spec.edge_thr / 65536.0 if spec.drop_edge is not None else 0.0
    qn = [int(n) if spec.drop_node is None else min(int(n), math.ceil(n * (1.0 - pn) + math.sqrt(lam * n))) for n in it.num_nodes]
    tix = {t: i for i, t in enumerate(it.ntypes)}
    stats = []
    for r in it.rels:
        u, v = it.edges[r]
        ns, nd = it.num_nodes[tix[r[0]]], it.num_nodes[tix[r[2]]]
        if r[0] == r[2]:
            loop = u == v
            c = torch.bincount(u, minlength=ns) + torch.bincount(v, minlength=ns) - torch.bincount(u[loop], minlength=ns)
            stats += [loop.sum(), (c * c).sum()]
        else:
            cu, cv = torch.bincount(u, minlength=ns), torch.bincount(v, minlength=nd)
            stats += [torch.zeros((), dtype=torch.int64, device=u.device), (cu * cu).sum() + (cv * cv).sum()]
    vals = torch.stack(stats).tolist() if stats else []
    qe = []
    for j, r in enumerate(it.rels):
        E, loops, csq = int(it.edges[r][0].numel()), vals[2 * j], vals[2 * j + 1]
        mu = (E - loops) * (1.0 - pn) ** 2 * (1.0 - pe) + loops * (1.0 - pn) * (1.0 - pe)
        qe.append(min(E, math.ceil(mu + math.sqrt(lam * (csq + E)))))
    cache[key] = (qn, qe)
    return cache[key]


class _DeviceOnly:
    """Stands where a host copy of an augmented GPU slot's counts would be: those counts live on the device, and reading them fails loudly."""

    def __init__(self, what: str):
        self.what = what

    def _fail(self, *a, **k):
        raise RuntimeError(f"BatchSlot: {self.what} of an augmented slot exists on the device only (the draw is not read back); "
                           "BatchSlot.counts() is the one explicit read-back")

    __iter__ = __len__ = __getitem__ = __bool__ = __call__ = _fail


class _DeviceOnlyCounts(dict):
    """``HeteroGraph._batch_num_nodes`` of an augmented GPU slot: the number of graphs is known (``batch_size``), the node counts are not."""

    def __getitem__(self, key):
        _DeviceOnly("batch_num_nodes")._fail()


class BatchSlot:
    """A batch of FIXED shape fed from a resident loader: the static tables of one padded batch - up to ``b_cap`` real slides, empty
    graphs up to ``b_cap``, one filler graph labelled -100 that takes what the slides leave of the capacities - and ONE ``HeteroGraph`` whose kernel
    plan and feature frames are views of those tables.  ``load(idxs)`` rewrites the tables for another batch (one descriptor upload, one launch:
    ``graph.slot_fill``); the graph object, its plan, its readout plan and every shape stay, so a step captured over ``slot.graph`` and
    ``slot.labels`` replays over the new batch (``trainer.CapturedSlotStep``).

    ``capacity``: ``(n_cap, e_cap)`` - nodes per node type, edges per destination node type - or ``(n_cap, e_cap, b_cap)``; ``None`` derives a
    bound every batch of the loader's bucket fits: per type the sum of the ``batch_size`` largest counts, plus one node.  Resident data sets
    only: a pinned-host data set has no device-side features to copy from.

    A loader with ``transform=`` a slot-compatible pipeline (``slot_augment_spec``) gives an AUGMENTED slot: ``load(idxs, draws)``
    fills it with ``[transform(slide_b, draws[b]).., empty graphs.., filler]`` - on the GPU the draw is taken on the device and the tables are
    written from device-side counts (``graph.slot_fill_augmented``: no read-back), on the CPU through the tensor formulation.  Capacities are
    those of the unaugmented batch (augmentation only removes), ``fits`` uses the stored counts plus one rule (see ``fits``), the host mirrors of
    the counts fail loudly on a GPU slot and ``counts()`` is the explicit read-back.

    ``per_relation_src=True``: the slot also owns HGT's plan - ``src``, ``colptr``, ``csc_eid``, ``csc_dst`` and a source order over
    one row per (relation, source node), shapes again functions of the capacities - installed as ``slot.graph.plan(per_relation_src=True)`` and
    re-derived on the device from the tables every ``load`` / ``load_augmented`` has just written (``graph.derive_rel_tables``: one C call behind
    the fill, no host arithmetic).  ``rel_sorted``: order those rows by out-degree, as ``graph.finish_plan`` does, instead of leaving them in
    row order - measured 2 % slower per replayed step (tools/hgt_slot_bench.py), so off.  The default allocates nothing and changes nothing.

    ``quota`` (augmented slots only): survivor QUOTAS - per stored slide an upper limit on the survivors of every node type and
    every relation that the host knows, enforced by the fill itself (truncation in node-id / input order: ``transforms.truncated``), so the
    slot can be sized for the draw instead of for the stored slides.  ``"bound"``: ``slot_quota_bound`` (binds with probability <= 2 ** -32 per
    table); a callable ``quota(idx) -> (qn, qe)`` sets limits by hand.  ``capacity=None`` then sums the ``batch_size`` largest quotas, ``fits``
    tests the quota sums, ``counts()`` returns the truncated counts, and ``overflows()`` / ``overflow_excess()`` read back how often and by how
    much a quota bound.  A truncated batch is a valid graph, just not the eager loader's batch for that draw.  ``None``: today's slot.

    ``type_mask``: ``True`` gives the slot ``type_present``, a float32 ``[T]`` table on its device - 1.0 where the REAL slides
    of the batch just filled (graphs ``0 .. b_cap - 1``, never the filler) hold a node of the type after augmentation and quota truncation,
    else 0.0 - re-derived on the device behind every fill (``graph.derive_type_present``: one wave next to ``_derive``, no read-back) and
    attached to the graph as ``slot.graph._type_present``, where the models' heads read it in place of their host-side test
    (``h[k].shape[0] > 0``) and ``optim``'s gate reads it in place of a ``None`` gradient.  A float32 ``[T]`` device tensor instead of
    ``True`` makes the slot write the caller's table (several slots then share one: ``share_type_table``).  Such a slot takes batches in
    which NO slide has a node of some type, and an augmented one drops the ``p ** n`` rule of ``fits``.  ``False``: today's slot.

    A homogeneous slot (one node type, one relation: ``graph.to_homogeneous`` slides) also keeps, re-derived on the device behind every fill,
    GraphConv's degree norms and ``live_rows`` = (float32 ``[N]`` 1 / 0 by row, the number of live rows as one float32 word):
    the rows of the real slides, over which ``models.GIN``'s BatchNorms take their statistics."""

    def __init__(self, loader: GraphBatchLoader, capacity=None, bucket: int = 0, per_relation_src: bool = False, quota=None, type_mask=False):
        if not loader.resident:
            raise RuntimeError("BatchSlot needs a device-resident data set (GraphBatchLoader(..., resident=True)): the fill copies the slides' features "
                               "device to device; a pinned-host loader stays on its own double-buffered path")
        self.spec = slot_augment_spec(loader.transform) if loader.transform is not None else None
        self.loader, self.device = loader, loader.device
        key = list(loader.buckets)[bucket]
        self.members = set(loader.buckets[key])
        ntypes, rels = list(key[0]), [tuple(r) for r in key[1]]
        its = [loader.items[i] for i in loader.buckets[key]]
        T = len(ntypes)
        self.quota, self._quotas = quota, {}
        if quota is not None:
            if self.spec is None:
                raise RuntimeError("BatchSlot(quota=...): quotas limit the survivors of a draw; the loader has no transform")
            if quota != "bound" and not callable(quota):
                raise ValueError('BatchSlot: quota is None, "bound" or a callable quota(idx) -> (qn, qe)')
            self._overflow = torch.zeros(3, dtype=torch.int64, device=self.device)     # fills in which a quota bound, largest node / edge excess
        if capacity is None and quota is not None:
            bs = loader.batch_size
            top = lambda xs: sum(sorted(xs, reverse=True)[:bs])
            qs = [self._quota_counts([i]) for i in loader.buckets[key]]
            n_cap = [top([q[0][0][t] for q in qs]) + 1 for t in range(T)]
            e_cap = [top([q[1][0][t] for q in qs]) for t in range(T)]
            b_cap = bs
        elif capacity is None:
            bs = loader.batch_size
            top = lambda xs: sum(sorted(xs, reverse=True)[:bs])
            n_cap = [top([it.num_nodes[t] for it in its]) + 1 for t in range(T)]
            e_cap = [top([it.pieces.ecount[t] for it in its]) for t in range(T)]
            b_cap = bs
        else:
            n_cap, e_cap = capacity[0], capacity[1]
            b_cap = capacity[2] if len(capacity) > 2 else loader.batch_size
        self.layout = _graph_mod.SlotLayout(ntypes, rels, n_cap, e_cap, b_cap, loader.in_dim)
        self.bufs = self.layout.buffers(self.device)
        locality = [it.pieces.locality for it in its]
        if any(locality) and not all(locality):
            raise ValueError("a data set mixes locality-ordered and plain graphs: apply graph.apply_locality_order to all of its slides or none")
        lay, hd = self.layout, self.layout.hd
        plan = _graph_mod.slot_plan(lay, self.bufs, locality=bool(locality and locality[0]))
        G = HeteroGraph._from_plan(OrderedDict(zip(ntypes, lay.n_cap)), rels,
                                   {t: torch.zeros(lay.graphs, dtype=torch.int64) for t in ntypes}, plan, None)
        feat = self.bufs["feat"]
        parts = []
        for i, t in enumerate(ntypes):
            v = feat[hd.type_off[i]:hd.type_off[i + 1]]
            G._nframes[t]["feat"] = v
            parts.append(v)
        # the caches that key on (data_ptr, _version) stay valid across fills - the kernel writes behind the version counters and the cached
        # objects ARE the static tables: the feature concatenation, the CSR-ordered sim, the features' row scales
        cache = G.__dict__.setdefault("_cat_cache", {})
        cache["feat"] = (tuple((p.data_ptr(), tuple(p.shape), p.dtype, p._version) for p in parts), feat)
        cache[("e", "sim")] = ((), self.bufs["sim"])
        if self.device.type == "cuda":
            from . import ops
            ops.attach_row_scales(feat, self.bufs["scales"])
            # the readout's plan (pooling.readout.all_types_plan caches it on the graph): static tables, refreshed by every fill
            rp = _slot_reduce_plan(ops)()
            rp.device, rp.num_segs, rp.num_chunks, rp.num_rows, rp.first_row = self.device, lay.num_segs, lay.c_cap, lay.N, 0
            rp.chunk_row, rp.chunk_seg, rp.seg_chunk = self.bufs["chunk_row"], self.bufs["chunk_seg"], self.bufs["seg_chunk"]
            rp._counts, rp._inv_counts, rp._nonempty = self.bufs["seg_counts"], self.bufs["seg_inv_counts"], self.bufs["seg_nonempty"]
            rp._row_seg = self.bufs["row_seg"]
            rp.type_rows = [(hd.type_off[i], hd.type_off[i + 1]) for i in range(T)]
            rp.type_segments = [(i * lay.graphs, (i + 1) * lay.graphs) for i in range(T)]
            G.__dict__.setdefault("_readout_plans", {})[("all", str(self.device))] = rp
            self.readout_plan = rp
        else:
            self.readout_plan = None
        self.graph, self.labels = G, self.bufs["labels"]
        self.num_real, self.batch, self.idxs, self.draws = 0, None, None, None
        # HGT's plan (source rows per (relation, source node)): four tables and a source order of the slot's own, derived on the
        # device from the tables every fill has just written; installed as the slot graph's cached per-relation plan
        self.per_relation_src, self.rel, self.rel_sorted = bool(per_relation_src), None, False
        if self.per_relation_src:
            hd.relation_table()
            if hd.max_src_rels > _graph_mod.PLAN_REL_MAX_RELS:
                raise ValueError(f"BatchSlot(per_relation_src=True): {hd.max_src_rels} relations leave one node type, the derivation supports "
                                 f"{_graph_mod.PLAN_REL_MAX_RELS}")
            self.rel = _graph_mod.plan_rel_buffers(hd, lay.E, self.device)
            G.__dict__["_plan_rel"] = _graph_mod.rel_plan_over(hd, plan, self.rel)
        # which node types the real slides hold: a device table behind every fill, read by the heads and by the optimizer's gate
        self.type_mask, self.type_present = type_mask is not False and type_mask is not None, None
        if self.type_mask:
            self.share_type_table(torch.ones(T, dtype=torch.float32, device=self.device) if type_mask is True else type_mask)

        # a homogeneous slot (one node type, one relation: graph.to_homogeneous slides): GraphConv's degree norms as two more
        # static tables, re-derived on the device behind every fill, under the slot graph's cached models.GCN.HomoPlan
        self.degree_norms = None
        if T == 1 and len(rels) == 1:
            from .models.GCN import HomoPlan
            mk = lambda: torch.empty(lay.N, dtype=torch.float32, device=self.device)
            self.degree_norms = self.bufs["in_norm"], self.bufs["out_norm"] = mk(), mk()
            G.__dict__["_homo_plan"] = HomoPlan.over_tables(plan, lay.N, lay.E, *self.degree_norms)
        # ... and which rows belong to the real slides, with their count: what models.GIN's BatchNorms normalise over - the
        # filler's rows, often most of the table, enter no statistic - installed where models.GIN.live_rows looks
        self.live_rows = None
        if T == 1 and len(rels) == 1:
            self.live_rows = self.bufs["live"], self.bufs["live_rows"] = (torch.ones(lay.N, dtype=torch.float32, device=self.device),
                                                                          torch.full((1,), float(lay.N), dtype=torch.float32, device=self.device))
            G.__dict__["_gin_live"] = self.live_rows

    def share_type_table(self, table: torch.Tensor) -> None:
        """Make ``table`` (float32 ``[T]`` on the slot's device) this slot's presence table: every later fill writes it, and the slot graph
        carries it.  A step captured over the slot before this call still reads the old table."""
        if not self.type_mask:
            raise RuntimeError("BatchSlot.share_type_table: the slot was built without type_mask")
        T = self.layout.T
        if (not isinstance(table, torch.Tensor) or table.dtype != torch.float32 or tuple(table.shape) != (T,) or not table.is_contiguous()
                or _resolve_device(table.device) != _resolve_device(self.device)):
            raise ValueError(f"BatchSlot: type_mask is True or a contiguous float32 [{T}] tensor on the slot's device ({self.device})")
        self.type_present = table
        self.graph._type_present = table

    def _derive(self) -> None:
        """The per-relation tables of the batch just filled in, on the current stream behind the fill (one C call and the source order)."""
        if self.rel is not None:
            _graph_mod.derive_rel_tables(self.layout.hd, self.graph._plan, self.rel, sort_sources=self.rel_sorted)
        if self.type_present is not None:
            _graph_mod.derive_type_present(self.layout, self.bufs, self.type_present)
        if self.degree_norms is not None:
            _graph_mod.derive_degree_norms(self.layout, self.bufs, *self.degree_norms)
        if self.live_rows is not None:
            _graph_mod.derive_live_rows(self.layout, self.bufs, *self.live_rows)

    def quota_of(self, idx: int):
        """``(qn, qe)`` of the loader's slide ``idx`` under this slot's quota rule, never above the stored counts (cached)."""
        if idx not in self._quotas:
            it = self.loader.items[idx]
            qn, qe = slot_quota_bound(it, self.spec) if self.quota == "bound" else self.quota(idx)
            if len(qn) != len(it.ntypes) or len(qe) != len(it.rels):
                raise ValueError("BatchSlot: quota(idx) returns one node quota per node type and one edge quota per relation")
            self._quotas[idx] = ([max(0, min(int(q), n)) for q, n in zip(qn, it.num_nodes)],
                                 [max(0, min(int(q), int(it.edges[r][0].numel()))) for q, r in zip(qe, it.rels)])
        return self._quotas[idx]

    def _quota_counts(self, idxs):
        """The most the slides ``idxs`` can hold under their quotas: (nodes[b][t], edges[b][t] by destination type)."""
        it = self.loader.items[idxs[0]]
        return _graph_mod.quota_counts(it.ntypes, it.rels, [self.loader.items[i].num_nodes for i in idxs], [self.quota_of(i) for i in idxs], self.spec)

    def _counts(self, idxs):
        if self.quota is not None:
            return self._quota_counts(idxs)
        its = [self.loader.items[i] for i in idxs]
        return [it.num_nodes for it in its], [it.pieces.ecount for it in its]

    def fits(self, idxs: Sequence[int]) -> bool:
        """Does the batch of the loader's slides ``idxs`` fit: same schema bucket, at most ``b_cap`` slides, and per node type at least one
        node and no fewer than zero edges left for the filler.  Without ``type_mask`` two more rules hold: every node type occurs in some
        slide, and on an augmented slot no draw can empty a type in practice (below)."""
        idxs = list(idxs)
        if not idxs or any(i not in self.members for i in idxs):
            return False
        counts, ecounts = self._counts(idxs)
        if not _graph_mod.SlotBatch.fits(self.layout, counts, ecounts, self.type_mask):
            return False
        if self.spec is not None and self.spec.node_thr > 0 and not self.type_mask:
            # augmented slot: the models switch a node type's head off when the batch has no node of the type - a host-side branch frozen into a
            # capture - so a draw that empties a type must be impossible in practice: p_node ** n[t] <= 2 ** -32 for every type (n >= 32 at 0.5)
            p = self.spec.node_thr / 65536.0
            stored = [self.loader.items[i].num_nodes for i in idxs]
            if any(p ** sum(c[t] for c in stored) > 2.0 ** -32 for t in range(self.layout.T)):
                return False
        return True

    def load(self, idxs: Sequence[int], draws: Optional[Sequence[int]] = None) -> "BatchSlot":
        """Fill the slot with the batch of slides ``idxs`` (in that order) on the current stream.  Raises ValueError when it does not fit.
        Augmented slot: ``draws[b]`` is the 32-bit draw of slide ``idxs[b]``; ``None`` takes ``augment_draw(loader.seed, counter, idxs[b])`` with
        the loader's running batch counter, which it advances by one - as ``GraphBatchLoader._augmented`` does."""
        idxs = list(idxs)
        if not self.fits(idxs):
            raise ValueError(f"BatchSlot.load: the batch {idxs} does not fit the slot (capacities: {self.layout.n_cap} nodes, {self.layout.e_cap} edges, "
                             f"{self.layout.b_cap} slides)")
        if self.spec is not None:
            if draws is None:
                counter, self.loader._batches_drawn = self.loader._batches_drawn, self.loader._batches_drawn + 1
                draws = [augment_draw(self.loader.seed, counter, i) for i in idxs]
            return self.load_augmented(idxs, draws)
        if draws is not None:
            raise ValueError("BatchSlot.load: draws= needs a loader with a transform")
        its = [self.loader.items[i] for i in idxs]
        T = self.layout.T
        scales = None
        if self.device.type == "cuda":
            scales = [[it.feat_scale(t) for t in range(T)] for it in its]
        sb = _graph_mod.slot_fill(self.layout, self.bufs, [it.pieces for it in its], [it.label for it in its], [it.feat for it in its], scales,
                                  self.type_mask)
        G, lay = self.graph, self.layout
        for i, t in enumerate(G.ntypes):
            G._batch_num_nodes[t] = torch.tensor(sb.counts[i], dtype=torch.int64)
        # per-relation COO / edge fields of the padded batch: rebuilt on demand only (HeteroGraph._edges); the HEAT path never asks
        ntypes, rels, dev = G.ntypes, G.canonical_etypes, self.device
        nf, ef, n = list(sb.nf), list(sb.ef), list(sb.n)

        def coo():
            edges, efields = _batch_coo(its, ntypes, rels)
            fg = _graph_mod.filler_graph(ntypes, rels, nf, ef, 0)
            tix = {t: i for i, t in enumerate(ntypes)}
            for r in rels:
                u, v = fg.edges(r)
                edges[r] = (torch.cat([edges[r][0], u.to(dev) + n[tix[r[0]]]]), torch.cat([edges[r][1], v.to(dev) + n[tix[r[2]]]]))
                efields[r] = {"sim": torch.cat([efields[r]["sim"], torch.zeros(u.numel(), dtype=torch.float32, device=dev)])}
            return edges, efields

        G._edges_store, G._edge_thunk = None, coo
        for r in rels:
            G._eframes[r].clear()
        if self.readout_plan is not None:
            self.readout_plan.ranges = list(sb.ranges)
            from . import ops
            ops.refresh_constant_cols(self.bufs["feat"])      # scaled GEMM modes: the features' cached column statistics describe the previous batch
        self.num_real, self.batch, self.idxs = sb.B, sb, idxs
        self._derive()
        return self

    def load_augmented(self, idxs: Sequence[int], draws: Sequence[int]) -> "BatchSlot":
        """``load`` of an augmented slot WITHOUT the ``fits`` rule on the node counts (the stored batch must fit the capacities): the fill itself is
        defined for every draw, one that empties a node type included (the filler then takes the whole type) - tests and diagnostics call this."""
        idxs, draws = list(idxs), [int(d) & 0xffffffff for d in draws]
        if self.spec is None:
            raise RuntimeError("BatchSlot.load_augmented: the loader has no transform")
        if len(draws) != len(idxs):
            raise ValueError("BatchSlot.load_augmented: one draw per slide")
        its = [self.loader.items[i] for i in idxs]
        lay, G = self.layout, self.graph
        if any(i not in self.members for i in idxs) or not _graph_mod.SlotBatch.fits(lay, *self._counts(idxs), True):
            raise ValueError(f"BatchSlot.load_augmented: the batch {idxs} does not fit the slot")
        ntypes, rels = G.ntypes, G.canonical_etypes
        quotas = [self.quota_of(i) for i in idxs] if self.quota is not None else None
        if self.device.type == "cuda":
            _graph_mod.slot_fill_augmented(lay, self.bufs, [it.pieces for it in its], [[it.edges[r] for r in rels] for it in its],
                                           [it.label for it in its], [it.feat for it in its], draws, self.spec, quotas,
                                           self._overflow if quotas is not None else None)
            # host mirrors of the counts: not current without a read-back - they fail loudly instead (the step reads none of them)
            G._batch_num_nodes = _DeviceOnlyCounts((t, torch.zeros(lay.graphs, dtype=torch.int64)) for t in ntypes)
            G._edges_store, G._edge_thunk = None, _DeviceOnly("the per-relation COO")
            self.batch = _DeviceOnly("the host layout (BatchSlot.batch)")
            self.readout_plan.ranges = _DeviceOnly("the readout plan's row ranges")
            from . import ops
            ops.refresh_constant_cols(self.bufs["feat"])
        else:
            # tensor route (and the kernels' oracle): every slide through the tensor formulation of the pipeline, stored anew, then the ordinary fill
            aug, keeps, over_n, over_e = [], [], 0, 0
            for b, (it, d) in enumerate(zip(its, draws)):
                g = HeteroGraph.from_coo(OrderedDict(zip(it.ntypes, it.num_nodes)), it.edges, feat=dict(zip(it.ntypes, it.feat)), sim=it.sims)
                keep = self.spec.node_keep(d, it.num_nodes, self.device)
                if quotas is None:
                    g = self.loader.transform(g, draw=d, fused=False)
                else:
                    from . import transforms as _tr
                    qn, qe = quotas[b]
                    g, xn, xe = _tr.truncated(self.loader.transform, g, d, qn, qe)
                    over_n, over_e = max([over_n] + xn), max([over_e] + xe)
                    if self.spec.drop_node is not None:
                        keep = [k & (torch.cumsum(k, 0) <= q) for k, q in zip(keep, qn)]
                aug.append(StoredGraph(g, it.label, self.device, True))
                keeps.append(keep)
            if quotas is not None:
                self._overflow += torch.tensor([int(over_n > 0 or over_e > 0), 0, 0])
                self._overflow[1:] = torch.maximum(self._overflow[1:], torch.tensor([over_n, over_e]))
            out = _graph_mod.slot_fill_torch(lay, [a.pieces for a in aug], [a.label for a in aug], [a.feat for a in aug], None, self.device, True)
            sb = out["batch"]
            out["order_dst"], out["order_src"] = _graph_mod.restricted_orders(lay, [it.pieces for it in its], keeps, sb)
            with torch.no_grad():
                for k, v in out.items():
                    if k != "batch":
                        self.bufs[k].copy_(v)
            for i, t in enumerate(ntypes):
                G._batch_num_nodes[t] = torch.tensor(sb.counts[i], dtype=torch.int64)
            nf, ef, n, dev = list(sb.nf), list(sb.ef), list(sb.n), self.device

            def coo():
                edges, efields = _batch_coo(aug, ntypes, rels)
                fg = _graph_mod.filler_graph(ntypes, rels, nf, ef, 0)
                tix = {t: i for i, t in enumerate(ntypes)}
                for r in rels:
                    u, v = fg.edges(r)
                    edges[r] = (torch.cat([edges[r][0], u.to(dev) + n[tix[r[0]]]]), torch.cat([edges[r][1], v.to(dev) + n[tix[r[2]]]]))
                    efields[r] = {"sim": torch.cat([efields[r]["sim"], torch.zeros(u.numel(), dtype=torch.float32, device=dev)])}
                return edges, efields

            G._edges_store, G._edge_thunk = None, coo
            self.batch = sb
        for r in rels:
            G._eframes[r].clear()
        self.num_real, self.idxs, self.draws = len(idxs), idxs, draws
        self._derive()
        return self

    def counts(self):
        """``(nodes, edges)`` of the last fill, ``[b][t]`` per real slide and node type (edges by destination type).  On an augmented GPU slot
        this is THE read-back of the device-side counts (one synchronising copy): for diagnostics and benchmarks, never inside a step."""
        if self.idxs is None:
            raise RuntimeError("BatchSlot.counts: nothing loaded")
        B, T = len(self.idxs), self.layout.T
        if self.spec is not None and self.device.type == "cuda":
            sc = self.bufs["_aug"]
            got = torch.cat([sc["ncnt"][:B * T], sc["fcnt"][:B * T]]).tolist()
            return [got[b * T:(b + 1) * T] for b in range(B)], [got[(B + b) * T:(B + b + 1) * T] for b in range(B)]
        if self.spec is not None:
            sb = self.batch
            return ([[sb.counts[t][b] for t in range(T)] for b in range(B)],
                    [[sb.eoff[(t, b + 1)] - sb.eoff[(t, b)] if b + 1 < B else sb.feb[t] - sb.eoff[(t, b)] for t in range(T)] for b in range(B)])
        n, e = self._counts(self.idxs)
        return [list(x) for x in n], [list(x) for x in e]

    def overflows(self) -> int:
        """Number of fills of this slot in which at least one quota bound, that is, in which the batch was truncated (0 on a slot without
        quotas).  On a GPU slot the explicit read-back of the slot's overflow words (one synchronising copy): once per epoch, never in a step."""
        return int(self._overflow[0]) if self.quota is not None else 0

    def overflow_excess(self):
        """``(nodes, edges)``: the largest number of survivors beyond its quota that any (slide, node type) and any (slide, relation) has had
        over the slot's life; edges counted in the node-truncated pipeline.  A read-back, as ``overflows``."""
        if self.quota is None:
            return 0, 0
        got = self._overflow.tolist()
        return got[1], got[2]

    def padded_share(self):
        """(share of the slot's rows, share of its edges) that the current batch's filler takes (``counts()``: a read-back on an augmented GPU slot)."""
        lay = self.layout
        n, e = self.counts()
        return (lay.N - sum(map(sum, n))) / max(lay.N, 1), (lay.E - sum(map(sum, e))) / max(lay.E, 1)


def _slot_reduce_plan(ops):
    class SlotReducePlan(ops.ReducePlan):
        """The readout plan of a slot: its tables are static buffers the fill rewrites, so nothing a step decides on the HOST may depend on the
        current batch - a slot always counts as having empty segments (the mask of empty segments is then always applied; it is exact)."""

        is_slot = True          # pooling.readout.slot_plan: the attention readout then reads these tables instead of host-side node counts

        def has_empty(self) -> bool:
            return True

    return SlotReducePlan
