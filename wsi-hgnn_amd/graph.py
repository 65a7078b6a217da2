"""Graph container for the WSI-HGNN hot path (replaces the DGLGraph the reference passes around).

The reference hands a ``dgl.DGLGraph`` to ``model.forward`` and only touches a small part of
its API: ``G.ntypes``, ``G.canonical_etypes``, ``G.nodes[t].data['feat']``
(models/HEATNet4.py:202), ``G.edata['sim']`` (models/HEATNet4.py:209), ``G.ndata`` /
``G.local_scope()`` (pooling/avg_pooling.py:12-13), ``batch_num_nodes(ntype)`` (behind
``dgl.readout.mean_nodes``), ``G.to(device)`` (trainer/train_gnn.py:60).  ``HeteroGraph``
offers exactly that surface, plus the device-side *plan* the HIP kernels consume:

* nodes of all types live in ONE type-major id space (global id = type offset + local id), so
  K/Q/V of every node type sit in one ``[N, 3*D]`` table in HBM and a kernel never branches on
  the node type;
* forward layout = two-level CSR by destination: ``node_seg[w] .. node_seg[w+1]`` are the
  relation slots of dst node ``w`` (one slot per canonical relation whose dst type is w's type,
  empty relations included — DGL's ``cross_reducer='mean'`` denominator),
  ``rowptr[seg] .. rowptr[seg+1]`` the in-edges of that (node, relation) segment;
* backward layout = CSC by source over the same edge numbering (``csc_eid`` points back into the
  CSR edge order), so gradients w.r.t. K/V are reduced without atomics.

Graph construction / pickles (construct_graph/, data.py) are out of scope; ``from_coo`` takes
plain COO tensors.
"""
from __future__ import annotations

import array
import collections

import os
import struct

import contextlib
from collections import OrderedDict
from typing import Dict, List, Optional, Sequence, Tuple

import torch

CanonicalEType = Tuple[str, str, str]


class _Frame(dict):
    """Per-type feature dict (``G.nodes['0'].data`` / per-relation edge data)."""


class _NodeTypeView:
    __slots__ = ("data",)

    def __init__(self, frame: _Frame):
        self.data = frame


class _NodesAccessor:
    def __init__(self, g: "HeteroGraph"):
        self._g = g

    def __getitem__(self, ntype: str) -> _NodeTypeView:
        return _NodeTypeView(self._g._nframes[ntype])


class _NDataAccessor:
    """``G.ndata[key]``: tensor for a one-type graph, ``{ntype: tensor}`` otherwise (DGL semantics)."""

    def __init__(self, g: "HeteroGraph"):
        self._g = g

    def __getitem__(self, key: str):
        g = self._g
        if len(g.ntypes) == 1:
            return g._nframes[g.ntypes[0]][key]
        return {t: g._nframes[t][key] for t in g.ntypes if key in g._nframes[t]}

    def __setitem__(self, key: str, value) -> None:
        g = self._g
        if isinstance(value, dict):
            for t, v in value.items():
                g._nframes[t][key] = v
        else:
            if len(g.ntypes) != 1:
                raise ValueError("assigning a tensor to ndata needs a single node type; pass a dict")
            g._nframes[g.ntypes[0]][key] = value

    def __contains__(self, key: str) -> bool:
        return any(key in self._g._nframes[t] for t in self._g.ntypes)


class _EDataAccessor:
    """``G.edata[key]``: tensor for a one-relation graph, ``{canonical_etype: tensor}`` otherwise."""

    def __init__(self, g: "HeteroGraph"):
        self._g = g

    def __getitem__(self, key: str):
        g = self._g
        if len(g.canonical_etypes) == 1:
            return g._eframes[g.canonical_etypes[0]][key]
        return {r: g._eframes[r][key] for r in g.canonical_etypes if key in g._eframes[r]}

    def __setitem__(self, key: str, value) -> None:
        g = self._g
        if isinstance(value, dict):
            for r, v in value.items():
                g._eframes[r][key] = v
        else:
            if len(g.canonical_etypes) != 1:
                raise ValueError("assigning a tensor to edata needs a single relation; pass a dict")
            g._eframes[g.canonical_etypes[0]][key] = value

    def __contains__(self, key: str) -> bool:
        return any(key in self._g._eframes[r] for r in self._g.canonical_etypes)


def _resolve_device(device) -> torch.device:
    """torch.device with the implicit CUDA index made explicit ('cuda' -> 'cuda:<current>'), so devices compare by value."""
    device = torch.device(device)
    if device.type == "cuda" and device.index is None:
        return torch.device("cuda", torch.cuda.current_device())
    return device


class GraphPlan:
    """Device-resident int32/fp32 index structures consumed by the HIP kernels (see module doc).

    All tensors live on ``device``.  Edge order "CSR" = sorted by (global dst, relation slot),
    stable in the input edge order; every per-edge tensor the kernels exchange uses that order.
    """

    def __init__(self):
        self.device = None
        self.num_nodes = 0          # N, all types
        self.num_edges = 0          # E, all relations
        self.num_segs = 0           # sum_t N_t * R_t
        self.type_off: List[int] = []   # [T+1] host ints, global id range of each ntype
        self.rel_slots: List[int] = []  # R_t per ntype (relations whose dst type is t)
        self.node_seg = None        # int32 [N+1]
        self.rowptr = None          # int32 [S+1]
        self.src = None             # int32 [E]   global src id, CSR order
        self.perm = None            # int64 [E]   CSR position -> position in the concatenated input edge list (None for
                                    #             loader-assembled plans: HeteroGraph._csr_perm recomputes it on demand)
        self.inv_rd = None          # fp32  [N]   1/R_t(type of node), 0 when R_t == 0
        self.colptr = None          # int32 [N+1] CSC by global src
        self.csc_eid = None         # int32 [E]   CSR edge id of the j-th CSC entry
        self.csc_dst = None         # int32 [E]   global dst of the j-th CSC entry
        self.order_dst = None       # int32 [N]   dst nodes, heaviest (most in-edges) first
        self.order_src = None       # int32 [N]   src nodes, heaviest (most out-edges) first
        self.num_heavy = 0          # leading entries of order_dst = the highest in-degree nodes (see wsi_heat_attn_fwd)
        self.locality = False       # orders follow the slides' locality positions ('_pos'): kernels walk them XCD-contiguously
        self.heavy_degree = HEAVY_DEGREE   # threshold the first `num_heavy` entries of order_dst were chosen with
        self.readout_ptr = None     # int32 [T*B+1] rows of (ntype t, graph b) = [ptr[t*B+b], ptr[t*B+b+1])
        self.batch_size = 1
        self.num_src_rows = 0       # rows of the k/v tables the CSC indexes: N, or sum_r N_src(r) (per-relation tables)
        self.rel_rows: List[Tuple[int, int]] = []   # per canonical relation: its row range in the per-relation tables


class HeteroGraph:
    """Heterogeneous (or homogeneous) multi-relation graph, optionally a block-diagonal batch."""

    def __init__(
        self,
        num_nodes: "OrderedDict[str, int] | Dict[str, int]",
        edges: "OrderedDict[CanonicalEType, Tuple[torch.Tensor, torch.Tensor]]",
        batch_num_nodes: Optional[Dict[str, torch.Tensor]] = None,
    ):
        # DGL keeps node types and canonical relations sorted as STRINGS ('10' < '2'), whatever order they were given in
        # (dgl.heterograph / dgl.to_heterogeneous); HEATNet4 concatenates per-type blocks in G.ntypes order (HEATNet4.py:236-242),
        # so the order is part of the arithmetic.
        self._num_nodes = OrderedDict((k, int(num_nodes[k0])) for k, k0 in sorted((str(k), k) for k in num_nodes))
        pairs = []
        for (s, e, d), (u, v) in edges.items():
            s, e, d = str(s), str(e), str(d)
            if s not in self._num_nodes or d not in self._num_nodes:
                raise KeyError(f"relation {(s, e, d)} uses an unknown node type")
            u = torch.as_tensor(u, dtype=torch.int64)
            v = torch.as_tensor(v, dtype=torch.int64)
            if u.shape != v.shape or u.dim() != 1:
                raise ValueError("src/dst must be 1-D tensors of equal length")
            pairs.append(((s, e, d), (u, v)))
        pairs.sort(key=lambda kv: kv[0])
        self._edges_store: "Optional[OrderedDict[CanonicalEType, Tuple[torch.Tensor, torch.Tensor]]]" = OrderedDict(pairs)
        self._rels: List[CanonicalEType] = [k for k, _ in pairs]
        self._edge_thunk = None         # loader batches: per-relation COO (+ per-relation edge fields) built on first use
        self._nframes: Dict[str, _Frame] = {t: _Frame() for t in self._num_nodes}
        self._eframes: Dict[CanonicalEType, _Frame] = {r: _Frame() for r in self._rels}
        if batch_num_nodes is None:
            self._batch_num_nodes = None
        else:
            self._batch_num_nodes = {t: torch.as_tensor(batch_num_nodes[t], dtype=torch.int64).cpu()
                                     for t in self._num_nodes}
        self._plan: Optional[GraphPlan] = None

    @property
    def _edges(self) -> "OrderedDict[CanonicalEType, Tuple[torch.Tensor, torch.Tensor]]":
        """Per-relation COO.  A loader batch (data.GraphBatchLoader) carries only its assembled kernel plan; its COO and
        per-relation edge fields are an offset-concatenation of the stored graphs' edges, done here on first use."""
        if self._edges_store is None:
            thunk, self._edge_thunk = self._edge_thunk, None
            edges, efields = thunk()
            self._edges_store = OrderedDict((r, edges[r]) for r in self._rels)
            for r in self._rels:
                for k, x in efields.get(r, {}).items():
                    self._eframes[r].setdefault(k, x)
        return self._edges_store

    @classmethod
    def _from_plan(cls, num_nodes, rels, batch_num_nodes, plan, edge_thunk) -> "HeteroGraph":
        """Loader batch: schema + assembled plan now, COO later (see ``_edges``).  ``rels`` must be sorted."""
        g = cls(num_nodes, OrderedDict(), batch_num_nodes)
        g._rels = [tuple(r) for r in rels]
        g._eframes = {r: _Frame() for r in g._rels}
        g._edges_store = None
        g._edge_thunk = edge_thunk
        g._plan = plan
        return g

    # ------------------------------------------------------------------ constructors
    @classmethod
    def from_coo(cls, num_nodes, edges, feat=None, sim=None) -> "HeteroGraph":
        g = cls(num_nodes, edges)
        if feat is not None:
            for t, x in feat.items():
                g._nframes[str(t)]["feat"] = x
        if sim is not None:
            for r, x in sim.items():
                g._eframes[tuple(str(a) for a in r)]["sim"] = x
        return g

    @classmethod
    def homogeneous(cls, num_nodes: int, src, dst, feat=None) -> "HeteroGraph":
        g = cls(OrderedDict([("_N", num_nodes)]), OrderedDict([(("_N", "_E", "_N"), (src, dst))]))
        if feat is not None:
            g._nframes["_N"]["feat"] = feat
        return g

    # ------------------------------------------------------------------ DGL-like surface
    @property
    def ntypes(self) -> List[str]:
        return list(self._num_nodes.keys())

    @property
    def canonical_etypes(self) -> List[CanonicalEType]:
        return list(self._rels)

    @property
    def etypes(self) -> List[str]:
        return [r[1] for r in self._rels]

    @property
    def is_homogeneous(self) -> bool:
        return len(self._num_nodes) == 1 and len(self._rels) == 1

    @property
    def nodes(self) -> _NodesAccessor:
        return _NodesAccessor(self)

    @property
    def ndata(self) -> _NDataAccessor:
        return _NDataAccessor(self)

    @property
    def edata(self) -> _EDataAccessor:
        return _EDataAccessor(self)

    def num_nodes(self, ntype: Optional[str] = None) -> int:
        if ntype is None:
            return sum(self._num_nodes.values())
        return self._num_nodes[ntype]

    number_of_nodes = num_nodes

    def num_edges(self, etype: Optional[CanonicalEType] = None) -> int:
        if etype is None:
            if self._edges_store is None:
                return int(self._plan.num_edges)
            return sum(int(u.numel()) for u, _ in self._edges.values())
        return int(self._edges[etype][0].numel())

    number_of_edges = num_edges

    def edges(self, etype: Optional[CanonicalEType] = None):
        if etype is None:
            if len(self._rels) != 1:
                raise ValueError("etype is required for a multi-relation graph")
            etype = self.canonical_etypes[0]
        return self._edges[etype]

    @property
    def batch_size(self) -> int:
        if self._batch_num_nodes is None:
            return 1
        return int(next(iter(self._batch_num_nodes.values())).numel())

    def batch_num_nodes(self, ntype: Optional[str] = None) -> torch.Tensor:
        if ntype is None:
            if len(self._num_nodes) != 1:
                raise ValueError("ntype is required for a multi-type graph")
            ntype = self.ntypes[0]
        if self._batch_num_nodes is None:
            return torch.tensor([self._num_nodes[ntype]], dtype=torch.int64)
        return self._batch_num_nodes[ntype]

    @property
    def device(self) -> torch.device:
        for fr in self._nframes.values():
            for v in fr.values():
                return v.device
        if self._edges_store is None:
            return self._plan.device
        for u, _ in self._edges_store.values():
            return u.device
        return torch.device("cpu")

    @contextlib.contextmanager
    def local_scope(self):
        """Frames written inside the scope are dropped on exit (DGL ``local_scope``)."""
        nsnap = {t: dict(fr) for t, fr in self._nframes.items()}
        esnap = {r: dict(fr) for r, fr in self._eframes.items()}
        try:
            yield self
        finally:
            for t, fr in self._nframes.items():
                fr.clear()
                fr.update(nsnap[t])
            for r, fr in self._eframes.items():
                fr.clear()
                fr.update(esnap[r])

    def to(self, device) -> "HeteroGraph":
        """``g.to(device)`` (trainer/train_gnn.py:60,64).  Returns ``self`` — with its cached kernel plan, contexts and
        concatenated tables — whenever no tensor would move ('cuda' and 'cuda:<current>' are the same device)."""
        device = _resolve_device(device)
        if self._all_on(device):
            return self
        edges = self._edges                      # a loader batch materialises its COO before it moves
        g = HeteroGraph(self._num_nodes, OrderedDict((r, (u.to(device), v.to(device))) for r, (u, v) in edges.items()),
                        self._batch_num_nodes)
        for t, fr in self._nframes.items():
            for k, v in fr.items():
                g._nframes[t][k] = v.to(device)
        for r, fr in self._eframes.items():
            for k, v in fr.items():
                g._eframes[r][k] = v.to(device)
        return g

    def _all_on(self, device) -> bool:
        for fr in list(self._nframes.values()) + list(self._eframes.values()):
            for v in fr.values():
                if _resolve_device(v.device) != device:
                    return False
        if self._edges_store is None:
            return _resolve_device(self._plan.device) == device
        for u, v in self._edges_store.values():
            if _resolve_device(u.device) != device or _resolve_device(v.device) != device:
                return False
        return True

    # ------------------------------------------------------------------ type-major helpers
    def type_offsets(self) -> List[int]:
        off = [0]
        for t in self.ntypes:
            off.append(off[-1] + self._num_nodes[t])
        return off

    def cat_ndata(self, key: str = "feat") -> torch.Tensor:
        """Concatenate a node field type-major into one ``[N, F]`` fp32 tensor (the kernels' layout).

        Cached per graph (keyed by the parts' storage), so a resident batch is concatenated once."""
        parts = [self._nframes[t][key] for t in self.ntypes]
        sig = tuple((p.data_ptr(), tuple(p.shape), p.dtype, p._version) for p in parts)
        cache = self.__dict__.setdefault("_cat_cache", {})
        hit = cache.get(key)
        if hit is not None and hit[0] == sig:
            return hit[1]
        out = parts[0] if len(parts) == 1 else torch.cat(parts, dim=0)
        out = out.to(torch.float32).contiguous()
        cache[key] = (sig, out)
        return out

    def cat_edata_csr(self, key: str = "sim") -> torch.Tensor:
        """Edge field of all relations, fp32, permuted into the plan's CSR edge order (cached; the cache follows
        re-assignment and in-place edits of the per-relation tensors)."""
        cache = self.__dict__.setdefault("_cat_cache", {})
        if self._edges_store is None and ("e", key) in cache:
            return cache[("e", key)][1]             # loader batch, per-relation fields never touched: stored at assembly time
        parts = [self._eframes[r][key] for r in self.canonical_etypes]
        sig = tuple((p.data_ptr(), tuple(p.shape), p.dtype, p._version) for p in parts)
        hit = cache.get(("e", key))
        if hit is not None and hit[0] == sig:
            return hit[1]
        plan = self.plan()
        if parts:
            flat = torch.cat([p.reshape(-1) for p in parts]).to(device=plan.device, dtype=torch.float32)
            out = flat[self._csr_perm()].contiguous() if flat.numel() else flat
        else:
            out = torch.empty(0, dtype=torch.float32, device=plan.device)
        cache[("e", key)] = (sig, out)
        return out

    def _csr_perm(self) -> torch.Tensor:
        """CSR position -> position in the relation-major concatenated edge list.  Loader-assembled plans do not carry
        it; their edge order is the same stable (segment, input order) sort, so it is recomputed from the COO."""
        plan = self.plan()
        if plan.perm is None:
            hd = PlanHeader(self.ntypes, self.canonical_etypes, [self.num_nodes(t) for t in self.ntypes])
            gseg = [hd.seg_off[hd.tindex[d]] + v.to(plan.device) * hd.R[hd.tindex[d]] + hd.slot_of_rel[ri]
                    for ri, ((s, e, d), (u, v)) in enumerate(self._edges.items())]
            gseg = torch.cat(gseg) if gseg else torch.empty(0, dtype=torch.int64, device=plan.device)
            plan.perm = torch.sort(gseg, stable=True).indices
        return plan.perm

    # ------------------------------------------------------------------ kernel plan
    def plan(self, per_relation_src: bool = False) -> GraphPlan:
        """Kernel plan.  ``per_relation_src``: source rows are numbered per (relation, source node) — the layout
        HGT needs, where every relation has its own transformed K/V table (models/HGT.py:92-97)."""
        if per_relation_src:
            cache = self.__dict__.setdefault("_plan_rel", None)
            if cache is None:
                self.__dict__["_plan_rel"] = cache = self._derived_rel_plan() or _build_plan(self, per_relation_src=True)
            return cache
        if self._plan is None:
            self._plan = _build_plan(self)
        return self._plan

    def _derived_rel_plan(self) -> Optional[GraphPlan]:
        """The per-relation-source plan of a GPU graph that was built from an assembled plan and holds no COO (loader batches, slot graphs),
        derived on the device from that plan (``plan_by_relation``) instead of rebuilding and sorting the COO; None where that does not apply
        (graphs made from COO, CPU graphs, more relations per source type than the kernel counts, per-relation rows that coincide with the
        nodes - ``finish_plan`` orders those sources by another rule)."""
        if not DERIVE_REL_PLAN or self._edges_store is not None or self._plan is None or self._plan.device.type != "cuda":
            return None
        hd = PlanHeader(self.ntypes, self.canonical_etypes, [self.num_nodes(t) for t in self.ntypes])
        hd.relation_table()
        if hd.max_src_rels > PLAN_REL_MAX_RELS or hd.rel_rows_total == hd.N or not hd.ntypes:
            return None
        return plan_by_relation(hd, self._plan)


class _PinnedArena:
    """Ring of page-locked host memory for small host->device transfers.

    On this ROCm stack a pageable ``torch.tensor(list, device='cuda')`` copy blocks the host until the GPU has drained
    (measured: the call took as long as the training step still queued), and ``tensor.pin_memory()`` per call costs a
    ``hipHostMalloc`` (also synchronising).  Both serialised batch preparation with the running step.  Carving the
    staging space out of one long-lived pinned buffer makes every small upload a plain asynchronous copy."""

    def __init__(self, nbytes: int = 32 << 20):
        self.buf = torch.empty(nbytes, dtype=torch.uint8).pin_memory()
        self.size = nbytes
        self.off = 0
        self.lap = 0
        self.pending = collections.deque()     # (lap, start, end, event) of the copies issued, in issue (= address, lap-major) order

    def stage(self, t: torch.Tensor, device: torch.device) -> torch.Tensor:
        nbytes = t.numel() * t.element_size()
        if nbytes == 0:
            return torch.empty(t.shape, dtype=t.dtype, device=device)
        need = (nbytes + 255) // 256 * 256
        if need > self.size:
            return t.to(device)                       # oversized: plain (blocking) copy
        if self.off + need > self.size:
            self.off = 0
            self.lap += 1
        start, end = self.off, self.off + need
        # a ring: only the copies of the PREVIOUS lap that still read from [start, end) must have left the buffer - the oldest
        # entries, long complete in steady state.  (Waiting for every pending copy at the wrap, as an earlier version did, also waits
        # for the ones just queued on the compute stream behind a whole training step: the host then idles until the GPU drains.)
        while self.pending:
            lap, a, b, evt = self.pending[0]
            if lap == self.lap or (lap == self.lap - 1 and a >= end):
                break
            evt.synchronize()
            self.pending.popleft()
        view = self.buf[start:start + nbytes].view(t.dtype).view(t.shape)
        view.copy_(t)
        out = view.to(device, non_blocking=True)
        evt = torch.cuda.Event()
        evt.record(torch.cuda.current_stream(device))
        self.off = end
        self.pending.append((self.lap, start, end, evt))
        return out


_ARENAS: dict = {}


def host_to_device(values, dtype, device) -> torch.Tensor:
    """Small host list/tensor -> device tensor as an ASYNCHRONOUS copy on the current stream (see _PinnedArena)."""
    t = values.to(dtype).contiguous() if isinstance(values, torch.Tensor) else torch.tensor(values, dtype=dtype)
    device = torch.device(device)
    if device.type != "cuda":
        return t
    key = device.index if device.index is not None else torch.cuda.current_device()
    arena = _ARENAS.get(key)
    if arena is None:
        arena = _ARENAS[key] = _PinnedArena()
    return arena.stage(t, device)


class SegmentTable:
    """Host builder of a segment descriptor table (include/wsi_hgnn.h, "Segment descriptor tables"): rows of ten words
    ``[out, in1, in2, tab_off, key, add, stride, n, mode, block_start]``, then the lookup tables.  Every segment is checked against the bounds of
    the table it writes before anything is launched.  ``who`` names the caller in the error messages.  Plain lists: this runs per batch."""

    def __init__(self, who: str):
        self.who, self.segs, self.tabs, self.names, self.blocks = who, [], [], {}, 0       # blocks: 1024-element blocks of the launch

    def table(self, name: str, words: Sequence[int]) -> int:
        """Register a lookup table behind the descriptors; the handle (also ``names[name]``) is what ``seg(tab=...)`` takes."""
        self.names[name] = len(self.tabs)
        self.tabs += words
        return self.names[name]

    def seg(self, out: torch.Tensor, off, n, in1=None, in2=None, tab=None, key=0, add=0, stride=0, mode=0, esize=4) -> None:
        """``n`` elements of ``esize`` bytes from element ``off`` of ``out`` (all numbers Python ints); nothing for ``n == 0``.  ``in1``: a tensor,
        or a raw pointer (mode 12's second output)."""
        if n <= 0:
            return
        if off < 0 or (off + n) * esize > out.nbytes:
            raise RuntimeError(f"{self.who}: a segment leaves the table it writes ({off} + {n} elements of {esize} bytes into {out.nbytes} bytes)")
        if in1 is None or isinstance(in1, int):
            p1 = in1 or 0
        else:
            if mode in (0, 1, 5) and in1.nbytes < n * (8 if mode == 0 else esize):
                raise RuntimeError(f"{self.who}: a segment reads past its source ({n} elements from {in1.nbytes} bytes)")
            p1 = in1.data_ptr()
        self.segs.append([out.data_ptr() + off * esize, p1, 0 if in2 is None else in2.data_ptr(), -1 if tab is None else tab,
                          key, add, stride, n, mode, self.blocks])
        self.blocks += (n + 1023) // 1024

    @property
    def nsegs(self) -> int:
        return len(self.segs)

    def upload(self, dev) -> torch.Tensor:
        """The device table (ONE upload), ``tab_off`` counted from the table's start.  The caller keeps it alive until the launch has run."""
        tab0 = len(self.segs) * 10
        words: List[int] = []
        for s_ in self.segs:
            words += s_
            if s_[3] >= 0:
                words[-7] += tab0
        words += self.tabs
        # (through array: torch.tensor walks a list of Python ints at twice the cost)
        return host_to_device(torch.frombuffer(array.array("q", words), dtype=torch.int64), torch.int64, dev)


def _count(idx: torch.Tensor, size: int) -> torch.Tensor:
    """``torch.bincount(idx, minlength=size)`` without its device->host sync (bincount reads max(idx) on the host)."""
    out = torch.zeros(size, dtype=torch.int64, device=idx.device)
    if idx.numel():
        out.index_add_(0, idx, torch.ones_like(idx))
    return out


class PlanHeader:
    """Host-side part of a plan: schema, per-type offsets, relation slots (no device work)."""

    def __init__(self, ntypes: List[str], rels: List[CanonicalEType], counts: List[int]):
        self.ntypes, self.rels, self.counts = ntypes, rels, counts
        self.tindex = {t: i for i, t in enumerate(ntypes)}
        self.type_off = [0]
        for c in counts:
            self.type_off.append(self.type_off[-1] + c)
        self.N = self.type_off[-1]
        slots: List[List[int]] = [[] for _ in ntypes]
        self.slot_of_rel: List[int] = []
        for ri, (s, e, d) in enumerate(rels):
            self.slot_of_rel.append(len(slots[self.tindex[d]]))
            slots[self.tindex[d]].append(ri)
        self.R = [len(x) for x in slots]                    # relations whose dst type is t (empty relations included)
        self.seg_off = [0]
        for ti in range(len(ntypes)):
            self.seg_off.append(self.seg_off[-1] + counts[ti] * self.R[ti])
        self.S = self.seg_off[-1]
        self.rel_rows: List[Tuple[int, int]] = []           # per-relation source row ranges (per_relation_src layout)
        off = 0
        for (s, e, d) in rels:
            ns = counts[self.tindex[s]]
            self.rel_rows.append((off, off + ns))
            off += ns
        self.rel_rows_total = off

    def relation_table(self) -> List[int]:
        """The int32 header table of ``wsi_plan_by_relation`` (include/wsi_hgnn.h): what maps an edge's softmax segment to its relation and a
        (relation, source node) to its row of the per-relation tables.  Also sets ``max_src_rels``: the most relations leaving one node type."""
        T, NR = len(self.ntypes), len(self.rels)
        slots: List[List[int]] = [[] for _ in range(T)]
        srel: List[List[int]] = [[] for _ in range(T)]
        rel_src, rel_k = [], []
        for ri, (s, e, d) in enumerate(self.rels):
            slots[self.tindex[d]].append(ri)
            rel_src.append(self.tindex[s])
            rel_k.append(len(srel[self.tindex[s]]))
            srel[self.tindex[s]].append(ri)
        ptr = lambda lists: [sum(len(x) for x in lists[:i]) for i in range(T + 1)]
        self.max_src_rels = max((len(x) for x in srel), default=0)
        return ([T, NR, self.rel_rows_total, self.N] + self.type_off + self.seg_off + self.R + ptr(slots) + [r for x in slots for r in x]
                + [lo for lo, _ in self.rel_rows] + rel_src + rel_k + ptr(srel) + [r for x in srel for r in x])


# In-degree above which a node goes to the cooperative hub kernels (passed to the kernels with every call: ops._attn_flags).
# Attention ms per step by threshold 32 / 64 / 96 / 128 / 192: synthetic hub batch 2.50 / 2.44 / 2.44 / 2.44 / 2.49; kNN study graphs
# in construction order 2.58 / 2.39 / - / 2.35 / -: one workgroup per node only pays for long chains.
HEAVY_DEGREE = 128
# Locality-ordered (kNN) graphs: every node that is pulled out of the position order into the hub prefix costs locality, and a
# single wave walks a few dozen neighbouring rows out of L2 quickly; measured on the WSI-like study graphs (attention ms per step):
# threshold 32 -> 2.15, 64 -> 2.56, 128 -> 3.04 with the top-N/32 candidates in the prefix; no hub split at all -> 1.93.  So only
# the nodes ABOVE a high threshold go to the hub kernels and nothing else leaves the position order.
HEAVY_DEGREE_LOCALITY = 128
# Two more plan switches (module attributes like the thresholds above; `set_plan_options` sets any of them - the package reads no environment
# variable): HUB_SPLIT = False never routes a node to the hub kernels; LOCALITY = False ignores the slides' '_pos' (heaviest-first orders).
HUB_SPLIT = True
LOCALITY = True
# False: ``HeteroGraph.plan(per_relation_src=True)`` always rebuilds from the COO (``_build_plan``), never derives from the assembled plan
# (``plan_by_relation``): the A/B switch of tools/hgt_slot_bench.py.
DERIVE_REL_PLAN = True


def set_plan_options(heavy_degree: Optional[int] = None, heavy_degree_locality: Optional[int] = None, hub_split: Optional[bool] = None,
                     locality: Optional[bool] = None) -> None:
    """Options of every kernel plan built FROM NOW ON (cached plans keep what they were built with)."""
    global HEAVY_DEGREE, HEAVY_DEGREE_LOCALITY, HUB_SPLIT, LOCALITY
    if heavy_degree is not None:
        HEAVY_DEGREE = int(heavy_degree)
    if heavy_degree_locality is not None:
        HEAVY_DEGREE_LOCALITY = int(heavy_degree_locality)
    if hub_split is not None:
        HUB_SPLIT = bool(hub_split)
    if locality is not None:
        LOCALITY = bool(locality)


def _new_plan(hd: PlanHeader, dev) -> GraphPlan:
    """An empty plan with the fields that come from the header alone."""
    p = GraphPlan()
    p.device = dev
    p.type_off, p.num_nodes, p.rel_slots, p.num_segs, p.rel_rows = hd.type_off, hd.N, hd.R, hd.S, list(hd.rel_rows)
    return p


def _set_readout_ptr(p: GraphPlan, hd: PlanHeader, batch_counts: List[List[int]]) -> None:
    """``batch_size`` and the readout pointers (first row of every (node type, graph)) of ``batch_counts[type][graph]``."""
    B = len(batch_counts[0]) if batch_counts else 1
    p.batch_size = B
    ptr = [0]
    for ti in range(len(hd.ntypes)):
        base, acc = hd.type_off[ti], 0
        for b in range(B):
            acc += int(batch_counts[ti][b])
            ptr.append(base + acc)
        if acc != hd.counts[ti]:
            raise ValueError(f"batch_num_nodes of type {hd.ntypes[ti]} does not sum to its node count")
    p.readout_ptr = host_to_device(ptr, torch.int32, p.device)


def finish_plan(hd: PlanHeader, gsrc, gdst, gseg, dev, per_relation_src: bool,
                batch_counts: List[List[int]], max_in_degree: Optional[int] = None, pos: Optional[torch.Tensor] = None) -> GraphPlan:
    """Device part of the plan from the concatenated global edge arrays (int64, any order): CSR by (dst, relation slot),
    CSC by source row, degree orders, readout pointers.  No device->host synchronisation when the caller knows
    ``max_in_degree`` (the loader does, per stored graph); otherwise it is read back once (one sync per plan)."""
    p = _new_plan(hd, dev)
    N, S = hd.N, hd.S
    node_seg = torch.empty(N + 1, dtype=torch.int64, device=dev)
    inv_rd = torch.empty(N, dtype=torch.float32, device=dev)
    for ti in range(len(hd.ntypes)):
        n = hd.counts[ti]
        a, b = hd.type_off[ti], hd.type_off[ti + 1]
        node_seg[a:b] = hd.seg_off[ti] + torch.arange(n, device=dev, dtype=torch.int64) * hd.R[ti]
        inv_rd[a:b] = (1.0 / hd.R[ti]) if hd.R[ti] > 0 else 0.0
    node_seg[N:].fill_(S)        # (not `node_seg[N] = S`: a scalar __setitem__ is a synchronising pageable copy)
    E = int(gsrc.numel())
    p.num_edges = E
    if E >= 2 ** 31 - 1 or S >= 2 ** 31 - 1:
        raise ValueError("graph too large for the int32 kernel plan")
    perm = torch.sort(gseg, stable=True).indices if E else gseg
    src_c = gsrc[perm]
    dst_c = gdst[perm]
    seg_c = gseg[perm]
    rowptr = torch.zeros(S + 1, dtype=torch.int64, device=dev)
    if E:
        rowptr[1:] = torch.cumsum(_count(seg_c, S), 0)
    p.perm = perm
    p.src = src_c.to(torch.int32).contiguous()
    p.rowptr = rowptr.to(torch.int32).contiguous()
    p.node_seg = node_seg.to(torch.int32).contiguous()
    p.inv_rd = inv_rd.contiguous()
    NS = hd.rel_rows_total if per_relation_src else N
    p.num_src_rows = NS
    cperm = torch.sort(src_c, stable=True).indices if E else src_c
    colptr = torch.zeros(NS + 1, dtype=torch.int64, device=dev)
    if E:
        colptr[1:] = torch.cumsum(_count(src_c, NS), 0)
    p.colptr = colptr.to(torch.int32).contiguous()
    p.csc_eid = cperm.to(torch.int32).contiguous()
    p.csc_dst = dst_c[cperm].to(torch.int32).contiguous() if E else dst_c.to(torch.int32)
    indeg = _count(dst_c, N)
    outdeg = colptr[1:] - colptr[:-1]
    B = len(batch_counts[0]) if batch_counts else 1
    p.batch_size = B
    # Processing orders.  dst side: the M highest in-degree nodes first (candidates for the hub kernel, wsi_heat_attn_fwd's
    # num_heavy), then graph-major and heaviest-first inside a graph: all CUs work on ONE graph's K/V rows at a time (41 MB
    # at 10k nodes, D=512), which the 256 MB Infinity Cache holds, instead of sweeping the whole batch's tables.
    M = 0 if not HUB_SPLIT else min(N, max(64, N // 32))
    if M > 0:
        if max_in_degree is None:
            max_in_degree = int(indeg.max().item()) if E else 0
        if max_in_degree <= HEAVY_DEGREE:      # no hubs in this batch: skip the second launch and its fork/join
            M = 0
    p.num_heavy = M
    if pos is not None and NS == N:
        # Locality order (graph.apply_locality_order): inside a graph, nodes are visited in the order of their positions in the
        # slide's bandwidth-reducing order, across node types, so that the waves in flight at any time gather K/V rows of
        # neighbouring patches (kNN graphs: a small, L2-sized set) — instead of heaviest-first, which scatters them.
        flat = [int(batch_counts[ti][b]) for ti in range(len(hd.ntypes)) for b in range(B)]
        gid = torch.arange(B, device=dev).repeat(len(hd.ntypes)).repeat_interleave(host_to_device(flat, torch.int64, dev), output_size=N)
        key = gid * (int(N) + 1) + pos.to(device=dev, dtype=torch.int64)
        kd = key.clone()
        p.heavy_degree = HEAVY_DEGREE_LOCALITY
        M = int((indeg > HEAVY_DEGREE_LOCALITY).sum().item()) if (M > 0 and max_in_degree > HEAVY_DEGREE_LOCALITY) else 0
        p.num_heavy = M
        if M > 0:                  # exactly the nodes above the threshold, heaviest first; everything else stays in position order
            top = torch.topk(indeg, M, sorted=True).indices
            kd[top] = torch.arange(M, device=dev, dtype=kd.dtype) - M
        p.order_dst = torch.sort(kd, stable=True).indices.to(torch.int32).contiguous()
        p.order_src = torch.sort(key, stable=True).indices.to(torch.int32).contiguous()
        p.locality = True
    elif B == 1 and M == 0:
        p.order_dst = torch.sort(indeg, descending=True, stable=True).indices.to(torch.int32).contiguous()
        p.order_src = torch.sort(outdeg, descending=True, stable=True).indices.to(torch.int32).contiguous()
    else:
        flat = [int(batch_counts[ti][b]) for ti in range(len(hd.ntypes)) for b in range(B)] if batch_counts else [N]
        reps = len(hd.ntypes) if batch_counts else 1
        gid = torch.arange(B, device=dev).repeat(reps).repeat_interleave(host_to_device(flat, torch.int64, dev), output_size=N)
        big = E + 1
        kd = gid * big + (E - indeg)
        if M > 0:
            top = torch.topk(indeg, M, sorted=True).indices
            kd[top] = torch.arange(M, device=dev, dtype=kd.dtype) - M           # negative keys: ahead of everything, by rank
        p.order_dst = torch.sort(kd, stable=True).indices.to(torch.int32).contiguous()
        p.order_src = torch.sort(gid[:NS] * big + (E - outdeg), stable=True).indices.to(torch.int32).contiguous() \
            if NS == N else torch.sort(outdeg, descending=True, stable=True).indices.to(torch.int32).contiguous()
    _set_readout_ptr(p, hd, batch_counts)
    return p


class PlanPieces:
    """Per-graph, per-node-type pieces of a single graph's kernel plan, kept on the device so that the plan of ANY batch
    containing the graph is a concatenation plus offset additions — no sort, no host synchronisation (data.py).

    The batch layout is type-major (all graphs' type-0 nodes, then type-1, ...), a single graph's plan is type-major too,
    so the edges whose destination has type t are one contiguous CSR range of the graph and the CSC entries whose source
    has type s likewise; inside a piece only local ids are stored, with the node type of the other endpoint per entry."""

    def __init__(self, hd: PlanHeader, plan: GraphPlan, sim_csr: torch.Tensor, pos: Optional[torch.Tensor] = None):
        dev = plan.device
        T = len(hd.ntypes)
        toff = torch.tensor(hd.type_off, dtype=torch.int64, device=dev)
        rowptr, colptr = plan.rowptr.long(), plan.colptr.long()
        e_start = rowptr[torch.tensor(hd.seg_off, dtype=torch.int64, device=dev)].tolist()          # one sync, once per graph
        c_start = colptr[toff].tolist()
        self.counts = list(hd.counts)
        self.ecount = [e_start[t + 1] - e_start[t] for t in range(T)]
        self.ccount = [c_start[t + 1] - c_start[t] for t in range(T)]
        src = plan.src.long()
        src_t = torch.bucketize(src, toff[1:], right=True)
        src_l = src - toff[src_t]
        eid = plan.csc_eid.long()
        es = torch.tensor(e_start, dtype=torch.int64, device=dev)
        dt = torch.bucketize(eid, es[1:], right=True)                    # destination type of each CSC entry's edge
        eid_l = eid - es[dt]
        dst_l = plan.csc_dst.long() - toff[dt]
        ns = plan.node_seg.long()
        indeg = rowptr[ns[1:]] - rowptr[ns[:-1]]
        outdeg = colptr[1:] - colptr[:-1]
        self.rp, self.src_l, self.src_t, self.sim = [], [], [], []
        self.cp, self.eid_l, self.ent_t, self.dst_l = [], [], [], []
        heavy_l, heavy_t, light_l, light_t, so_l, so_t, nheavy = [], [], [], [], [], [], []
        for t in range(T):
            a, b = hd.seg_off[t], hd.seg_off[t + 1]
            self.rp.append(rowptr[a:b] - e_start[t])
            sl = slice(e_start[t], e_start[t + 1])
            self.src_l.append(src_l[sl]); self.src_t.append(src_t[sl]); self.sim.append(sim_csr[sl])
            na, nb = hd.type_off[t], hd.type_off[t + 1]
            self.cp.append(colptr[na:nb] - c_start[t])
            cl = slice(c_start[t], c_start[t + 1])
            self.eid_l.append(eid_l[cl]); self.ent_t.append(dt[cl]); self.dst_l.append(dst_l[cl])
            deg = indeg[na:nb]
            od = torch.sort(deg, descending=True, stable=True).indices
            h = int((deg > (HEAVY_DEGREE_LOCALITY if pos is not None else HEAVY_DEGREE)).sum().item())
            nheavy.append(h)
            tt = torch.full((nb - na,), t, dtype=torch.int64, device=dev)
            heavy_l.append(od[:h]); heavy_t.append(tt[:h]); light_l.append(od[h:]); light_t.append(tt[h:])
            so_l.append(torch.sort(outdeg[na:nb], descending=True, stable=True).indices); so_t.append(tt)
        cat = lambda xs: torch.cat(xs) if xs else torch.empty(0, dtype=torch.int64, device=dev)
        self.heavy_l, self.heavy_t, self.light_l, self.light_t = cat(heavy_l), cat(heavy_t), cat(light_l), cat(light_t)
        self.so_l, self.so_t = cat(so_l), cat(so_t)
        self.locality = pos is not None
        if pos is not None:      # locality order (apply_locality_order): light destinations and all sources by slide-wide position
            pos = pos.to(device=dev, dtype=torch.int64)
            gl = self.light_l + toff[self.light_t]
            o = torch.sort(pos[gl], stable=True).indices
            self.light_l, self.light_t = self.light_l[o], self.light_t[o]
            gs_ = self.so_l + toff[self.so_t]
            o = torch.sort(pos[gs_], stable=True).indices
            self.so_l, self.so_t = self.so_l[o], self.so_t[o]
        self.num_heavy = sum(nheavy)
        self.max_in_degree = int(indeg.max().item()) if indeg.numel() else 0
        # what an augmented slot fill needs of the plan's sort (slot_fill_augmented): CSR position -> position in the slide's concatenated COO
        # (relations in sorted order), global CSC entry -> CSR position, the CSR / CSC range of every type; the packed maps are built on first use
        self._perm, self._csc_eid, self._e_start, self._c_start = getattr(plan, "perm", None), eid, e_start, c_start
        self._coo_maps = None

    def coo_maps(self, rel_sizes: Sequence[int]):
        """(csr_map[t], csc_map[t]): int64 per CSR edge into / CSC entry out of node type t, ``(relation << 40) | index in the slide's concatenated
        COO`` (relations in sorted order, ``rel_sizes`` edges each): which COO edge an entry of the stored pieces is.  Built once per stored graph."""
        if self._coo_maps is None:
            if self._perm is None:
                raise RuntimeError("PlanPieces.coo_maps: the plan was not built from COO (no sort permutation kept)")
            dev = self._perm.device
            perm = self._perm.to(torch.int64)
            bounds = torch.tensor([sum(rel_sizes[:j + 1]) for j in range(len(rel_sizes))], dtype=torch.int64, device=dev)
            packed = perm | (torch.bucketize(perm, bounds, right=True) << 40) if perm.numel() else perm
            by_csc = packed[self._csc_eid] if perm.numel() else perm
            T = len(self.counts)
            self._coo_maps = ([packed[self._e_start[t]:self._e_start[t + 1]].contiguous() for t in range(T)],
                              [by_csc[self._c_start[t]:self._c_start[t + 1]].contiguous() for t in range(T)])
        return self._coo_maps


def plan_frame(hd: PlanHeader, dev, batch_counts: List[List[int]]) -> GraphPlan:
    """The parts of a plan that depend on the node counts only: node_seg, inv_rd, readout pointers."""
    p = _new_plan(hd, dev)
    N, S = hd.N, hd.S
    node_seg = torch.empty(N + 1, dtype=torch.int64, device=dev)
    inv_rd = torch.empty(N, dtype=torch.float32, device=dev)
    for ti in range(len(hd.ntypes)):
        n = hd.counts[ti]
        a, b = hd.type_off[ti], hd.type_off[ti + 1]
        node_seg[a:b] = hd.seg_off[ti] + torch.arange(n, device=dev, dtype=torch.int64) * hd.R[ti]
        inv_rd[a:b] = (1.0 / hd.R[ti]) if hd.R[ti] > 0 else 0.0
    node_seg[N:].fill_(S)        # (not `node_seg[N] = S`: a scalar __setitem__ is a synchronising pageable copy)
    p.node_seg = node_seg.to(torch.int32).contiguous()
    p.inv_rd = inv_rd.contiguous()
    _set_readout_ptr(p, hd, batch_counts)
    return p


def _batch_offsets(hd: PlanHeader, pieces: Sequence[PlanPieces], batch_counts: List[List[int]]):
    """Where the pieces go in a dense block-diagonal batch: ``pre[b][t]`` nodes of type t in front of slide b, ``node_tab[b*T + t]`` the first
    global id of (slide, type), ``eoff / coff[(t, b)]`` the first CSR edge / CSC entry of the piece, ``edge_tab[b*T + t]``, the edge count."""
    T, B = len(hd.ntypes), len(pieces)
    pre = [[0] * T for _ in range(B + 1)]
    for b in range(B):
        for t in range(T):
            pre[b + 1][t] = pre[b][t] + batch_counts[t][b]
    node_tab = [hd.type_off[t] + pre[b][t] for b in range(B) for t in range(T)]
    eoff, coff, acc_e, acc_c = {}, {}, 0, 0
    for t in range(T):
        for b in range(B):
            eoff[(t, b)], coff[(t, b)] = acc_e, acc_c
            acc_e += pieces[b].ecount[t]
            acc_c += pieces[b].ccount[t]
    if acc_e >= 2 ** 31 - 1 or hd.S >= 2 ** 31 - 1:
        raise ValueError("graph too large for the int32 kernel plan")
    return pre, node_tab, eoff, coff, [eoff[(t, b)] for b in range(B) for t in range(T)], acc_e


def _finish_assembled(p: GraphPlan, pieces: Sequence[PlanPieces]) -> None:
    """What an assembled plan takes from its pieces' flags: the hub prefix, the locality order (all of the slides or none), the threshold."""
    p.num_heavy = sum(pc.num_heavy for pc in pieces) if HUB_SPLIT else 0
    p.locality = all(pc.locality for pc in pieces)
    if any(pc.locality for pc in pieces) and not p.locality:
        raise ValueError("a batch mixes locality-ordered and plain graphs: apply graph.apply_locality_order to all of a data set's slides or none")
    p.heavy_degree = HEAVY_DEGREE_LOCALITY if p.locality else HEAVY_DEGREE


def _piece_segments(tb: SegmentTable, out: Dict[str, torch.Tensor], hd: PlanHeader, pc: PlanPieces, t: int, key: int, so: int, row: int, eo: int, co: int):
    """The plan segments of one (node type, slide): relation-slot segments from ``so``, nodes from ``row``, CSR edges from ``eo``, CSC entries
    from ``co``; ``key`` = slide * T, the slide's row of the "node" / "edge" lookup tables."""
    node, edge = tb.names["node"], tb.names["edge"]
    nc, ne, ncc = pc.counts[t], pc.ecount[t], pc.ccount[t]
    tb.seg(out["rowptr"], so, nc * hd.R[t], in1=pc.rp[t], add=eo)
    tb.seg(out["colptr"], row, nc, in1=pc.cp[t], add=co)
    tb.seg(out["src"], eo, ne, in1=pc.src_l[t], in2=pc.src_t[t], tab=node, key=key)
    tb.seg(out["sim"], eo, ne, in1=pc.sim[t], mode=1)
    tb.seg(out["csc_eid"], co, ncc, in1=pc.eid_l[t], in2=pc.ent_t[t], tab=edge, key=key)
    tb.seg(out["csc_dst"], co, ncc, in1=pc.dst_l[t], in2=pc.ent_t[t], tab=node, key=key)


def _order_segments(tb: SegmentTable, out: Dict[str, torch.Tensor], pc: PlanPieces, key: int, ho: int, lo: int, oo: int):
    """The processing-order segments of one slide: its hubs from ``ho`` and its light destinations from ``lo`` of order_dst, its sources from
    ``oo`` of order_src.  Returns the three positions behind them."""
    node = tb.names["node"]
    nh, nl, no = int(pc.heavy_l.numel()), int(pc.light_l.numel()), int(pc.so_l.numel())
    tb.seg(out["order_dst"], ho, nh, in1=pc.heavy_l, in2=pc.heavy_t, tab=node, key=key)
    tb.seg(out["order_dst"], lo, nl, in1=pc.light_l, in2=pc.light_t, tab=node, key=key)
    tb.seg(out["order_src"], oo, no, in1=pc.so_l, in2=pc.so_t, tab=node, key=key)
    return ho + nh, lo + nl, oo + no


def _frame_segments(tb: SegmentTable, out: Dict[str, torch.Tensor], hd: PlanHeader, E: int) -> None:
    """node_seg and inv_rd of the header's node counts, and the closing words of rowptr, colptr and node_seg."""
    for t in range(len(hd.ntypes)):
        R = hd.R[t]
        tb.seg(out["node_seg"], hd.type_off[t], hd.counts[t], add=hd.seg_off[t], stride=R)
        tb.seg(out["inv_rd"], hd.type_off[t], hd.counts[t], add=_float_bits([(1.0 / R) if R > 0 else 0.0])[0], mode=2)
    tb.seg(out["rowptr"], hd.S, 1, add=E)
    tb.seg(out["colptr"], hd.N, 1, add=E)
    tb.seg(out["node_seg"], hd.N, 1, add=hd.S)


def assemble_plan(hd: PlanHeader, pieces: Sequence[PlanPieces], dev, batch_counts: List[List[int]]):
    """Plan of the block-diagonal batch of the graphs whose pieces are given (+ the CSR-ordered ``sim``).  Every table is a concatenation of
    the pieces with per-piece offsets (node / edge ids through two small lookup tables): on the GPU ONE launch over a table of segment
    descriptors (``wsi_plan_assemble``; one upload), no sort, no device->host synchronisation.  ``assemble_plan_torch`` is the same thing as
    ~90 tensor operations (CPU graphs; the kernel's test compares the two bit for bit)."""
    dev = torch.device(dev)
    if dev.type != "cuda":
        return assemble_plan_torch(hd, pieces, dev, batch_counts)
    from . import _native as N
    T = len(hd.ntypes)
    p = _new_plan(hd, dev)
    _set_readout_ptr(p, hd, batch_counts)
    Nn, S = hd.N, hd.S
    pre, node_tab, eoff, coff, edge_tab, E = _batch_offsets(hd, pieces, batch_counts)
    p.num_edges, p.num_src_rows = E, Nn
    mk = lambda n, dt=torch.int32: torch.empty(n, dtype=dt, device=dev) if n > 0 else torch.empty(1, dtype=dt, device=dev)[:0]
    out = {"rowptr": mk(S + 1), "colptr": mk(Nn + 1), "node_seg": mk(Nn + 1), "src": mk(E), "csc_eid": mk(E), "csc_dst": mk(E),
           "order_dst": mk(Nn), "order_src": mk(Nn), "sim": mk(E, torch.float32), "inv_rd": mk(Nn, torch.float32)}
    tb = SegmentTable("plan_assemble")
    tb.table("node", node_tab)
    tb.table("edge", edge_tab)
    for t in range(T):
        for b, pc in enumerate(pieces):
            _piece_segments(tb, out, hd, pc, t, b * T, hd.seg_off[t] + pre[b][t] * hd.R[t], node_tab[b * T + t], eoff[(t, b)], coff[(t, b)])
    pos = (0, sum(pc.num_heavy for pc in pieces), 0)
    for b, pc in enumerate(pieces):                 # processing orders: exact hub list first, then graph-major / heaviest-first inside (graph, type)
        pos = _order_segments(tb, out, pc, b * T, *pos)
    _frame_segments(tb, out, hd, E)
    desc = tb.upload(dev)
    N.check(N.load().wsi_plan_assemble(N.ptr(desc), tb.nsegs, tb.blocks, N.stream()), "wsi_plan_assemble")
    sim = out.pop("sim")
    for k, v in out.items():
        setattr(p, k, v)
    p._assembly_desc = desc             # (the pieces are owned by the stored graphs; the descriptor table must outlive the launch: held by the plan)
    _finish_assembled(p, pieces)
    return p, sim


def assemble_plan_torch(hd: PlanHeader, pieces: Sequence[PlanPieces], dev, batch_counts: List[List[int]]):
    """``assemble_plan`` as tensor operations: concatenations, two small offset tables and a few gathers (~90 launches on a GPU)."""
    T, B = len(hd.ntypes), len(pieces)
    p = plan_frame(hd, dev, batch_counts)
    N, S = hd.N, hd.S
    _, node_tab, eoff, coff, edge_tab, E = _batch_offsets(hd, pieces, batch_counts)
    p.num_edges, p.num_src_rows = E, N
    order = [(t, b) for t in range(T) for b in range(B)]
    tabs = host_to_device([node_tab, edge_tab], torch.int64, dev)     # [2, B*T]
    meta = host_to_device([[eoff[k] for k in order], [pieces[b].counts[t] * hd.R[t] for (t, b) in order],
                           [coff[k] for k in order], [pieces[b].counts[t] for (t, b) in order],
                           [b * T for (t, b) in order], [pieces[b].ecount[t] for (t, b) in order],
                           [pieces[b].ccount[t] for (t, b) in order]], torch.int64, dev)                        # [7, T*B]
    ri = torch.repeat_interleave
    rowptr = torch.empty(S + 1, dtype=torch.int64, device=dev)
    torch.add(torch.cat([pieces[b].rp[t] for (t, b) in order]), ri(meta[0], meta[1], output_size=S), out=rowptr[:S])
    rowptr[S:].fill_(E)
    colptr = torch.empty(N + 1, dtype=torch.int64, device=dev)
    torch.add(torch.cat([pieces[b].cp[t] for (t, b) in order]), ri(meta[2], meta[3], output_size=N), out=colptr[:N])
    colptr[N:].fill_(E)
    ekey = ri(meta[4], meta[5], output_size=E)                        # b*T of every CSR edge
    ckey = ri(meta[4], meta[6], output_size=E)                        # b*T of every CSC entry
    src = torch.cat([pieces[b].src_l[t] for (t, b) in order]) + tabs[0][ekey + torch.cat([pieces[b].src_t[t] for (t, b) in order])]
    ent = ckey + torch.cat([pieces[b].ent_t[t] for (t, b) in order])
    csc_eid = torch.cat([pieces[b].eid_l[t] for (t, b) in order]) + tabs[1][ent]
    csc_dst = torch.cat([pieces[b].dst_l[t] for (t, b) in order]) + tabs[0][ent]
    sim = torch.cat([pieces[b].sim[t] for (t, b) in order])
    # processing orders: exact hub list first, then graph-major / heaviest-first inside (graph, type)
    bkeys = host_to_device([[b * T for b in range(B)], [int(pc.heavy_l.numel()) for pc in pieces],
                            [int(pc.light_l.numel()) for pc in pieces], [int(pc.so_l.numel()) for pc in pieces]], torch.int64, dev)
    H = sum(pc.num_heavy for pc in pieces)
    heavy = torch.cat([pc.heavy_l for pc in pieces]) + tabs[0][ri(bkeys[0], bkeys[1], output_size=H) + torch.cat([pc.heavy_t for pc in pieces])]
    light = torch.cat([pc.light_l for pc in pieces]) + tabs[0][ri(bkeys[0], bkeys[2], output_size=N - H) + torch.cat([pc.light_t for pc in pieces])]
    osrc = torch.cat([pc.so_l for pc in pieces]) + tabs[0][ri(bkeys[0], bkeys[3], output_size=N) + torch.cat([pc.so_t for pc in pieces])]
    p.rowptr, p.colptr = rowptr.to(torch.int32), colptr.to(torch.int32)
    p.src, p.csc_eid, p.csc_dst = src.to(torch.int32), csc_eid.to(torch.int32), csc_dst.to(torch.int32)
    p.order_dst = torch.cat([heavy, light]).to(torch.int32)
    p.order_src = osrc.to(torch.int32)
    _finish_assembled(p, pieces)
    return p, sim


# ------------------------------------------------------------------ padded batch slots
# A SLOT is a batch of fixed shape: up to ``b_cap`` real slides, empty graphs up to ``b_cap``, and one FILLER graph that takes every node and
# edge the real slides leave of the slot's capacities.  The filler's label is -100, so it adds nothing to the loss or to any gradient, and a
# block-diagonal batch keeps it away from the real slides' logits: a training step captured once over the slot's static buffers replays over
# every batch that fits (data.BatchSlot, trainer.CapturedSlotStep).

def filler_graph(ntypes: Sequence[str], rels: Sequence[CanonicalEType], nf: Sequence[int], ef: Sequence[int], in_dim: int) -> HeteroGraph:
    """The filler of a slot as an ordinary graph: ``nf[t]`` all-zero nodes of node type ``ntypes[t]`` (sorted, as ``HeteroGraph.ntypes``) and,
    for every destination type t with ``ef[t] > 0``, ``ef[t]`` edges with ``sim = 0`` in the first relation (sorted order) whose destination
    type is t: edge j runs from source ``j mod nf[s]`` to destination ``j mod nf[t]`` - spread over both endpoints, so that neither the
    destination-major nor the source-major kernels meet a hub.  Every other relation is present and empty."""
    ntypes = [str(t) for t in ntypes]
    rels = sorted(tuple(str(x) for x in r) for r in rels)
    hd = PlanHeader(ntypes, rels, [int(x) for x in nf])
    edges, sim = OrderedDict(), {}
    for ri, (s, e, d) in enumerate(rels):
        td, ts = hd.tindex[d], hd.tindex[s]
        k = int(ef[td]) if hd.slot_of_rel[ri] == 0 else 0
        if k and (nf[td] < 1 or nf[ts] < 1):
            raise ValueError("filler_graph: edges need at least one node at both ends")
        j = torch.arange(k, dtype=torch.int64)
        edges[(s, e, d)] = (j % max(int(nf[ts]), 1), j % max(int(nf[td]), 1))
        sim[(s, e, d)] = torch.zeros(k, dtype=torch.float32)
    for t in range(len(ntypes)):
        if ef[t] and hd.R[t] == 0:
            raise ValueError(f"filler_graph: node type {ntypes[t]!r} has no incoming relation to carry edges")
    feat = {t: torch.zeros((int(nf[i]), int(in_dim)), dtype=torch.float32) for i, t in enumerate(ntypes)}
    return HeteroGraph.from_coo(OrderedDict(zip(ntypes, [int(x) for x in nf])), edges, feat=feat, sim=sim)


READOUT_CHUNK = 128     # rows per chunk of the readout's ReducePlan (ops.ReducePlan.from_ptr's default, which pooling.readout uses)


class SlotLayout:
    """Capacities of a slot and what follows from them alone: ``n_cap[t]`` nodes per node type, ``e_cap[t]`` edges per DESTINATION node type
    (0 where the type has no incoming relation), ``b_cap`` slides.  All shapes of the padded batch are functions of these."""

    def __init__(self, ntypes: Sequence[str], rels: Sequence[CanonicalEType], n_cap: Sequence[int], e_cap: Sequence[int], b_cap: int, in_dim: int):
        self.ntypes, self.rels = [str(t) for t in ntypes], [tuple(str(x) for x in r) for r in rels]
        if self.ntypes != sorted(self.ntypes) or self.rels != sorted(self.rels):
            raise ValueError("SlotLayout: node types and relations in sorted order (HeteroGraph.ntypes / canonical_etypes)")
        self.n_cap, self.e_cap, self.b_cap, self.in_dim = [int(x) for x in n_cap], [int(x) for x in e_cap], int(b_cap), int(in_dim)
        self.T, self.graphs = len(self.ntypes), self.b_cap + 1
        self.hd = hd = PlanHeader(self.ntypes, self.rels, self.n_cap)
        if self.b_cap < 1 or any(n < 1 for n in self.n_cap) or any(e < 0 for e in self.e_cap):
            raise ValueError("SlotLayout: b_cap >= 1, n_cap >= 1 (the filler keeps one node of every type), e_cap >= 0")
        self.src_type = [-1] * self.T                      # source type of relation slot 0 of every destination type: where filler edges come from
        for ri, (s, e, d) in enumerate(self.rels):
            if hd.slot_of_rel[ri] == 0:
                self.src_type[hd.tindex[d]] = hd.tindex[s]
        if any(self.e_cap[t] and hd.R[t] == 0 for t in range(self.T)):
            raise ValueError("SlotLayout: e_cap must be 0 for a node type without incoming relation")
        self.ebase = [0]
        for e in self.e_cap:
            self.ebase.append(self.ebase[-1] + e)
        self.N, self.S, self.E = hd.N, hd.S, self.ebase[-1]
        if self.E >= 2 ** 31 - 1 or self.S >= 2 ** 31 - 1:
            raise ValueError("slot too large for the int32 kernel plan")
        self.num_segs = self.T * self.graphs               # readout segments (node type, graph)
        # every graph adds at most one short chunk per node type to the ceil(n / chunk) full ones
        self.c_cap = sum((n + READOUT_CHUNK - 1) // READOUT_CHUNK + self.graphs for n in self.n_cap)

    def buffers(self, device) -> Dict[str, torch.Tensor]:
        """The slot's static tables (uninitialised): written by ``slot_fill``, read by every step on the slot."""
        dev = torch.device(device)
        mk = lambda n, dt: torch.empty(max(int(n), 1), dtype=dt, device=dev)[:int(n)]
        i32, f32 = torch.int32, torch.float32
        N, S, E, K, C = self.N, self.S, self.E, self.num_segs, self.c_cap
        return {"rowptr": mk(S + 1, i32), "colptr": mk(N + 1, i32), "node_seg": mk(N + 1, i32), "src": mk(E, i32), "csc_eid": mk(E, i32),
                "csc_dst": mk(E, i32), "order_dst": mk(N, i32), "order_src": mk(N, i32), "sim": mk(E, f32), "inv_rd": mk(N, f32),
                "readout_ptr": mk(K + 1, i32), "labels": mk(self.graphs, torch.int64), "feat": mk(N * self.in_dim, f32).view(N, self.in_dim),
                "scales": mk(N, i32).view(N, 1), "edge_seg": mk(E, i32), "row_seg": mk(N, i32),
                "chunk_row": mk(C + 1, i32), "chunk_seg": mk(C, i32), "seg_chunk": mk(K + 1, i32),
                "seg_counts": mk(K, f32).view(K, 1), "seg_inv_counts": mk(K, f32).view(K, 1), "seg_nonempty": mk(K, f32).view(K, 1)}


class SlotBatch:
    """Host arithmetic of ONE batch placed in a slot: where every piece of every table goes.  Raises ValueError when the batch does not fit:
    more than ``b_cap`` slides, or for some node type t fewer than one node (``nf[t] = n_cap[t] - n[t] >= 1``) or fewer than zero edges
    (``ef[t] = e_cap[t] - e[t] >= 0``) left for the filler."""

    @staticmethod
    def fits(lay: SlotLayout, counts: Sequence[Sequence[int]], ecounts: Sequence[Sequence[int]], allow_empty_type: bool = False) -> bool:
        """``counts[b][t]`` / ``ecounts[b][t]``: nodes / edges (by destination type) of slide b.  ``allow_empty_type``: the layout of a batch in
        which some node type has no real node is still defined (an augmented batch after an unlucky draw: the filler takes the whole type) -
        ``BatchSlot.fits`` lets such a batch be STEPPED on a slot only when the slot carries a device-side presence table
        (``BatchSlot(type_mask=...)``, DESIGN 3.29: heads and optimizer then read, on the device, which types the real slides hold)."""
        if not 1 <= len(counts) <= lay.b_cap:
            return False
        if allow_empty_type:
            return all(lay.n_cap[t] - sum(c[t] for c in counts) >= 1 and lay.e_cap[t] - sum(e[t] for e in ecounts) >= 0 for t in range(lay.T))
        # a node type NO slide of the batch has is not padded: the models skip such a type's prediction head altogether (models/HEATNet4.py:216-221,
        # ``h[k].shape[0] > 0``), the filler's nodes would switch it on - such a batch does not fit and is stepped eagerly
        if any(sum(c[t] for c in counts) < 1 for t in range(lay.T)):
            return False
        return all(lay.n_cap[t] - sum(c[t] for c in counts) >= 1 and lay.e_cap[t] - sum(e[t] for e in ecounts) >= 0 for t in range(lay.T))

    def __init__(self, lay: SlotLayout, pieces: Sequence[PlanPieces], allow_empty_type: bool = False):
        T, hd, B = lay.T, lay.hd, len(pieces)
        if not SlotBatch.fits(lay, [pc.counts for pc in pieces], [pc.ecount for pc in pieces], allow_empty_type):
            raise ValueError("the batch does not fit the slot")
        self.B = B
        self.n = [sum(pc.counts[t] for pc in pieces) for t in range(T)]
        self.e = [sum(pc.ecount[t] for pc in pieces) for t in range(T)]
        self.nf = [lay.n_cap[t] - self.n[t] for t in range(T)]
        self.ef = [lay.e_cap[t] - self.e[t] for t in range(T)]
        self.pre = [[0] * T for _ in range(B + 1)]
        for b in range(B):
            for t in range(T):
                self.pre[b + 1][t] = self.pre[b][t] + pieces[b].counts[t]
        self.node_tab = [hd.type_off[t] + self.pre[b][t] for b in range(B) for t in range(T)]          # [b*T + t]: first global id of (slide, type)
        self.fb = [hd.type_off[t] + self.n[t] for t in range(T)]                                        # first filler node of the type
        self.feb = [lay.ebase[t] + self.e[t] for t in range(T)]                                         # first filler CSR edge into the type
        self.eoff, self.coff, self.cfb, acc_c = {}, {}, [], 0
        for t in range(T):
            acc_e = lay.ebase[t]
            for b in range(B):
                self.eoff[(t, b)], self.coff[(t, b)] = acc_e, acc_c
                acc_e += pieces[b].ecount[t]
                acc_c += pieces[b].ccount[t]
            self.cfb.append(acc_c)                                                                      # first CSC entry of the type's filler sources
            acc_c += sum(self.ef[d] for d in range(T) if lay.src_type[d] == t)
        if acc_c != lay.E:
            raise ValueError("slot: the pieces' CSR and CSC edge counts disagree")
        self.edge_tab = [self.eoff[(t, b)] for b in range(B) for t in range(T)]
        self.counts = [[pc.counts[t] for pc in pieces] + [0] * (lay.b_cap - B) + [self.nf[t]] for t in range(T)]    # [t][graph]
        self.readout_ptr = [0]
        for t in range(T):
            for c in self.counts[t]:
                self.readout_ptr.append(self.readout_ptr[-1] + c)
        self.filler_block = [T] + [w for t in range(T) for w in (self.nf[t], self.ef[t], self.fb[t], self.feb[t], lay.src_type[t], hd.R[t], self.cfb[t])]
        # the readout's ReducePlan (ops.ReducePlan.from_ranges over readout_ptr), padded to the slot's chunk capacity with empty chunks that no
        # segment owns: the launches over chunks keep one grid, the second stages never read them
        self.ranges = [(self.readout_ptr[i], self.readout_ptr[i + 1]) for i in range(lay.num_segs)]
        chunk_row, chunk_seg, seg_chunk = [], [], [0]
        for s_, (a, b_) in enumerate(self.ranges):
            r = a
            while r < b_:
                chunk_row.append(r)
                chunk_seg.append(s_)
                r = min(b_, r + READOUT_CHUNK)
            seg_chunk.append(len(chunk_row))
        pad = lay.c_cap - len(chunk_seg)
        if pad < 0:
            raise ValueError("slot: readout chunk capacity exceeded")
        self.chunk_row = chunk_row + [lay.N] * (pad + 1)
        self.chunk_seg = chunk_seg + [lay.num_segs - 1] * pad
        self.seg_chunk = seg_chunk
        self.seg_counts = [float(b_ - a) for a, b_ in self.ranges]
        self.seg_inv_counts = [1.0 / (b_ - a) if b_ > a else 0.0 for a, b_ in self.ranges]
        self.seg_nonempty = [1.0 if b_ > a else 0.0 for a, b_ in self.ranges]


def _piece_edge_seg(pc: PlanPieces, t: int, R: int) -> torch.Tensor:
    """int64 [ecount[t]]: the softmax segment (local: node * R + slot) of every CSR edge into node type t of a stored graph; expanded on the
    device once per stored graph (output size known: no synchronisation)."""
    cache = pc.__dict__.setdefault("_edge_seg", {})
    if t not in cache:
        rp = pc.rp[t]
        cnt = torch.cat([rp[1:], rp.new_full((1,), int(pc.ecount[t]))]) - rp if rp.numel() else rp
        cache[t] = torch.repeat_interleave(torch.arange(rp.numel(), dtype=torch.int64, device=rp.device), cnt, output_size=int(pc.ecount[t]))
    return cache[t]


def _float_bits(xs: Sequence[float]) -> List[int]:
    """The int32 bit patterns of the floats (rounded to fp32 to nearest)."""
    return list(struct.unpack(f"<{len(xs)}i", struct.pack(f"<{len(xs)}f", *xs)))


def slot_fill(lay: SlotLayout, bufs: Dict[str, torch.Tensor], pieces: Sequence[PlanPieces], labels: Sequence[int],
              feats: Sequence[Sequence[torch.Tensor]], scales: Optional[Sequence[Sequence[torch.Tensor]]] = None,
              allow_empty_type: bool = False) -> SlotBatch:
    """Write the padded batch of the stored graphs ``pieces`` (labels ``labels``, per-type fp32 feature tables ``feats[b][t]`` and, optionally,
    their row scales ``scales[b][t]``) into the slot's static tables ``bufs`` (``SlotLayout.buffers``): on the GPU ONE upload (a descriptor
    table) and ONE launch (``wsi_slot_fill``), no allocation inside the library, no read-back, no synchronisation, on the current stream; the
    filler's tables come from index arithmetic in the kernel.  On the CPU: ``slot_fill_torch`` copied into ``bufs``.  ``allow_empty_type``: as ``SlotBatch.fits`` (a slot with a presence
    table, ``derive_type_present``).  Features and plan share
    the launch: every mode works on 1024-element blocks (the feature copy on 16-byte elements).  The fill writes behind PyTorch's version
    counters - see DESIGN 3.15 for what that means for caches."""
    dev = bufs["rowptr"].device
    if dev.type != "cuda":
        out = slot_fill_torch(lay, pieces, labels, feats, scales, dev, allow_empty_type)
        with torch.no_grad():
            for k, v in out.items():
                if k != "batch":
                    bufs[k].copy_(v)
        return out["batch"]
    from . import _native as N
    sb, tb = _slot_descriptors(lay, bufs, pieces, labels, feats, scales, allow_empty_type)
    desc = tb.upload(dev)
    N.check(N.load().wsi_slot_fill(N.ptr(desc), tb.nsegs, tb.blocks, N.stream()), "wsi_slot_fill")
    bufs["_desc"] = desc            # (stream-ordered: the table must outlive the launch; the next fill replaces it behind this one)
    return sb


def _slot_descriptors(lay: SlotLayout, bufs, pieces, labels, feats, scales, allow_empty_type: bool = False):
    """The descriptor table of ``slot_fill``: (SlotBatch, SegmentTable)."""
    dev = bufs["rowptr"].device
    sb = SlotBatch(lay, pieces, allow_empty_type)
    T, hd, B, G = lay.T, lay.hd, sb.B, lay.graphs
    F = lay.in_dim
    tb = SegmentTable("slot_fill")
    for name, words in (("node", sb.node_tab), ("edge", sb.edge_tab), ("fill", sb.filler_block), ("readout_ptr", sb.readout_ptr),
                        ("labels", [int(y) for y in labels] + [-100] * (G - B)), ("chunk_row", sb.chunk_row), ("chunk_seg", sb.chunk_seg),
                        ("seg_chunk", sb.seg_chunk), ("seg_counts", _float_bits(sb.seg_counts)), ("seg_inv_counts", _float_bits(sb.seg_inv_counts)),
                        ("seg_nonempty", _float_bits(sb.seg_nonempty))):
        tb.table(name, words)
    seg, fill = tb.seg, tb.names["fill"]
    pos = (0, sum(pc.num_heavy for pc in pieces), 0)
    for b, pc in enumerate(pieces):             # the real nodes in the order of the unpadded batch's plan (graph.assemble_plan) ...
        pos = _order_segments(tb, bufs, pc, b * T, *pos)
    pos = sum(sb.n)
    for t in range(T):                          # ... the filler's last
        seg(bufs["order_dst"], pos, sb.nf[t], add=sb.fb[t], stride=1)
        seg(bufs["order_src"], pos, sb.nf[t], add=sb.fb[t], stride=1)
        pos += sb.nf[t]
    wide = F % 4 == 0 and bufs["feat"].data_ptr() % 16 == 0
    for t in range(T):
        R = hd.R[t]
        for b, pc in enumerate(pieces):
            row, eo = sb.node_tab[b * T + t], sb.eoff[(t, b)]
            so = hd.seg_off[t] + sb.pre[b][t] * R
            nc, ne = pc.counts[t], pc.ecount[t]
            _piece_segments(tb, bufs, hd, pc, t, b * T, so, row, eo, sb.coff[(t, b)])
            seg(bufs["edge_seg"], eo, ne, in1=_piece_edge_seg(pc, t, R) if ne else None, add=so)
            x = feats[b][t]
            if nc:
                if x.dtype != torch.float32 or not x.is_contiguous() or tuple(x.shape) != (nc, F) or x.device != dev:
                    raise ValueError("slot_fill: features must be contiguous fp32 [nodes, in_dim] tables on the slot's device")
                if wide and x.data_ptr() % 16 == 0:
                    seg(bufs["feat"], row * F // 4, nc * F // 4, in1=x, mode=5, esize=16)
                else:
                    seg(bufs["feat"], row * F, nc * F, in1=x, mode=1)
                if scales is not None:
                    seg(bufs["scales"], row, nc, in1=scales[b][t], mode=1)
        so = hd.seg_off[t] + sb.n[t] * R
        seg(bufs["rowptr"], so, sb.nf[t] * R, tab=fill, key=t, mode=10)
        seg(bufs["colptr"], sb.fb[t], sb.nf[t], tab=fill, key=t, mode=13)
        seg(bufs["src"], sb.feb[t], sb.ef[t], tab=fill, key=t, mode=11)
        seg(bufs["sim"], sb.feb[t], sb.ef[t], add=0, mode=2)
        seg(bufs["edge_seg"], sb.feb[t], sb.ef[t], tab=fill, key=t, add=so, stride=R, mode=14)
        seg(bufs["csc_eid"], 0, sb.ef[t], in1=bufs["csc_dst"].data_ptr(), tab=fill, key=t, mode=12)
        if wide:
            seg(bufs["feat"], sb.fb[t] * F // 4, sb.nf[t] * F // 4, mode=5, esize=16)       # (in1 null: zero rows)
        else:
            seg(bufs["feat"], sb.fb[t] * F, sb.nf[t] * F, add=0, mode=2)
        seg(bufs["scales"], sb.fb[t], sb.nf[t], add=0, mode=2)                               # the scale of an all-zero row: absmax bits 0
    _frame_segments(tb, bufs, hd, lay.E)
    seg(bufs["labels"], 0, G, tab=tb.names["labels"], mode=4, esize=8)
    for name in ("readout_ptr", "chunk_row", "chunk_seg", "seg_chunk", "seg_counts", "seg_inv_counts", "seg_nonempty"):
        seg(bufs[name], 0, bufs[name].numel(), tab=tb.names[name], mode=3)
    for s_, (a, b_) in enumerate(sb.ranges):
        seg(bufs["row_seg"], a, b_ - a, add=s_)
    return sb, tb


def derive_type_present(lay: SlotLayout, bufs: Dict[str, torch.Tensor], out: torch.Tensor) -> None:
    """``out[t] = 1.0`` when a REAL slide of the batch just filled into ``bufs`` holds a node of type t, else 0.0 (float32 ``[T]``):
    from the slot's readout table ``seg_nonempty`` (segment ``t * graphs + b``; graphs ``0 .. b_cap - 1`` are never the filler) as the fill
    has just written it, on the current stream - on the GPU ``wsi_type_present`` (one wave, no read-back, no host arithmetic), on the CPU
    the same in tensor operations (the kernel's oracle)."""
    ne = bufs["seg_nonempty"]
    if tuple(out.shape) != (lay.T,) or out.dtype != torch.float32 or out.device != ne.device or not out.is_contiguous():
        raise ValueError(f"derive_type_present: the table is a contiguous float32 [{lay.T}] tensor on the slot's device")
    if ne.device.type != "cuda":
        with torch.no_grad():
            out.copy_((ne.reshape(lay.T, lay.graphs)[:, :lay.b_cap] != 0).any(dim=1).to(torch.float32))
        return
    from . import _native as N
    N.check(N.load().wsi_type_present(N.ptr(ne), lay.T, lay.graphs, lay.b_cap, N.ptr(out), N.stream()), "wsi_type_present")


def derive_degree_norms(lay: SlotLayout, bufs: Dict[str, torch.Tensor], in_norm: torch.Tensor, out_norm: torch.Tensor) -> None:
    """GraphConv's degree norms of the batch just filled into a HOMOGENEOUS slot's ``bufs`` (one node type, one relation: ``rowptr`` has one
    segment per node): ``clamp(in-degree, min=1) ** -0.5`` and the same of the out-degree for all ``lay.N`` nodes, the filler's included - what
    ``models.GCN.HomoPlan`` computes per graph - on the current stream behind the fill: ``wsi_degree_norms`` on the GPU (one launch, no
    read-back), the same tensor operations on the CPU (the kernel's oracle)."""
    if lay.T != 1 or len(lay.rels) != 1:
        raise ValueError("derive_degree_norms: a homogeneous slot (one node type, one relation)")
    n, rowptr, colptr = lay.N, bufs["rowptr"], bufs["colptr"]
    for t in (in_norm, out_norm):
        if tuple(t.shape) != (n,) or t.dtype != torch.float32 or t.device != rowptr.device or not t.is_contiguous():
            raise ValueError(f"derive_degree_norms: the tables are contiguous float32 [{n}] tensors on the slot's device")
    if rowptr.device.type != "cuda":
        with torch.no_grad():
            in_norm.copy_((rowptr[1:n + 1] - rowptr[:n]).to(torch.float32).clamp(min=1).pow(-0.5))
            out_norm.copy_((colptr[1:n + 1] - colptr[:n]).to(torch.float32).clamp(min=1).pow(-0.5))
        return
    from . import _native as N
    N.check(N.load().wsi_degree_norms(N.ptr(rowptr), N.ptr(colptr), n, N.ptr(in_norm), N.ptr(out_norm), N.stream()), "wsi_degree_norms")


def derive_live_rows(lay: SlotLayout, bufs: Dict[str, torch.Tensor], live: torch.Tensor, live_rows: torch.Tensor) -> None:
    """The live rows of the batch just filled into a HOMOGENEOUS slot's ``bufs`` (one node type: readout segment = graph), for a BatchNorm
    that must not see the filler (``models.GIN``): ``live[i] = 1.0`` where row i belongs to a real slide (``row_seg[i] < b_cap``;
    the empty graphs have no rows, the filler's are dead), else 0.0, and ``live_rows[0]`` = the number of those rows, the sum of the first
    ``b_cap`` words of ``seg_counts`` in index order (integers: exact in fp32).  On the current stream behind the fill: ``wsi_slot_live_rows``
    on the GPU (one launch, no read-back - an augmented slot's counts exist on the device only), the same tensor operations on the CPU (the
    kernel's oracle)."""
    if lay.T != 1:
        raise ValueError("derive_live_rows: a homogeneous slot (one node type)")
    n, row_seg, counts = lay.N, bufs["row_seg"], bufs["seg_counts"]
    if (tuple(live.shape) != (n,) or tuple(live_rows.shape) != (1,) or any(t.dtype != torch.float32 or t.device != row_seg.device or
                                                                           not t.is_contiguous() for t in (live, live_rows))):
        raise ValueError(f"derive_live_rows: the tables are contiguous float32 [{n}] and [1] tensors on the slot's device")
    if row_seg.device.type != "cuda":
        with torch.no_grad():
            live.copy_((row_seg < lay.b_cap).to(torch.float32))
            live_rows.copy_(counts.reshape(-1)[:lay.b_cap].sum().reshape(1))      # (integers below 2^24: exact in any order)
        return
    from . import _native as N
    N.check(N.load().wsi_slot_live_rows(N.ptr(row_seg), N.ptr(counts), n, lay.graphs, lay.b_cap, N.ptr(live), N.ptr(live_rows), N.stream()),
            "wsi_slot_live_rows")


def slot_fill_torch(lay: SlotLayout, pieces: Sequence[PlanPieces], labels: Sequence[int], feats: Sequence[Sequence[torch.Tensor]],
                    scales: Optional[Sequence[Sequence[torch.Tensor]]] = None, device="cpu", allow_empty_type: bool = False) -> Dict[str, object]:
    """``slot_fill`` as tensor operations: the CPU path and the kernel's test oracle (the GPU test compares the two bit for bit).  The real
    slides' parts are offset copies of their pieces; the filler's parts come from SORTING its explicit edge list (``filler_graph``'s
    ``j -> (j mod nf[s], j mod nf[t])``), not from the kernel's closed forms.  Returns the tables by the names of ``SlotLayout.buffers``, plus
    ``"batch"``: the ``SlotBatch``."""
    dev = torch.device(device)
    sb = SlotBatch(lay, pieces, allow_empty_type)
    T, hd, B, G, F = lay.T, lay.hd, sb.B, lay.graphs, lay.in_dim
    N, S, E = lay.N, lay.S, lay.E
    i64 = lambda n: torch.zeros(int(n), dtype=torch.int64, device=dev)
    ar = lambda n: torch.arange(int(n), dtype=torch.int64, device=dev)
    on = lambda x: x.to(dev)
    rowptr, colptr = i64(S + 1), i64(N + 1)
    src, csc_eid, csc_dst = i64(E), i64(E), i64(E)
    sim = torch.zeros(E, dtype=torch.float32, device=dev)
    feat = torch.zeros((N, F), dtype=torch.float32, device=dev)
    scl = torch.zeros((N, 1), dtype=torch.int32, device=dev)
    node_tab = torch.tensor(sb.node_tab, dtype=torch.int64, device=dev)
    edge_tab = torch.tensor(sb.edge_tab, dtype=torch.int64, device=dev)
    for t in range(T):
        R = hd.R[t]
        for b, pc in enumerate(pieces):
            row, eo, co = sb.node_tab[b * T + t], sb.eoff[(t, b)], sb.coff[(t, b)]
            so = hd.seg_off[t] + sb.pre[b][t] * R
            nc, ne, ncc = pc.counts[t], pc.ecount[t], pc.ccount[t]
            rowptr[so:so + nc * R] = on(pc.rp[t]) + eo
            colptr[row:row + nc] = on(pc.cp[t]) + co
            src[eo:eo + ne] = on(pc.src_l[t]) + node_tab[b * T + on(pc.src_t[t])]
            sim[eo:eo + ne] = on(pc.sim[t])
            ent = b * T + on(pc.ent_t[t])
            csc_eid[co:co + ncc] = on(pc.eid_l[t]) + edge_tab[ent]
            csc_dst[co:co + ncc] = on(pc.dst_l[t]) + node_tab[ent]
            if nc:
                feat[row:row + nc] = on(feats[b][t])
                if scales is not None:
                    scl[row:row + nc] = on(scales[b][t])
    # the filler: its edges in CSR order (destination type, destination, j), then a stable sort by source for the CSC side
    f_eid, f_src, f_dst = [i64(0)], [i64(0)], [i64(0)]
    for t in range(T):
        R, nf, ef = hd.R[t], sb.nf[t], sb.ef[t]
        deg = i64(nf * R)
        if ef:
            s_ = lay.src_type[t]
            j = ar(ef)
            d, u = j % nf, j % sb.nf[s_]
            o = torch.sort(d, stable=True).indices
            src[sb.feb[t]:sb.feb[t] + ef] = sb.fb[s_] + u[o]
            f_eid.append(sb.feb[t] + ar(ef)); f_src.append(sb.fb[s_] + u[o]); f_dst.append(sb.fb[t] + d[o])
            deg[::R] = _count(d, nf)
        so = hd.seg_off[t] + sb.n[t] * R
        rowptr[so:so + nf * R] = sb.feb[t] + torch.cumsum(deg, 0) - deg
    rowptr[S] = E
    f_eid, f_src, f_dst = torch.cat(f_eid), torch.cat(f_src), torch.cat(f_dst)
    o = torch.sort(f_src, stable=True).indices
    f_eid, f_src, f_dst = f_eid[o], f_src[o], f_dst[o]
    for s_ in range(T):
        m = (f_src >= sb.fb[s_]) & (f_src < sb.fb[s_] + sb.nf[s_])
        k = int(m.sum())
        csc_eid[sb.cfb[s_]:sb.cfb[s_] + k] = f_eid[m]
        csc_dst[sb.cfb[s_]:sb.cfb[s_] + k] = f_dst[m]
        od = _count(f_src[m] - sb.fb[s_], sb.nf[s_])
        colptr[sb.fb[s_]:sb.fb[s_] + sb.nf[s_]] = sb.cfb[s_] + torch.cumsum(od, 0) - od
    colptr[N] = E
    frame = plan_frame(hd, dev, sb.counts)            # node_seg, inv_rd, readout_ptr of the padded batch's node counts
    H = sum(pc.num_heavy for pc in pieces)
    tabs = node_tab
    cat = lambda xs: torch.cat([on(x) for x in xs]) if xs else i64(0)
    bkey = lambda sizes: torch.repeat_interleave(ar(B) * T, torch.tensor(sizes, dtype=torch.int64, device=dev))
    heavy = cat([pc.heavy_l for pc in pieces]) + tabs[bkey([int(pc.heavy_l.numel()) for pc in pieces]) + cat([pc.heavy_t for pc in pieces])]
    light = cat([pc.light_l for pc in pieces]) + tabs[bkey([int(pc.light_l.numel()) for pc in pieces]) + cat([pc.light_t for pc in pieces])]
    osrc = cat([pc.so_l for pc in pieces]) + tabs[bkey([int(pc.so_l.numel()) for pc in pieces]) + cat([pc.so_t for pc in pieces])]
    fill_nodes = torch.cat([sb.fb[t] + ar(sb.nf[t]) for t in range(T)])
    i32 = lambda x: x.to(torch.int32)
    rp32 = i32(rowptr)
    edge_seg = torch.repeat_interleave(torch.arange(S, dtype=torch.int32, device=dev), (rowptr[1:] - rowptr[:-1]), output_size=E)
    row_seg = torch.repeat_interleave(torch.arange(lay.num_segs, dtype=torch.int32, device=dev),
                                      torch.tensor([b_ - a for a, b_ in sb.ranges], dtype=torch.int64, device=dev), output_size=N)
    col = lambda xs: torch.tensor(xs, dtype=torch.float32, device=dev).view(-1, 1)
    t32 = lambda xs: torch.tensor(xs, dtype=torch.int32, device=dev)
    return {"batch": sb, "rowptr": rp32, "colptr": i32(colptr), "node_seg": frame.node_seg, "src": i32(src), "csc_eid": i32(csc_eid),
            "csc_dst": i32(csc_dst), "order_dst": i32(torch.cat([heavy, light, fill_nodes])), "order_src": i32(torch.cat([osrc, fill_nodes])),
            "sim": sim, "inv_rd": frame.inv_rd, "readout_ptr": t32(sb.readout_ptr),
            "labels": torch.tensor([int(y) for y in labels] + [-100] * (G - B), dtype=torch.int64, device=dev), "feat": feat, "scales": scl,
            "edge_seg": edge_seg, "row_seg": row_seg, "chunk_row": t32(sb.chunk_row), "chunk_seg": t32(sb.chunk_seg), "seg_chunk": t32(sb.seg_chunk),
            "seg_counts": col(sb.seg_counts), "seg_inv_counts": col(sb.seg_inv_counts), "seg_nonempty": col(sb.seg_nonempty)}


# ------------------------------------------------------------------ augmented slides in a slot
class AugmentSpec:
    """What a slot-compatible pipeline (``transforms.Compose`` of at most one each of DropNode, DropEdge, NodeShuffle, FeatMask(['feat'])) comes
    down to: per kind ``(number in the pipeline, 16-bit threshold)`` or None.  ``data.slot_augment_spec`` builds it."""

    def __init__(self, drop_node=None, drop_edge=None, node_shuffle=None, feat_mask=None):
        self.drop_node, self.drop_edge, self.node_shuffle, self.feat_mask = drop_node, drop_edge, node_shuffle, feat_mask
        self.node_thr = drop_node[1] if drop_node else 0
        self.edge_thr = drop_edge[1] if drop_edge else 0
        self.mask_thr = feat_mask[1] if feat_mask else 0
        # DropEdge behind an effective DropNode draws by the rank among the relation's surviving edges (ops.augment_graph's rule)
        self.by_rank = int(self.node_thr > 0 and self.edge_thr > 0 and drop_edge[0] > drop_node[0])
        # NodeShuffle: 0 none, 1 over the stored nodes (in front of DropNode, or no effective DropNode), 2 over DropNode's survivors
        self.ns_mode = 0 if node_shuffle is None else (1 if (self.node_thr == 0 or node_shuffle[0] < drop_node[0]) else 2)

    def node_keep(self, draw: int, counts: Sequence[int], device="cpu") -> List[torch.Tensor]:
        """DropNode's keep flags of every node type under ``draw``, by the draw contract (bool [counts[t]])."""
        from . import ops
        if self.node_thr == 0:
            return [torch.ones(int(n), dtype=torch.bool, device=device) for n in counts]
        return [~ops.augment_drawn(int(n), ops.augment_subseed(draw, self.drop_node[0], t), self.node_thr, device) for t, n in enumerate(counts)]


def quota_counts(ntypes: Sequence[str], rels: Sequence[CanonicalEType], stored: Sequence[Sequence[int]], quotas, spec: "AugmentSpec"):
    """What a batch under survivor quotas can hold at most, as ``SlotBatch.fits`` takes it: ``(nodes[b][t], edges[b][t])``, edges by destination
    type.  ``stored[b][t]``: the stored node counts (a node quota holds only with a DropNode in the pipeline); ``quotas[b] = (qn, qe)``."""
    T, dst = len(ntypes), [list(ntypes).index(r[2]) for r in rels]
    nodes = [[min(int(q[0][t]), int(st[t])) if spec.drop_node is not None else int(st[t]) for t in range(T)] for q, st in zip(quotas, stored)]
    edges = [[sum(max(0, int(x)) for x, d in zip(q[1], dst) if d == t) for t in range(T)] for q in quotas]
    return nodes, edges


def restricted_orders(lay: SlotLayout, pieces: Sequence[PlanPieces], keeps: Sequence[Sequence[torch.Tensor]], sb: SlotBatch):
    """The processing orders of an augmented slot: the order tables the unaugmented fill writes for the same slides (heavy destinations of every
    slide, then the light ones; sources apart), restricted to the surviving nodes in the same relative order and renumbered; the filler's nodes
    follow, ascending.  ``pieces``: the STORED slides'; ``keeps[b][t]``: DropNode's keep flags; ``sb``: the augmented batch's layout."""
    T = lay.T
    dev = keeps[0][0].device
    node_tab = torch.tensor(sb.node_tab, dtype=torch.int64, device=dev)
    new_id = [[torch.cumsum(k.to(torch.int64), 0) - 1 for k in kb] for kb in keeps]

    def pick(b, l, t):
        l, t = l.to(dev), t.to(dev)
        out = []
        for i in range(int(l.numel())):
            li, ti = int(l[i]), int(t[i])
            if bool(keeps[b][ti][li]):
                out.append(int(node_tab[b * T + ti]) + int(new_id[b][ti][li]))
        return out

    dst = [x for b, pc in enumerate(pieces) for x in pick(b, pc.heavy_l, pc.heavy_t)] + [x for b, pc in enumerate(pieces) for x in pick(b, pc.light_l, pc.light_t)]
    src = [x for b, pc in enumerate(pieces) for x in pick(b, pc.so_l, pc.so_t)]
    fill = [sb.fb[t] + i for t in range(T) for i in range(sb.nf[t])]
    return torch.tensor(dst + fill, dtype=torch.int32, device=dev), torch.tensor(src + fill, dtype=torch.int32, device=dev)


def slot_fill_augmented(lay: SlotLayout, bufs: Dict[str, torch.Tensor], pieces: Sequence[PlanPieces], edges: Sequence[Sequence[Tuple[torch.Tensor, torch.Tensor]]],
                        labels: Sequence[int], feats: Sequence[Sequence[torch.Tensor]], draws: Sequence[int], spec: AugmentSpec,
                        quotas=None, overflow: Optional[torch.Tensor] = None) -> None:
    """Write the padded batch ``[transform(slide_b, draws[b]).., empty graphs.., filler]`` of the STORED slides ``pieces`` (per-relation COO
    ``edges[b][j]`` in sorted relation order, fp32 feature tables ``feats[b][t]``) into the GPU slot's tables ``bufs``, drawing the augmentation on
    the device: ONE descriptor upload, no read-back, no synchronisation, no atomics, scratch sized by the stored counts, ~20 launches whatever
    the draw and the pipeline (csrc/slot_aug.hip; include/wsi_hgnn.h, wsi_slot_aug_*).  ``bufs["_aug"]`` keeps the scratch of the last fill
    (``ncnt`` / ``fcnt``: the survivors' counts, for ``BatchSlot.counts``).  ``bufs["scales"]`` = row absmax of the filled feature table.

    ``quotas[b] = (qn[T], qe[R])``: survivor quotas of slide b per node type and per relation - the truncated pipeline of
    ``transforms.truncated``, enforced by the kernels that produce the counts (the node quota only with a DropNode in the pipeline).  The QUOTA
    sums must then fit the slot, not the stored counts.  ``overflow``: the slot's device int64 [3] table (fills in which a quota bound, largest
    node excess, largest edge excess), updated by one single-thread launch."""
    from . import _native as N
    from . import ops
    dev = bufs["rowptr"].device
    if dev.type != "cuda":
        raise RuntimeError("slot_fill_augmented runs on the GPU only (HIP kernels); a CPU slot takes the tensor route (data.BatchSlot.load)")
    T, hd, B, G, F = lay.T, lay.hd, len(pieces), lay.graphs, lay.in_dim
    R = len(lay.rels)
    tix = hd.tindex
    if quotas is None:
        if not SlotBatch.fits(lay, [pc.counts for pc in pieces], [pc.ecount for pc in pieces], True):
            raise ValueError("the stored batch does not fit the slot")
        qn_word, qe_word = (lambda s: 0), (lambda s: 0)
    else:
        if len(quotas) != B or any(len(q[0]) != T or len(q[1]) != R for q in quotas) or overflow is None:
            raise ValueError("slot_fill_augmented: quotas[b] = (one node quota per type, one edge quota per relation), with the overflow table")
        qn, qe = quota_counts(lay.ntypes, lay.rels, [pc.counts for pc in pieces], quotas, spec)
        if not SlotBatch.fits(lay, qn, qe, True):
            raise ValueError("the batch's quotas do not fit the slot")
        # the rows carry quota + 1 (0: none); a node quota acts inside DropNode only
        qn_word = (lambda s: min(int(quotas[s // T][0][s % T]), n_st[s]) + 1) if spec.drop_node is not None else (lambda s: 0)
        qe_word = lambda s: max(0, int(quotas[s // R][1][s % R])) + 1
    seed = lambda st, draw, j: ops.augment_subseed(draw, st[0], j) if st else 0
    n_st = [pc.counts[t] for pc in pieces for t in range(T)]                      # [b * T + t]
    rel_sizes = [[int(edges[b][j][0].numel()) for j in range(R)] for b in range(B)]
    # ---- wsi_augment_nodes / wsi_augment_edges rows
    nwords, ntiles, noff = ops._segment_rows(n_st, lambda s: (seed(spec.drop_node, draws[s // T], s % T), spec.node_thr, qn_word(s)))
    nodes_stored = sum(n_st)

    def erow(s):
        b, j = divmod(s, R)
        u, v = edges[b][j]
        if u.dtype != torch.int64 or v.dtype != torch.int64 or not u.is_contiguous() or not v.is_contiguous() or u.device != dev:
            raise ValueError("slot_fill_augmented: contiguous int64 COO on the slot's device")
        sr, _, ds = lay.rels[j]
        return (u.data_ptr(), v.data_ptr(), 0, noff[b * T + tix[sr]], noff[b * T + tix[ds]], seed(spec.drop_edge, draws[b], j), spec.edge_thr,
                spec.by_rank, pieces[b].counts[tix[sr]], pieces[b].counts[tix[ds]], qe_word(s))

    ewords, etiles, eoff = ops._segment_rows([m for rs in rel_sizes for m in rs], erow)
    coo_total = sum(sum(rs) for rs in rel_sizes)
    coo_base = [eoff[b * R] if R else 0 for b in range(B)]
    # ---- flag segments (what is scanned) and push segments (what the real slides write)
    maps = [pc.coo_maps(rel_sizes[b]) for b, pc in enumerate(pieces)]
    flag_n, flag_extra = [], []
    for b, pc in enumerate(pieces):
        for t in range(T):
            flag_n.append(pc.ecount[t]); flag_extra.append((0, maps[b][0][t].data_ptr(), 0, b, 0))
    for b, pc in enumerate(pieces):
        for t in range(T):
            flag_n.append(pc.ccount[t]); flag_extra.append((0, maps[b][1][t].data_ptr(), 0, b, 0))
    for l_, t_ in (("heavy_l", "heavy_t"), ("light_l", "light_t"), ("so_l", "so_t")):
        for b, pc in enumerate(pieces):
            flag_n.append(int(getattr(pc, l_).numel())); flag_extra.append((1, getattr(pc, l_).data_ptr(), getattr(pc, t_).data_ptr(), b, 0))
    fwords, ftiles, foff = ops._segment_rows(flag_n, lambda s: flag_extra[s])
    flag_total = sum(flag_n)
    pwords, blocks, npush = [], 0, 0

    def push(n, kind, b, t, ptrs, fseg):
        nonlocal blocks, npush
        if n > 0:
            pwords.extend([int(n), blocks, kind, b, t] + [p.data_ptr() for p in ptrs] + [0] * (4 - len(ptrs)) + [fseg])
            blocks += (int(n) + 1023) // 1024
            npush += 1

    aligned = bufs["feat"].data_ptr() % 16 == 0
    xwords = []
    for b, pc in enumerate(pieces):
        for t in range(T):
            Rt = hd.R[t]
            push(pc.counts[t], 0, b, t, [pc.rp[t], pc.cp[t]], 0)
            push(pc.ecount[t], 1, b, t, [pc.src_l[t], pc.src_t[t], pc.sim[t], _piece_edge_seg(pc, t, Rt) if pc.ecount[t] else pc.src_l[t]], b * T + t)
            push(pc.ccount[t], 2, b, t, [pc.eid_l[t], pc.ent_t[t], pc.dst_l[t]], B * T + b * T + t)
            x = feats[b][t]
            if pc.counts[t] and (x.dtype != torch.float32 or not x.is_contiguous() or tuple(x.shape) != (pc.counts[t], F) or x.device != dev):
                raise ValueError("slot_fill_augmented: features must be contiguous fp32 [nodes, in_dim] tables on the slot's device")
            aligned = aligned and (pc.counts[t] == 0 or x.data_ptr() % 16 == 0)
            xwords += [x.data_ptr() if pc.counts[t] else 0, pc.counts[t], seed(spec.feat_mask, draws[b], t)]
        push(int(pc.heavy_l.numel()), 3, b, 0, [pc.heavy_l, pc.heavy_t], 2 * B * T + b)
        push(int(pc.light_l.numel()), 4, b, 0, [pc.light_l, pc.light_t], 2 * B * T + B + b)
        push(int(pc.so_l.numel()), 5, b, 0, [pc.so_l, pc.so_t], 2 * B * T + 2 * B + b)
    shape = [T, B, lay.b_cap, READOUT_CHUNK, lay.c_cap]
    for t in range(T):
        shape += [lay.n_cap[t], lay.e_cap[t], hd.type_off[t], lay.ebase[t], lay.src_type[t], hd.R[t], hd.seg_off[t]]
    misc = list(noff) + n_st + coo_base + [int(y) for y in labels] + [-100] * (G - B) + [seed(spec.node_shuffle, draws[s // T], s % T) for s in range(B * T)]
    words, offs = [], {}
    for name, part in (("node", nwords), ("edge", ewords), ("flag", fwords), ("push", pwords), ("feat", xwords), ("shape", shape), ("misc", misc)):
        offs[name] = len(words)
        words += part
    desc = host_to_device(words, torch.int64, dev)
    i32 = lambda m: torch.empty(max(int(m), 1), dtype=torch.int32, device=dev)
    i64 = lambda m: torch.empty(max(int(m), 1), dtype=torch.int64, device=dev)
    sc = {"desc": desc, "new_id": i32(nodes_stored), "kept": i64(nodes_stored), "ncnt": i32(B * T), "tsum_n": i32(ntiles + 1), "rank1": i32(coo_total),
          "tsum_e": i32(2 * (etiles + 1)), "out_u": i64(coo_total), "out_v": i64(coo_total), "out_eid": i64(coo_total),
          "out_sim": torch.empty(max(coo_total, 1), dtype=torch.float32, device=dev), "ecnt_rel": i32(B * R), "ftile": i32(ftiles + 1),
          "frank": i32(flag_total), "fcnt": i32(len(flag_n)), "keys": i64(nodes_stored), "L": i64(4 * B * T + 9 * T + 3 * B + 2), "maps": maps}
    lib = N.load()
    st = N.stream()
    dp = desc.data_ptr()
    N.check(lib.wsi_augment_nodes(dp + 8 * offs["node"], B * T, ntiles, N.ptr(sc["tsum_n"]), N.ptr(sc["new_id"]), N.ptr(sc["kept"]), N.ptr(sc["ncnt"]), st),
            "wsi_augment_nodes")
    if R > 0:
        N.check(lib.wsi_augment_edges(dp + 8 * offs["edge"], B * R, etiles, N.ptr(sc["new_id"]), N.ptr(sc["tsum_e"]), N.ptr(sc["rank1"]), N.ptr(sc["out_u"]),
                                      N.ptr(sc["out_v"]), N.ptr(sc["out_sim"]), N.ptr(sc["out_eid"]), N.ptr(sc["ecnt_rel"]), st), "wsi_augment_edges")
    if quotas is not None:
        N.check(lib.wsi_slot_aug_quota(dp + 8 * offs["node"], B * T, N.ptr(sc["tsum_n"]), dp + 8 * offs["edge"], B * R, etiles, N.ptr(sc["tsum_e"]),
                                       N.ptr(overflow), st), "wsi_slot_aug_quota")
    import ctypes
    names = ("desc", "off_node", "off_edge", "off_flag", "off_push", "off_feat", "off_shape", "off_misc", "B", "T", "R", "N", "S", "E", "G", "nflag",
             "flag_tiles", "npush", "push_blocks", "nodes_stored", "ns_mode", "F", "mask_thr", "feat_aligned", "new_id", "kept", "ncnt", "rank1", "ftile",
             "frank", "fcnt", "keys", "perm", "L", "rowptr", "colptr", "node_seg", "src", "csc_eid", "csc_dst", "order_dst", "order_src", "sim", "inv_rd",
             "readout_ptr", "labels", "feat", "edge_seg", "row_seg", "chunk_row", "chunk_seg", "seg_chunk", "seg_counts", "seg_inv_counts", "seg_nonempty")
    val = {"desc": dp, "B": B, "T": T, "R": R, "N": lay.N, "S": lay.S, "E": lay.E, "G": G, "nflag": len(flag_n), "flag_tiles": ftiles, "npush": npush,
           "push_blocks": blocks, "nodes_stored": nodes_stored, "ns_mode": spec.ns_mode, "F": F, "mask_thr": spec.mask_thr, "feat_aligned": int(aligned), "perm": 0}
    val.update({"off_" + k: v for k, v in offs.items()})
    val.update({k: sc[k].data_ptr() for k in ("new_id", "kept", "ncnt", "rank1", "ftile", "frank", "fcnt", "keys", "L")})
    val.update({k: bufs[k].data_ptr() for k in names[34:]})
    args = (ctypes.c_int64 * len(names))(*[val[k] for k in names])                # the 55 argument words of wsi_slot_aug_* (include/wsi_hgnn.h)
    N.check(lib.wsi_slot_aug_keys(ctypes.addressof(args), st), "wsi_slot_aug_keys")
    sc["perm"] = torch.sort(sc["keys"][:nodes_stored], stable=True).indices if nodes_stored else sc["keys"]
    args[names.index("perm")] = sc["perm"].data_ptr()
    N.check(lib.wsi_slot_aug_scan(ctypes.addressof(args), st), "wsi_slot_aug_scan")
    N.check(lib.wsi_slot_aug_write(ctypes.addressof(args), st), "wsi_slot_aug_write")
    N.check(lib.wsi_row_absmax(N.ptr(bufs["feat"]), F, lay.N, F, N.ptr(bufs["scales"]), st), "wsi_row_absmax")
    bufs["_aug"] = sc                # (stream-ordered: descriptors and scratch must outlive the launches; the next fill replaces them behind this one)


def slot_plan(lay: SlotLayout, bufs: Dict[str, torch.Tensor], locality: bool = False) -> GraphPlan:
    """The kernel plan whose tables ARE the slot's static buffers.  ``num_heavy = 0``: every destination takes the light path (correct for any
    degree); a hub prefix of fixed size is not part of a slot."""
    p = _new_plan(lay.hd, bufs["rowptr"].device)
    p.num_edges, p.num_src_rows, p.batch_size = lay.E, lay.N, lay.graphs
    for k in ("rowptr", "colptr", "node_seg", "src", "csc_eid", "csc_dst", "order_dst", "order_src", "inv_rd", "readout_ptr"):
        setattr(p, k, bufs[k])
    p.num_heavy, p.locality = 0, bool(locality)
    p.heavy_degree = HEAVY_DEGREE_LOCALITY if locality else HEAVY_DEGREE
    p.__dict__["_edge_seg"] = bufs["edge_seg"]       # (ops._edge_segments: derived from rowptr once per plan - here refreshed by every fill)
    return p


# ------------------------------------------------------------------ the per-relation-source plan, derived from the base plan
PLAN_REL_MAX_RELS = 32      # WSI_PLAN_REL_MAX_RELS: relations leaving one node type the kernel keeps running counts for


def _plan_edge_seg(plan: GraphPlan) -> torch.Tensor:
    """int32 [E]: the softmax segment of every CSR edge (``ops._edge_segments``: expanded from ``rowptr`` once per plan; a slot's buffer)."""
    es = plan.__dict__.get("_edge_seg")
    if es is None:
        counts = (plan.rowptr[1:] - plan.rowptr[:-1]).to(torch.int64)
        es = torch.repeat_interleave(torch.arange(plan.num_segs, dtype=torch.int32, device=counts.device), counts, output_size=plan.num_edges)
        plan.__dict__["_edge_seg"] = es
    return es


def plan_rel_buffers(hd: PlanHeader, num_edges: int, device) -> Dict[str, torch.Tensor]:
    """Caller-owned tables of ``plan_by_relation(out=...)`` - shapes are functions of the header's node counts and the edge count alone - with
    the header table uploaded (once) and the kernel's scratch."""
    dev = torch.device(device)
    mk = lambda n: torch.empty(max(int(n), 1), dtype=torch.int32, device=dev)[:int(n)]
    NS, E = hd.rel_rows_total, int(num_edges)
    words = hd.relation_table()
    out = {"src": mk(E), "colptr": mk(NS + 1), "csc_eid": mk(E), "csc_dst": mk(E), "order_src": mk(NS),
           "header": host_to_device(words, torch.int32, dev), "scratch": mk(NS + (NS + 1023) // 1024 + 1)}
    return out


def _rel_plan_frame(hd: PlanHeader, base: GraphPlan) -> GraphPlan:
    """The derived plan with everything it SHARES with the base plan: the destination side, the readout, the flags."""
    if base.num_src_rows != base.num_nodes or base.num_nodes != hd.N or base.num_segs != hd.S:
        raise ValueError("plan_by_relation: the base plan must be the ordinary plan (source rows = nodes) of the header's node counts")
    p = _new_plan(hd, base.device)
    p.num_edges, p.num_src_rows, p.batch_size = base.num_edges, hd.rel_rows_total, base.batch_size
    for k in ("rowptr", "node_seg", "inv_rd", "order_dst", "readout_ptr", "perm"):
        setattr(p, k, getattr(base, k))
    p.num_heavy, p.heavy_degree, p.locality = base.num_heavy, base.heavy_degree, base.locality
    p.__dict__["_edge_seg"] = _plan_edge_seg(base)
    return p


def plan_by_relation_torch(hd: PlanHeader, base: GraphPlan, out: Optional[Dict[str, torch.Tensor]] = None) -> GraphPlan:
    """``plan_by_relation`` as tensor operations: the CPU path and the kernel's oracle.  The relation of an edge follows from its softmax
    segment, its row from the relation and the source; the CSC by row is a STABLE sort of the base CSC entries by their row - a source's base
    entries are in CSR order, so this is the order a stable sort of the CSR edges by row gives (``finish_plan``)."""
    p = _rel_plan_frame(hd, base)
    dev, E, NS, T = base.device, base.num_edges, hd.rel_rows_total, len(hd.ntypes)
    i64 = lambda xs: torch.tensor(xs, dtype=torch.int64, device=dev)
    if E:
        seg = _plan_edge_seg(base).long()
        seg_off, R = i64(hd.seg_off), i64(hd.R)
        t = torch.bucketize(seg, seg_off[1:], right=True).clamp_(max=T - 1)          # destination type (types without segments are skipped)
        slot_ptr = i64([sum(hd.R[:i]) for i in range(T)])
        slot_rel = [0] * len(hd.rels)
        for ri, (s, e, d) in enumerate(hd.rels):
            slot_rel[sum(hd.R[:hd.tindex[d]]) + hd.slot_of_rel[ri]] = ri
        rel = i64(slot_rel)[slot_ptr[t] + (seg - seg_off[t]) % R[t].clamp(min=1)]
        rel_lo = i64([lo for lo, _ in hd.rel_rows])
        rel_first = i64([hd.type_off[hd.tindex[s]] for s, _, _ in hd.rels])
        src = rel_lo[rel] + base.src.long() - rel_first[rel]
        row = src[base.csc_eid.long()]                                               # per base CSC entry
        order = torch.sort(row, stable=True).indices
        csc_eid, csc_dst = base.csc_eid[order], base.csc_dst[order]
        colptr = torch.zeros(NS + 1, dtype=torch.int64, device=dev)
        colptr[1:] = torch.cumsum(_count(row, NS), 0)
    else:
        src = csc_eid = csc_dst = torch.empty(0, dtype=torch.int32, device=dev)
        colptr = torch.zeros(NS + 1, dtype=torch.int64, device=dev)
    outdeg = colptr[1:] - colptr[:-1]
    tabs = {"src": src, "colptr": colptr, "csc_eid": csc_eid, "csc_dst": csc_dst,
            "order_src": torch.sort(outdeg, descending=True, stable=True).indices}
    for k, v in tabs.items():
        v = v.to(torch.int32).contiguous()
        if out is not None:
            out[k].copy_(v)
            v = out[k]
        setattr(p, k, v)
    return p


def plan_by_relation(hd: PlanHeader, base: GraphPlan, out: Optional[Dict[str, torch.Tensor]] = None) -> GraphPlan:
    """The per-relation-source plan (``HeteroGraph.plan(per_relation_src=True)``: HGT's) DERIVED from the ordinary plan ``base`` of the same
    graph: it shares the base plan's destination side (``rowptr``, ``node_seg``, ``inv_rd``, ``order_dst``, the hub prefix, the readout
    pointers, the edges' softmax segments) and owns ``src``, ``colptr``, ``csc_eid``, ``csc_dst``, ``order_src`` over
    ``hd.rel_rows_total`` source rows.  On the GPU one C call (``wsi_plan_by_relation``: five launches on the current stream, no sort of the
    edges, no read-back) and a stable descending sort of the rows' out-degrees for ``order_src`` (``finish_plan``'s rule for per-relation
    rows); every table equals ``_build_plan(g, per_relation_src=True)``'s.  ``out``: ``plan_rel_buffers`` the tables are written INTO (a
    slot's static buffers; the returned plan's tables are those tensors).  CPU plans: ``plan_by_relation_torch``."""
    if base.device.type != "cuda":
        return plan_by_relation_torch(hd, base, out)
    if out is None:
        out = plan_rel_buffers(hd, base.num_edges, base.device)
    p = rel_plan_over(hd, base, out)
    derive_rel_tables(hd, base, out)
    return p


def rel_plan_over(hd: PlanHeader, base: GraphPlan, out: Dict[str, torch.Tensor]) -> GraphPlan:
    """The derived plan OBJECT whose own tables are ``out``'s (``plan_rel_buffers``), nothing launched: ``derive_rel_tables`` fills them -
    once for an ordinary plan, after every fill for a slot."""
    p = _rel_plan_frame(hd, base)
    if out["src"].numel() != base.num_edges or out["colptr"].numel() != hd.rel_rows_total + 1:
        raise ValueError("plan_by_relation: out= was made for other node or edge counts")
    for k in ("src", "colptr", "csc_eid", "csc_dst", "order_src"):
        setattr(p, k, out[k])
    p._rel_tables = out             # (header table and scratch are stream-ordered inputs of the launches: held by the plan)
    return p


def derive_rel_tables(hd: PlanHeader, base: GraphPlan, out: Dict[str, torch.Tensor], sort_sources: bool = True) -> None:
    """Fill ``out`` from the base plan's CURRENT tables on the current stream: ``wsi_plan_by_relation`` (five launches), then ``order_src`` -
    the rows by out-degree, heaviest first, ties in row order (a stable sort on the device of ``colptr``'s differences: ``finish_plan``'s
    rule), or with ``sort_sources=False`` the rows in their own order.  No host arithmetic, no read-back."""
    if base.device.type != "cuda":
        plan_by_relation_torch(hd, base, out)
        if not sort_sources:
            out["order_src"].copy_(torch.arange(hd.rel_rows_total, dtype=torch.int32))
        return
    from . import _native as N
    if getattr(hd, "max_src_rels", None) is None:
        hd.relation_table()
    if hd.max_src_rels > PLAN_REL_MAX_RELS:
        raise RuntimeError(f"plan_by_relation: {hd.max_src_rels} relations leave one node type, the kernel supports {PLAN_REL_MAX_RELS}")
    N.check(N.load().wsi_plan_by_relation(N.ptr(base.src), N.ptr(base.colptr), N.ptr(base.csc_eid), N.ptr(base.csc_dst),
                                          N.ptr(_plan_edge_seg(base)), hd.N, base.num_edges, hd.S, N.ptr(out["header"]), out["header"].numel(),
                                          len(hd.ntypes), len(hd.rels), hd.rel_rows_total, hd.max_src_rels, N.ptr(out["src"]),
                                          N.ptr(out["colptr"]), N.ptr(out["csc_eid"]), N.ptr(out["csc_dst"]), N.ptr(out["scratch"]),
                                          out["scratch"].numel(), N.stream()), "wsi_plan_by_relation")
    colptr, NS = out["colptr"], hd.rel_rows_total
    if NS and sort_sources:
        out["order_src"].copy_(torch.sort(colptr[1:] - colptr[:-1], descending=True, stable=True).indices)
    elif NS:
        torch.arange(NS, dtype=torch.int32, device=colptr.device, out=out["order_src"])


def _build_plan(g: HeteroGraph, per_relation_src: bool = False) -> GraphPlan:
    dev = g.device
    hd = PlanHeader(g.ntypes, g.canonical_etypes, [g.num_nodes(t) for t in g.ntypes])
    gsrc, gdst, gseg = [], [], []
    for ri, (s, e, d) in enumerate(hd.rels):
        u, v = g._edges[(s, e, d)]
        u = u.to(dev)
        v = v.to(dev)
        ti_d = hd.tindex[d]
        gsrc.append(u + (hd.rel_rows[ri][0] if per_relation_src else hd.type_off[hd.tindex[s]]))
        gdst.append(v + hd.type_off[ti_d])
        gseg.append(hd.seg_off[ti_d] + v * hd.R[ti_d] + hd.slot_of_rel[ri])
    if gsrc:
        gsrc, gdst, gseg = torch.cat(gsrc), torch.cat(gdst), torch.cat(gseg)
    else:
        gsrc = gdst = gseg = torch.empty(0, dtype=torch.int64, device=dev)
    pos = None
    if g.ntypes and all("_pos" in g._nframes[t] for t in g.ntypes) and LOCALITY:
        pos = torch.cat([g._nframes[t]["_pos"].reshape(-1) for t in g.ntypes])
    return finish_plan(hd, gsrc, gdst, gseg, dev, per_relation_src,
                       [g.batch_num_nodes(t).tolist() for t in g.ntypes], pos=pos)


def batch(graphs: Sequence[HeteroGraph]) -> HeteroGraph:
    """Block-diagonal batch (``dgl.batch``): same ntypes/relations required."""
    graphs = list(graphs)
    if not graphs:
        raise ValueError("empty batch")
    g0 = graphs[0]
    for g in graphs[1:]:
        if g.ntypes != g0.ntypes or g.canonical_etypes != g0.canonical_etypes:
            raise ValueError("dgl.batch semantics: all graphs must share node types and relations")
    num_nodes = OrderedDict((t, sum(g.num_nodes(t) for g in graphs)) for t in g0.ntypes)
    bnn = {t: torch.cat([g.batch_num_nodes(t) for g in graphs]) for t in g0.ntypes}
    edges = OrderedDict()
    for r in g0.canonical_etypes:
        s, _, d = r
        us, vs = [], []
        so = do = 0
        for g in graphs:
            u, v = g._edges[r]
            us.append(u + so)
            vs.append(v + do)
            so += g.num_nodes(s)
            do += g.num_nodes(d)
        edges[r] = (torch.cat(us), torch.cat(vs))
    out = HeteroGraph(num_nodes, edges, bnn)
    for t in g0.ntypes:
        for k in g0._nframes[t]:
            out._nframes[t][k] = torch.cat([g._nframes[t][k] for g in graphs], dim=0)
    for r in g0.canonical_etypes:
        for k in g0._eframes[r]:
            out._eframes[r][k] = torch.cat([g._eframes[r][k] for g in graphs], dim=0)
    return out


@contextlib.contextmanager
def message_scale(g: HeteroGraph, scale: torch.Tensor):
    """For the duration of the block, every message of every ``GraphConv`` / ``GATConv`` forward on ``g`` is multiplied by
    ``scale[e]`` (``scale``: [E], in the graph's EDGE order, any finite values; gradients flow back to it).  This is what the
    reference's ``ExplainGraph.update_all`` does with ``sigmoid(edge_mask)`` (explainers/gnn_explainer.py:21-33); degree norms and
    the readout poolings are those of the unmasked graph, as there.  The tensor is kept permuted into the plan's CSR edge order
    (plain indexing: autograd carries the gradient back to edge order) and removed on exit, also when the block raises.
    Homogeneous graphs only: the reference's hijack works on a ``DGLGraph`` with a single edge frame."""
    if not g.is_homogeneous:
        raise ValueError("message_scale needs a homogeneous graph (one node type, one relation): the reference's update_all hijack "
                         "does not reach multi_update_all")
    E = g.num_edges()
    if scale.dim() != 1 or scale.numel() != E:
        raise ValueError(f"message_scale: scale must be [{E}] (one value per edge, in edge order), got {tuple(scale.shape)}")
    previous = g.__dict__.get("_message_scale")
    g.__dict__["_message_scale"] = scale.to(torch.float32)[g._csr_perm().to(scale.device)] if E else scale.to(torch.float32)
    try:
        yield g
    finally:
        if previous is None:
            g.__dict__.pop("_message_scale", None)
        else:
            g.__dict__["_message_scale"] = previous


def message_scale_of(g: HeteroGraph) -> Optional[torch.Tensor]:
    """The scale attached by an enclosing ``message_scale`` block, in CSR edge order, or None."""
    return g.__dict__.get("_message_scale")


def to_homogeneous(g: HeteroGraph, add_self_loop: bool = False) -> HeteroGraph:
    """``dgl.to_homogeneous(g, ndata=['feat', ...])`` (+ ``dgl.add_self_loop``): one node type holding all nodes in
    type-major order (DGL's order), one relation holding every edge (relations concatenated in canonical order);
    used by models/GCN_NTPool.py:90-91."""
    off = g.type_offsets()
    tindex = {t: i for i, t in enumerate(g.ntypes)}
    us, vs = [], []
    for (s, e, d) in g.canonical_etypes:
        u, v = g._edges[(s, e, d)]
        us.append(u + off[tindex[s]])
        vs.append(v + off[tindex[d]])
    n = off[-1]
    dev = g.device
    u = torch.cat(us) if us else torch.empty(0, dtype=torch.int64, device=dev)
    v = torch.cat(vs) if vs else torch.empty(0, dtype=torch.int64, device=dev)
    if add_self_loop:
        loop = torch.arange(n, dtype=torch.int64, device=u.device)
        u = torch.cat([u, loop])
        v = torch.cat([v, loop])
    out = HeteroGraph.homogeneous(n, u, v)
    keys = set.intersection(*[set(g._nframes[t].keys()) for t in g.ntypes]) if g.ntypes else set()
    for k in keys:
        if k == "_ID":
            continue
        out._nframes["_N"][k] = g.cat_ndata(k) if k == "feat" else torch.cat([g._nframes[t][k] for t in g.ntypes], dim=0)
    return out


def remove_nodes(g: HeteroGraph, nids: torch.Tensor, ntype: Optional[str] = None) -> HeteroGraph:
    """``dgl.remove_nodes(g, nids, ntype=...)`` on a single (unbatched) graph: the nodes and every edge that touches them go, the
    remaining nodes of that type keep their relative order (ids shift down), node and edge fields follow, and the set of
    relations is kept even when one becomes empty (DGL keeps the metagraph: SURVEY Appendix A.1.5)."""
    if g._batch_num_nodes is not None and g.batch_size > 1:
        raise ValueError("remove_nodes works on single graphs (the reference resets _batch_num_nodes before calling it)")
    if ntype is None:
        if len(g.ntypes) != 1:
            raise ValueError("ntype is required for a multi-type graph")
        ntype = g.ntypes[0]
    ntype = str(ntype)
    n = g.num_nodes(ntype)
    dev = g.device
    keep = torch.ones(n, dtype=torch.bool, device=dev)
    keep[torch.as_tensor(nids, dtype=torch.int64, device=dev)] = False
    new_id = torch.cumsum(keep, 0) - 1
    counts = OrderedDict((t, g.num_nodes(t)) for t in g.ntypes)
    counts[ntype] = int(keep.sum().item()) if dev.type != "cpu" else int(keep.sum())
    edges, emask = OrderedDict(), {}
    for (s, e, d) in g.canonical_etypes:
        u, v = g._edges[(s, e, d)]
        m = torch.ones(u.numel(), dtype=torch.bool, device=u.device)
        if s == ntype:
            m &= keep.to(u.device)[u]
        if d == ntype:
            m &= keep.to(v.device)[v]
        uu, vv = u[m], v[m]
        if s == ntype:
            uu = new_id.to(u.device)[uu]
        if d == ntype:
            vv = new_id.to(v.device)[vv]
        edges[(s, e, d)] = (uu, vv)
        emask[(s, e, d)] = m
    out = HeteroGraph(counts, edges)
    for t in g.ntypes:
        for k, x in g._nframes[t].items():
            out._nframes[t][k] = x[keep.to(x.device)] if t == ntype else x
    for r in g.canonical_etypes:
        for k, x in g._eframes[r].items():
            out._eframes[r][k] = x[emask[r].to(x.device)]
    return out


class LeaveOneOutTables:
    """Host-side degree tables of one (graph, node type): what ``leave_one_out_batch`` needs to size every copy without asking the device.

    ``out_degree[j]``, ``in_degree[j]``, ``self_loops[j]``: int64 CPU tensors ``[n_t]`` for relation j of ``g.canonical_etypes`` — edges whose
    source / destination / both ends are node i of ``ntype`` — or None where that side of the relation has another type (self loops: unless both
    have it).  Removing node r takes ``out(r) + in(r) - loops(r)`` edges of the relation away (a self loop is in both degrees)."""

    def __init__(self, ntype: str, num_nodes: int, num_edges: List[int], out_degree, in_degree, self_loops, signature):
        self.ntype, self.num_nodes, self.num_edges = ntype, int(num_nodes), list(num_edges)
        self.out_degree, self.in_degree, self.self_loops = out_degree, in_degree, self_loops
        self.signature = signature
        removed = torch.zeros((len(num_edges), self.num_nodes), dtype=torch.int64)
        for j in range(len(num_edges)):
            if out_degree[j] is not None:
                removed[j] += out_degree[j]
            if in_degree[j] is not None:
                removed[j] += in_degree[j]
            if self_loops[j] is not None:
                removed[j] -= self_loops[j]
        self._removed = removed

    def surviving_edges(self, nid: int) -> List[int]:
        """Edges of every relation (canonical order) in the graph without node ``nid`` of the type:
        ``E_j - out_j(r)[s==t] - in_j(r)[d==t] + loops_j(r)[s==t==d]``."""
        if self.num_nodes == 0:
            raise IndexError("the node type has no node")
        return [e - r for e, r in zip(self.num_edges, self._removed[:, int(nid)].tolist())]


def _edge_signature(g: HeteroGraph):
    return tuple((u.data_ptr(), v.data_ptr(), int(u.numel()), u._version, v._version) for u, v in g._edges.values())


def leave_one_out_tables(g: HeteroGraph, ntype: Optional[str] = None) -> LeaveOneOutTables:
    """Per-node out-degree, in-degree and self-loop count of every relation that touches ``ntype``: counted on the graph's device, brought to
    the host in ONE copy.  Compute once per (graph, type) and pass to every ``leave_one_out_batch`` call on it."""
    if ntype is None:
        if len(g.ntypes) != 1:
            raise ValueError("ntype is required for a multi-type graph")
        ntype = g.ntypes[0]
    ntype = str(ntype)
    n = g.num_nodes(ntype)
    dev = g.device
    rows, where = [], []            # where[k] = (relation index, 0 out / 1 in / 2 loops)
    num_edges = []
    for j, (s, e, d) in enumerate(g.canonical_etypes):
        u, v = g._edges[(s, e, d)]
        u, v = u.to(dev), v.to(dev)
        num_edges.append(int(u.numel()))
        if s == ntype:
            rows.append(_count(u, n))
            where.append((j, 0))
        if d == ntype:
            rows.append(_count(v, n))
            where.append((j, 1))
        if s == ntype and d == ntype:       # (index_add_ of the flag, not a boolean selection: that would read its size back)
            rows.append(torch.zeros(n, dtype=torch.int64, device=dev).index_add_(0, u, (u == v).to(torch.int64)))
            where.append((j, 2))
    R = len(num_edges)
    out_d, in_d, loops = [None] * R, [None] * R, [None] * R
    if rows:
        host = torch.stack(rows).cpu()          # THE device->host copy
        for k, (j, kind) in enumerate(where):
            (out_d, in_d, loops)[kind][j] = host[k]
    return LeaveOneOutTables(ntype, n, num_edges, out_d, in_d, loops, _edge_signature(g))


def leave_one_out_batch(g: HeteroGraph, nids, ntype: Optional[str] = None, tables: Optional[LeaveOneOutTables] = None,
                        check: bool = False) -> HeteroGraph:
    """``batch([remove_nodes(g, [i], ntype) for i in nids])``: one copy of ``g`` per entry of ``nids`` (any host sequence of node ids of
    ``ntype``; repeats allowed, order kept), each without that one node — the batches of the GEM explainers.  Same ``num_nodes``,
    ``batch_num_nodes``, edges and node / edge fields as the composition, value for value.

    On a CPU graph the result IS that composition.  On a GPU graph it comes from ``csrc/loo.hip`` (``ops.leave_one_out_batch``) with no
    device->host read: every size comes from ``tables`` (``leave_one_out_tables(g, ntype)``; built on first use and kept with the graph when
    not passed).  ``check=True`` reads the kernel's per-copy edge counts back and raises when one differs from the tables' prediction
    (tests and debugging)."""
    if g._batch_num_nodes is not None and g.batch_size > 1:
        raise ValueError("leave_one_out_batch works on single graphs, as remove_nodes does")
    if ntype is None:
        if len(g.ntypes) != 1:
            raise ValueError("ntype is required for a multi-type graph")
        ntype = g.ntypes[0]
    ntype = str(ntype)
    if ntype not in g._num_nodes:
        raise KeyError(f"unknown node type {ntype!r}")
    nids = [int(i) for i in nids]
    if not nids:
        raise ValueError("leave_one_out_batch needs at least one node id")
    n = g.num_nodes(ntype)
    for i in nids:
        if not 0 <= i < n:
            raise IndexError(f"node id {i} outside [0, {n}) of node type {ntype!r}")
    if g.device.type != "cuda":
        return batch([remove_nodes(g, torch.tensor([i]), ntype) for i in nids])
    if tables is None:
        cache = g.__dict__.setdefault("_loo_tables", {})
        tables = cache.get(ntype)
        if tables is None or tables.signature != _edge_signature(g):
            tables = cache[ntype] = leave_one_out_tables(g, ntype)
    elif tables.ntype != ntype or tables.num_nodes != n or tables.num_edges != [int(u.numel()) for u, _ in g._edges.values()]:
        raise ValueError("leave_one_out_batch: the tables were built for another graph or node type")
    from . import ops
    return ops.leave_one_out_batch(g, nids, ntype, tables, check)


def permute_nodes(g: HeteroGraph, perm: Dict[str, torch.Tensor]) -> HeteroGraph:
    """The same graph with the nodes of every type renumbered: new node i of type t is old node ``perm[t][i]``.
    Node fields follow their nodes, edges are relabelled, edge order and edge fields are untouched, so every model output
    is unchanged (message passing is permutation-equivariant, the readouts are permutation-invariant)."""
    inv = {}
    for t in g.ntypes:
        p = perm[t].to(torch.int64)
        if p.numel() != g.num_nodes(t):
            raise ValueError(f"perm[{t!r}] has {p.numel()} entries for {g.num_nodes(t)} nodes")
        q = torch.empty_like(p)
        q[p] = torch.arange(p.numel(), dtype=torch.int64, device=p.device)
        inv[t] = q
    edges = OrderedDict()
    for (s, e, d) in g.canonical_etypes:
        u, v = g._edges[(s, e, d)]
        edges[(s, e, d)] = (inv[s].to(u.device)[u], inv[d].to(v.device)[v])
    if g._batch_num_nodes is not None and g.batch_size > 1:
        raise ValueError("permute single graphs before batching them (a batch's node order encodes its graphs)")
    out = HeteroGraph(OrderedDict((t, g.num_nodes(t)) for t in g.ntypes), edges)
    for t in g.ntypes:
        for k, x in g._nframes[t].items():
            out._nframes[t][k] = x[perm[t].to(x.device)]
    for r in g.canonical_etypes:
        for k, x in g._eframes[r].items():
            out._eframes[r][k] = x
    return out


def locality_order(g: HeteroGraph, positions: Optional[Dict[str, torch.Tensor]] = None) -> Dict[str, torch.Tensor]:
    """A node order under which graph neighbours get nearby ids: reverse Cuthill-McKee on the symmetrised homogeneous
    adjacency, restricted to each node type.  WSI graphs are k-NN graphs in feature space, i.e. strongly clustered; with
    this order the K/V rows one workgroup gathers for neighbouring destinations fall into a few hundred KB instead of the
    whole 20 MB table, so the gathers hit the 4 MiB L2 instead of streaming from the Infinity Cache.  One-off, on the CPU,
    per slide (scipy); apply with ``permute_nodes`` before the graph is stored / batched.  Pure performance hint: results
    do not depend on it."""
    import numpy as np
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import reverse_cuthill_mckee
    off = g.type_offsets()
    n = off[-1]
    tindex = {t: i for i, t in enumerate(g.ntypes)}
    rows, cols = [], []
    for (s, e, d) in g.canonical_etypes:
        u, v = g._edges[(s, e, d)]
        rows.append(u.cpu().numpy() + off[tindex[s]])
        cols.append(v.cpu().numpy() + off[tindex[d]])
    if not rows or n == 0:
        if positions is not None:
            for i, t in enumerate(g.ntypes):
                positions[t] = off[i] + torch.arange(g.num_nodes(t))
        return {t: torch.arange(g.num_nodes(t)) for t in g.ntypes}
    r, c = np.concatenate(rows), np.concatenate(cols)
    a = coo_matrix((np.ones(2 * r.size, dtype=np.int8), (np.concatenate([r, c]), np.concatenate([c, r]))), shape=(n, n)).tocsr()
    order = np.asarray(reverse_cuthill_mckee(a, symmetric_mode=True), dtype=np.int64)       # order[i] = old global id at new position i
    out = {}
    for i, t in enumerate(g.ntypes):
        m = (order >= off[i]) & (order < off[i + 1])
        out[t] = torch.from_numpy((order[m] - off[i]).copy())
        if positions is not None:
            positions[t] = torch.from_numpy(np.nonzero(m)[0].astype(np.int64))      # slide-wide position of each node of type t, new order
    return out


def apply_locality_order(g: HeteroGraph) -> HeteroGraph:
    """``permute_nodes(g, locality_order(g))`` + the node field ``'_pos'`` (position of every node in the slide-wide order,
    across node types).  A plan built from graphs that carry ``'_pos'`` walks destination and source nodes in that order and
    the attention kernels walk it XCD-contiguously (``GraphPlan.locality``): the K/V rows gathered by the waves in flight on
    one XCD are those of neighbouring patches — on kNN (real WSI) graphs a working set its 4 MiB L2 can hold; on the random
    benchmark graphs there is no such order and the default heaviest-first one is used.  Results do not depend on it."""
    positions: Dict[str, torch.Tensor] = {}
    perm = locality_order(g, positions)
    out = permute_nodes(g, perm)
    for t in out.ntypes:
        # on the graph's own device: a CPU field on a device-resident graph would make every ``g.to(device)`` copy the whole graph
        # (and drop its cached plan) - once per trainer step
        out._nframes[t]["_pos"] = positions.get(t, torch.arange(out.num_nodes(t))).to(out.device)
    return out
