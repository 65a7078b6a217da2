"""torch.autograd.Function wrappers around the C-ABI (include/wsi_hgnn.h).

PyTorch is plumbing here: it owns the device memory, the stream and the autograd tape; every
arithmetic kernel on the hot path is a hand-written HIP kernel reached through ``_native``.

Operator API mirrored (there is no native operator layer in the reference; these are the DGL /
torch calls of models/HEATNet4.py the ops stand in for):
  grouped_linear      <- nn.Linear per node type        (HEATNet4.py:100-102,134,202,219)
  heat_attention      <- apply_edges(v_dot_u) * ea / sqrt_dk ; edge_softmax ; multi_update_all(u_mul_e, sum, 'mean')
                         (HEATNet4.py:103-119)
  segment_reduce      <- dgl.readout.{sum,mean,max}_nodes  (pooling/*_pooling.py)
"""
from __future__ import annotations

import array
import ctypes
import contextlib
from collections import namedtuple
from typing import List, Optional, Sequence, Tuple

import torch

from . import _native as N
from .graph import GraphPlan, SegmentTable, host_to_device



# ------------------------------------------------------------------------------------------------
# optional per-kernel timing (bench.py): HIP events recorded on the launch stream around each C-ABI call
# ------------------------------------------------------------------------------------------------
_TIMING = {"on": False, "records": []}


def enable_kernel_timing(on: bool) -> None:
    _TIMING["on"] = bool(on)
    _TIMING["records"] = []


class _Timed:
    def __init__(self, name: str, flops: float = 0.0, mfma_flops: float = 0.0):
        self.name, self.flops, self.mfma_flops = name, flops, mfma_flops

    def __enter__(self):
        if _TIMING["on"]:
            self.e0 = torch.cuda.Event(enable_timing=True)
            self.e1 = torch.cuda.Event(enable_timing=True)
            self.e0.record()
        return self

    def __exit__(self, *exc):
        if _TIMING["on"]:
            self.e1.record()
            _TIMING["records"].append((self.name, self.flops, self.mfma_flops, self.e0, self.e1))
        return False


def kernel_timing_summary() -> dict:
    """{family: {ms, launches, flops, mfma_flops}} over everything recorded since enable_kernel_timing(True); ``flops`` are
    algorithmic (2MNK), ``mfma_flops`` what the matrix cores execute for them (x6 under bf16x6, x3 / x6 under fp16x3)."""
    torch.cuda.synchronize()
    out = {}
    for name, flops, mfma, e0, e1 in _TIMING["records"]:
        d = out.setdefault(name, {"ms": 0.0, "launches": 0, "flops": 0.0, "mfma_flops": 0.0})
        d["ms"] += e0.elapsed_time(e1)
        d["launches"] += 1
        d["flops"] += flops
        d["mfma_flops"] += mfma
    return out

# ------------------------------------------------------------------------------------------------
# grouped GEMM
# ------------------------------------------------------------------------------------------------
_GEMM_MODES = {"fp32": N.WSI_GEMM_FP32, "bf16x6": N.WSI_GEMM_BF16X6, "fp16x3": N.WSI_GEMM_FP16X3, "auto": N.WSI_GEMM_AUTO}
_SCALED_MODES = ("fp16x3", "auto")          # modes whose launches exchange row scales
_PRECISION = {"mode": "fp32"}


def set_gemm_precision(mode: str) -> None:
    """Arithmetic of every projection GEMM this host module launches from now on (passed PER CALL to wsi_gemm_grouped; the
    library keeps no mode).  "fp32" (default): IEEE fp32 MFMA.  "bf16x6": exact 3-way bf16 split of
    both operands, 6 cross products accumulated in fp32 on the bf16 matrix cores — fp32-class error, not a reduced-precision
    mode.  "fp16x3": per-row power-of-two scaling, 2-way fp16 split (2^-23 relative, per product <= 2^-21), 3 cross products on the fp16 matrix
    cores — the same error class at half the matrix work (include/wsi_hgnn.h).  "auto": per launch, fp16x3 where its pre-pass
    is amortised (large projections), bf16x6 otherwise."""
    if mode not in _GEMM_MODES:
        raise ValueError(f"unknown GEMM precision {mode!r}; expected one of {sorted(_GEMM_MODES)}")
    _PRECISION["mode"] = mode


def gemm_precision() -> str:
    return _PRECISION["mode"]


# ------------------------------------------------------------------------------------------------
# facts that travel WITH a tensor between autograd nodes
# ------------------------------------------------------------------------------------------------
# A producer on the path knows things about the tensor it hands on that its consumer would otherwise recompute with a pass over it (the absmax
# bits of its rows: the fp16x3 scales) or could never recover (that a readout's gradient is a broadcast of S distinct rows).  The fact is attached
# to THE TENSOR OBJECT, with the version counter it was true at, and read from the object the consumer receives: autograd hands a Python tensor
# from one node to the next unchanged (PyTorch preserves a tensor's Python object while the tensor lives), so this is an argument passed
# explicitly from producer to consumer - there is no process-wide table to match against, nothing another model or thread in the process can
# evict or alias.  Whatever is not that very object at that very version (a view, a detached alias, a gradient the engine accumulated with
# another contribution - in place: the version moves - or into a new tensor) carries no valid fact and the consumer takes its general path.
def _annotate(t: torch.Tensor, name: str, payload) -> None:
    setattr(t, name, (t._version, payload))


def _annotation(t: torch.Tensor, name: str):
    hit = getattr(t, name, None)
    if hit is None or hit[0] != t._version:
        return None
    return hit[1]


EXCHANGE_STATS = {"row_scale_hits": 0, "broadcast_hits": 0}       # how often a consumer found its producer's fact (tests read these)


def attach_row_scales(t: torch.Tensor, bits: torch.Tensor) -> None:
    """``bits`` [rows, parts] int32: partial absmax bit patterns of the rows of ``t`` as it is NOW (include/wsi_hgnn.h, wsi_gemm_group_t.a_absmax)."""
    _annotate(t, "_wsi_row_scales", bits)


def row_scales_of(t: torch.Tensor) -> Optional[torch.Tensor]:
    """The row scales ``t``'s producer attached, if the arithmetic uses scales and ``t`` has not been written since; else None."""
    if _PRECISION["mode"] not in _SCALED_MODES:
        return None
    bits = _annotation(t, "_wsi_row_scales")
    if bits is not None:
        EXCHANGE_STATS["row_scale_hits"] += 1
    return bits


def _auto_scaled(rows: int, width: int) -> bool:
    """WSI_GEMM_AUTO's NT / NN rule (csrc/gemm_f32.hip::kernel_precision) for a projection that reads a [rows, width] tensor over all node types
    (K = width, about as many output columns, up to three projections per launch), conservatively: >= 12 GFLOP and K >= 384 always; on LARGE batches
    (>= 49152 rows: the step is GPU-bound) from 5 GFLOP and K >= 256."""
    flop = float(rows) * width * width * 2.0 * 3.0
    return (width >= 384 and flop >= 12e9) or (rows >= 49152 and width >= 256 and flop >= 5e9)


def _new_row_scale(rows: int, parts: int, device, width: int = 1 << 30, zero: bool = True) -> Optional[torch.Tensor]:
    """A zeroed [rows, parts] table of partial absmax bits for producers to fill (each its own slots, plain stores; the
    consumer takes the row maximum - include/wsi_hgnn.h, wsi_gemm_group_t.a_absmax), or None outside the scaled modes.
    ``width``: columns of the tensor the scales describe = the K of the projection that would consume them; under "auto" a
    narrow or short tensor gets no table (its consumer runs bf16x6 anyway - WSI_GEMM_AUTO's rule - and the table would only
    cost a fill and epilogue stores per launch: 0.4 ms per HGT step).  ``zero=False`` when the producers are known to write every
    slot of every row (slots nobody writes must read 0)."""
    mode = _PRECISION["mode"]
    if mode not in _SCALED_MODES or (mode == "auto" and not _auto_scaled(rows, width)):
        return None
    if rows <= 32:
        return None     # a tensor this short is produced and consumed by the skinny kernels (fp32 FMAs, no scales; a launch that
                        # asks for c_absmax would be kept off them, and the arithmetic must not depend on whether scales are wanted)
    return (torch.zeros if zero else torch.empty)((max(int(rows), 1), int(parts)), dtype=torch.int32, device=device)


def remember_constant_rows(x: torch.Tensor, holder=None) -> None:
    """Scaled modes: make sure ``x`` - a tensor that does not change from step to step, e.g. the input features of a resident graph - carries
    its row scales, so that the projection reading it skips its absmax pass: computed once (``wsi_row_absmax``) and attached to the tensor
    itself (``holder``, the graph that keeps ``x`` alive, is accepted for the callers' sake and not used)."""
    if _PRECISION["mode"] not in _SCALED_MODES or x.dim() != 2 or not x.is_cuda or x.stride(1) != 1:
        return
    if _PRECISION["mode"] == "auto" and not _auto_scaled(x.shape[0], x.shape[1]):
        return                                       # its consumer runs bf16x6 (WSI_GEMM_AUTO's rule)
    if _annotation(x, "_wsi_row_scales") is None:
        attach_row_scales(x, row_absmax(x))


def scaled_gemm_mode() -> bool:
    """True when the projections run (or may run) scaled-fp16 and row scales are worth keeping."""
    return _PRECISION["mode"] in _SCALED_MODES


def row_absmax(x: torch.Tensor) -> torch.Tensor:
    """[rows, 1] int32 absmax bit patterns of the rows of a 2-D fp32 tensor (``wsi_row_absmax``)."""
    N.require_cuda(x)
    bits = torch.empty((x.shape[0], 1), dtype=torch.int32, device=x.device)
    N.check(N.load().wsi_row_absmax(N.ptr(x), x.stride(0), x.shape[0], x.shape[1], N.ptr(bits), N.stream()), "wsi_row_absmax")
    return bits


def _scale_in(bits: Optional[torch.Tensor], r0: int) -> dict:
    """Group fields that hand the row scales ``bits`` ([rows, parts], starting at row ``r0``) to a projection as its A scales."""
    if bits is None:
        return {}
    return dict(a_absmax=N.ptr(bits, r0 * bits.shape[1] * 4), a_absmax_parts=bits.shape[1])


def _scale_out(bits: Optional[torch.Tensor], r0: int, col_off: int = 0) -> dict:
    """Group fields that make a projection leave the scales of the rows it writes (from row ``r0``, columns from ``col_off``)."""
    if bits is None:
        return {}
    return dict(c_absmax=N.ptr(bits, r0 * bits.shape[1] * 4), c_absmax_parts=bits.shape[1], c_absmax_first=2 * (col_off // 128))


# ------------------------------------------------------------------------------------------------
# column statistics for the scaled-fp16 weight gradients (include/wsi_hgnn.h: c_colmax / a_colmax ...)
# ------------------------------------------------------------------------------------------------
class ColStats:
    """What a producer knows about the COLUMNS of a tensor it wrote: per row range (one per grouped-GEMM group = node type) partial absmax bits
    (and partial sums): ``bits`` [parts, width] int32, ``sums`` [parts, width] fp32 or None; ``ranges[(r0, r1)] = (first part, parts)`` of the rows
    [r0, r1) (a GEMM epilogue: one part per 128-row tile).  ``col0``: column of the tables that column 0 of the annotated tensor is (the aggregate t
    of a HEAT layer is bounded column by column by V, whose statistics sit at columns [2D, 3D) of the K|Q|V table's)."""

    def __init__(self, bits, sums, ranges, col0=0):
        self.bits, self.sums, self.ranges, self.col0 = bits, sums, dict(ranges), int(col0)

    @classmethod
    def allocate(cls, rows, width: int, device, sums: bool) -> Optional["ColStats"]:
        """Tables for a grouped NT / NN launch whose groups write the row ranges ``rows`` (one part per 128-row tile of each distinct range)."""
        ranges, p = {}, 0
        for (a, b) in rows:
            if (a, b) not in ranges and b > a:
                n = (b - a + 127) // 128
                ranges[(a, b)] = (p, n)
                p += n
        if p == 0:
            return None
        bits = torch.empty((p, width), dtype=torch.int32, device=device)
        return cls(bits, torch.empty((p, width), dtype=torch.float32, device=device) if sums else None, ranges)

    def shifted(self, col0: int) -> "ColStats":
        """The same tables seen from a tensor whose column 0 is their column ``col0``."""
        return ColStats(self.bits, self.sums, self.ranges, self.col0 + col0)

    def produce(self, r0: int, r1: int, col: int) -> dict:
        """Group fields that make an NT / NN group writing rows [r0, r1), columns from ``col`` on, leave its statistics."""
        hit = self.ranges.get((r0, r1))
        if hit is None:
            return {}
        w = self.bits.shape[1]
        d = dict(c_colmax=N.ptr(self.bits, (hit[0] * w + col) * 4), c_col_ld=w)
        if self.sums is not None:
            d["c_colsum"] = N.ptr(self.sums, (hit[0] * w + col) * 4)
        return d

    def consume(self, side: str, r0: int, r1: int, col: int, want_sums: bool = False) -> dict:
        """Group fields of a TN group whose operand ``side`` ('a' / 'b') is rows [r0, r1), columns from ``col`` on, of the annotated tensor
        (empty when the range is not one the producer wrote, or sums are wanted and were not kept)."""
        hit = self.ranges.get((r0, r1))
        if hit is None or (want_sums and self.sums is None):
            return {}
        w = self.bits.shape[1]
        off = (hit[0] * w + self.col0 + col) * 4
        d = {side + "_colmax": N.ptr(self.bits, off), side + "_col_ld": w, side + "_col_parts": hit[1]}
        if side == "a" and want_sums:
            d["a_colsum"] = N.ptr(self.sums, off)
        return d


def attach_col_stats(t: torch.Tensor, stats: Optional[ColStats]) -> None:
    if stats is not None:
        _annotate(t, "_wsi_col_stats", stats)


def col_stats_of(t: torch.Tensor) -> Optional[ColStats]:
    """The column statistics ``t``'s producer attached, if the arithmetic uses scales and ``t`` has not been written since; else None."""
    if _PRECISION["mode"] not in _SCALED_MODES:
        return None
    st = _annotation(t, "_wsi_col_stats")
    if st is not None:
        EXCHANGE_STATS["col_stat_hits"] = EXCHANGE_STATS.get("col_stat_hits", 0) + 1
    return st


_TN_AUTO = {"flop": 4e9}          # WSI_GEMM_AUTO's weight-gradient threshold (csrc/gemm_f32.hip::kernel_precision; tools move both for A/B runs)


def want_col_stats(total_rows: int, out_cols: int, in_cols: int) -> bool:
    """Will the weight gradient dW [out_cols, in_cols] over ``total_rows`` rows run on the scaled-fp16 TN kernel (so that its operands' producers
    should leave column statistics)?  WSI_GEMM_AUTO's rule for TN launches (csrc/gemm_f32.hip::kernel_precision), conservatively."""
    mode = _PRECISION["mode"]
    if mode not in _SCALED_MODES:
        return False
    flop = 2.0 * total_rows * out_cols * in_cols
    return mode == "fp16x3" or (min(out_cols, in_cols) >= 192 and ((flop >= 3e10 and total_rows >= 3 * 2048) or (flop >= _TN_AUTO["flop"] and total_rows >= 49152)))


_SIDE_STATS = {"enabled": True, "launches": 0, "reasons": set()}
# HIP streams of this module beside the caller's.  ONE by default: the background weight gradients ("work") and the column statistics / early
# skip-gate gradient ("stats") take turns on it (measured equal to two: 5.85 against 5.87 ms per step, bench.py --side-streams).  Why the count
# matters: the runtime gives every stream in use a hardware queue of its own up to GPU_MAX_HW_QUEUES (4) and lets further streams SHARE queues.
# Measured on this GPU (round 5, bench.py --pcie; profiles/r05_pcie_side_streams.txt):
#   * a FOURTH hardware queue in use beside H2D transfers stretches every kernel of the step (small launches to ~50 us each): 10.0 ms per
#     loader-fed step against 6.7 - with the caller's stream, two streams here and the loader's copy stream; gone under GPU_MAX_HW_QUEUES=3 and
#     with four unrelated streams used in between (the copy stream then shares a queue);
#   * two of these streams SHARING one queue serialise behind each other: 7.5 ms per step against 5.9.
# So: one side stream; the pinned-host loader borrows it for its transfers (it keeps the steps it feeds in order anyway - block_side_streams) rather
# than making a stream of its own; a data-parallel step has the caller's stream, this one and RCCL's.
_SIDE_STREAMS = {"count": 1, "streams": {}}


def set_side_stream_count(n: int) -> None:
    if n not in (1, 2):
        raise ValueError("set_side_stream_count: 1 or 2")
    _SIDE_STREAMS["count"] = int(n)          # (streams already made are kept: a new one would take - or, past the runtime's limit, SHARE - one more hardware queue)


def side_stream(device, role: str = "work") -> "torch.cuda.Stream":
    dev = torch.device(device)
    key = (dev.index, role if _SIDE_STREAMS["count"] == 2 else "work")
    st = _SIDE_STREAMS["streams"].get(key)
    if st is None:
        st = _SIDE_STREAMS["streams"][key] = torch.cuda.Stream(device=dev)
    return st


def _side_stats_on() -> bool:
    return _SIDE_STATS["enabled"] and not _SIDE_STATS["reasons"] and not torch.cuda.is_current_stream_capturing()


def block_side_streams(blocked: bool, who: str) -> None:
    """Keep EVERY launch of the step on the caller's stream while ``who`` says so: no background weight gradients, no statistics stream.
    (data.GraphBatchLoader while it feeds steps from pinned host memory: with H2D transfers in flight, kernels of a second compute stream
    stretch the whole step - the small launches of the caller's stream to ~50 us each - 10.0 ms per loader-fed step against 6.7 in order,
    profiles/r05_pcie_side_streams.txt; the transfer, 5.9 ms at 55 GB/s, bounds that step anyway.)"""
    (_SIDE_STATS["reasons"].add if blocked else _SIDE_STATS["reasons"].discard)(who)
    block_background_weight_gradients(blocked, who=who)


def set_side_column_statistics(on: bool) -> None:
    """On (default): the column statistics of the attention gradients (no producer leaves them: one wave per node, four nodes per workgroup) are taken
    by ``wsi_col_stats`` on a stream of its own, beside the matrix-bound dX projection that reads the same table, instead of in line inside the weight
    gradient (its own pass: 0.15 ms per step on the bench batch, bandwidth-bound).  Off: the weight gradient makes its pass."""
    _SIDE_STATS["enabled"] = bool(on)


def _col_stats_side(x: torch.Tensor, rows: Sequence[Tuple[int, int]], device):
    """(ColStats of the row ranges of ``x`` - partial absmax bits and sums per 256 rows -, event) computed on the statistics stream, which first waits
    for everything the caller's stream holds so far; None inside a stream capture or when switched off.  The consumer waits for the event."""
    if not _side_stats_on():
        return None
    lib = N.load()
    dev = torch.device(device)
    width = x.shape[1]
    wpad = (width + 3) & ~3
    ranges, p = {}, 0
    for (a, b) in rows:
        if (a, b) not in ranges and b > a:
            n_ = lib.wsi_col_stats_parts(b - a)
            ranges[(a, b)] = (p, n_)
            p += n_
    if p == 0:
        return None
    bits = torch.empty((p, wpad), dtype=torch.int32, device=dev)
    sums = torch.empty((p, wpad), dtype=torch.float32, device=dev)
    side = side_stream(dev, "stats")
    main = torch.cuda.current_stream(dev)
    side.wait_stream(main)
    for (a, b), (p0, n_) in ranges.items():
        N.check(lib.wsi_col_stats(N.ptr(x, a * x.stride(0) * 4), x.stride(0), b - a, width, N.ptr(bits, p0 * wpad * 4), N.ptr(sums, p0 * wpad * 4), wpad,
                                  ctypes.c_void_p(side.cuda_stream)), "wsi_col_stats")
        _SIDE_STATS["launches"] += 1
    ev = torch.cuda.Event()
    ev.record(side)
    for t_ in (x, bits, sums):
        t_.record_stream(side)
    return ColStats(bits, sums, ranges), ev


def remember_constant_cols(x: torch.Tensor, rows: Sequence[Tuple[int, int]]) -> None:
    """Scaled modes: make sure ``x`` - a weight-gradient operand that does not change from step to step: the input features of a resident graph -
    carries its column statistics (one part per row range: ``wsi_col_absmax``, once), so that the input projection's weight gradient skips its pass
    over it."""
    if _PRECISION["mode"] not in _SCALED_MODES or x.dim() != 2 or not x.is_cuda or x.stride(1) != 1:
        return
    st = _annotation(x, "_wsi_col_stats")
    if st is not None and all(r in st.ranges for r in rows if r[1] > r[0]):
        return
    lib = N.load()
    width = x.shape[1]
    ranges, bits_rows = {}, []
    for (a, b) in rows:
        if (a, b) in ranges or b <= a:
            continue
        out = torch.empty(width, dtype=torch.int32, device=x.device)
        nbytes = lib.wsi_col_absmax_workspace_bytes(b - a, width)
        ws = torch.empty(max(nbytes // 4, 4), dtype=torch.int32, device=x.device)
        N.check(lib.wsi_col_absmax(N.ptr(x, a * x.stride(0) * 4), x.stride(0), b - a, width, N.ptr(out), N.ptr(ws), nbytes, N.stream()), "wsi_col_absmax")
        ranges[(a, b)] = (len(bits_rows), 1)
        bits_rows.append(out)
    if bits_rows:
        attach_col_stats(x, ColStats(torch.stack(bits_rows), None, ranges))


def refresh_constant_cols(x: torch.Tensor) -> None:
    """``x`` was rewritten BEHIND its version counter (a batch slot's feature table, ``graph.slot_fill``): recompute the column statistics
    ``remember_constant_cols`` attached, into the same tables - a step recorded into a hipGraph reads them by address.  Nothing to do when
    none are attached."""
    st = _annotation(x, "_wsi_col_stats")
    if st is None or st.sums is not None:
        return
    lib = N.load()
    width = x.shape[1]
    for (a, b), (p0, _) in st.ranges.items():
        nbytes = lib.wsi_col_absmax_workspace_bytes(b - a, width)
        ws = torch.empty(max(nbytes // 4, 4), dtype=torch.int32, device=x.device)
        N.check(lib.wsi_col_absmax(N.ptr(x, a * x.stride(0) * 4), x.stride(0), b - a, width, N.ptr(st.bits, p0 * st.bits.shape[1] * 4), N.ptr(ws), nbytes,
                                   N.stream()), "wsi_col_absmax")


# ------------------------------------------------------------------------------------------------
# weights packed once per optimizer step (wsi_gemm_group_t.b_packed)
# ------------------------------------------------------------------------------------------------
# The scaled-fp16 NT / NN kernel reads its B operand (the weights) as two fp16 planes in MFMA fragment order; wsi_gemm_grouped packs them per call -
# one more launch in front of every projection, seven per step, for weights that change once per step.  Here the packed form is kept per
# (op, weights, chunking): ``repack_weights`` (called by optim.Adam.step behind its update) refreshes every entry in ONE launch per op and ARMS
# it; a projection uses an armed entry once (a weight is read once per step in each form: NT in the forward, NN in the backward) and disarms it.
# An entry nobody re-armed is packed again at its next use - so under any OTHER optimizer nothing is ever reused across a parameter update:
# version counters alone cannot be trusted with that (torch.optim.Adam(fused=True, capturable=True) updates parameters without moving them -
# found with tools/graph_capture_probe.py: a cache keyed on versions trained on stale weights).  They are still checked (load_state_dict, manual
# in-place surgery between the optimizer step and the next forward); a change through ``.data`` between those two points would go unnoticed:
# ``invalidate_packed_weights()`` after such surgery, or ``set_packed_weight_cache(False)``.
_PACKED = {"enabled": True, "entries": {}, "hits": 0, "packs": 0}


def set_packed_weight_cache(on: bool) -> None:
    _PACKED["enabled"] = bool(on)
    if not on:
        _PACKED["entries"].clear()


def invalidate_packed_weights() -> None:
    _PACKED["entries"].clear()


def _pack_groups(op: int, items, arm: bool) -> None:
    """``items``: (entry, group dict) pairs to (re)pack; one wsi_gemm_pack_b launch per WSI_GEMM_MAX_GROUPS of them."""
    lib = N.load()
    for i in range(0, len(items), N.WSI_GEMM_MAX_GROUPS):
        chunk = items[i:i + N.WSI_GEMM_MAX_GROUPS]
        arr = _group_array([g for _, g in chunk])
        N.check(lib.wsi_gemm_pack_b(op, arr, len(chunk), N.stream()), "wsi_gemm_pack_b")
        _PACKED["packs"] += 1
        for e, _ in chunk:
            e["versions"] = tuple(w._version for w in e["weights"])
            e["armed"] = arm


def _attach_packed(op: int, chunk: Sequence[dict], arr) -> None:
    """Give every group of an NT / NN launch that runs scaled-fp16 the packed form of its weights if an ARMED one exists (``repack_weights``), and
    register the weights so that the next ``repack_weights`` packs them; a group without an armed entry is packed by the call itself, as always."""
    import weakref
    ent = _PACKED["entries"]
    for gi, g in enumerate(chunk):
        ws_ = g.get("Bw")
        if not ws_ or any(not isinstance(w, torch.nn.Parameter) for w in ws_):
            continue                                  # (only module PARAMETERS live from step to step.  A computed weight - HGT's relation-folded projections, and
                                                      # under no_grad also every per-call temporary: LEConv's concatenated weight, a sliced attention vector -
                                                      # is a new tensor per call whose entry would push the real parameters out of the table)
        key = (op, tuple(w.data_ptr() for w in ws_), g["N"], g["K"], g.get("b_chunk", 0), g["ldb"])
        e = ent.get(key)
        if e is not None and any(r() is not w for r, w in zip(e["refs"], ws_)):
            e = None                                  # the address was recycled for another tensor
        if e is None:
            if len(ent) >= 256:
                dead = [k_ for k_, e_ in ent.items() if any(r() is None for r in e_["refs"])]
                for k_ in dead:
                    ent.pop(k_)                      # entries of weights that no longer exist go first
                if len(ent) >= 256:
                    ent.pop(next(iter(ent)))
            nbytes = N.load().wsi_gemm_packed_b_bytes(g["N"], g["K"])
            e = ent[key] = {"buf": torch.empty(nbytes // 4, dtype=torch.int32, device=ws_[0].device), "refs": [weakref.ref(w) for w in ws_],
                            "weights": None, "versions": None, "op": op, "armed": False,
                            "group": dict(B=g["B"], B1=g.get("B1"), B2=g.get("B2"), ldb=g["ldb"], N=g["N"], K=g["K"], b_chunk=g.get("b_chunk", 0))}
            e["group"]["b_packed"] = N.ptr(e["buf"])
            continue
        if e["armed"] and e["versions"] == tuple(w._version for w in ws_):
            _PACKED["hits"] += 1
            e["armed"] = False                        # one use per refresh
            arr[gi].b_packed = e["group"]["b_packed"]


def repack_weights() -> None:
    """Refresh and arm every packed weight (optim.Adam.step calls this behind its update): one launch per op instead of one in front of every
    projection of the next step."""
    if not _PACKED["enabled"] or not _PACKED["entries"] or torch.cuda.is_current_stream_capturing():
        return                                       # (inside a stream capture every projection packs for itself: the recorded step must not depend on this cache)
    by_op = {}
    dead = []
    for key, e in _PACKED["entries"].items():
        ws_ = [r() for r in e["refs"]]
        if any(w is None for w in ws_):
            dead.append(key)
            continue
        e["weights"] = ws_
        by_op.setdefault(e["op"], []).append((e, e["group"]))
    for key in dead:
        _PACKED["entries"].pop(key, None)
    for op, items in by_op.items():
        _pack_groups(op, items, arm=True)
    for e in _PACKED["entries"].values():
        e["weights"] = None


def _gemm(op: int, epilogue: int, groups: Sequence[dict], device) -> bool:
    """Launch wsi_gemm_grouped (chunks of WSI_GEMM_MAX_GROUPS). Each group dict: A,B,C(+bias,R,gate) as
    (tensor, byte_offset) or raw ints, lda/ldb/ldc/ldr, M,N,K.  Returns True when every group that asked for column statistics
    (``c_colmax``) got them (``wsi_gemm_writes_colstats``: only the LDS-DMA scaled-fp16 kernel leaves them)."""
    lib = N.load()
    prec = _GEMM_MODES[_PRECISION["mode"]]
    groups = [g for g in groups if g["M"] > 0 and g["N"] > 0]
    wrote = True
    for i in range(0, len(groups), N.WSI_GEMM_MAX_GROUPS):
        chunk = groups[i:i + N.WSI_GEMM_MAX_GROUPS]
        # positional construction: one C call per group (field-by-field assignment costs ~25 attribute stores each)
        arr = _group_array(chunk)
        if any(g.get("c_colmax") for g in chunk):
            wrote = wrote and bool(lib.wsi_gemm_writes_colstats(op, prec, arr, len(chunk)))
        ws = None
        ws_bytes = 0
        kernel = lib.wsi_gemm_kernel_precision(op, prec, arr, len(chunk))      # resolves "auto" / the TN launches of fp16x3
        if kernel == N.WSI_GEMM_FP16X3 and op != N.WSI_GEMM_TN and _PACKED["enabled"] and not torch.cuda.is_current_stream_capturing():
            _attach_packed(op, chunk, arr)
        if op == N.WSI_GEMM_TN or kernel == N.WSI_GEMM_FP16X3:
            ws_bytes = lib.wsi_gemm_workspace_bytes(op, prec, arr, len(chunk))
            ws = torch.empty(max(ws_bytes // 4, 1), dtype=torch.float32, device=device)
        if not _TIMING["on"]:               # (the common case: no event pairs, no flop count - this function runs ~20 times per step)
            N.check(lib.wsi_gemm_grouped(op, epilogue, prec, arr, len(chunk), N.ptr(ws), ws_bytes, N.stream()), "wsi_gemm_grouped")
            continue
        flops = sum(2.0 * g["M"] * g["N"] * g["K"] for g in chunk)
        products = {N.WSI_GEMM_FP32: 1.0, N.WSI_GEMM_BF16X6: 6.0, N.WSI_GEMM_FP16X3: 3.0}[kernel]
        with _Timed("gemm", flops, flops * products), _Timed(("gemm_nt", "gemm_nn", "gemm_tn")[op] + ("_fp32", "_bf16x6", "_fp16x3")[kernel], flops, flops * products):
            N.check(lib.wsi_gemm_grouped(op, epilogue, prec, arr, len(chunk), N.ptr(ws), ws_bytes, N.stream()), "wsi_gemm_grouped")
    return wrote


_GROUP_FIELDS = [f[0] for f in N.GemmGroup._fields_]
_GROUP_INDEX = {name: i for i, name in enumerate(_GROUP_FIELDS)}
_GROUP_DEFAULT = tuple(1.0 if name == "drop_scale" else (None if N.GemmGroup._fields_[i][1] is ctypes.c_void_p else 0) for i, name in enumerate(_GROUP_FIELDS))


def _group_array(chunk):
    """The wsi_gemm_group_t table of a launch from its group dicts (keys = the struct's field names; anything else - ``Bw`` - is the host's own).
    Positional construction from a default row with only the PRESENT keys written: the struct has 43 fields, a group sets about a dozen, and this
    runs ~35 times per step (one ``dict.get`` per field was 0.6 ms of a launch-bound one-slide step)."""
    index, default = _GROUP_INDEX, _GROUP_DEFAULT
    rows = []
    for g in chunk:
        vals = list(default)
        for k, v in g.items():
            i = index.get(k)
            if i is not None:
                vals[i] = v
        rows.append(N.GemmGroup(*vals))
    return (N.GemmGroup * len(rows))(*rows)


_SMALL_PAIR = {"enabled": True}


def _gemm_small_pair(dx_groups: Sequence[dict], dx_epilogue: int, dw_groups: Sequence[dict], dw_epilogue: int, device) -> bool:
    """dX = dY W (NN groups) and dW = dY^T X (+ db; TN groups) of small Linear layers in ONE launch (``wsi_gemm_small_pair``) - the classifier
    head's levels are one row per graph.  False (nothing launched) when a group is not small or asks for scales: the caller makes its two calls."""
    dx_groups = [g for g in dx_groups if g["M"] > 0 and g["N"] > 0]
    dw_groups = [g for g in dw_groups if g["M"] > 0 and g["N"] > 0]
    if (not _SMALL_PAIR["enabled"] or not dx_groups or not dw_groups or len(dx_groups) + len(dw_groups) > 16
            or any(g["M"] > 32 or g.get("c_absmax") or g.get("b_chunk") for g in dx_groups) or any(g["K"] > 32 or g.get("c_absmax") for g in dw_groups)):
        return False
    flops = sum(2.0 * g["M"] * g["N"] * g["K"] for g in list(dx_groups) + list(dw_groups))
    with _Timed("gemm", flops, flops), _Timed("gemm_small_pair", flops, flops):
        N.check(N.load().wsi_gemm_small_pair(_group_array(dx_groups), len(dx_groups), dx_epilogue, _group_array(dw_groups), len(dw_groups), dw_epilogue,
                                             N.stream()), "wsi_gemm_small_pair")
    return True


# ------------------------------------------------------------------------------------------------
# weight gradients in the background
# ------------------------------------------------------------------------------------------------
# A layer's weight gradients are read by nobody before the optimizer; the attention backward of the layer BELOW is bound by what the fabric
# delivers to its gathers and leaves the matrix cores idle.  The dW launches issued ahead of such a phase (a layer's a_linear dW, and the
# K|Q|V dW of the layer above) therefore go to a second stream, capped at one workgroup per CU (WSI_EPI_BACKGROUND) so that the attention
# waves keep their share of registers and LDS: measured on the bench shapes 1.47 -> 1.29 ms for one dW + one attention backward
# (tools/overlap_probe.py; uncapped: 1.37).  The main stream waits for the side stream once, when the whole backward pass is over
# (autograd's final callback) - before anything can read a gradient.  Off while a data-parallel bucket is armed: its hooks pack gradients
# while backward is still running.
_BACKGROUND = {"enabled": True, "min_flop": 3.0e10, "queued": [], "pending": [], "armed": False, "blocked": False,
               "launches": 0, "task": -1, "written": set()}
# "armed" / "task": the backward pass (autograd graph task id) whose final callback will join the side stream.  The state is keyed to that pass: a pass
# that RAISES skips its final callbacks (OOM on a large slide, a hook error), and whatever it left behind - the flag, queued launches that pin their
# operands, streams nobody waits for - is cleared by the next thing that could be hurt by it (``_background_recover``: the next pass's first queueing
# attempt, every fused-layer forward, ``optim.Adam.step``).  "written": ids of the parameters whose gradient buffers the side stream is still writing.


def set_background_weight_gradients(on: bool) -> None:
    _BACKGROUND["enabled"] = bool(on)


def block_background_weight_gradients(blocked: bool, who: str = "bucket") -> None:
    """dist.GradBucket.arm(): gradients are consumed by hooks DURING backward - every launch stays on the caller's stream.  (``who``: the
    blockers are independent - an armed bucket, a loader that prefetches on a side stream of its own.)"""
    reasons = _BACKGROUND.setdefault("reasons", set())
    (reasons.add if blocked else reasons.discard)(who)
    _BACKGROUND["blocked"] = bool(reasons)


def _background_flush(device, to_side: bool = True) -> None:
    """Launch the queued weight-gradient GEMMs.  Called where an attention backward is about to be launched (``to_side``: on the side stream, which
    first waits for everything the caller's stream holds so far - they then run UNDER that attention phase and not beside the projection
    GEMMs in front of it) and at the join (whatever is still queued has no such phase left to hide under: in order, on the caller's stream)."""
    st = _BACKGROUND
    if not st["queued"]:
        return
    queued, st["queued"] = [q for q in st["queued"] if _outputs_alive(q[4])], []
    queued = [q[:4] for q in queued]
    if not queued:
        return
    dev = torch.device(device)
    if not to_side:
        for epilogue, groups, keep, events in queued:
            for ev in events:
                torch.cuda.current_stream(dev).wait_event(ev)
            _gemm(N.WSI_GEMM_TN, epilogue, groups, dev)
        return
    side = side_stream(dev, "work")
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        for epilogue, groups, keep, events in queued:
            for ev in events:
                side.wait_event(ev)
            _gemm(N.WSI_GEMM_TN, epilogue | N.WSI_EPI_BACKGROUND, groups, dev)
            st["launches"] += 1
    st["pending"].append((side, [k for _, _, keep, _ in queued for k in keep]))


def _outputs_alive(outs) -> bool:
    """Do the buffers a queued launch WRITES still exist?  The queue must not hold them (AccumulateGrad adopts a gradient only when nobody else
    references it), so each is remembered as (weak reference to the tensor the backward returned, weak reference to its parameter, address): alive
    while autograd still holds the tensor, or once the parameter's ``.grad`` IS that buffer.  Neither: the pass that queued the launch died and its
    gradients were released - the launch is dropped."""
    for tref, pref, ptr in outs:
        if tref() is not None:
            continue
        p = pref()
        if p is None or p.grad is None or p.grad.data_ptr() != ptr:
            return False
    return True


def _background_wait_pending() -> None:
    """Order the caller's stream behind every side stream that carries weight gradients; drop the references that kept the operands alive."""
    st = _BACKGROUND
    pend, st["pending"] = st["pending"], []
    done = set()
    for side, _ in pend:
        if id(side) not in done:
            torch.cuda.current_stream(side.device).wait_stream(side)
            done.add(id(side))
    st["written"].clear()


def _background_join() -> None:
    """End of the backward pass: launch what is still queued, order the caller's stream behind the side stream, drop the references that kept the
    operands alive."""
    st = _BACKGROUND
    st["armed"] = False
    st["task"] = -1
    if st["queued"]:
        _background_flush(st["queued"][0][2][0].device, to_side=False)
    _background_wait_pending()


def _background_recover() -> None:
    """Leftovers of a backward pass that never reached its final callback (it raised): queued launches are DROPPED (their pass is dead, nobody will
    read those gradients; launching them now would only write into buffers of a finished step), what the side stream already holds is waited for.
    A no-op in the normal case - called from places that run between passes (a fused layer's forward, the optimizer step) and from the first
    queueing attempt of a new pass."""
    st = _BACKGROUND
    if not (st["armed"] or st["queued"] or st["pending"]):
        return
    cur = torch._C._current_graph_task_id()
    if st["armed"] and st["task"] == cur:
        return                                       # the pass that armed it is still running (a forward inside a backward: checkpointing)
    if cur >= 0:
        return                                       # inside ANOTHER backward pass (nested in the arming one): the arming pass owns the queue and the flag
    st["armed"] = False
    st["task"] = -1
    st["queued"] = []
    _background_wait_pending()


def _background_safe(params: Sequence[Optional[torch.Tensor]]) -> bool:
    """May the gradients of ``params`` be written by the side stream?  Only when each goes STRAIGHT into an AccumulateGrad that adopts the buffer
    without reading it: a leaf with an empty ``.grad``, no tensor hook and no post-accumulate-grad hook (a data-parallel bucket's hooks, a user's
    gradient clipping hook: they would read the buffer on the caller's stream before the side stream has written it), and not already being
    written by this pass (a parameter used twice in the graph: weight tying - the second contribution would be ADDED to the first at once)."""
    st = _BACKGROUND
    foreign = st["armed"] and st["task"] != torch._C._current_graph_task_id()      # another pass holds the queue: see _gemm_tn_background
    for p in params:
        if p is None:
            continue
        if foreign and id(p) not in st["written"]:
            continue
        if (not p.is_leaf or p.grad_fn is not None or p.grad is not None or getattr(p, "_backward_hooks", None)
                or getattr(p, "_post_accumulate_grad_hooks", None) or id(p) in st["written"]):
            if id(p) in st["written"]:
                # the earlier contribution is still in flight on the side stream: AccumulateGrad is about to read it - finish it first
                if st["queued"]:
                    _background_flush(p.device, to_side=False)
                _background_wait_pending()
            return False
    return not foreign


def _gemm_tn_background(epilogue: int, groups: Sequence[dict], device, keep: Sequence[torch.Tensor], written: Sequence[torch.Tensor] = (), events=(),
                        outs=()) -> bool:
    """Queue a weight-gradient GEMM for the side stream (returns False - nothing queued - when the mechanism is off).  ``keep``: every tensor
    the launch READS (at least one); held until the join so that the allocator cannot hand their memory to a later allocation.  The gradients it
    WRITES must reach autograd with no second reference to them and meet an empty ``.grad`` of a plain leaf without hooks (``written``: those
    parameters; the callers check them with ``_background_safe`` first): AccumulateGrad then adopts the buffer without reading it; with a reference
    left, a gradient to add to or a hook, something would read it on the caller's stream at once - before the values exist."""
    st = _BACKGROUND
    if not st["enabled"] or st["blocked"] or torch.is_grad_enabled():        # (create_graph=True: AccumulateGrad never adopts a buffer)
        return False
    dev = torch.device(device)
    if dev.type != "cuda":
        return False
    # worth it only under a long attention backward: on one 10k-node slide the step is launch-bound and the capped launch + the join cost more than
    # they hide (HEATNet4 2.75 -> 3.35 ms eager; replayed as a hipGraph 1.6 -> 2.8 ms: tools/r04_probe_a.sh) - small launches and captures stay in order
    if sum(2.0 * g["M"] * g["N"] * g["K"] for g in groups) < st["min_flop"] or torch.cuda.is_current_stream_capturing():
        return False
    task = torch._C._current_graph_task_id()
    if task < 0:
        return False                                                                       # not inside a backward pass: stay in order
    if st["armed"] and st["task"] != task:
        # Another backward pass holds the queue: a reentrant pass nested inside it (torch.utils.checkpoint(use_reentrant=True), autograd.backward in a
        # hook: the outer pass is ALIVE and will read its gradients) - or a new pass right after one that raised.  The two cannot be told apart from
        # here, so nothing is dropped and nothing is touched: this pass's launches stay in order (a parameter the other pass is still writing is
        # finished first: _background_safe), the queue stays with the pass that armed it - its own final callback joins it; a dead pass's leftovers
        # are dropped by the next forward / optimizer step (_background_recover outside any backward pass) and a launch whose output buffers are
        # gone is never issued (_outputs_alive).
        return False
    if not st["armed"]:
        try:
            torch.autograd.Variable._execution_engine.queue_callback(_background_join)     # runs once, after the last node of this backward pass
        except RuntimeError:
            return False
        st["armed"] = True
        st["task"] = task
    import weakref
    st["queued"].append((epilogue, list(groups), list(keep), list(events),
                         [(weakref.ref(g_), weakref.ref(p_), g_.data_ptr()) for p_, g_ in outs if p_ is not None and g_ is not None]))
    st["written"].update(id(p) for p in written if p is not None)
    return True


class LinearSpec:
    """Static description of a grouped linear: group i maps rows ``rows[i]`` of x through weight i into rows
    ``out_rows[i]`` (default: the same rows) and columns ``[col_off[i], col_off[i]+out_i)`` of y."""

    def __init__(self, rows: Sequence[Tuple[int, int]], col_off: Sequence[int], out_cols: int, num_rows: int,
                 out_rows: Optional[Sequence[Tuple[int, int]]] = None, num_out_rows: Optional[int] = None):
        self.rows = [(int(a), int(b)) for a, b in rows]
        self.out_rows = [(int(a), int(b)) for a, b in (out_rows if out_rows is not None else rows)]
        for (a, b), (c, d) in zip(self.rows, self.out_rows):
            if b - a != d - c:
                raise ValueError("LinearSpec: input and output row ranges differ in length")
        self.col_off = [int(c) for c in col_off]
        self.out_cols = int(out_cols)
        self.num_rows = int(num_rows)
        self.num_out_rows = int(num_out_rows if num_out_rows is not None else num_rows)
        # distinct INPUT row ranges (dX accumulation rounds) and distinct OUTPUT row ranges (bias column sums)
        self.ranges: List[Tuple[int, int]] = []
        self.range_of: List[int] = []
        self.oranges: List[Tuple[int, int]] = []
        self.orange_of: List[int] = []
        for r, o in zip(self.rows, self.out_rows):
            if r not in self.ranges:
                self.ranges.append(r)
            self.range_of.append(self.ranges.index(r))
            if o not in self.oranges:
                self.oranges.append(o)
            self.orange_of.append(self.oranges.index(o))
        self.in_covered = sum(b - a for a, b in self.ranges) == self.num_rows
        self._rplan = None

    def out_covered(self, widths: Sequence[int]) -> bool:
        return sum((b - a) * w for (a, b), w in zip(self.out_rows, widths)) == self.num_out_rows * self.out_cols

    def bias_rplan(self, device):
        """(ReducePlan over the sorted, gap-filled OUTPUT row ranges, segment index of each distinct range)."""
        if self._rplan is None or self._rplan[0].device != device:
            order = sorted(range(len(self.oranges)), key=lambda i: self.oranges[i])
            filled: List[Tuple[int, int]] = []
            seg_of = [0] * len(self.oranges)
            pos = self.oranges[order[0]][0] if order else 0
            for i in order:
                a, b = self.oranges[i]
                if a > pos:
                    filled.append((pos, a))      # gap rows: reduced but never read back
                elif a < pos and b > a:
                    raise ValueError("LinearSpec: overlapping output row ranges")
                seg_of[i] = len(filled)
                filled.append((a, b))
                pos = max(pos, b)
            self._rplan = (ReducePlan.from_ranges(filled, device, chunk=512), seg_of)
        return self._rplan


class _GroupedLinear(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, spec: LinearSpec, epilogue: int, n_w: int, *params):
        N.require_cuda(x)
        weights = params[:n_w]
        biases = params[n_w:]
        x = x.contiguous()
        covered = spec.out_covered([w.shape[0] for w in weights])
        y = (torch.empty if covered else torch.zeros)((spec.num_out_rows, spec.out_cols), dtype=torch.float32, device=x.device)
        K = x.shape[1]
        x_max = row_scales_of(x)                       # fp16x3: row scales of x if its producer left them
        # (a producer's slots are addressed by 128-column tile: only column blocks that start on one can leave scales)
        # (every group a whole number of 128-column tiles and the groups tile the output: every slot of every row gets written - no fill)
        y_max = (_new_row_scale(spec.num_out_rows, N.gemm_absmax_parts(spec.out_cols), x.device, spec.out_cols,
                                zero=not (covered and all(w.shape[0] % 128 == 0 for w in weights)))
                 if all(c % 128 == 0 for c in spec.col_off) else None)
        # column statistics of y for the weight gradient that will read it as its second operand (a layer's K|Q|V gradients read the layer input)
        y_cols = (ColStats.allocate(spec.out_rows, spec.out_cols, x.device, sums=False)
                  if (covered and spec.num_out_rows > 32 and want_col_stats(spec.num_out_rows, spec.out_cols, spec.out_cols)) else None)
        groups = []
        for i, w in enumerate(weights):
            r0, r1 = spec.rows[i]
            o0, o1 = spec.out_rows[i]
            b = biases[i]
            groups.append(dict(A=N.ptr(x, r0 * K * 4), lda=K, B=N.ptr(w), ldb=w.stride(0), Bw=[w],
                               C=N.ptr(y, (o0 * spec.out_cols + spec.col_off[i]) * 4), ldc=spec.out_cols,
                               bias=N.ptr(b), M=r1 - r0, N=w.shape[0], K=K,
                               **_scale_in(x_max, r0), **_scale_out(y_max, o0, spec.col_off[i]),
                               **(y_cols.produce(o0, o1, spec.col_off[i]) if y_cols is not None else {})))
        epi = (N.WSI_EPI_BIAS if any(b is not None for b in biases) else 0) | epilogue
        wrote = _gemm(N.WSI_GEMM_NT, epi, groups, x.device)
        if y_max is not None:
            attach_row_scales(y, y_max)
        if y_cols is not None and wrote:
            attach_col_stats(y, y_cols)
        ctx.x_cols = col_stats_of(x)                   # (the weight gradient's second operand: constant features carry theirs - remember_constant_cols)
        ctx.spec, ctx.n_w = spec, n_w
        ctx.has_bias = [b is not None for b in biases]
        ctx.save_for_backward(x, *weights)
        return y

    @staticmethod
    def backward(ctx, gy):
        spec, n_w = ctx.spec, ctx.n_w
        x, *weights = ctx.saved_tensors
        gy = gy.contiguous()
        K = x.shape[1]
        dev = x.device
        gws: List[Optional[torch.Tensor]] = [None] * n_w
        gbs: List[Optional[torch.Tensor]] = [None] * n_w
        need_w = [ctx.needs_input_grad[4 + i] for i in range(n_w)]
        need_b = [ctx.has_bias[i] and ctx.needs_input_grad[4 + n_w + i] for i in range(n_w)]
        wgroups = []
        gy_cols, x_cols = col_stats_of(gy), getattr(ctx, "x_cols", None)
        for i in range(n_w):
            if not need_w[i]:
                continue
            r0, r1 = spec.rows[i]
            o0, o1 = spec.out_rows[i]
            w = weights[i]
            gws[i] = torch.empty_like(w, memory_format=torch.contiguous_format)
            if need_b[i]:      # bias gradient = column sums of dY, taken from the tiles the dW GEMM stages anyway
                gbs[i] = torch.empty(w.shape[0], dtype=torch.float32, device=dev)
                need_b[i] = False
            wgroups.append(dict(A=N.ptr(gy, (o0 * spec.out_cols + spec.col_off[i]) * 4), lda=spec.out_cols,
                                B=N.ptr(x, r0 * K * 4), ldb=K, C=N.ptr(gws[i]), ldc=K, colsum_out=N.ptr(gbs[i]),
                                M=w.shape[0], N=K, K=r1 - r0,
                                **(gy_cols.consume("a", o0, o1, spec.col_off[i], want_sums=gbs[i] is not None) if gy_cols is not None else {}),
                                **(x_cols.consume("b", r0, r1, 0) if x_cols is not None else {})))
        gx = None
        if ctx.needs_input_grad[0]:
            gx = (torch.empty if spec.in_covered else torch.zeros)((spec.num_rows, K), dtype=torch.float32, device=dev)
            # rounds: the r-th group of every distinct input row range; round 0 overwrites, later rounds accumulate
            seen = [0] * len(spec.ranges)
            rounds: List[List[int]] = []
            for i in range(n_w):
                r = seen[spec.range_of[i]]
                seen[spec.range_of[i]] += 1
                while len(rounds) <= r:
                    rounds.append([])
                rounds[r].append(i)
            # fp16x3 row scales: dY's are usable when every group reads whole rows of it; dX's are final after ONE round only
            whole = all(spec.col_off[i] == 0 and weights[i].shape[0] == spec.out_cols for i in range(n_w))
            small = len(rounds) == 1 and spec.num_rows <= 32       # (the classifier head: one row per graph - no scales, one launch for dX and dW)
            gy_max = row_scales_of(gy) if (whole and not small) else None
            gx_max = _new_row_scale(spec.num_rows, N.gemm_absmax_parts(K), dev, K) if (len(rounds) == 1 and not small) else None
            for r, idxs in enumerate(rounds):
                groups = []
                for i in idxs:
                    r0, r1 = spec.rows[i]
                    o0 = spec.out_rows[i][0]
                    w = weights[i]
                    groups.append(dict(A=N.ptr(gy, (o0 * spec.out_cols + spec.col_off[i]) * 4), lda=spec.out_cols,
                                       B=N.ptr(w), ldb=w.stride(0), Bw=[w], C=N.ptr(gx, r0 * K * 4), ldc=K,
                                       M=r1 - r0, N=K, K=w.shape[0], **_scale_in(gy_max, o0), **_scale_out(gx_max, r0)))
                if small and wgroups and _gemm_small_pair(groups, 0, wgroups, 0, dev):
                    wgroups = []
                    continue
                _gemm(N.WSI_GEMM_NN, N.WSI_EPI_ACCUMULATE if r > 0 else 0, groups, dev)
            if gx_max is not None:
                attach_row_scales(gx, gx_max)
        if wgroups:
            _gemm(N.WSI_GEMM_TN, 0, wgroups, dev)
        if any(need_b):
            rp, seg_of = spec.bias_rplan(dev)
            colsum = _segment_reduce_raw(gy, rp, N.WSI_RED_SUM)[0]   # [n_segments, out_cols]
            for i in range(n_w):
                if need_b[i]:
                    c0 = spec.col_off[i]
                    gbs[i] = colsum[seg_of[spec.orange_of[i]], c0:c0 + weights[i].shape[0]]
        return (gx, None, None, None, *gws, *gbs)


def grouped_linear(x: torch.Tensor, spec: LinearSpec, weights: Sequence[torch.Tensor],
                   biases: Sequence[Optional[torch.Tensor]]) -> torch.Tensor:
    """y[rows_i, col_off_i : col_off_i+out_i] = x[rows_i] @ W_i^T + b_i for every group, one launch."""
    return _GroupedLinear.apply(x, spec, 0, len(weights), *weights, *biases)


_LINEAR_SPECS: dict = {}


def linear(x: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor]) -> torch.Tensor:
    """nn.Linear forward/backward on the MFMA GEMM (single group)."""
    key = (x.shape[0], weight.shape[0], str(x.device))
    spec = _LINEAR_SPECS.get(key)
    if spec is None:   # cached: the spec owns device-side chunk tables (bias gradient) that must not be rebuilt per step
        if len(_LINEAR_SPECS) >= 512:                   # bounded: graphs of ever-changing sizes must not grow it forever
            _LINEAR_SPECS.pop(next(iter(_LINEAR_SPECS)))
        spec = _LINEAR_SPECS[key] = LinearSpec([(0, x.shape[0])], [0], weight.shape[0], x.shape[0])
    return _GroupedLinear.apply(x, spec, 0, 1, weight, bias)


# ------------------------------------------------------------------------------------------------
# HEAT relation attention
# ------------------------------------------------------------------------------------------------
def _attn_flags(plan: GraphPlan) -> int:
    return (N.WSI_ATTN_XCD_CONTIGUOUS if getattr(plan, "locality", False) else 0) | ((int(plan.heavy_degree) & 0xffff) << 8)



class _HeatAttention(torch.autograd.Function):
    @staticmethod
    def forward(ctx, kqv, e_weight, e_bias, plan: GraphPlan, sim_csr, D: int, H: int):
        N.require_cuda(kqv, sim_csr)
        lib = N.load()
        kqv = kqv.contiguous()
        n, E, S = plan.num_nodes, plan.num_edges, plan.num_segs
        ld = kqv.shape[1]
        dev = kqv.device
        t = torch.empty((n, D), dtype=torch.float32, device=dev)
        score = torch.empty((max(E, 1), H), dtype=torch.float32, device=dev)
        lse = torch.empty((max(S, 1), H), dtype=torch.float32, device=dev)
        ew = e_weight.reshape(-1)
        eb = e_bias.reshape(-1)
        with _Timed("heat_attn"):
            N.check(lib.wsi_heat_attn_fwd(
                N.ptr(kqv, D * 4), ld, N.ptr(kqv, 0), ld, N.ptr(kqv, 2 * D * 4), ld,
                n, D, H,
                N.ptr(plan.node_seg), N.ptr(plan.rowptr), N.ptr(plan.src), N.ptr(sim_csr), N.ptr(plan.order_dst), plan.num_heavy, _attn_flags(plan),
                N.ptr(ew), N.ptr(eb),
                N.ptr(t), D, N.ptr(score), N.ptr(lse), None, N.context(), N.stream()), "wsi_heat_attn_fwd")
        ctx.plan, ctx.D, ctx.H = plan, D, H
        ctx.save_for_backward(kqv, ew, eb, sim_csr, score, lse)
        return t

    @staticmethod
    def backward(ctx, g_t):
        lib = N.load()
        plan, D, H = ctx.plan, ctx.D, ctx.H
        kqv, ew, eb, sim_csr, score, lse = ctx.saved_tensors
        g_t = g_t.contiguous()
        n, E = plan.num_nodes, plan.num_edges
        ld = kqv.shape[1]
        dev = kqv.device
        a = torch.empty_like(score)   # pass 1 reads the saved logits and writes the probabilities here
        scratch = torch.empty((3, max(E, 1), H), dtype=torch.float32, device=dev)
        red_ws = torch.empty(1024, dtype=torch.float32, device=dev)
        gkqv = torch.empty_like(kqv)
        g_e = torch.empty(2, dtype=torch.float32, device=dev)
        with _Timed("heat_attn"):
          N.check(lib.wsi_heat_attn_bwd(
            N.ptr(kqv, D * 4), ld, N.ptr(kqv, 0), ld, N.ptr(kqv, 2 * D * 4), ld,
            n, plan.num_src_rows, E, D, H,
            N.ptr(plan.node_seg), N.ptr(plan.rowptr), N.ptr(plan.src), N.ptr(sim_csr),
            N.ptr(plan.colptr), N.ptr(plan.csc_eid), N.ptr(plan.csc_dst),
            N.ptr(plan.inv_rd), N.ptr(plan.order_dst), plan.num_heavy, N.ptr(plan.order_src), _attn_flags(plan),
            N.ptr(ew), N.ptr(eb),
            N.ptr(g_t), g_t.shape[1], None, N.ptr(score), N.ptr(a), N.ptr(lse),
            N.ptr(scratch[0]), N.ptr(scratch[1]), N.ptr(scratch[2]), N.ptr(red_ws),
            N.ptr(gkqv, D * 4), ld, N.ptr(gkqv, 0), ld, N.ptr(gkqv, 2 * D * 4), ld,
            N.ptr(g_e), None, None, N.context(), N.stream()), "wsi_heat_attn_bwd")
        return gkqv, g_e[0:1].view(1, 1), g_e[1:2], None, None, None, None


def heat_attention(kqv: torch.Tensor, e_weight: torch.Tensor, e_bias: torch.Tensor, plan: GraphPlan,
                   sim_csr: torch.Tensor, D: int, H: int) -> torch.Tensor:
    """t[N,D] from the fused K|Q|V table ``kqv`` [N,3D] (K at column 0, Q at D, V at 2D)."""
    return _HeatAttention.apply(kqv, e_weight, e_bias, plan, sim_csr, D, H)


# ------------------------------------------------------------------------------------------------
# segmented reduction
# ------------------------------------------------------------------------------------------------
class ReducePlan:
    """Chunk tables for wsi_segment_reduce_* (see include/wsi_hgnn.h)."""

    def __init__(self):
        self.device = None
        self.num_segs = 0
        self.num_chunks = 0
        self.num_rows = 0
        self.first_row = 0
        self.chunk_row = None
        self.chunk_seg = None
        self.seg_chunk = None
        self.ranges: List[Tuple[int, int]] = []      # host copy of the segments' row ranges
        self._counts = None
        self._inv_counts = None
        self._row_seg = None
        self._nonempty = None
        self._seg_of = {}
        self.type_rows = None          # optional record of the builder: the row ranges the plan was made for ...
        self.type_segments = None      # ... and the run of segments of each

    @classmethod
    def from_ptr(cls, seg_ptr: Sequence[int], device, chunk: int = 128) -> "ReducePlan":
        return cls.from_ranges([(int(seg_ptr[i]), int(seg_ptr[i + 1])) for i in range(len(seg_ptr) - 1)], device, chunk)

    @classmethod
    def from_ranges(cls, ranges: Sequence[Tuple[int, int]], device, chunk: int = 128) -> "ReducePlan":
        """``ranges`` = row range of every segment, sorted and gap-free (each start == previous end)."""
        p = cls()
        chunk_row: List[int] = []
        chunk_seg: List[int] = []
        seg_chunk = [0]
        pos = ranges[0][0] if ranges else 0
        first = pos
        for s, (a, b) in enumerate(ranges):
            if a != pos or b < a:
                raise ValueError("ReducePlan: segments must be sorted and contiguous")
            r = a
            while r < b:
                chunk_row.append(r)
                chunk_seg.append(s)
                r = min(b, r + chunk)
            pos = b
            seg_chunk.append(len(chunk_row))
        chunk_row.append(pos)
        p.device = device
        p.ranges = [(int(a), int(b)) for a, b in ranges]
        p.num_segs = len(ranges)
        p.num_chunks = len(chunk_seg)
        p.num_rows = pos - first
        p.first_row = first
        # ONE upload for everything the plan keeps on the device (a new batch of a loader-fed run builds two plans per step: seven small
        # uploads each were a quarter of a millisecond of host time): the three chunk tables, then counts / inverse counts / non-empty flags as
        # float bits.  The attributes are views into that buffer.
        cs = chunk_seg if chunk_seg else [0]
        cnt = [float(b - a) for a, b in p.ranges] or [0.0]
        inv = [1.0 / (b - a) if b > a else 0.0 for a, b in p.ranges] or [0.0]
        non = [1.0 if b > a else 0.0 for a, b in p.ranges] or [0.0]
        host = torch.cat([torch.tensor(chunk_row + cs + seg_chunk, dtype=torch.int32), torch.tensor(cnt + inv + non, dtype=torch.float32).view(torch.int32)])
        buf = host_to_device(host, torch.int32, device)
        o1 = len(chunk_row); o2 = o1 + len(cs); o3 = o2 + len(seg_chunk); k = len(cnt)
        p.chunk_row, p.chunk_seg, p.seg_chunk = buf[:o1], buf[o1:o2], buf[o2:o3]
        p._counts = buf[o3:o3 + k].view(torch.float32).view(-1, 1)
        p._inv_counts = buf[o3 + k:o3 + 2 * k].view(torch.float32).view(-1, 1)
        p._nonempty = buf[o3 + 2 * k:o3 + 3 * k].view(torch.float32).view(-1, 1)
        return p


    def counts(self) -> torch.Tensor:
        """[num_segs, 1] fp32 row counts of the segments (device)."""
        if self._counts is None:
            self._counts = host_to_device([float(b - a) for a, b in self.ranges] or [0.0], torch.float32, self.device).view(-1, 1)
        return self._counts

    def inv_counts(self) -> torch.Tensor:
        """[num_segs, 1]: 1 / rows of the segment, 0 for an empty one."""
        if self._inv_counts is None:
            self._inv_counts = host_to_device([1.0 / (b - a) if b > a else 0.0 for a, b in self.ranges] or [0.0], torch.float32, self.device).view(-1, 1)
        return self._inv_counts

    def prepare_broadcast(self) -> None:
        """Upload the small per-segment tables the low-rank readout gradient path uses (``SegmentBroadcast``), from the thread and
        at the time the plan is first used - not from inside the backward pass of the first step that meets a new batch."""
        self.counts(); self.inv_counts(); self.nonempty(); self.row_segment()

    def has_empty(self) -> bool:
        return any(b == a for a, b in self.ranges)

    def nonempty(self) -> torch.Tensor:
        """[num_segs, 1]: 1.0 for a segment with rows, 0.0 for an empty one."""
        if self._nonempty is None:
            self._nonempty = host_to_device([1.0 if b > a else 0.0 for a, b in self.ranges] or [0.0], torch.float32, self.device).view(-1, 1)
        return self._nonempty

    def row_segment(self) -> torch.Tensor:
        """[num_rows] int32: the segment of every row (device)."""
        if self._row_seg is None:
            # expanded ON THE DEVICE from the S counts (output size known: no sync).  A [num_rows] table built on the host costs a
            # multi-threaded CPU copy into the staging buffer per new batch - measured 70-100 ms stalls of the whole process on a
            # CPU-quota'd box (the OpenMP workers spin after the copy and the cgroup gets throttled).
            dev = torch.device(self.device)
            if dev.type == "cuda":
                # one upload + one launch: a run of `rows` copies of the segment number per segment (wsi_plan_assemble, mode 0 with add = s)
                out = torch.empty(max(self.num_rows, 1), dtype=torch.int32, device=dev)[:self.num_rows]
                tb = SegmentTable("row_segment")
                for s_, (a, b) in enumerate(self.ranges):
                    tb.seg(out, a - self.first_row, b - a, add=s_)
                if tb.nsegs:
                    self._row_seg_desc = tb.upload(dev)
                    N.check(N.load().wsi_plan_assemble(N.ptr(self._row_seg_desc), tb.nsegs, tb.blocks, N.stream()), "wsi_plan_assemble")
                self._row_seg = out
            else:
                reps = torch.tensor([b - a for a, b in self.ranges], dtype=torch.int64)
                self._row_seg = torch.repeat_interleave(torch.arange(len(self.ranges), dtype=torch.int32), reps)
        return self._row_seg

    def segments_of(self, rows: Sequence[Tuple[int, int]]) -> Optional[List[Tuple[int, int]]]:
        """For row ranges that are unions of consecutive segments: the segment index range of each; None if one is not.  A plan built for
        known row ranges (``type_rows`` / ``type_segments``, set by its builder: the readout plan's B segments per node type) answers from
        that record - an EMPTY segment on a boundary between two ranges belongs to exactly one of them, which row numbers alone cannot
        tell.  Otherwise sorted, gap-free ranges are matched by a walk in which such a segment goes with the range on its LEFT."""
        key = tuple(rows)
        hit = self._seg_of.get(key)
        if hit is None:
            res: Optional[List[Tuple[int, int]]]
            if self.type_rows is not None and list(self.type_rows) == [tuple(r) for r in rows]:
                res = list(self.type_segments)
            else:
                res, cur = [], 0
                for a, b in rows:
                    if a == b:
                        res.append((0, 0))
                        continue
                    s0 = cur
                    if s0 >= len(self.ranges) or self.ranges[s0][0] != a:
                        res = None
                        break
                    s1 = s0
                    while s1 < len(self.ranges) and self.ranges[s1][1] <= b and self.ranges[s1][0] >= a:
                        s1 += 1
                    if s1 == s0 or self.ranges[s1 - 1][1] != b:
                        res = None
                        break
                    res.append((s0, s1))
                    cur = s1
            hit = self._seg_of[key] = (res,)
        return hit[0]


def _segment_reduce_raw(x: torch.Tensor, rp: ReducePlan, op: int):
    lib = N.load()
    D = x.shape[1]
    dev = x.device
    out = torch.empty((rp.num_segs, D), dtype=torch.float32, device=dev)
    extra = 2 if op == N.WSI_RED_MAX else 1
    partial = torch.empty(max(rp.num_chunks * D * extra, 1), dtype=torch.float32, device=dev)
    argmax = torch.empty((rp.num_segs, D), dtype=torch.int32, device=dev) if op == N.WSI_RED_MAX else None
    N.check(lib.wsi_segment_reduce_fwd(N.ptr(x), x.stride(0), D, op, N.ptr(rp.chunk_row), rp.num_chunks,
                                       N.ptr(rp.seg_chunk), rp.num_segs, N.ptr(partial), N.ptr(out), D,
                                       N.ptr(argmax), N.stream()), "wsi_segment_reduce_fwd")
    return out, argmax


class SegmentBroadcast:
    """What the backward of a sum / mean readout knows about the gradient it hands down: ``gx[row] = g_row[segment of row]`` -
    a matrix of rank <= num_segs (graphs x node types), not of rank num_rows.  The layer that receives ``gx`` unchanged
    (``_HeatLayerFused.backward``) computes its output-projection gradients from the [num_segs, D] factors instead of running
    [num_rows]-deep GEMMs over identical rows.  ``x_ptr`` / ``x_version`` identify the tensor the readout reduced and ``x_mean`` its segment means."""

    def __init__(self, g_seg, rp, op, pooled, x_ptr, x_version):
        if op == N.WSI_RED_MEAN:
            self.g_row = g_seg * rp.inv_counts()        # gradient of every row of the segment
            self.g_sum = g_seg * rp.nonempty() if rp.has_empty() else g_seg      # count x g_row: the segment's rows summed
            self.x_mean = pooled
        else:
            self.g_row = g_seg
            self.g_sum = g_seg * rp.counts()
            self.x_mean = pooled * rp.inv_counts()
        self.rp, self.x_ptr, self.x_version = rp, x_ptr, x_version

    @classmethod
    def from_parts(cls, rp, g_row: torch.Tensor, g_sum: torch.Tensor, x_mean: torch.Tensor) -> "SegmentBroadcast":
        """The factors as ``wsi_pool_bwd_prep`` leaves them (same meaning as ``from_pooled_gradient`` computes with tensor operations)."""
        self = cls.__new__(cls)
        self.rp, self.x_ptr, self.x_version, self.x_mean, self.g_row, self.g_sum = rp, None, None, x_mean, g_row, g_sum
        return self

    @classmethod
    def from_pooled_gradient(cls, g_pool: torch.Tensor, rp, op: int, x_mean: torch.Tensor) -> "SegmentBroadcast":
        """The same factors for a layer that returned its readout itself (``_HeatLayerFused(pool=)``): ``g_pool`` is the gradient of the pooled
        rows [num_segs, D] (zero weight on empty segments: the forward masked them), ``x_mean`` the segment means of the never-formed output."""
        self = cls.__new__(cls)
        self.rp, self.x_ptr, self.x_version, self.x_mean = rp, None, None, x_mean
        if op == N.WSI_RED_MEAN:
            self.g_row = g_pool * rp.inv_counts()
            self.g_sum = g_pool * rp.nonempty() if rp.has_empty() else g_pool
        else:
            self.g_row, self.g_sum = g_pool, g_pool * rp.counts()
        return self


_LOW_RANK = {"enabled": True}


_COLLAPSE_V = {"enabled": True, "min_work": 4.0e9}


def set_value_collapse(on: bool, min_work: Optional[float] = None) -> None:
    """On (default): a readout-fused last layer never forms V or g_v (rank <= segments x heads): ``wsi_attn_pool_t``.  Off: V goes through
    the K|Q|V projections like K and Q (A/B measurements, parity tests of both forms).  ``min_work``: rows x D x D below which the layer
    keeps V anyway - the collapse trades three [rows, D] x [D, D] projections for ~25 small launches and a heavier pass 1 (measured on one
    MI355X: 80 000 x 512^2 = 2.1e10: 7.38 -> 7.02 ms per step; 40 000 x 256^2 = 2.6e9: 2.24 -> 2.57 ms; default threshold 4e9)."""
    _COLLAPSE_V["enabled"] = bool(on)
    if min_work is not None:
        _COLLAPSE_V["min_work"] = float(min_work)


def set_low_rank_readout_grad(on: bool) -> None:
    """On (default): the layer under a sum / mean readout uses the rank-(graphs x node types) structure of the gradient it
    receives (see ``SegmentBroadcast``).  Off: every gradient goes through the full-depth GEMMs (A/B measurements, parity tests)."""
    _LOW_RANK["enabled"] = bool(on)


class _SegmentReduce(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, rp: ReducePlan, op: int):
        N.require_cuda(x)
        x = x.contiguous()
        out, argmax = _segment_reduce_raw(x, rp, op)
        ctx.rp, ctx.op, ctx.shape = rp, op, x.shape
        ctx.x_id = (x.data_ptr(), x._version)
        ctx.save_for_backward(argmax) if argmax is not None else ctx.save_for_backward(out)
        return out

    @staticmethod
    def backward(ctx, gout):
        lib = N.load()
        rp, op = ctx.rp, ctx.op
        gout = gout.contiguous()
        n, D = ctx.shape
        argmax = ctx.saved_tensors[0] if op == N.WSI_RED_MAX else None
        # rows not covered by any segment (none in practice) and max-pool non-argmax rows get zero
        covered = rp.num_rows == n and op != N.WSI_RED_MAX
        gx = (torch.empty if covered else torch.zeros)((n, D), dtype=torch.float32, device=gout.device)
        N.check(lib.wsi_segment_reduce_bwd(N.ptr(gout), gout.stride(0), D, op, N.ptr(rp.chunk_row), N.ptr(rp.chunk_seg),
                                           rp.num_chunks, N.ptr(rp.seg_chunk), rp.num_segs, N.ptr(argmax),
                                           N.ptr(gx), D, N.stream()), "wsi_segment_reduce_bwd")
        if covered and _LOW_RANK["enabled"] and rp.first_row == 0 and rp.num_segs * 8 <= n:
            _annotate(gx, "_wsi_broadcast", SegmentBroadcast(gout, rp, op, ctx.saved_tensors[0], *ctx.x_id))
        return gx, None, None


def segment_reduce(x: torch.Tensor, rp: ReducePlan, op: str) -> torch.Tensor:
    """[num_rows, D] -> [num_segs, D]; op in {'sum','mean','max'}; empty segments give 0."""
    code = {"sum": N.WSI_RED_SUM, "mean": N.WSI_RED_MEAN, "max": N.WSI_RED_MAX}[op]
    return _SegmentReduce.apply(x, rp, code)


def segment_weighted_sums(x: torch.Tensor, w: torch.Tensor, rp: "ReducePlan") -> torch.Tensor:
    """out[s, j, :] = sum over the rows r of segment s of w[r, j] * x[r, :];  x [rows, D], w [rows, J] -> [num_segs, J, D]."""
    N.require_cuda(x, w)
    x, w = x.contiguous(), w.contiguous()
    D, J = x.shape[1], w.shape[1]
    out = torch.empty((rp.num_segs, J, D), dtype=torch.float32, device=x.device)
    partial = torch.empty(max(rp.num_chunks * J * D, 1), dtype=torch.float32, device=x.device)
    N.check(N.load().wsi_segment_weighted_sums(N.ptr(x), D, D, N.ptr(w), J, J, N.ptr(rp.chunk_row), rp.num_chunks, N.ptr(rp.seg_chunk),
                                               rp.num_segs, N.ptr(partial), N.ptr(out), N.stream()), "wsi_segment_weighted_sums")
    return out


# ------------------------------------------------------------------------------------------------
# bag softmax pooling and the DSMIL score step (wsi_bag_softmax_pool_* / wsi_bag_scores_*: the MIL baselines, wsi_hgnn_amd.mil)
# ------------------------------------------------------------------------------------------------
def _bag_rows(what: str, rp: ReducePlan, *tensors) -> None:
    for t in tensors:
        if t.dim() != 2 or t.dtype != torch.float32:
            raise ValueError(f"{what}: expected 2-D float32 tensors, got {tuple(t.shape)} {t.dtype}")
        if rp.first_row != 0 or rp.num_rows != t.shape[0]:
            raise ValueError(f"{what}: the plan covers rows [{rp.first_row}, {rp.first_row + rp.num_rows}) but a tensor has {t.shape[0]} rows")


class _BagSoftmaxPool(torch.autograd.Function):
    @staticmethod
    def forward(ctx, scores, values, rp: ReducePlan, scale: float):
        N.require_cuda(scores, values)
        _bag_rows("bag_softmax_pool", rp, scores, values)
        scores, values = scores.contiguous(), values.contiguous()
        C, D, dev = scores.shape[1], values.shape[1], values.device
        out = torch.empty((rp.num_segs, C, D), dtype=torch.float32, device=dev)
        lse = torch.empty((rp.num_segs, C), dtype=torch.float32, device=dev)
        stats = torch.empty((rp.num_segs, C, 2), dtype=torch.float32, device=dev)
        partial = torch.empty(max(rp.num_chunks * C * (D + 2), 1), dtype=torch.float32, device=dev)
        N.check(N.load().wsi_bag_softmax_pool_fwd(N.ptr(scores), C, C, scale, N.ptr(values), D, D, N.ptr(rp.chunk_row), rp.num_chunks,
                                                  N.ptr(rp.seg_chunk), rp.num_segs, N.ptr(partial), N.ptr(out), N.ptr(lse), N.ptr(stats),
                                                  N.stream()), "wsi_bag_softmax_pool_fwd")
        ctx.rp, ctx.scale = rp, scale
        ctx.save_for_backward(scores, values, out, stats)
        ctx.mark_non_differentiable(lse, stats)
        return out, lse, stats

    @staticmethod
    def backward(ctx, g_out, _g_lse, _g_stats):
        scores, values, out, stats = ctx.saved_tensors
        rp = ctx.rp
        g_out = g_out.contiguous()
        C, D, dev = scores.shape[1], values.shape[1], values.device
        g_scores = torch.empty_like(scores) if ctx.needs_input_grad[0] else None
        g_values = torch.empty_like(values) if ctx.needs_input_grad[1] else None
        delta = torch.empty(max(rp.num_segs * C, 1), dtype=torch.float32, device=dev) if g_scores is not None else None
        N.check(N.load().wsi_bag_softmax_pool_bwd(N.ptr(g_out), N.ptr(out), N.ptr(scores), C, C, ctx.scale, N.ptr(stats), N.ptr(values), D, D,
                                                  N.ptr(rp.chunk_row), N.ptr(rp.chunk_seg), rp.num_chunks, rp.num_segs, N.ptr(delta),
                                                  N.ptr(g_scores), C, N.ptr(g_values), D, N.stream()), "wsi_bag_softmax_pool_bwd")
        return g_scores, g_values, None, None


def bag_softmax_pool_lse(scores: torch.Tensor, values: torch.Tensor, rp: ReducePlan, scale: float = 1.0):
    """(out, lse, stats): ``bag_softmax_pool`` together with lse [num_segs, C] = logsumexp over the segment's rows of scale * scores and
    with stats [num_segs, C, 2] = its two terms apart (the segment's maximum, the log of the sum rescaled by it) - neither differentiable.
    The backward and ``bag_attention`` form the weights from ``stats``: the float32 sum of the two has an ulp of 1e-3 at scores near -1e4."""
    return _BagSoftmaxPool.apply(scores, values, rp, float(scale))


def bag_softmax_pool(scores: torch.Tensor, values: torch.Tensor, rp: ReducePlan, scale: float = 1.0) -> torch.Tensor:
    """out[s, c, :] = sum over the rows r of segment s of softmax_r(scale * scores[:, c])[r] * values[r, :];  scores [rows, C] (C <= 8),
    values [rows, D] -> [num_segs, C, D].  The softmax runs over the rows of each segment (bag) alone; an empty segment gives 0."""
    return _BagSoftmaxPool.apply(scores, values, rp, float(scale))[0]


def bag_attention(scores: torch.Tensor, lse: torch.Tensor, rp: ReducePlan, scale: float = 1.0) -> torch.Tensor:
    """[rows, C]: the normalised attention exp(scale * scores - lse[segment of the row]) the MIL references return as ``A`` (detached).
    ``lse``: [num_segs, C], or the ``stats`` [num_segs, C, 2] of ``bag_softmax_pool_lse`` (its two terms, subtracted one after the other)."""
    N.require_cuda(scores, lse)
    per_row = lse.detach().index_select(0, rp.row_segment())
    s = scores.detach() * float(scale)
    return torch.exp(s - per_row) if lse.dim() == 2 else torch.exp((s - per_row[..., 0]) - per_row[..., 1])


class _BagScores(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q, onehot, rp: ReducePlan):
        N.require_cuda(q, onehot)
        _bag_rows("bag_scores", rp, q, onehot)
        q, onehot = q.contiguous(), onehot.contiguous()
        C, D = onehot.shape[1], q.shape[1]
        q_max = segment_weighted_sums(q, onehot, rp)                     # [S, C, D]: the marked row of every (bag, column); 0 where none is
        scores = torch.empty((q.shape[0], C), dtype=torch.float32, device=q.device)
        N.check(N.load().wsi_bag_scores_fwd(N.ptr(q), D, D, N.ptr(q_max), C, N.ptr(rp.chunk_row), N.ptr(rp.chunk_seg), rp.num_chunks,
                                            N.ptr(scores), C, N.stream()), "wsi_bag_scores_fwd")
        ctx.rp = rp
        ctx.save_for_backward(q, onehot, q_max)
        return scores

    @staticmethod
    def backward(ctx, g_scores):
        q, onehot, q_max = ctx.saved_tensors
        rp = ctx.rp
        if not ctx.needs_input_grad[0]:
            return None, None, None
        g_scores = g_scores.contiguous()
        C, D = onehot.shape[1], q.shape[1]
        g_q_max = segment_weighted_sums(q, g_scores, rp)                 # [S, C, D]: sum_r g_scores[r, c] * q[r]
        g_q = torch.empty_like(q)
        # a row's own score term, and - where the row is a marked one - the gradient of the q_max it supplied (dense: no scatter-add)
        N.check(N.load().wsi_bag_scores_bwd(N.ptr(g_scores), C, N.ptr(q_max), N.ptr(onehot), C, N.ptr(g_q_max), C, D, N.ptr(rp.chunk_row),
                                            N.ptr(rp.chunk_seg), rp.num_chunks, N.ptr(g_q), D, N.stream()), "wsi_bag_scores_bwd")
        return g_q, None, None


def bag_scores(q: torch.Tensor, onehot: torch.Tensor, rp: ReducePlan) -> torch.Tensor:
    """DSMIL's score step over many bags: scores[r, c] = <q[r], q_max[seg(r), c]> where q_max[s, c] = sum over the rows of bag s of
    onehot[r, c] * q[r] - the query of the critical instance ``onehot`` [rows, C] marks (an all-zero column: q_max = 0).  The gradient
    reaches ``q`` through both factors, in a number of launches that does not depend on the number of bags and without atomics."""
    return _BagScores.apply(q, onehot, rp)


# ------------------------------------------------------------------------------------------------
# global attention readout (wsi_attn_readout_*: pooling.GlobalAttentionPooling, graph_pooling_type 'att')
# ------------------------------------------------------------------------------------------------
_FUSED_ATT_READOUT = {"enabled": False}


def set_fused_attention_readout(on: bool) -> None:
    """On: ``pooling.GlobalAttentionPooling`` runs as ``attention_readout`` (one pass over the node table, wsi_attn_readout_fwd / _bwd) on
    every graph.  Off (default): the composite form (a one-column GEMM, three segmented reductions, an exp and ``x * (ex / den)``) - except
    on a slot's padded batch, which has no host-side node counts to expand and always takes the fused path."""
    _FUSED_ATT_READOUT["enabled"] = bool(on)


def fused_attention_readout() -> bool:
    return _FUSED_ATT_READOUT["enabled"]


def attention_readout_reference(x: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor], rp: ReducePlan) -> torch.Tensor:
    """``attention_readout`` as tensor operations under autograd, in the dtype of ``x``: what a CPU tensor takes, and the oracle the kernels
    are held against.  The row -> segment table is the plan's (``rp.row_segment()``), so it runs from a slot's device tables as well."""
    seg = rp.row_segment().to(torch.int64)
    S = rp.num_segs
    gate = x @ weight.reshape(-1).to(x.dtype)
    if bias is not None:
        gate = gate + bias.reshape(()).to(x.dtype)
    mx = torch.zeros(S, dtype=x.dtype, device=x.device).scatter_reduce(0, seg, gate.detach(), "amax", include_self=False)
    ex = torch.exp(gate - mx.index_select(0, seg))
    den = torch.zeros(S, dtype=x.dtype, device=x.device).index_add(0, seg, ex)
    p = ex / den.index_select(0, seg)
    return torch.zeros((S, x.shape[1]), dtype=x.dtype, device=x.device).index_add(0, seg, p.unsqueeze(1) * x)


def _attn_readout_forward(x: torch.Tensor, w: torch.Tensor, b: Optional[torch.Tensor], rp: ReducePlan):
    """Both forward stages, one C call (wsi_attn_readout_fwd).  Returns (out [S, D], gate [rows], stats [S, 2])."""
    (n, D), dev = x.shape, x.device
    out = torch.empty((rp.num_segs, D), dtype=torch.float32, device=dev)
    gate = torch.empty(max(n, 1), dtype=torch.float32, device=dev)[:n]
    stats = torch.empty((rp.num_segs, 2), dtype=torch.float32, device=dev)
    partial = torch.empty(max(rp.num_chunks * (D + 2), 1), dtype=torch.float32, device=dev)
    N.check(N.load().wsi_attn_readout_fwd(N.ptr(x), x.stride(0), D, N.ptr(w), N.ptr(b), N.ptr(rp.chunk_row), rp.num_chunks, N.ptr(rp.seg_chunk),
                                          rp.num_segs, N.ptr(partial), N.ptr(out), N.ptr(gate), N.ptr(stats), N.stream()), "wsi_attn_readout_fwd")
    return out, gate, stats


def _attn_readout_backward(g_out: torch.Tensor, out, gate, stats, x, w, rp: ReducePlan, want_gx: bool):
    """delta, the row pass and the reduction of the chunks' g_w | g_b partials, one C call (wsi_attn_readout_bwd).  ``want_gx`` False: the
    [rows, D] gradient is neither formed nor written (layer 0's input is the feature table).  Returns (g_x or None, g_wb [D + 1])."""
    (n, D), dev = x.shape, x.device
    g_x = torch.empty((n, D), dtype=torch.float32, device=dev) if want_gx else None
    g_wb = torch.empty(D + 1, dtype=torch.float32, device=dev)
    scratch = torch.empty(rp.num_segs + rp.num_chunks * (D + 1) + 1, dtype=torch.float32, device=dev)
    N.check(N.load().wsi_attn_readout_bwd(N.ptr(g_out), N.ptr(out), N.ptr(gate), N.ptr(stats), N.ptr(x), x.stride(0), D, N.ptr(w),
                                          N.ptr(rp.chunk_row), N.ptr(rp.chunk_seg), rp.num_chunks, rp.num_segs, N.ptr(scratch),
                                          N.ptr(g_x), D, N.ptr(g_wb), N.stream()), "wsi_attn_readout_bwd")
    return g_x, g_wb


class _AttentionReadout(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, rp: ReducePlan):
        N.require_cuda(x, weight, bias)
        _bag_rows("attention_readout", rp, x)
        if x.stride(1) != 1:
            x = x.contiguous()
        w = weight.reshape(-1).contiguous()
        out, gate, stats = _attn_readout_forward(x, w, bias, rp)
        ctx.rp = rp
        ctx.weight_shape, ctx.has_bias = weight.shape, bias is not None
        ctx.save_for_backward(x, w, out, gate, stats)
        return out

    @staticmethod
    def backward(ctx, g_out):
        x, w, out, gate, stats = ctx.saved_tensors
        g_x, g_wb = _attn_readout_backward(g_out.contiguous(), out, gate, stats, x, w, ctx.rp, ctx.needs_input_grad[0])
        D = x.shape[1]
        g_w = g_wb[:D].reshape(ctx.weight_shape) if ctx.needs_input_grad[1] else None
        g_b = g_wb[D:].reshape(1) if (ctx.has_bias and ctx.needs_input_grad[2]) else None
        return g_x, g_w, g_b, None


def attention_readout(x: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor], rp: ReducePlan) -> torch.Tensor:
    """dgl's GlobalAttentionPooling with a one-column ``gate_nn`` over the segments of ``rp``, as one autograd node:
    gate = x @ weight^T + bias;  p = softmax of gate over the rows of each segment;  out[s] = sum of p[r] * x[r] -> [num_segs, D].
    ``x`` [rows, D] float32 (a row stride of its own is fine), ``weight`` [1, D] or [D], ``bias`` [1] or None; an empty segment gives 0.
    On the GPU: wsi_attn_readout_fwd / _bwd (D <= 2048), reading only the plan's device tables - a slot's static ones included.  A CPU
    tensor, or any other dtype, takes ``attention_readout_reference``."""
    if x.dim() != 2 or weight.numel() != x.shape[1] or (bias is not None and bias.numel() != 1):
        raise ValueError(f"attention_readout: x {tuple(x.shape)} needs a gate weight of {x.shape[-1]} entries and a bias of one, got "
                         f"{tuple(weight.shape)} and {None if bias is None else tuple(bias.shape)}")
    if not x.is_cuda or x.dtype != torch.float32:
        return attention_readout_reference(x, weight, bias, rp)
    return _AttentionReadout.apply(x, weight, bias, rp)


# ------------------------------------------------------------------------------------------------
# patch dropout of many bags and the fill of a padded bag slot (wsi_bag_dropout_select / wsi_bag_slot_fill: mil.dropout_patches, mil.BagSlot)
# ------------------------------------------------------------------------------------------------
BAG_DESC_WORDS = 8


def bag_descriptors(sources: Sequence[torch.Tensor], counts: Sequence[Tuple[int, int]], draws: Sequence[int], feats: int) -> Tuple[List[int], int]:
    """The descriptor words of wsi_bag_dropout_select / wsi_bag_slot_fill (eight per bag: [src, stride, n, k, m, dst_row, draw, 0]) for the
    bags ``sources`` ([n_i, feats] fp32 device tensors with unit column stride; a row stride of their own is fine) laid one after the other,
    ``counts[i] = (k_i, m_i)``; returns (words, total rows).  Everything is checked here: the kernels trust the table."""
    words: List[int] = []
    row = 0
    for t, (k, m), d in zip(sources, counts, draws):
        if t.dim() != 2 or t.dtype != torch.float32 or t.shape[1] != feats or (t.shape[0] > 0 and feats > 1 and t.stride(1) != 1):
            raise ValueError(f"bag rows: expected [n, {feats}] float32 with unit column stride, got {tuple(t.shape)} {t.dtype} strides {t.stride()}")
        n = t.shape[0]
        if not (0 <= k <= n and 0 <= m <= k):
            raise ValueError(f"bag rows: cannot keep {k} and repeat {m} of {n} rows")
        if n >= 1 << 31:
            raise ValueError("bag rows: a bag of 2^31 rows or more")
        words += [t.data_ptr(), t.stride(0) if n > 1 else feats, n, k, m, row, int(d) & 0xffffffff, 0]
        row += k + m
    return words, row


def bag_dropout_rows(sources: Sequence[torch.Tensor], counts: Sequence[Tuple[int, int]], draws: Sequence[int], key_bits: int = 32):
    """(rows [sum(k + m), feats], sel int32 [sum(k + m)]): the bags ``sources`` after the patch dropout of the draw contract in
    include/wsi_hgnn.h - per bag the k kept rows, then the m repeated ones; ``sel`` = the source row (within its bag) of every output row.
    One upload and two launches whatever the number of bags; no read-back."""
    N.require_cuda(*sources)
    if not sources:
        raise ValueError("bag_dropout_rows: no bag")
    feats, dev = sources[0].shape[1], sources[0].device
    words, total = bag_descriptors(sources, counts, draws, feats)
    rows = torch.empty((total, feats), dtype=torch.float32, device=dev)
    sel = torch.empty(total, dtype=torch.int32, device=dev)
    if total:
        desc = host_to_device(torch.frombuffer(array.array("q", words), dtype=torch.int64), torch.int64, dev)
        lib = N.load()
        N.check(lib.wsi_bag_dropout_select(N.ptr(desc), len(sources), int(key_bits), N.ptr(sel), total, N.stream()), "wsi_bag_dropout_select")
        N.check(lib.wsi_bag_slot_fill(N.ptr(desc), len(sources), N.ptr(sel), N.ptr(rows), feats, feats, total, None, 0, None, None, 0,
                                      N.stream()), "wsi_bag_slot_fill")
    return rows, sel


# ------------------------------------------------------------------------------------------------
# ReMix: the k-means step over many bags and the prototype mixing (wsi_bag_kmeans_step / wsi_remix_*: wsi_hgnn_amd.mil.remix)
# ------------------------------------------------------------------------------------------------
KMEANS_MAX_K = 16
REMIX_OPS = {"keep": N.WSI_REMIX_KEEP, "append": N.WSI_REMIX_APPEND, "interpolate": N.WSI_REMIX_INTERPOLATE, "cov": N.WSI_REMIX_COV}


def bag_kmeans_step(x: torch.Tensor, rp: ReducePlan, centroids: torch.Tensor, normalize: bool = True, update: bool = True):
    """One Lloyd iteration over every bag of the plan (``wsi_bag_kmeans_step``): x [rows, D] fp32 with unit column stride (a row stride is
    taken as it is), centroids [num_segs, K, D], K <= 16.  Returns (labels [rows] int32, counts [num_segs, K] int32, objective [num_segs],
    new_centroids [num_segs, K, D] or None with ``update=False``: assign only).  Nothing is read back."""
    N.require_cuda(x, centroids)
    if x.dim() != 2 or x.dtype != torch.float32 or (x.shape[1] > 1 and x.stride(1) != 1):
        raise ValueError("bag_kmeans_step: an fp32 [rows, D] table with contiguous rows")
    if rp.first_row != 0 or rp.num_rows != x.shape[0]:
        raise ValueError(f"bag_kmeans_step: the plan covers {rp.num_rows} rows, the table has {x.shape[0]}")
    D = x.shape[1]
    if centroids.dim() != 3 or centroids.shape[0] != rp.num_segs or centroids.shape[2] != D or centroids.dtype != torch.float32:
        raise ValueError(f"bag_kmeans_step: centroids [{rp.num_segs}, K, {D}] fp32 expected, got {tuple(centroids.shape)} {centroids.dtype}")
    centroids = centroids.contiguous()
    K, dev = centroids.shape[1], x.device
    labels = torch.empty(max(x.shape[0], 1), dtype=torch.int32, device=dev)[:x.shape[0]]
    counts = torch.empty((rp.num_segs, K), dtype=torch.int32, device=dev)
    objective = torch.empty(rp.num_segs, dtype=torch.float32, device=dev)
    new = torch.empty_like(centroids) if update else None
    partial = torch.empty(max(rp.num_chunks * K * (D + 2), 1), dtype=torch.float32, device=dev)
    ldx = x.stride(0) if x.shape[0] > 1 else D
    with _Timed("bag_kmeans_step"):
        N.check(N.load().wsi_bag_kmeans_step(N.ptr(x), ldx, D, N.ptr(centroids), K, int(bool(normalize)), N.ptr(rp.chunk_row), N.ptr(rp.chunk_seg),
                                             rp.num_chunks, N.ptr(rp.seg_chunk), rp.num_segs, N.ptr(partial), N.ptr(labels), N.ptr(counts),
                                             N.ptr(objective), N.ptr(new), N.stream()), "wsi_bag_kmeans_step")
    return labels, counts, objective, new


def remix_nearest(protos: torch.Tensor, src: torch.Tensor, tgt: torch.Tensor) -> torch.Tensor:
    """[B, K] int32: for every prototype of bag src[b] the closest prototype of bag tgt[b] (first minimum); protos [S, K, D] fp32."""
    N.require_cuda(protos, src, tgt)
    protos = protos.contiguous()
    S, K, D = protos.shape
    src, tgt = src.to(torch.int32).contiguous(), tgt.to(torch.int32).contiguous()
    B = int(src.numel())
    out = torch.empty((B, K), dtype=torch.int32, device=protos.device)
    N.check(N.load().wsi_remix_nearest(N.ptr(protos), S, K, D, N.ptr(src), N.ptr(tgt), B, N.ptr(out), N.stream()), "wsi_remix_nearest")
    return out


def remix_rows(protos: torch.Tensor, shifts: Optional[torch.Tensor], nearest: torch.Tensor, desc: torch.Tensor) -> torch.Tensor:
    """[rows, D]: every output row of a step's mixed bags from the descriptor table desc [rows, 8] int32 (``wsi_remix_rows``; the table is
    built by ``mil.remix.draw_mix``); protos [S, K, D], shifts [S, K, V, D] or None, nearest = ``remix_nearest``'s [B, K]."""
    N.require_cuda(protos, shifts, nearest, desc)
    protos = protos.contiguous()
    S, K, D = protos.shape
    V = 0
    if shifts is not None:
        shifts = shifts.contiguous()
        if shifts.dim() != 4 or shifts.shape[:2] != (S, K) or shifts.shape[3] != D or shifts.dtype != torch.float32:
            raise ValueError(f"remix_rows: shifts [{S}, {K}, V, {D}] fp32 expected, got {tuple(shifts.shape)}")
        V = shifts.shape[2]
    if desc.dim() != 2 or desc.shape[1] != 8 or desc.dtype != torch.int32:
        raise ValueError("remix_rows: desc is an int32 [rows, 8] table")
    desc, nearest = desc.contiguous(), nearest.contiguous()
    rows = desc.shape[0]
    out = torch.empty((rows, D), dtype=torch.float32, device=protos.device)
    N.check(N.load().wsi_remix_rows(N.ptr(protos), N.ptr(shifts), S, K, V, D, N.ptr(nearest), int(nearest.numel()), N.ptr(desc), rows, N.ptr(out),
                                    N.stream()), "wsi_remix_rows")
    return out


def gemm_tn_fp32(groups: Sequence[dict], device) -> None:
    """C = A^T B for every group in exact fp32 whatever ``gemm_precision()`` says (the weight-gradient kernel of ``wsi_gemm_grouped``), at most
    ``WSI_GEMM_MAX_GROUPS`` groups per call.  Group dicts as for ``_gemm``: A [K, M] / lda, B [K, N] / ldb, C [M, N] / ldc."""
    lib = N.load()
    groups = [g for g in groups if g["M"] > 0 and g["N"] > 0]
    for i in range(0, len(groups), N.WSI_GEMM_MAX_GROUPS):
        arr = _group_array(groups[i:i + N.WSI_GEMM_MAX_GROUPS])
        ws_bytes = lib.wsi_gemm_workspace_bytes(N.WSI_GEMM_TN, N.WSI_GEMM_FP32, arr, len(arr))
        ws = torch.empty(max(ws_bytes // 4, 1), dtype=torch.float32, device=device)
        N.check(lib.wsi_gemm_grouped(N.WSI_GEMM_TN, 0, N.WSI_GEMM_FP32, arr, len(arr), N.ptr(ws), ws_bytes, N.stream()), "wsi_gemm_grouped")


# ------------------------------------------------------------------------------------------------
# segment dot (skip-gate gradient)
# ------------------------------------------------------------------------------------------------
def _unit_columns(t: torch.Tensor) -> torch.Tensor:
    """``t`` itself where the kernels can walk it by a row stride alone (adjacent columns, rows a non-negative stride apart), else a copy."""
    if (t.shape[1] == 1 or t.stride(1) == 1) and (t.shape[0] <= 1 or t.stride(0) >= t.shape[1]):
        return t
    return t.contiguous()


def segment_dot_diff(g: torch.Tensor, a: torch.Tensor, b: torch.Tensor, rp: "ReducePlan") -> torch.Tensor:
    """out[s] = sum over rows of segment s and all columns of g * (a - b).  g, a, b: [rows, D] float32 on the GPU, rows >= the plan's last
    row.  A row-strided view (a column slice of a wider table) is read in place; a view whose columns are not adjacent is copied first."""
    N.require_cuda(g, a, b)
    for name, t in (("g", g), ("a", a), ("b", b)):
        if t.dim() != 2 or t.dtype != torch.float32:
            raise ValueError(f"segment_dot_diff: {name} must be a 2-D float32 tensor, got {tuple(t.shape)} {t.dtype}")
        if t.shape != g.shape or t.device != g.device:
            raise ValueError(f"segment_dot_diff: {name} is {tuple(t.shape)} on {t.device}, g is {tuple(g.shape)} on {g.device}")
    if g.shape[1] < 1 or g.shape[0] < rp.first_row + rp.num_rows:
        raise ValueError(f"segment_dot_diff: the plan covers rows [{rp.first_row}, {rp.first_row + rp.num_rows}) but the tensors are {tuple(g.shape)}")
    g, a, b = _unit_columns(g), _unit_columns(a), _unit_columns(b)
    lib = N.load()
    D = g.shape[1]
    out = torch.empty(rp.num_segs, dtype=torch.float32, device=g.device)
    partial = torch.empty(max(rp.num_chunks * ((D + 255) // 256), 1), dtype=torch.float32, device=g.device)
    N.check(lib.wsi_segment_dot_diff(N.ptr(g), g.stride(0), N.ptr(a), a.stride(0), N.ptr(b), b.stride(0), D,
                                     N.ptr(rp.chunk_row), rp.num_chunks, N.ptr(rp.seg_chunk), rp.num_segs,
                                     N.ptr(partial), N.ptr(out), N.stream()), "wsi_segment_dot_diff")
    return out


# ------------------------------------------------------------------------------------------------
# counter-based dropout (WSI_EPI_DROPOUT / wsi_dropout_apply; the hash is specified in include/wsi_hgnn.h)
# ------------------------------------------------------------------------------------------------
class CounterDropout:
    """One draw of ``nn.Dropout(p)`` over a [rows, cols] tensor as a FUNCTION of (seed, row, col) instead of a mask tensor: the projection's
    epilogue applies it while it writes the tensor, the backward regenerates it (``dropout_apply``) - nothing is generated, stored or read back
    (models/HEATNet4.py:135 ``self.drop(self.a_linears[...](t))``; two passes over [N, D] for torch's mask, one read in the epilogue and one in the
    backward go away).  ``p`` is quantised to 1/65536; kept values are scaled by 1 / (1 - p) exactly as nn.Dropout scales them."""

    def __init__(self, p: float, seed: int, seed_base: Optional[torch.Tensor] = None):
        """``seed_base``: an optional one-element int32 DEVICE tensor whose value is added to ``seed`` (mod 2^32) when the kernels run - see
        ``dropout_seed_base``: what lets a step captured into a hipGraph draw new masks at every replay."""
        if not 0.0 <= p < 1.0:
            raise ValueError("dropout probability must be in [0, 1)")
        self.p = float(p)
        self.seed = int(seed) & 0xffffffff
        self.seed_base = seed_base
        self.threshold = int(round(self.p * 65536.0))
        self.scale = 1.0 / (1.0 - self.p)

    def effective_seed(self) -> int:
        """seed + the CURRENT value of the device word (a synchronising read: tests only)."""
        return (self.seed + (int(self.seed_base.item()) if self.seed_base is not None else 0)) & 0xffffffff

    def group_fields(self, row0: int, cols: int, col0: int = 0) -> dict:
        return dict(drop_seed=self.seed, drop_threshold=self.threshold, drop_scale=self.scale, drop_row0=int(row0), drop_cols=int(cols), drop_col0=int(col0),
                    drop_seed_base=N.ptr(self.seed_base))


def next_dropout_seed() -> int:
    """A fresh 32-bit seed per dropout draw, taken from torch's default CPU generator (a host-side draw: no device round trip): the sequence of
    masks follows ``torch.manual_seed`` exactly as nn.Dropout's does - re-seeding replays it."""
    return int(torch.empty((), dtype=torch.int64).random_(0, 1 << 32).item())


_SEED_BASE: dict = {}           # device index -> the one-element int32 tensor every CounterDropout created meanwhile adds to its seed
SEED_STRIDE = -1640531527       # 0x9E3779B9 as int32: what one step advances the word by


@contextlib.contextmanager
def dropout_seed_base(base: Optional[torch.Tensor]):
    """While active, every dropout draw on ``base``'s device is ``CounterDropout(p, host seed, seed_base=base)``: its mask is a function of
    host seed + the value ``base`` holds WHEN THE KERNEL RUNS.  ``trainer.CapturedStep`` records a step under it and lets the recorded step advance
    ``base`` (``advance_dropout_seed_base``): the host seeds are frozen into the graph, the word is not - every replay draws new masks, forward and
    backward of one replay the same ones."""
    if base is None:
        yield
        return
    if not (base.is_cuda and base.dtype == torch.int32 and base.numel() == 1):
        raise ValueError("dropout_seed_base: a one-element int32 CUDA tensor")
    key = base.device.index
    prev = _SEED_BASE.get(key)
    _SEED_BASE[key] = base
    try:
        yield
    finally:
        if prev is None:
            _SEED_BASE.pop(key, None)
        else:
            _SEED_BASE[key] = prev


def current_dropout_seed_base(device) -> Optional[torch.Tensor]:
    device = torch.device(device)
    return _SEED_BASE.get(device.index if device.index is not None else torch.cuda.current_device()) if device.type == "cuda" else None


def advance_dropout_seed_base(base: torch.Tensor) -> None:
    """One step further (an in-place device add: part of the recorded step)."""
    base.add_(SEED_STRIDE)


def _mul32(a: torch.Tensor, b: int) -> torch.Tensor:
    """(a * b) mod 2^32 for int64 tensors holding 32-bit values, without overflowing int64."""
    lo = (a & 0xffff) * b
    hi = (((a >> 16) * b) & 0xffff) << 16
    return (lo + hi) & 0xffffffff


def dropout_keep_mask(drop: CounterDropout, rows: int, cols: int, device="cpu", row0: int = 0) -> torch.Tensor:
    """The boolean keep mask of ``drop`` for rows [row0, row0 + rows) of a tensor with ``cols`` columns, replayed with integer tensor arithmetic from
    the specification in include/wsi_hgnn.h (independent of the kernels: the tests compare them with it)."""
    r = torch.arange(row0, row0 + rows, dtype=torch.int64, device=device).view(-1, 1)
    c = torch.arange(cols, dtype=torch.int64, device=device).view(1, -1)
    pairs = (cols + 1) // 2
    idx = (_mul32(r & 0xffffffff, pairs) + (c >> 1)) & 0xffffffff
    h = (_mul32(idx, 0x9E3779B1) + drop.effective_seed()) & 0xffffffff
    h = h ^ (h >> 16)
    h = _mul32(h, 0x85EBCA6B)
    h = h ^ (h >> 13)
    h = _mul32(h, 0xC2B2AE35)
    h = h ^ (h >> 16)
    bits = torch.where((c & 1) == 1, h >> 16, h & 0xffff)
    return bits >= drop.threshold


def dropout_apply(x: torch.Tensor, drop: CounterDropout, row0: int = 0) -> torch.Tensor:
    """x * mask * 1/(1-p) with the regenerated mask of ``drop`` (``wsi_dropout_apply``); x: [rows, cols] whose row 0 is row ``row0`` of the masked tensor."""
    N.require_cuda(x)
    x = x.contiguous()
    out = torch.empty_like(x)
    N.check(N.load().wsi_dropout_apply(N.ptr(x), x.stride(0), N.ptr(out), out.stride(0), x.shape[0], x.shape[1], int(row0), x.shape[1], 0,
                                       drop.seed, N.ptr(drop.seed_base), drop.threshold, drop.scale, N.stream()), "wsi_dropout_apply")
    return out


# ------------------------------------------------------------------------------------------------
# fused HEAT layer: K|Q|V GEMM -> relation attention -> output GEMM with the sigmoid-gated skip in its
# epilogue; hand-written backward so no elementwise pass, gather or gradient accumulation is left to
# eager PyTorch (models/HEATNet4.py:85-138 as ONE autograd node).
# ------------------------------------------------------------------------------------------------
def _value_collapse_applies(hctx, prp, n: int, D: int, H: int) -> bool:
    """The last layer's V never needs forming (wsi_attn_pool_t): fast attention kernels, <= 8 node types, HEAT-style source rows, and the
    readout plan numbered type-major (segment = type * graphs + graph) over exactly the layer's node-type row ranges."""
    T = len(hctx.rows)
    bseg = prp.num_segs // max(T, 1)
    return (_COLLAPSE_V["enabled"] and float(n) * D * D >= _COLLAPSE_V["min_work"]
            and D in (128, 256, 512) and H in (1, 2, 4, 8, 16) and 1 <= T <= 8 and hctx.plan.num_src_rows == n
            and prp.num_rows == n and prp.num_segs == T * bseg
            and prp.segments_of(hctx.rows) == [(i * bseg, (i + 1) * bseg) for i in range(T)])


def _edge_segments(plan) -> torch.Tensor:
    """[E] int32: the softmax segment (row of ``lse``) of every CSR edge, expanded on the device from ``rowptr`` once per plan."""
    es = plan.__dict__.get("_edge_seg")
    if es is None:
        counts = (plan.rowptr[1:] - plan.rowptr[:-1]).to(torch.int64)
        es = torch.repeat_interleave(torch.arange(plan.num_segs, dtype=torch.int32, device=counts.device), counts, output_size=plan.num_edges)
        plan.__dict__["_edge_seg"] = es
    return es


def _segment_dst(plan) -> torch.Tensor:
    """[num softmax segments] int32: the destination node of every softmax segment, expanded on the device from ``node_seg`` once per plan."""
    sd = plan.__dict__.get("_seg_dst")
    if sd is None:
        counts = (plan.node_seg[1:] - plan.node_seg[:-1]).to(torch.int64)
        sd = torch.repeat_interleave(torch.arange(counts.shape[0], dtype=torch.int32, device=counts.device), counts, output_size=plan.num_segs)
        plan.__dict__["_seg_dst"] = sd
    return sd


def _pooled_factors(h, ctab, prp, T: int, H: int, with_mean: bool = False):
    """hp[seg, h, tau, :] = sum over the source rows u of type tau in seg's graph of ctab[u, type(seg), h] * h[u, :]  and  csum[tau, seg, h] = the same
    sum of the coefficients alone - one weighted-sums pass over the (source type, graph) segments whose second stage writes both where their
    consumers read them (``wsi_pool_factors``: two launches)."""
    n, D = h.shape
    S, J = prp.num_segs, T * H
    hp = torch.empty((S, H, T, D), dtype=torch.float32, device=h.device)
    csum = torch.empty((T, S, H), dtype=torch.float32, device=h.device)
    partial = torch.empty(max(prp.num_chunks * (J + 1) * (D + 1), 1), dtype=torch.float32, device=h.device)
    h_mean = torch.empty((S, D), dtype=torch.float32, device=h.device) if with_mean else None      # (the same pass: one more weight column of ones)
    N.check(N.load().wsi_pool_factors(N.ptr(h), D, D, N.ptr(ctab), J, T, H, S // T, N.ptr(prp.chunk_row), prp.num_chunks, N.ptr(prp.seg_chunk),
                                      N.ptr(partial), N.ptr(hp), N.ptr(csum), N.ptr(h_mean), N.stream()), "wsi_pool_factors")
    return (hp, csum, h_mean) if with_mean else (hp, csum)


def _ptr_array(tensors):
    """HOST array of device pointers (``const float* const*`` arguments of the wsi_pool_* entry points)."""
    return (ctypes.c_void_p * len(tensors))(*[None if t is None else t.data_ptr() for t in tensors])


def _gate_table(hctx, skip, name: str, segs=None, num_segs: int = 0) -> torch.Tensor:
    """The small host-built tables that map graph node types and readout segments to model gates (indices into ``skip``), uploaded once per layer
    context and readout plan (``hctx.cache[(name, segs, num_segs)]``).  With gate(i) = hctx.nid[i] for a node type i the layer projects and -1
    for one it passes through, and gate(s) = that of the type whose run of segments ``segs[i]`` holds s:
      "type_gate" [T] int32 = gate(i)                          "seg_gate" [num_segs] int32 = gate(s)
      "gate_of_row_type" [T, G] fp32 = [gate(i) == g]          "gate_of_seg" [G, num_segs] fp32 = [gate(s) == g]"""
    key = (name, None if segs is None else tuple(segs), num_segs)
    hit = hctx.cache.get(key)
    if hit is None:
        T, G = len(hctx.rows), skip.shape[0]
        tg = [hctx.nid[i] if hctx.incoming[i] else -1 for i in range(T)]
        sg = [-1] * num_segs
        for i, (s0, s1) in enumerate(segs or ()):
            sg[s0:s1] = [tg[i]] * (s1 - s0)
        rows, dtype = {"type_gate": (tg, torch.int32),
                       "seg_gate": (sg or [-1], torch.int32),
                       "gate_of_seg": ([[float(x == g_) for x in sg] for g_ in range(G)], torch.float32),
                       "gate_of_row_type": ([[float(x == g_) for g_ in range(G)] for x in tg], torch.float32)}[name]
        hit = hctx.cache[key] = host_to_device(rows, dtype, skip.device)
    return hit


def _gate_ptr(skip, hctx, i: int):
    """Pointer to the skip-gate logit of graph node type i (the ``gate`` field of a GEMM group)."""
    return N.ptr(skip, 4 * hctx.nid[i])


# What _HeatLayerFused.forward hands its backward, every field set on every path.  Besides tensors: pool = (ReducePlan, WSI_RED_SUM | WSI_RED_MEAN)
# when the layer returned its readout, None when its output;  no_v: readout-fused and V never formed (kqv is K | Q; ctab, hp, csum are saved);
# dropout: None, the CounterDropout (regenerated in the backward) or "mask" (the saved keep-mask tensor);  h_cols / t_cols: ColStats or None.
_HeatState = namedtuple("_HeatState", "hctx H pool no_v dropout h_cols t_cols background_dw")
# The saved tensors, None where the path does not form one: t, out at full depth;  t_mean, h_mean, z_mean (segment means of t, h and the
# never-formed output) readout-fused;  ctab, hp, csum (``_pooled_factors``) without V;  mask: the dropout keep mask that came as a tensor.
_HeatSaved = namedtuple("_HeatSaved", "h kqv score lse skip ew eb sim_csr t out t_mean h_mean z_mean ctab hp csum mask params", defaults=(None,) * 10)


def _heat_save(ctx, sv: _HeatSaved) -> None:
    ctx.save_for_backward(*sv[:-1], *sv.params)


def _heat_saved(ctx) -> _HeatSaved:
    k = len(_HeatSaved._fields) - 1
    return _HeatSaved(*ctx.saved_tensors[:k], params=ctx.saved_tensors[k:])


# ---- stages of _HeatLayerFused.forward ----
def _heat_project(h, h_max, hctx, P, nproj: int, v_stats: bool):
    """One grouped NT GEMM with the bias epilogue: kqv [n, nproj * D] = K | Q (| V) in column blocks 0, 1 (, 2), every node type's rows through
    its own weights.  Returns (kqv, t_cols): with ``v_stats`` the V groups leave their column maxima, which bound t's (a row of t is a convex
    combination of V rows: a few binades loose at most, which the 17-binade full-precision window of the scaled-fp16 split absorbs)."""
    n, D = h.shape
    dev, ldp = h.device, nproj * D
    v_cols = ColStats.allocate(hctx.rows, D, dev, sums=False) if v_stats else None
    kqv = torch.empty((n, ldp), dtype=torch.float32, device=dev)
    groups = []
    for i, (r0, r1) in enumerate(hctx.rows):
        for j in range(nproj):
            groups.append(dict(A=N.ptr(h, r0 * D * 4), lda=D, B=N.ptr(P[i][j]), ldb=D, Bw=[P[i][j]],
                               C=N.ptr(kqv, (r0 * ldp + j * D) * 4), ldc=ldp, bias=N.ptr(P[i][4 + j]),
                               M=r1 - r0, N=D, K=D, **_scale_in(h_max, r0),
                               **(v_cols.produce(r0, r1, 0) if (v_cols is not None and j == 2) else {})))
    if not _gemm(N.WSI_GEMM_NT, N.WSI_EPI_BIAS, groups, dev) or v_cols is None:
        return kqv, None
    # a row of t mixes V rows of EVERY source type that reaches its node: the bound of each of t's row ranges is the maximum over ALL parts
    return kqv, ColStats(v_cols.bits, None, {r: (0, v_cols.bits.shape[0]) for r in hctx.rows if r[1] > r[0]})


def _heat_attend(kqv, t_max, hctx, H: int, edge):
    """Full attention, one launch (wsi_heat_attn_fwd): (t [n, D], score [E, H], lse [softmax segments, H]); ``t_max`` receives t's row scales.
    ``edge`` = (e_weight, e_bias, sim in CSR order), here and below."""
    plan, (ew, eb, sim_csr) = hctx.plan, edge
    n, D, dev = kqv.shape[0], kqv.shape[1] // 3, kqv.device
    score = torch.empty((max(plan.num_edges, 1), H), dtype=torch.float32, device=dev)
    lse = torch.empty((max(plan.num_segs, 1), H), dtype=torch.float32, device=dev)
    t = torch.empty((n, D), dtype=torch.float32, device=dev)
    with _Timed("heat_attn"), _Timed("heat_attn_fwd_full"):
        N.check(N.load().wsi_heat_attn_fwd(
            N.ptr(kqv, D * 4), 3 * D, N.ptr(kqv), 3 * D, N.ptr(kqv, 2 * D * 4), 3 * D, n, D, H,
            N.ptr(plan.node_seg), N.ptr(plan.rowptr), N.ptr(plan.src), N.ptr(sim_csr), N.ptr(plan.order_dst), plan.num_heavy, _attn_flags(plan),
            N.ptr(ew), N.ptr(eb), N.ptr(t), D, N.ptr(score), N.ptr(lse), N.ptr(t_max), N.context(), N.stream()), "wsi_heat_attn_fwd")
    return t, score, lse


def _heat_attend_pooled(h, kqv, hctx, H: int, edge, prp, P):
    """Readout-fused without V: the segment means of t and h without forming V or t.  The scores and softmax statistics alone
    (wsi_heat_attn_scores_fwd); per source node the coefficients ctab [n, T, H] with which its value row enters each (destination type, graph)
    segment sum of t (wsi_heat_pool_coeff); the weighted sums of h (``_pooled_factors``, which takes mean_seg(h) in the same pass); their
    products with W_v per (head, source type) (one grouped NT GEMM into tpart[tau]); the sum over tau + the value-bias term + the 1 / count
    scaling (wsi_pool_tmean):   sum_seg(t)[:, head hh] = sum_tau ( hp[:, hh, tau, :] (W_v^tau rows of head hh)^T + csum[tau, :, hh] b_v^tau (head hh) ).
    Returns (score, lse, ctab, hp, csum, h_mean, t_mean)."""
    plan, (ew, eb, sim_csr) = hctx.plan, edge
    (n, D), dev, T, S, dk = h.shape, h.device, len(hctx.rows), prp.num_segs, h.shape[1] // H
    lib = N.load()
    score = torch.empty((max(plan.num_edges, 1), H), dtype=torch.float32, device=dev)
    lse = torch.empty((max(plan.num_segs, 1), H), dtype=torch.float32, device=dev)
    with _Timed("heat_attn"), _Timed("heat_attn_fwd_pooled"):
        N.check(lib.wsi_heat_attn_scores_fwd(
            N.ptr(kqv, D * 4), 2 * D, N.ptr(kqv), 2 * D, n, D, H,
            N.ptr(plan.node_seg), N.ptr(plan.rowptr), N.ptr(plan.src), N.ptr(sim_csr), N.ptr(plan.order_dst), plan.num_heavy, _attn_flags(plan),
            N.ptr(ew), N.ptr(eb), N.ptr(score), N.ptr(lse), N.context(), N.stream()), "wsi_heat_attn_scores_fwd")
        ctab = torch.empty((n, T, H), dtype=torch.float32, device=dev)
        N.check(lib.wsi_heat_pool_coeff(N.ptr(score), N.ptr(lse), N.ptr(_edge_segments(plan)), N.ptr(plan.colptr), N.ptr(plan.csc_eid),
                                        N.ptr(plan.csc_dst), N.ptr(plan.inv_rd), N.ptr(prp.row_segment()), prp.num_segs // T, T, H, n,
                                        N.ptr(ctab), N.stream()), "wsi_heat_pool_coeff")
    hp, csum, h_mean = _pooled_factors(h, ctab, prp, T, H, with_mean=True)
    tpart = torch.empty((T, S, D), dtype=torch.float32, device=dev)
    groups = [dict(A=N.ptr(hp, (hh * T + tau) * D * 4), lda=H * T * D, B=N.ptr(P[tau][2], hh * dk * D * 4), ldb=D,
                   C=N.ptr(tpart, (tau * S * D + hh * dk) * 4), ldc=D, M=S, N=dk, K=D) for tau in range(T) for hh in range(H)]
    _gemm(N.WSI_GEMM_NT, 0, groups, dev)
    t_mean = torch.empty((S, D), dtype=torch.float32, device=dev)
    N.check(lib.wsi_pool_tmean(N.ptr(tpart), T, S, D, H, N.ptr(csum), _ptr_array([P[tau][6] for tau in range(T)]),
                               N.ptr(prp.inv_counts()), N.ptr(t_mean), N.stream()), "wsi_pool_tmean")
    return score, lse, ctab, hp, csum, h_mean, t_mean


def _heat_output_means(t_mean, h_mean, hctx, P, skip, pool):
    """Readout-fused output stage, one grouped NT GEMM with the gated-skip epilogue on the segment means: z_mean = s (t_mean Wa^T + ba) +
    (1 - s) h_mean (mean_seg(h) for a type the layer passes through, models/HEATNet4.py:129-133); then the readout.  Returns (z_mean, pooled)."""
    prp, pop = pool
    D, segs = h_mean.shape[1], prp.segments_of(hctx.rows)
    z_mean = torch.empty_like(h_mean) if all(hctx.incoming) else h_mean.clone()
    groups = []
    for i in hctx.a_types:
        s0, s1 = segs[i]
        groups.append(dict(A=N.ptr(t_mean, s0 * D * 4), lda=D, B=N.ptr(P[i][3]), ldb=D, C=N.ptr(z_mean, s0 * D * 4), ldc=D,
                           bias=N.ptr(P[i][7]), R=N.ptr(h_mean, s0 * D * 4), ldr=D, gate=_gate_ptr(skip, hctx, i),
                           M=s1 - s0, N=D, K=D))
    _gemm(N.WSI_GEMM_NT, N.WSI_EPI_GATED_SKIP, groups, h_mean.device)
    # an empty segment reads 0 (not s * ba): the readout kernels' convention, dgl.readout semantics
    pooled = z_mean * prp.counts() if pop == N.WSI_RED_SUM else (z_mean * prp.nonempty() if prp.has_empty() else z_mean)
    return z_mean, pooled


def _heat_output_rows(h, t, scales, hctx, P, skip, dropout):
    """Full-depth output stage, one grouped NT GEMM with the gated-skip epilogue (and the dropout draw or mask in it): out = s * drop(t Wa^T + ba)
    + (1 - s) * h (models/HEATNet4.py:128-135); then a row copy per node type that no relation enters (:129-133).  ``scales`` = (h's, t's row
    scales); ``out`` leaves with its own row scales and column statistics attached for the next layer.  Returns out."""
    n, D = h.shape
    dev, (h_max, t_max) = h.device, scales
    counter = dropout if isinstance(dropout, CounterDropout) else None
    mask = dropout if counter is None else None
    # every node type gets the projection: its epilogue writes all slots of all rows
    out_max = _new_row_scale(n, N.gemm_absmax_parts(D), dev, D, zero=not all(hctx.incoming))
    out = torch.empty((n, D), dtype=torch.float32, device=dev)
    out_cols = ColStats.allocate([hctx.rows[i] for i in hctx.a_types], D, dev, sums=False) if want_col_stats(n, D, D) else None
    groups = []
    for i in hctx.a_types:
        r0, r1 = hctx.rows[i]
        groups.append(dict(A=N.ptr(t, r0 * D * 4), lda=D, B=N.ptr(P[i][3]), ldb=D, Bw=[P[i][3]], C=N.ptr(out, r0 * D * 4), ldc=D,
                           bias=N.ptr(P[i][7]), R=N.ptr(h, r0 * D * 4), ldr=D, gate=_gate_ptr(skip, hctx, i),
                           Mm=N.ptr(mask, r0 * D * 4) if mask is not None else None, ldm=D,
                           M=r1 - r0, N=D, K=D, **_scale_in(t_max, r0), **_scale_out(out_max, r0),
                           **(counter.group_fields(r0, D) if counter is not None else {}),
                           **(out_cols.produce(r0, r1, 0) if out_cols is not None else {})))
    drop_epi = N.WSI_EPI_DROPOUT if counter is not None else (N.WSI_EPI_MUL_M if mask is not None else 0)
    if not _gemm(N.WSI_GEMM_NT, N.WSI_EPI_GATED_SKIP | drop_epi, groups, dev):
        out_cols = None
    for i, (r0, r1) in enumerate(hctx.rows):
        if not hctx.incoming[i]:
            out[r0:r1] = h[r0:r1]
            if out_max is not None:
                if h_max is not None and h_max.shape[1] <= out_max.shape[1]:
                    out_max[r0:r1, :h_max.shape[1]] = h_max[r0:r1]
                else:
                    out_max = None                      # (scales of those rows unknown: the consumer makes its own pass)
    if out_max is not None:
        attach_row_scales(out, out_max)
    attach_col_stats(out, out_cols)                    # (after the pass-through copies: they move the version; those row ranges have no entry)
    return out


# ---- stages of _HeatLayerFused.backward ----
def _heat_row_gradient(g_out, hctx, n: int):
    """Full-depth intake.  The layer under a sum / mean readout receives a gradient of ONE distinct row per (graph, node type), and the readout's
    backward says so on the very tensor it hands down (``SegmentBroadcast``).  Returns (g_out contiguous, bc, segs, annotated): the broadcast
    and each node type's run of its segments - None, None without an annotation whose plan respects the node types; ``annotated``: there was one."""
    g_out = g_out.contiguous()
    bc = _annotation(g_out, "_wsi_broadcast") if _LOW_RANK["enabled"] else None
    if bc is None:
        return g_out, None, None, False
    EXCHANGE_STATS["broadcast_hits"] += 1
    segs = bc.rp.segments_of(hctx.rows) if bc.rp.num_rows == n else None
    return g_out, (bc if segs is not None else None), segs, True


def _heat_pooled_gradient(g_pool, sv: _HeatSaved, st: _HeatState):
    """Readout-fused intake: the gradient arrives as S rows, one per segment of the readout.  Returns (bc, pre): the factors the low-rank
    stages work with (row gradient and row-summed gradient per segment) and, up to 8192 segments, pre = (g_skip, omg [T] = 1 - sigmoid(skip)
    per node type, 1 where the layer passes h through) from the same single launch (wsi_pool_bwd_prep: the two scalings, the segment dots
    against mean(out) - mean(h), the gate map).  Above that the factors are tensor operations and pre is None."""
    prp, pop = st.pool
    g_pool = g_pool.contiguous()
    if prp.num_segs > 8192:
        return SegmentBroadcast.from_pooled_gradient(g_pool, prp, pop, sv.z_mean), None
    T, skip = len(st.hctx.rows), sv.skip
    seg_gate = _gate_table(st.hctx, skip, "seg_gate", prp.segments_of(st.hctx.rows), prp.num_segs)
    type_gate = _gate_table(st.hctx, skip, "type_gate")
    g_row, g_sum = torch.empty_like(g_pool), torch.empty_like(g_pool)
    pre = (torch.empty_like(skip), torch.empty(T, dtype=torch.float32, device=skip.device))
    N.check(N.load().wsi_pool_bwd_prep(N.ptr(g_pool), prp.num_segs, g_pool.shape[1], pop, N.ptr(prp.counts()), N.ptr(sv.z_mean), N.ptr(sv.h_mean),
                                       N.ptr(seg_gate), N.ptr(skip), skip.shape[0], N.ptr(type_gate), T, N.ptr(g_row), N.ptr(g_sum),
                                       N.ptr(pre[0]), N.ptr(pre[1]), N.stream()), "wsi_pool_bwd_prep")
    return SegmentBroadcast.from_parts(prp, g_row, g_sum, sv.z_mean), pre


def _heat_broadcast_rows(bc, n: int, D: int):
    """Readout-fused with V kept: the [n, D] gradient of the never-formed output for the residual term of the K|Q|V dX epilogue, one launch."""
    prp = bc.rp
    g_out = torch.empty((n, D), dtype=torch.float32, device=bc.g_row.device)
    N.check(N.load().wsi_segment_reduce_bwd(N.ptr(bc.g_row), D, D, N.WSI_RED_SUM, N.ptr(prp.chunk_row), N.ptr(prp.chunk_seg),
                                            prp.num_chunks, N.ptr(prp.seg_chunk), prp.num_segs, None,
                                            N.ptr(g_out), D, N.stream()), "wsi_segment_reduce_bwd")
    return g_out


def _heat_gate_launch(g_out, sv: _HeatSaved, hctx, stream_ptr, before_launch=None):
    """The skip-gate gradient from the rows, two launches on ``stream_ptr`` (wsi_gate_grad): the per-type dots sum_rows g_out (out - h), then the
    gate map and the sigmoid factor - a streaming pass over three [n, D] tensors.  Everything the launch reads that is produced on the CALLER's
    stream - the gate table (an asynchronous upload on a cache miss: the first backward of every new graph context) and the buffers (the
    caching allocator hands out blocks whose last use is ordered on that stream) - exists before ``before_launch`` (the side stream's wait
    for the caller's stream) runs.  Returns (g_skip, the scratch it must outlive)."""
    T, D, rp = len(hctx.rows), sv.h.shape[1], hctx.type_rplan()
    seg_gate = _gate_table(hctx, sv.skip, "seg_gate", [(i, i + 1) for i in range(T)], T)
    g_skip = torch.empty_like(sv.skip)
    partial = torch.empty(max(rp.num_chunks * ((D + 255) // 256), 1), dtype=torch.float32, device=sv.h.device)
    if before_launch is not None:
        before_launch()
    N.check(N.load().wsi_gate_grad(N.ptr(g_out), g_out.stride(0), N.ptr(sv.out), sv.out.stride(0), N.ptr(sv.h), sv.h.stride(0), D,
                                   N.ptr(rp.chunk_row), rp.num_chunks, N.ptr(rp.seg_chunk), rp.num_segs, N.ptr(seg_gate), N.ptr(sv.skip),
                                   sv.skip.shape[0], N.ptr(partial), N.ptr(g_skip), stream_ptr), "wsi_gate_grad")
    return g_skip, partial


def _heat_early_gate(g_out, sv: _HeatSaved, hctx):
    """``_heat_gate_launch`` on the statistics stream, beside the matrix-bound output-projection gradient that follows: the pass is
    bandwidth-bound and nobody reads g_skip before the backward returns.  Returns (g_skip, the event the backward joins on)."""
    dev = sv.h.device
    side = side_stream(dev, "stats")
    g_skip, partial = _heat_gate_launch(g_out, sv, hctx, ctypes.c_void_p(side.cuda_stream), lambda: side.wait_stream(torch.cuda.current_stream(dev)))
    ev = torch.cuda.Event()
    ev.record(side)
    for t_ in (g_out, sv.out, sv.h, g_skip, partial, sv.skip):
        t_.record_stream(side)
    return g_skip, ev


def _heat_out_proj_low_rank(bc, segs, sv: _HeatSaved, hctx, P, grads):
    """Output-projection gradients from the S distinct gradient rows, in one paired launch of small GEMMs (else an NN and a TN one):
        g_t[row] = s * g_row[seg] Wa : S rows through the projection (the attention backward reads them through row -> segment);
        gWa = s * sum_seg g_sum[seg] (x) mean_seg(t)  (= s * g_out^T t with the rows of a segment summed first);  gba = s * sum_seg g_sum[seg].
    A full-depth layer takes mean_seg(t) first (wsi_segment_reduce_fwd).  Fills ``grads``; returns (gt_seg [S, D], row -> segment [n])."""
    S, D, dev, T = bc.rp.num_segs, sv.h.shape[1], sv.h.device, len(hctx.rows)
    gt_seg = (torch.empty if len(hctx.a_types) == T else torch.zeros)((S, D), dtype=torch.float32, device=dev)
    t_mean = sv.t_mean if sv.t_mean is not None else _segment_reduce_raw(sv.t, bc.rp, N.WSI_RED_MEAN)[0]
    groups, wgroups = [], []
    for i in hctx.a_types:
        s0, s1 = segs[i]
        groups.append(dict(A=N.ptr(bc.g_row, s0 * D * 4), lda=D, B=N.ptr(P[i][3]), ldb=D, C=N.ptr(gt_seg, s0 * D * 4), ldc=D,
                           gate=_gate_ptr(sv.skip, hctx, i), M=s1 - s0, N=D, K=D))
        gw, gb = torch.empty_like(P[i][3]), torch.empty_like(P[i][7])
        grads[8 * i + 3], grads[8 * i + 7] = gw, gb
        wgroups.append(dict(A=N.ptr(bc.g_sum, s0 * D * 4), lda=D, B=N.ptr(t_mean, s0 * D * 4), ldb=D, C=N.ptr(gw), ldc=D,
                            gate=_gate_ptr(sv.skip, hctx, i), colsum_out=N.ptr(gb), M=D, N=D, K=s1 - s0))
    if not _gemm_small_pair(groups, N.WSI_EPI_SCALE_GATE, wgroups, N.WSI_EPI_SCALE_GATE, dev):
        _gemm(N.WSI_GEMM_NN, N.WSI_EPI_SCALE_GATE, groups, dev)
        _gemm(N.WSI_GEMM_TN, N.WSI_EPI_SCALE_GATE, wgroups, dev)
    return gt_seg, bc.rp.row_segment()


def _heat_out_proj_rows(g_y, sv: _HeatSaved, st: _HeatState, P, grads):
    """Output-projection gradients at full depth: g_t = s * g_y Wa (one grouped NN GEMM), then gWa = s * g_y^T t and gba = s * colsum(g_y)
    (one grouped TN GEMM) - which has the whole attention backward of this layer in front of it: queued for the background.
    Fills ``grads``; returns g_t [n, D]."""
    hctx, (n, D), dev, t, skip = st.hctx, sv.h.shape, sv.h.device, sv.t, sv.skip
    g_t = torch.empty((n, D), dtype=torch.float32, device=dev)
    gy_max = row_scales_of(g_y)                # fp16x3 row scales: left by the layer above (its dX epilogue), if any
    gy_cols, t_cols = col_stats_of(g_y), st.t_cols      # column statistics for the weight gradient, likewise
    groups, wgroups = [], []
    for i in hctx.a_types:
        r0, r1 = hctx.rows[i]
        groups.append(dict(A=N.ptr(g_y, r0 * D * 4), lda=D, B=N.ptr(P[i][3]), ldb=D, Bw=[P[i][3]], C=N.ptr(g_t, r0 * D * 4), ldc=D,
                           gate=_gate_ptr(skip, hctx, i), M=r1 - r0, N=D, K=D, **_scale_in(gy_max, r0)))
        gw, gb = torch.empty_like(P[i][3]), torch.empty_like(P[i][7])
        grads[8 * i + 3], grads[8 * i + 7] = gw, gb
        wgroups.append(dict(A=N.ptr(g_y, r0 * D * 4), lda=D, B=N.ptr(t, r0 * D * 4), ldb=D, C=N.ptr(gw), ldc=D,
                            gate=_gate_ptr(skip, hctx, i), colsum_out=N.ptr(gb), M=D, N=D, K=r1 - r0,
                            **(gy_cols.consume("a", r0, r1, 0, want_sums=True) if gy_cols is not None else {}),
                            **(t_cols.consume("b", r0, r1, 0) if t_cols is not None else {})))
    _gemm(N.WSI_GEMM_NN, N.WSI_EPI_SCALE_GATE, groups, dev)
    wr = [P[i][k] for i in hctx.a_types for k in (3, 7)]
    keep = [g_y, t, skip] + [c_.bits for c_ in (gy_cols, t_cols) if c_ is not None] + [c_.sums for c_ in (gy_cols,) if c_ is not None and c_.sums is not None]
    outs = [(P[i][k], grads[8 * i + k]) for i in hctx.a_types for k in (3, 7)]
    if not (_background_safe(wr) and _gemm_tn_background(N.WSI_EPI_SCALE_GATE, wgroups, dev, keep, wr, outs=outs)):
        _gemm(N.WSI_GEMM_TN, N.WSI_EPI_SCALE_GATE, wgroups, dev)
    return g_t


def _heat_skip_gate_grad(g_out, sv: _HeatSaved, hctx, bc, segs, pre, early):
    """d loss / d skip[g] = (1 - sigmoid(skip[g])) * sum over the graph node types i mapped to g of dots[i],
    dots[i] = sum over the rows of type i of g_out * (out - h).  Four sources, the first that applies:
      1. ``pre``: a readout-fused layer of up to 8192 segments got it from wsi_pool_bwd_prep with the scalings of the gradient - no launch here;
      2. ``bc`` for the layer's own output (a readout-fused layer never formed it; at full depth the annotation must be of this very ``out``):
         sum_rows g_out * (out - h) = sum_seg g_sum[seg] . (mean_seg(out) - mean_seg(h)), and the readout already holds mean_seg(out) -
         S-row tensor operations (after wsi_segment_reduce_fwd for mean_seg(h) at full depth) instead of a pass over three [n, D] tensors;
      3. ``early``: at full depth and large n the row pass was launched on the statistics stream before the output-projection gradients;
      4. otherwise that row pass now, on the caller's stream (``_heat_gate_launch``)."""
    if pre is not None:
        return pre[0]
    if bc is not None and (sv.out is None or (bc.x_ptr == sv.out.data_ptr() and bc.x_version == sv.out._version)):
        h_mean = sv.h_mean if sv.h_mean is not None else _segment_reduce_raw(sv.h, bc.rp, N.WSI_RED_MEAN)[0]
        qs = _gate_table(hctx, sv.skip, "gate_of_seg", segs, bc.rp.num_segs)
        return (qs @ (bc.g_sum * (bc.x_mean - h_mean)).sum(dim=1)) * (1.0 - torch.sigmoid(sv.skip))
    if early is not None:
        return early[0]
    return _heat_gate_launch(g_out, sv, hctx, N.stream())[0]


def _heat_collapse_tables(gt_seg, bc, sv: _HeatSaved, st: _HeatState, P, omg):
    """The tables with which the attention backward never forms g_v (rank <= S x H; ``wsi_attn_pool_t``).  One grouped NN GEMM:
        y[tau, seg, hh, :] = g_t[seg]_hh (W_v^tau rows of head hh): what one unit of c[u, bin, hh] adds to g_h[u].
    When the forward never computed V (``_heat_collapse_lookups``): beta, the value-bias gradients and, where it fits, gtab.
    ``omg`` [T] = 1 - sigmoid(skip) of the type from wsi_pool_bwd_prep, or None: taken here by tensor operations.
    Returns (the N.AttnPool descriptor;  r_out [n, D], where pass 3 leaves the residual term of the K|Q dX epilogue, g_v W_v included;  ctab [n, T, H],
    the forward's coefficients or where pass 3 leaves them;  gbv [T, D] when the forward's coefficient sums gave it already;  what the descriptor points at)."""
    hctx, H, h, skip = st.hctx, st.H, sv.h, sv.skip
    (n, D), dev, T, S, plan = h.shape, h.device, len(hctx.rows), bc.rp.num_segs, hctx.plan
    dk = D // H
    ytab = torch.empty((T, S, H, D), dtype=torch.float32, device=dev)
    groups = [dict(A=N.ptr(gt_seg, hh * dk * 4), lda=D, B=N.ptr(P[tau][2], hh * dk * D * 4), ldb=D,
                   C=N.ptr(ytab, ((tau * S) * H + hh) * D * 4), ldc=H * D, M=S, N=D, K=dk) for tau in range(T) for hh in range(H)]
    _gemm(N.WSI_GEMM_NN, 0, groups, dev)
    if omg is None:           # [T]: 1 - s of the type; 1 where the layer passes h through
        omg = 1.0 - _gate_table(hctx, skip, "gate_of_row_type") @ torch.sigmoid(skip)
    r_out = torch.empty((n, D), dtype=torch.float32, device=dev)
    if st.no_v:
        ctab, (beta, gbv, gtab) = sv.ctab, _heat_collapse_lookups(gt_seg, ytab, bc.rp, sv, P, H)
    else:
        ctab, beta, gbv, gtab = torch.empty((n, T, H), dtype=torch.float32, device=dev), None, None, None
    desc = N.AttnPool(row_seg=N.ptr(bc.rp.row_segment()), segs_per_type=S // T, n_types=T, y=N.ptr(ytab), g_row=N.ptr(bc.g_row),
                      omg=N.ptr(omg), r_out=N.ptr(r_out), ldr=D, ctab=N.ptr(ctab), ctab_ready=1 if st.no_v else 0,
                      h=N.ptr(h) if st.no_v else None, ldh=D, beta=N.ptr(beta), gtab=N.ptr(gtab),
                      edge_seg=N.ptr(_edge_segments(plan)) if gtab is not None else None,
                      seg_dst=N.ptr(_segment_dst(plan)) if gtab is not None else None)
    return desc, r_out, ctab, gbv, (ytab, omg, beta, gtab)


def _heat_collapse_lookups(gt_seg, ytab, prp, sv: _HeatSaved, P, H: int):
    """Collapse after a forward without V.  One launch (wsi_pool_bwd_bias): beta[tau, s, hh] = g_t[seg]_hh . b_v^tau (head hh), and the
    value-bias gradients gbv [T, D] from the forward's coefficient sums.  Then, within wsi_heat_pool_gtab's limits (J = T * H <= 32 columns,
    table in 64 KB of LDS), gtab [n, T, H]: pass 1's dot products taken once per SOURCE node (T * H per node, one pass over h) instead of H per
    edge against gathered rows.  Returns (beta, gbv, gtab or None)."""
    h, T, S = sv.h, len(P), prp.num_segs
    (n, D), dev, lib = h.shape, h.device, N.load()
    gbv = torch.empty((T, D), dtype=torch.float32, device=dev)
    beta = torch.empty((T, S, H), dtype=torch.float32, device=dev)
    N.check(lib.wsi_pool_bwd_bias(N.ptr(gt_seg), T, S, D, H, _ptr_array([P[tau][6] for tau in range(T)]), N.ptr(sv.csum), N.ptr(beta), N.ptr(gbv),
                                  N.stream()), "wsi_pool_bwd_bias")
    if not (T * H <= 32 and T * H * (D + 4) * 4 <= 64 * 1024):
        return beta, gbv, None
    gtab = torch.empty((n, T, H), dtype=torch.float32, device=dev)
    with _Timed("heat_attn"), _Timed("heat_attn_bwd_pooled"):
        N.check(lib.wsi_heat_pool_gtab(N.ptr(h), D, D, H, N.ptr(ytab), N.ptr(beta), N.ptr(prp.chunk_row), N.ptr(prp.chunk_seg),
                                       prp.num_chunks, S // T, T, N.ptr(gtab), N.stream()), "wsi_heat_pool_gtab")
    return beta, gbv, gtab


def _heat_attention_backward(g_t, gt_row, sv: _HeatSaved, st: _HeatState, pool_desc):
    """Relation attention backward, one C call (wsi_heat_attn_bwd; pass 1 reads the saved logits and writes the probabilities): the queued weight
    gradients (this layer's a_linear, the layer above's K|Q|V) are flushed to run under it, and the column statistics of its result go to the
    side stream right after it, beside the dX projection (``_col_stats_side``).  ``g_t`` [n, D], or [S, D] read through ``gt_row``.
    Returns (gkqv like kqv - the V block is not written under a collapse -, its row scales, g_e [2], the side statistics or None)."""
    hctx, H, kqv = st.hctx, st.H, sv.kqv
    plan, (n, D), dev, ldp = hctx.plan, sv.h.shape, sv.h.device, kqv.shape[1]
    a = torch.empty_like(sv.score)
    scratch = torch.empty((3, max(plan.num_edges, 1), H), dtype=torch.float32, device=dev)
    red_ws = torch.empty(1024, dtype=torch.float32, device=dev)
    gkqv = torch.empty_like(kqv)
    g_e = torch.empty(2, dtype=torch.float32, device=dev)
    # pass 2: slot 0 of all n, pass 3: slot 1 of the source rows
    gkqv_max = _new_row_scale(max(n, plan.num_src_rows), 2, dev, 3 * D, zero=plan.num_src_rows != n)
    v, gv = (None, None) if st.no_v else (N.ptr(kqv, 2 * D * 4), N.ptr(gkqv, 2 * D * 4))
    _background_flush(dev)
    with _Timed("heat_attn"), _Timed("heat_attn_bwd_pooled" if pool_desc is not None else "heat_attn_bwd_full"):
        N.check(N.load().wsi_heat_attn_bwd(
            N.ptr(kqv, D * 4), ldp, N.ptr(kqv), ldp, v, ldp, n, plan.num_src_rows, plan.num_edges, D, H,
            N.ptr(plan.node_seg), N.ptr(plan.rowptr), N.ptr(plan.src), N.ptr(sv.sim_csr),
            N.ptr(plan.colptr), N.ptr(plan.csc_eid), N.ptr(plan.csc_dst),
            N.ptr(plan.inv_rd), N.ptr(plan.order_dst), plan.num_heavy, N.ptr(plan.order_src), _attn_flags(plan), N.ptr(sv.ew), N.ptr(sv.eb),
            N.ptr(g_t), D, N.ptr(gt_row), N.ptr(sv.score), N.ptr(a), N.ptr(sv.lse), N.ptr(scratch[0]), N.ptr(scratch[1]), N.ptr(scratch[2]), N.ptr(red_ws),
            N.ptr(gkqv, D * 4), ldp, N.ptr(gkqv), ldp, gv, ldp,
            N.ptr(g_e), N.ptr(gkqv_max), ctypes.byref(pool_desc) if pool_desc is not None else None, N.context(), N.stream()), "wsi_heat_attn_bwd")
    gk_side = _col_stats_side(gkqv, hctx.rows, dev) if (want_col_stats(n, D, D) and (D % 32 == 0)) else None
    return gkqv, gkqv_max, g_e, gk_side


def _heat_dx_chunked(gkqv, gkqv_max, resid, nproj: int, hctx, P, skip):
    """K|Q(|V) dX for D % 32 == 0: g_h = gkqv [Wk; Wq(; Wv)] + residual, the weights as chunks of one reduction (K = nproj * D) - one grouped NN
    GEMM per epilogue.  ``skip`` None (collapsed: ``resid`` = r_out already carries the 1 - s factor and g_v W_v): one launch over all node
    types.  Else ``resid`` = g_out: the gated types with (1 - s) * g_out in the epilogue, then the passed-through types with g_out as it is.
    g_h is the dY of the weight gradient below it (the lower layer's output projection, or the input projection): the epilogue leaves its row
    scales and column statistics - absmax and sums (the bias gradient) - that launch would otherwise take a pass over g_h for.  Returns g_h."""
    T, n, D, dev, ldp = len(hctx.rows), gkqv.shape[0], resid.shape[1], gkqv.device, gkqv.shape[1]
    g_h = torch.empty((n, D), dtype=torch.float32, device=dev)
    gh_max = _new_row_scale(n, N.gemm_absmax_parts(D), dev, D, zero=False)   # the launches cover every row
    gh_cols = ColStats.allocate(hctx.rows, D, dev, sums=True) if want_col_stats(n, D, D) else None
    wrote = True
    for idxs in ([list(range(T))] if skip is None else [[i for i in range(T) if hctx.incoming[i] == w_] for w_ in (True, False)]):
        if not idxs:
            continue
        gated = skip is not None and hctx.incoming[idxs[0]]
        groups = []
        for i in idxs:
            r0, r1 = hctx.rows[i]
            ws = list(P[i][:nproj])
            groups.append(dict(A=N.ptr(gkqv, r0 * ldp * 4), lda=ldp, b_chunk=D, ldb=D, Bw=ws, **dict(zip(("B", "B1", "B2"), map(N.ptr, ws))),
                               C=N.ptr(g_h, r0 * D * 4), ldc=D, R=N.ptr(resid, r0 * D * 4), ldr=D,
                               gate=_gate_ptr(skip, hctx, i) if gated else None, M=r1 - r0, N=D, K=nproj * D,
                               **_scale_in(gkqv_max, r0), **_scale_out(gh_max, r0),
                               **(gh_cols.produce(r0, r1, 0) if gh_cols is not None else {})))
        wrote = _gemm(N.WSI_GEMM_NN, N.WSI_EPI_ADD_R | (N.WSI_EPI_R_1MG if gated else 0), groups, dev) and wrote
    if gh_max is not None:
        attach_row_scales(g_h, gh_max)
    if gh_cols is not None and wrote:
        attach_col_stats(g_h, gh_cols)
    return g_h


def _heat_dx_by_block(gkqv, g_out, hctx, P, skip):
    """K|Q|V dX for a width that is no multiple of 32 (the chunked launch needs it): per epilogue - gated types, then passed-through ones -
    three grouped NN GEMMs, the K block with the residual epilogue and the Q and V blocks accumulating.  Returns g_h (no statistics attached)."""
    T, (n, D), dev = len(hctx.rows), g_out.shape, gkqv.device
    g_h = torch.empty((n, D), dtype=torch.float32, device=dev)
    for with_gate in (True, False):
        idxs = [i for i in range(T) if hctx.incoming[i] == with_gate]
        if not idxs:
            continue
        epi = N.WSI_EPI_ADD_R | (N.WSI_EPI_R_1MG if with_gate else 0)
        for j in range(3):
            groups = []
            for i in idxs:
                r0, r1 = hctx.rows[i]
                groups.append(dict(A=N.ptr(gkqv, (r0 * 3 * D + j * D) * 4), lda=3 * D, B=N.ptr(P[i][j]), ldb=D,
                                   C=N.ptr(g_h, r0 * D * 4), ldc=D, R=N.ptr(g_out, r0 * D * 4), ldr=D,
                                   gate=_gate_ptr(skip, hctx, i) if with_gate else None, M=r1 - r0, N=D, K=D))
            _gemm(N.WSI_GEMM_NN, epi if j == 0 else N.WSI_EPI_ACCUMULATE, groups, dev)
    return g_h


def _heat_kqv_weight_grads(gkqv, gk_side, nproj: int, sv: _HeatSaved, st: _HeatState, P, grads) -> None:
    """K|Q(|V) weight and bias gradients, one grouped TN GEMM: gW = gkqv^T h, gb = colsum(gkqv), per node type and column block.  In a layer
    with another HEAT layer below it (``st.background_dw``) it is queued to run under THAT layer's attention backward; else it runs here,
    after the side stream's column statistics (``gk_side``) are there.  Fills ``grads``."""
    hctx, h, h_cols, dev = st.hctx, sv.h, st.h_cols, sv.h.device
    T, D, ldp = len(hctx.rows), h.shape[1], gkqv.shape[1]
    wgroups = []
    for i, (r0, r1) in enumerate(hctx.rows):
        for j in range(nproj):
            gw, gb = torch.empty_like(P[i][j]), torch.empty_like(P[i][4 + j])
            grads[8 * i + j], grads[8 * i + 4 + j] = gw, gb
            wgroups.append(dict(A=N.ptr(gkqv, (r0 * ldp + j * D) * 4), lda=ldp, B=N.ptr(h, r0 * D * 4), ldb=D,
                                C=N.ptr(gw), ldc=D, colsum_out=N.ptr(gb), M=D, N=D, K=r1 - r0,
                                **(gk_side[0].consume("a", r0, r1, j * D, want_sums=True) if gk_side is not None else {}),
                                **(h_cols.consume("b", r0, r1, 0) if h_cols is not None else {})))
    wr = [P[i][k] for i in range(T) for j in range(nproj) for k in (j, 4 + j)]
    keep = [gkqv, h] + ([h_cols.bits] if h_cols is not None else []) + ([gk_side[0].bits, gk_side[0].sums] if gk_side is not None else [])
    outs = [(P[i][k], grads[8 * i + k]) for i in range(T) for j in range(nproj) for k in (j, 4 + j)]
    evs = [gk_side[1]] if gk_side is not None else []
    if not (st.background_dw and _background_safe(wr) and _gemm_tn_background(0, wgroups, dev, keep, wr, evs, outs=outs)):
        for ev in evs:
            torch.cuda.current_stream(dev).wait_event(ev)
        _gemm(N.WSI_GEMM_TN, 0, wgroups, dev)


def _heat_factors_from_pass3(gt_seg, ctab, prp, h, T: int, H: int):
    """Collapse after a forward that kept V: the weighted sums of h from the coefficients pass 3 left (``_pooled_factors``: two launches),
    and the value-bias gradients from their sums (wsi_pool_bwd_bias).  Returns (hp, gbv [T, D])."""
    hp, csum = _pooled_factors(h, ctab, prp, T, H)
    gbv = torch.empty((T, h.shape[1]), dtype=torch.float32, device=h.device)
    N.check(N.load().wsi_pool_bwd_bias(N.ptr(gt_seg), T, prp.num_segs, h.shape[1], H, None, N.ptr(csum), None, N.ptr(gbv), N.stream()),
            "wsi_pool_bwd_bias")
    return hp, gbv


def _heat_value_weight_grads(gt_seg, hp, gbv, P, H: int, grads) -> None:
    """Value-weight gradients under the collapse, one grouped TN GEMM over the S segment rows:
        dW_v^tau (rows of head hh) = sum_seg g_t[seg]_hh (x) hp[seg, hh, tau, :]    (hp: weighted sums of h over the (source type, graph) segments);
    db_v^tau = gbv[tau].  Fills ``grads``."""
    T, (S, D) = len(P), gt_seg.shape
    dk = D // H
    wgroups = []
    for tau in range(T):
        gw = torch.empty_like(P[tau][2])
        grads[8 * tau + 2], grads[8 * tau + 6] = gw, gbv[tau]
        for hh in range(H):
            wgroups.append(dict(A=N.ptr(gt_seg, hh * dk * 4), lda=D, B=N.ptr(hp, (hh * T + tau) * D * 4), ldb=H * T * D,
                                C=N.ptr(gw, hh * dk * D * 4), ldc=D, M=dk, N=D, K=S))
    _gemm(N.WSI_GEMM_TN, 0, wgroups, gt_seg.device)


class _HeatLayerFused(torch.autograd.Function):
    """inputs: h [N,D], hctx (HeatContext), H, skip [T_model], e_weight [1,1], e_bias [1], drop_mask ([N,D] keep mask
    scaled by 1/(1-p) for the nn.Dropout of HEATNet4.py:135, a CounterDropout, or None), then per graph node type i (in hctx order) 8 tensors:
    Wk, Wq, Wv, Wa, bk, bq, bv, ba.

    ``pool`` = (ReducePlan, WSI_RED_SUM | WSI_RED_MEAN) or None.  With a pool the function returns the READOUT of the layer's output,
    [num_segs, D], and never forms the output itself: a sum / mean over node rows commutes with the affine output stage,
        mean_seg( s (t Wa^T + ba) + (1 - s) h ) = s (mean_seg(t) Wa^T + ba) + (1 - s) mean_seg(h)
    (models/HEATNet4.py:128-135 followed by pools[0] at :219, with no dropout between them) - the [N, D] x [D, D] projection becomes
    two segment means and an [S, D] x [D, D] one, and the backward starts from the S gradient rows it would otherwise meet broadcast
    to N (``SegmentBroadcast``).  Every segment of the plan must lie inside one node type's row range.

    Four formulations share the stages (``_heat_*`` above, one per launch group; DESIGN 3.7 has the table): full depth (pool None);
    full depth under a broadcast gradient (``_heat_row_gradient`` finds the readout's annotation: the output projection works on S rows);
    readout-fused (t formed, then the segment means of t and h); readout-fused without V.  The two predicates of the last:
      no_v     (forward)  = pool is not None and _value_collapse_applies(...): V is never projected, kqv is K | Q;
      collapse (backward) = no_v or the same question asked again: g_v is never formed - the attention backward takes the pool descriptor,
                            dX and dW the K and Q blocks only.  They differ only if ``set_value_collapse`` moved between the two passes."""

    @staticmethod
    def forward(ctx, h, hctx, H, skip, e_weight, e_bias, drop_mask, pool, background_dw, *params):
        N.require_cuda(h)
        _background_recover()                  # (leftovers of a backward pass that raised: nothing in the normal case)
        h = h.contiguous()
        n, D = h.shape
        P = [params[8 * i:8 * i + 8] for i in range(len(hctx.rows))]
        if isinstance(drop_mask, CounterDropout) and drop_mask.threshold == 0:
            drop_mask = None                    # p quantises to 0: nothing is dropped
        if pool is not None and (drop_mask is not None or pool[0].segments_of(hctx.rows) is None or pool[0].num_rows != n
                                 or pool[1] not in (N.WSI_RED_SUM, N.WSI_RED_MEAN)):        # refused before anything is launched
            raise ValueError("heat_layer_fused(pool=...): needs a sum / mean plan over all rows whose segments respect the node types, and no dropout mask")
        no_v = pool is not None and _value_collapse_applies(hctx, pool[0], n, D, H)
        # fp16x3 row scales (absmax bits) travel with the activations: h's from its producer, t's from the attention kernel,
        # out's from the epilogue that writes it - no projection makes its own pass over an operand the path just produced
        h_max = row_scales_of(h)
        h_cols = col_stats_of(h)
        edge = (e_weight.reshape(-1), e_bias.reshape(-1), hctx.sim_csr)          # (sim fetched once per forward; the backward uses the same tensor)
        kqv, t_cols = _heat_project(h, h_max, hctx, P, 2 if no_v else 3, v_stats=pool is None and want_col_stats(n, D, D))
        st = _HeatState(hctx, H, pool, no_v, "mask" if isinstance(drop_mask, torch.Tensor) else drop_mask, h_cols, t_cols, bool(background_dw))
        ctx.st = st
        if no_v:
            score, lse, ctab, hp, csum, h_mean, t_mean = _heat_attend_pooled(h, kqv, hctx, H, edge, pool[0], P)
            z_mean, pooled = _heat_output_means(t_mean, h_mean, hctx, P, skip, pool)
            _heat_save(ctx, _HeatSaved(h, kqv, score, lse, skip, *edge, t_mean=t_mean, h_mean=h_mean, z_mean=z_mean, ctab=ctab, hp=hp, csum=csum, params=params))
            return pooled
        t_max = _new_row_scale(n, 1, h.device, D, zero=False)                          # the attention kernel writes every row
        t, score, lse = _heat_attend(kqv, t_max, hctx, H, edge)
        if pool is not None:
            t_mean = _segment_reduce_raw(t, pool[0], N.WSI_RED_MEAN)[0]
            h_mean = _segment_reduce_raw(h, pool[0], N.WSI_RED_MEAN)[0]
            z_mean, pooled = _heat_output_means(t_mean, h_mean, hctx, P, skip, pool)
            _heat_save(ctx, _HeatSaved(h, kqv, score, lse, skip, *edge, t_mean=t_mean, h_mean=h_mean, z_mean=z_mean, params=params))
            return pooled
        out = _heat_output_rows(h, t, (h_max, t_max), hctx, P, skip, drop_mask)
        _heat_save(ctx, _HeatSaved(h, kqv, score, lse, skip, *edge, t=t, out=out, mask=drop_mask if st.dropout == "mask" else None, params=params))
        return out

    @staticmethod
    def backward(ctx, g_out):
        st, sv = ctx.st, _heat_saved(ctx)
        hctx, H, T, (n, D) = st.hctx, st.H, len(st.hctx.rows), sv.h.shape
        P = [sv.params[8 * i:8 * i + 8] for i in range(T)]
        grads = [None] * (8 * T)
        collapse = st.pool is not None and (st.no_v or _value_collapse_applies(hctx, st.pool[0], n, D, H))
        # 1) gradient intake, 2) dropout on the gradient; at full depth and size the skip-gate launch goes to the statistics stream here,
        # in front of the output-projection groups
        if st.pool is None:
            g_out, bc, segs, annotated = _heat_row_gradient(g_out, hctx, n)
            # (the counter's mask regenerated from (seed, row, column) in one launch, never stored; or the saved mask tensor)
            g_y = dropout_apply(g_out, st.dropout) if isinstance(st.dropout, CounterDropout) else (g_out if st.dropout is None else g_out * sv.mask)
            pre = None
            early = _heat_early_gate(g_out, sv, hctx) if (not annotated and _side_stats_on() and float(n) * D >= 2.0e7) else None
        else:
            bc, pre = _heat_pooled_gradient(g_out, sv, st)
            segs = bc.rp.segments_of(hctx.rows)
            g_out = None if collapse else _heat_broadcast_rows(bc, n, D)       # (collapse: the residual term of the dX epilogue comes out of pass 3)
            g_y = early = None                                                  # (no dropout under a readout; the S rows go through stage 3 as they are)
        # 3) output-projection gradients
        if bc is not None and st.dropout is None:
            g_t, gt_row = _heat_out_proj_low_rank(bc, segs, sv, hctx, P, grads)
        else:
            g_t, gt_row = _heat_out_proj_rows(g_y, sv, st, P, grads), None
        # 4) skip-gate gradient
        g_skip = _heat_skip_gate_grad(g_out, sv, hctx, bc, segs, pre, early)
        if collapse:
            # 5) collapse tables, 6) attention backward, 7) dX and 8) dW on the K and Q blocks, 9) value-weight gradients from the factors
            pool_desc, r_out, ctab, gbv, _alive = _heat_collapse_tables(g_t, bc, sv, st, P, pre[1] if pre is not None else None)
            gkqv, gkqv_max, g_e, gk_side = _heat_attention_backward(g_t, gt_row, sv, st, pool_desc)
            g_h = _heat_dx_chunked(gkqv, gkqv_max, r_out, 2, hctx, P, None)
            _heat_kqv_weight_grads(gkqv, gk_side, 2, sv, st, P, grads)
            hp, gbv = (sv.hp, gbv) if st.no_v else _heat_factors_from_pass3(g_t, ctab, bc.rp, sv.h, T, H)
            _heat_value_weight_grads(g_t, hp, gbv, P, H, grads)
        else:
            # 6) attention backward, 7) K|Q|V dX: g_h = gkqv [Wk; Wq; Wv] + (1 - s) g_out, 8) K|Q|V dW
            gkqv, gkqv_max, g_e, gk_side = _heat_attention_backward(g_t, gt_row, sv, st, None)
            g_h = _heat_dx_chunked(gkqv, gkqv_max, g_out, 3, hctx, P, sv.skip) if D % 32 == 0 else _heat_dx_by_block(gkqv, g_out, hctx, P, sv.skip)
            _heat_kqv_weight_grads(gkqv, gk_side, 3, sv, st, P, grads)
        if early is not None:
            torch.cuda.current_stream(sv.h.device).wait_event(early[1])
        return (g_h, None, None, g_skip, g_e[0:1].view(1, 1), g_e[1:2], None, None, None, *grads)


def heat_layer_fused(h, hctx, H, skip, e_weight, e_bias, params, drop_mask=None, pool=None, background_dw=False):
    """``pool`` = (ReducePlan, "sum" | "mean"): return the readout of the layer's output instead of the output (see _HeatLayerFused).
    ``background_dw``: another HEAT layer's backward follows this one's (it is not the first layer): its K|Q|V weight gradient may run on the
    side stream under that layer's attention backward (``_gemm_tn_background``)."""
    if pool is not None:
        pool = (pool[0], {"sum": N.WSI_RED_SUM, "mean": N.WSI_RED_MEAN}[pool[1]])
    return _HeatLayerFused.apply(h, hctx, H, skip, e_weight, e_bias, drop_mask, pool, background_dw, *params)


# ------------------------------------------------------------------------------------------------
# the trainer's loss
# ------------------------------------------------------------------------------------------------
class _CrossEntropy(torch.autograd.Function):
    """torch.nn.CrossEntropyLoss() with its defaults (mean over the batch; parser.py:182-183) as ONE launch forward (``wsi_cross_entropy``: the loss
    and the gradient factor together) and one tiny scaling backward, where torch takes log_softmax + nll_loss and their two backward kernels
    plus fills.  A label of -100 (the default ``ignore_index``) is ignored as torch ignores it (zero gradient row, mean over the others); any
    other label outside [0, C) - torch's device assert - makes the loss NaN with a zero gradient row and sets the flag the returned tensor carries
    as ``_wsi_bad_label`` (a one-element int32 device tensor; ``trainer.train_one_step`` raises on it where it synchronises anyway)."""

    @staticmethod
    def forward(ctx, logits, labels, bad):
        N.require_cuda(logits, labels)
        logits = logits.contiguous()
        labels = labels.contiguous()
        if labels.dtype != torch.int64 or logits.dim() != 2 or labels.shape != logits.shape[:1]:
            raise ValueError("cross_entropy: logits [B, C] fp32 and int64 labels [B]")
        B, C = logits.shape
        out = torch.empty(1 + B * C, dtype=torch.float32, device=logits.device)
        N.check(N.load().wsi_cross_entropy(N.ptr(logits), N.ptr(labels), B, C, N.ptr(out), N.ptr(out, 4), N.ptr(bad), N.stream()), "wsi_cross_entropy")
        ctx.save_for_backward(out)
        ctx.shape = (B, C)
        return out[0]

    @staticmethod
    def backward(ctx, g):
        (out,) = ctx.saved_tensors
        return out[1:].view(ctx.shape) * g, None, None


def cross_entropy(logits: torch.Tensor, labels: torch.Tensor) -> torch.Tensor:
    """Mean cross entropy (a 0-dim tensor), ``F.cross_entropy(logits, labels)`` with default arguments."""
    bad = torch.zeros(1, dtype=torch.int32, device=logits.device)
    loss = _CrossEntropy.apply(logits, labels, bad)
    loss._wsi_bad_label = bad
    return loss


# ------------------------------------------------------------------------------------------------
# general relation attention (separate q table and stacked K|V table) — HGT
# ------------------------------------------------------------------------------------------------
class _RelationAttention(torch.autograd.Function):
    """t[N,D] from q [N,D] and kv [R,2D] (K at column 0, V at D); plan.src / plan.colptr index kv rows."""

    @staticmethod
    def forward(ctx, q, kv, e_weight, e_bias, plan: GraphPlan, sim_csr, D: int, H: int):
        N.require_cuda(q, kv)
        lib = N.load()
        q = q.contiguous()
        kv = kv.contiguous()
        n, E, S = plan.num_nodes, plan.num_edges, plan.num_segs
        dev = q.device
        t = torch.empty((n, D), dtype=torch.float32, device=dev)
        score = torch.empty((max(E, 1), H), dtype=torch.float32, device=dev)
        lse = torch.empty((max(S, 1), H), dtype=torch.float32, device=dev)
        ew, eb = e_weight.reshape(-1), e_bias.reshape(-1)
        with _Timed("heat_attn"):
            N.check(lib.wsi_heat_attn_fwd(
                N.ptr(q), q.stride(0), N.ptr(kv, 0), kv.stride(0), N.ptr(kv, D * 4), kv.stride(0), n, D, H,
                N.ptr(plan.node_seg), N.ptr(plan.rowptr), N.ptr(plan.src), N.ptr(sim_csr), N.ptr(plan.order_dst), plan.num_heavy, _attn_flags(plan),
                N.ptr(ew), N.ptr(eb), N.ptr(t), D, N.ptr(score), N.ptr(lse), None, N.context(), N.stream()), "wsi_heat_attn_fwd")
        ctx.plan, ctx.D, ctx.H = plan, D, H
        ctx.save_for_backward(q, kv, ew, eb, sim_csr, score, lse)
        return t

    @staticmethod
    def backward(ctx, g_t):
        lib = N.load()
        plan, D, H = ctx.plan, ctx.D, ctx.H
        q, kv, ew, eb, sim_csr, score, lse = ctx.saved_tensors
        g_t = g_t.contiguous()
        n, E = plan.num_nodes, plan.num_edges
        dev = q.device
        a = torch.empty_like(score)
        scratch = torch.empty((3, max(E, 1), H), dtype=torch.float32, device=dev)
        red_ws = torch.empty(1024, dtype=torch.float32, device=dev)
        gq = torch.empty_like(q)
        gkv = torch.empty_like(kv)
        g_e = torch.empty(2, dtype=torch.float32, device=dev)
        with _Timed("heat_attn"):
            N.check(lib.wsi_heat_attn_bwd(
                N.ptr(q), q.stride(0), N.ptr(kv, 0), kv.stride(0), N.ptr(kv, D * 4), kv.stride(0),
                n, plan.num_src_rows, E, D, H,
                N.ptr(plan.node_seg), N.ptr(plan.rowptr), N.ptr(plan.src), N.ptr(sim_csr),
                N.ptr(plan.colptr), N.ptr(plan.csc_eid), N.ptr(plan.csc_dst),
                N.ptr(plan.inv_rd), N.ptr(plan.order_dst), plan.num_heavy, N.ptr(plan.order_src), _attn_flags(plan), N.ptr(ew), N.ptr(eb),
                N.ptr(g_t), g_t.stride(0), None, N.ptr(score), N.ptr(a), N.ptr(lse), N.ptr(scratch[0]), N.ptr(scratch[1]), N.ptr(scratch[2]), N.ptr(red_ws),
                N.ptr(gq), gq.stride(0), N.ptr(gkv, 0), gkv.stride(0), N.ptr(gkv, D * 4), gkv.stride(0),
                N.ptr(g_e), None, None, N.context(), N.stream()), "wsi_heat_attn_bwd")
        return gq, gkv, g_e[0:1].view(1, 1), g_e[1:2], None, None, None, None


def relation_attention(q, kv, e_weight, e_bias, plan: GraphPlan, sim_csr, D: int, H: int) -> torch.Tensor:
    return _RelationAttention.apply(q, kv, e_weight, e_bias, plan, sim_csr, D, H)


# ------------------------------------------------------------------------------------------------
# gated linear:  z[rows_i] = s_i * (t[rows_i] W_i^T + b_i) + (1 - s_i) * h[rows_i],  s_i = sigmoid(skip[nid_i])
# (models/HGT.py:121-122, models/HEATNet4.py:134-135 when not fused into the whole layer)
# ------------------------------------------------------------------------------------------------
class _GatedLinear(torch.autograd.Function):
    @staticmethod
    def forward(ctx, t, h, skip, rows, nids, rplan, seg_of, n_g, drop_mask, *params):
        N.require_cuda(t, h)
        t = t.contiguous()
        h = h.contiguous()
        dev = t.device
        n, D = h.shape
        K = t.shape[1]
        ws, bs = params[:n_g], params[n_g:]
        covered = sum(b - a for a, b in rows) == n
        z = torch.empty((n, D), dtype=torch.float32, device=dev) if covered else h.clone()
        groups = []
        for i, (r0, r1) in enumerate(rows):
            groups.append(dict(A=N.ptr(t, r0 * K * 4), lda=K, B=N.ptr(ws[i]), ldb=K, C=N.ptr(z, r0 * D * 4), ldc=D,
                               bias=N.ptr(bs[i]), R=N.ptr(h, r0 * D * 4), ldr=D, gate=N.ptr(skip, 4 * nids[i]),
                               Mm=N.ptr(drop_mask, r0 * D * 4) if drop_mask is not None else None, ldm=D,
                               M=r1 - r0, N=D, K=K))
        _gemm(N.WSI_GEMM_NT, N.WSI_EPI_GATED_SKIP | (N.WSI_EPI_MUL_M if drop_mask is not None else 0), groups, dev)
        ctx.rows, ctx.nids, ctx.rplan, ctx.seg_of, ctx.n_g, ctx.covered = rows, nids, rplan, seg_of, n_g, covered
        ctx.has_mask = drop_mask is not None
        ctx.save_for_backward(t, h, z, skip, *(() if drop_mask is None else (drop_mask,)), *ws)
        return z

    @staticmethod
    def backward(ctx, g_z):
        rows, nids, rp, seg_of, n_g = ctx.rows, ctx.nids, ctx.rplan, ctx.seg_of, ctx.n_g
        t, h, z, skip, *ws = ctx.saved_tensors
        g_z = g_z.contiguous()
        g_y = g_z                         # gradient w.r.t. the (un-dropped) linear output, before the gate scaling
        if ctx.has_mask:
            g_y = g_z * ws[0]
            ws = ws[1:]
        dev = t.device
        n, D = h.shape
        K = t.shape[1]
        gate = lambda i: N.ptr(skip, 4 * nids[i])
        g_t = (torch.empty if ctx.covered else torch.zeros)((n, K), dtype=torch.float32, device=dev)
        gws, gbs, groups, wgroups = [], [], [], []
        for i, (r0, r1) in enumerate(rows):
            groups.append(dict(A=N.ptr(g_y, r0 * D * 4), lda=D, B=N.ptr(ws[i]), ldb=K, C=N.ptr(g_t, r0 * K * 4), ldc=K,
                               gate=gate(i), M=r1 - r0, N=K, K=D))
            gw = torch.empty_like(ws[i])
            gws.append(gw)
            gbs.append(torch.empty(D, dtype=torch.float32, device=dev))
            wgroups.append(dict(A=N.ptr(g_y, r0 * D * 4), lda=D, B=N.ptr(t, r0 * K * 4), ldb=K, C=N.ptr(gw), ldc=K,
                                gate=gate(i), colsum_out=N.ptr(gbs[-1]), M=D, N=K, K=r1 - r0))
        _gemm(N.WSI_GEMM_NN, N.WSI_EPI_SCALE_GATE, groups, dev)
        _gemm(N.WSI_GEMM_TN, N.WSI_EPI_SCALE_GATE, wgroups, dev)
        sig = torch.sigmoid(skip)
        dots = segment_dot_diff(g_z, z, h, rp)                          # segment seg_of[i] of rp == rows[i]
        g_skip = torch.zeros_like(skip)
        scale = torch.ones(n, 1, dtype=torch.float32, device=dev)       # rows outside `rows` pass h through: dz/dh = 1
        for i, (r0, r1) in enumerate(rows):
            s_i = sig[nids[i]]
            g_skip[nids[i]] = g_skip[nids[i]] + dots[seg_of[i]] * (1.0 - s_i)
            scale[r0:r1] = 1.0 - s_i
        g_h = g_z * scale
        return (g_t, g_h, g_skip, None, None, None, None, None, None, *gws, *gbs)


def gated_linear(t, h, skip, rows, nids, rplan, seg_of, weights, biases, drop_mask=None):
    """``rplan``: ReducePlan over (gap-filled) row ranges; ``seg_of[i]`` = its segment holding ``rows[i]``.  ``drop_mask``: [n, D]
    keep mask already scaled by 1 / (1 - p) (the nn.Dropout between the linear and the gate, models/HGT.py:121), or None."""
    return _GatedLinear.apply(t, h, skip, rows, nids, rplan, seg_of, len(weights), drop_mask, *weights, *biases)


# ------------------------------------------------------------------------------------------------
# GELU, LayerNorm, GraphConv aggregation
# ------------------------------------------------------------------------------------------------
class _Gelu(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        N.require_cuda(x)
        x = x.contiguous()
        y = torch.empty_like(x)
        N.check(N.load().wsi_gelu_fwd(N.ptr(x), N.ptr(y), x.numel(), N.stream()), "wsi_gelu_fwd")
        ctx.save_for_backward(x)
        return y

    @staticmethod
    def backward(ctx, gy):
        (x,) = ctx.saved_tensors
        gy = gy.contiguous()
        gx = torch.empty_like(x)
        N.check(N.load().wsi_gelu_bwd(N.ptr(x), N.ptr(gy), N.ptr(gx), x.numel(), N.stream()), "wsi_gelu_bwd")
        return gx


def gelu(x: torch.Tensor) -> torch.Tensor:
    return _Gelu.apply(x)


class _LayerNorm(torch.autograd.Function):
    """Per-row LayerNorm with per-node-type affine parameters: gamma/beta [P,D], row_param[n] int32 -> P;
    ``rplan`` segments = row ranges sharing a parameter row, ``seg_param[s]`` = that parameter row."""

    @staticmethod
    def forward(ctx, x, gamma, beta, row_param, rplan, seg_param, eps):
        N.require_cuda(x)
        x = x.contiguous()
        gamma = gamma.contiguous()
        beta = beta.contiguous()
        n, D = x.shape
        y = torch.empty_like(x)
        stats = torch.empty((max(n, 1), 2), dtype=torch.float32, device=x.device)
        N.check(N.load().wsi_layernorm_fwd(N.ptr(x), D, n, D, float(eps), N.ptr(gamma), N.ptr(beta), N.ptr(row_param),
                                           N.ptr(y), D, N.ptr(stats), N.stream()), "wsi_layernorm_fwd")
        ctx.rplan, ctx.seg_param = rplan, seg_param
        ctx.save_for_backward(x, gamma, row_param, stats)
        return y

    @staticmethod
    def backward(ctx, gy):
        x, gamma, row_param, stats = ctx.saved_tensors
        gy = gy.contiguous()
        n, D = x.shape
        gx = torch.empty_like(x)
        xhat_gy = torch.empty_like(x)
        N.check(N.load().wsi_layernorm_bwd(N.ptr(gy), D, N.ptr(x), D, n, D, N.ptr(gamma), N.ptr(row_param), N.ptr(stats),
                                           N.ptr(gx), D, N.ptr(xhat_gy), D, N.stream()), "wsi_layernorm_bwd")
        gg_seg = _segment_reduce_raw(xhat_gy, ctx.rplan, N.WSI_RED_SUM)[0]     # [S, D]
        gb_seg = _segment_reduce_raw(gy, ctx.rplan, N.WSI_RED_SUM)[0]
        ggamma = torch.zeros_like(gamma)
        gbeta = torch.zeros_like(gamma)
        for s_, p_ in enumerate(ctx.seg_param):
            ggamma[p_] = ggamma[p_] + gg_seg[s_]
            gbeta[p_] = gbeta[p_] + gb_seg[s_]
        return gx, ggamma, gbeta, None, None, None, None


def layer_norm(x, gamma, beta, row_param, rplan, seg_param, eps=1e-5):
    return _LayerNorm.apply(x, gamma, beta, row_param, rplan, seg_param, eps)


class _GraphConvAggregate(torch.autograd.Function):
    """y = act(indeg^-1/2 * sum_{e: u->w} s_e * outdeg^-1/2[u] * z[u] + bias)   (DGL GraphConv norm='both', after/before the GEMM).
    ``edge_scale`` None: s = the plan's constant edge weights (or 1); only y is saved.  ``edge_scale`` [E] (CSR order): it receives a gradient,
    g_s[e] = indeg^-1/2[w] outdeg^-1/2[u] <g_y[w] * act', z[u]> (``wsi_sddmm_dot``), for which z is saved as well."""

    @staticmethod
    def forward(ctx, z, bias, edge_scale, hp, relu: bool):
        N.require_cuda(z, bias, edge_scale)
        if edge_scale is not None and getattr(hp, "edge_w", None) is not None:
            raise RuntimeError("graph_conv_aggregate: edge_scale on a plan that already carries constant edge weights (EdgeCSR.with_weights)")
        z = z.contiguous()
        s = edge_scale.detach().to(torch.float32).contiguous() if edge_scale is not None else None
        n, D = z.shape
        y = torch.empty_like(z)
        N.check(N.load().wsi_spmm_sum(N.ptr(z), D, n, D, N.ptr(hp.rowptr), N.ptr(hp.src), N.ptr(getattr(hp, "edge_w", None) if s is None else s),
                                      N.ptr(hp.out_norm), N.ptr(hp.in_norm),
                                      N.ptr(bias), 1 if relu else 0, None, 0, N.ptr(y), D, N.stream()), "wsi_spmm_sum")
        ctx.hp, ctx.relu, ctx.has_bias, ctx.scaled = hp, relu, bias is not None, s is not None
        ctx.save_for_backward(*((y,) if s is None else (y, z, s)))
        return y

    @staticmethod
    def backward(ctx, gy):
        y, *zs = ctx.saved_tensors
        hp = ctx.hp
        gy = gy.contiguous()
        n, D = y.shape
        gz = gb = gs = None
        need = ctx.needs_input_grad if ctx.scaled else (True, True, False)     # (without a scale gz and gb are written whether asked for or not)
        if need[0]:
            gz = torch.empty_like(y)
            w_csc = zs[1][hp.csc_eid.long()] if ctx.scaled else getattr(hp, "edge_w_csc", None)
            N.check(N.load().wsi_spmm_sum(N.ptr(gy), D, n, D, N.ptr(hp.colptr), N.ptr(hp.csc_dst), N.ptr(w_csc), N.ptr(hp.in_norm), N.ptr(hp.out_norm),
                                          None, 0, N.ptr(y) if ctx.relu else None, D, N.ptr(gz), D, N.stream()), "wsi_spmm_sum")
        if ctx.has_bias and need[1]:
            gb = (gy * (y > 0).to(gy.dtype)).sum(0) if ctx.relu else gy.sum(0)
        if need[2]:
            gs = torch.empty_like(zs[1])
            N.check(N.load().wsi_sddmm_dot(N.ptr(gy), D, N.ptr(zs[0]), D, n, D, N.ptr(hp.rowptr), N.ptr(hp.src), N.ptr(hp.out_norm), N.ptr(hp.in_norm),
                                           N.ptr(y) if ctx.relu else None, D, N.ptr(gs), N.stream()), "wsi_sddmm_dot")
        return gz, gb, gs, None, None


def _check_edge_scale(what: str, edge_scale: torch.Tensor, plan) -> None:
    if edge_scale.dim() != 1 or edge_scale.numel() != plan.num_edges:
        raise ValueError(f"{what}: edge_scale must be [{plan.num_edges}] (one value per edge, CSR order), got {tuple(edge_scale.shape)}")


def graph_conv_aggregate(z, bias, hplan, relu: bool, edge_scale: Optional[torch.Tensor] = None):
    """``edge_scale`` [E] (the plan's CSR edge order; None = the plain aggregation, unchanged): every message is multiplied by it and it
    receives a gradient (GNNExplainer's sigmoid(edge_mask): ``graph.message_scale``)."""
    if edge_scale is not None:
        _check_edge_scale("graph_conv_aggregate", edge_scale, hplan)
    return _GraphConvAggregate.apply(z, bias, edge_scale, hplan, relu)


# ------------------------------------------------------------------------------------------------
# GINConv aggregation (csrc/gin.hip; models/GIN.py)
# ------------------------------------------------------------------------------------------------
GIN_MODES = {"sum": N.WSI_GIN_SUM, "mean": N.WSI_GIN_MEAN, "max": N.WSI_GIN_MAX}
_gin_project_first = True


def set_gin_project_first(on: bool) -> None:
    """``models.GIN.GINConv`` with a sum or mean reducer and in_features > out_features runs the first Linear of its MLP BEFORE the
    aggregation (both are linear: W((1 + eps) x + agg x) + b = (1 + eps) z + agg z + b with z = x W^T), which gathers out_features instead of
    in_features columns per edge.  On by default; off: aggregate first, as the reference computes it.  Host state, no environment variable."""
    global _gin_project_first
    _gin_project_first = bool(on)


def gin_project_first() -> bool:
    return _gin_project_first


def _gin_check(x: torch.Tensor, eps: torch.Tensor, plan, mode: str, bias, edge_scale) -> None:
    if mode not in GIN_MODES:
        raise ValueError(f"gin_aggregate: mode {mode!r} (one of {sorted(GIN_MODES)})")
    if x.dim() != 2 or x.shape[0] != plan.num_nodes:
        raise ValueError(f"gin_aggregate: x must be [{plan.num_nodes}, D] (one row per node of the plan), got {tuple(x.shape)}")
    if eps.numel() != 1:
        raise ValueError(f"gin_aggregate: eps holds one value, got {tuple(eps.shape)}")
    if bias is not None and tuple(bias.shape) != (x.shape[1],):
        raise ValueError(f"gin_aggregate: bias must be [{x.shape[1]}], got {tuple(bias.shape)}")
    if edge_scale is not None:
        _check_edge_scale("gin_aggregate", edge_scale, plan)


def gin_aggregate_reference(x: torch.Tensor, eps: torch.Tensor, plan, mode: str, bias: Optional[torch.Tensor] = None,
                            edge_scale: Optional[torch.Tensor] = None, return_arg: bool = False):
    """``gin_aggregate`` with tensor operations, in x's dtype on x's device: what the kernels are held against, the CPU path and what
    ``kernels=False`` runs.  ``max`` takes the FIRST CSR position among equal messages (``return_arg``: also the int32 [n, D] table of
    those positions, -1 in rows without in-edges) and routes the gradient there."""
    _gin_check(x, eps, plan, mode, bias, edge_scale)
    n, D = x.shape
    dev = x.device
    rowptr = plan.rowptr.to(dev).long()
    src = plan.src.to(dev).long()
    deg = rowptr[1:n + 1] - rowptr[:n]
    E = int(src.numel())
    dst = torch.repeat_interleave(torch.arange(n, device=dev), deg, output_size=E)
    msg = x[src]
    if edge_scale is not None:
        msg = msg * edge_scale.to(x.dtype).view(-1, 1)
    arg = None
    if mode == "max":
        m = msg.detach()
        idx = dst.view(-1, 1).expand(E, D)
        top = torch.full((n, D), float("-inf"), dtype=x.dtype, device=dev).scatter_reduce(0, idx, m, "amax", include_self=True)
        pos = torch.arange(E, device=dev).view(-1, 1).expand(E, D)
        first = torch.full((n, D), E, dtype=torch.int64, device=dev).scatter_reduce(0, idx, torch.where(m == top[dst], pos, E), "amin", include_self=True)
        chosen = (pos == first[dst]).to(x.dtype)
        neigh = torch.zeros((n, D), dtype=x.dtype, device=dev).index_add(0, dst, msg * chosen)
        arg = torch.where(first < E, first, -1).to(torch.int32)
    else:
        neigh = torch.zeros((n, D), dtype=x.dtype, device=dev).index_add(0, dst, msg)
        if mode == "mean":
            neigh = neigh / deg.clamp(min=1).to(x.dtype).view(-1, 1)
    out = (1 + eps.to(x.dtype).reshape(())) * x + neigh
    if bias is not None:
        out = out + bias.to(x.dtype)
    return (out, arg) if return_arg else out


class _GinAggregate(torch.autograd.Function):
    """out[w] = (1 + eps) x[w] + reduce_{e: u -> w}(s_e x[u]) (+ bias) on ``wsi_gin_aggregate_fwd``; the backward launches only what is asked
    for: g_x (``wsi_gin_aggregate_bwd``), g_eps (``wsi_gin_eps_grad``, two launches), g_edge_scale (``wsi_gin_edge_grad``); g_bias = column sums.
    eps is read by the kernels from its own device storage."""

    @staticmethod
    def forward(ctx, x, eps, bias, edge_scale, plan, mode: int):
        N.require_cuda(x, eps, bias, edge_scale)
        if eps.dtype != torch.float32:
            raise ValueError("gin_aggregate: eps is an fp32 tensor on the device (the kernels read its storage)")
        x = x if x.dtype == torch.float32 and x.is_contiguous() else x.to(torch.float32).contiguous()
        e = eps.detach()
        b = None if bias is None else bias.detach().to(torch.float32).contiguous()
        s = None if edge_scale is None else edge_scale.detach().to(torch.float32).contiguous()
        n, D = x.shape
        need = ctx.needs_input_grad
        out = torch.empty((n, D), dtype=torch.float32, device=x.device)
        arg = torch.empty((n, D), dtype=torch.int32, device=x.device) if mode == N.WSI_GIN_MAX and (need[0] or need[3]) else None
        N.check(N.load().wsi_gin_aggregate_fwd(N.ptr(x), D, n, D, N.ptr(plan.rowptr), N.ptr(plan.src), N.ptr(s), N.ptr(e), mode, N.ptr(b),
                                               N.ptr(out), D, N.ptr(arg), N.stream()), "wsi_gin_aggregate_fwd")
        ctx.plan, ctx.mode, ctx.shape = plan, mode, (n, D)
        ctx.save_for_backward(x if (need[1] or need[3]) else None, e, s, arg)
        return out

    @staticmethod
    def backward(ctx, gy):
        x, e, s, arg = ctx.saved_tensors
        plan, mode, (n, D) = ctx.plan, ctx.mode, ctx.shape
        need = ctx.needs_input_grad
        gy = gy if gy.dtype == torch.float32 and gy.is_contiguous() else gy.to(torch.float32).contiguous()
        lib = N.load()
        gx = ge = gb = gs = None
        if need[0]:
            gx = torch.empty((n, D), dtype=torch.float32, device=gy.device)
            N.check(lib.wsi_gin_aggregate_bwd(N.ptr(gy), D, n, D, N.ptr(plan.rowptr), N.ptr(plan.colptr), N.ptr(plan.csc_eid), N.ptr(plan.csc_dst),
                                              N.ptr(s), N.ptr(e), mode, N.ptr(arg), N.ptr(gx), D, N.stream()), "wsi_gin_aggregate_bwd")
        if need[1]:
            ge = torch.zeros_like(e)
            if n > 0:
                partial = torch.empty(lib.wsi_gin_eps_partials(), dtype=torch.float32, device=gy.device)
                N.check(lib.wsi_gin_eps_grad(N.ptr(gy), D, N.ptr(x), D, n, D, N.ptr(partial), N.ptr(ge), N.stream()), "wsi_gin_eps_grad")
        if need[2]:
            gb = gy.sum(0)
        if need[3]:
            gs = torch.zeros_like(s)
            N.check(lib.wsi_gin_edge_grad(N.ptr(gy), D, N.ptr(x), D, n, D, N.ptr(plan.rowptr), N.ptr(plan.src), mode, N.ptr(arg), N.ptr(gs),
                                          N.stream()), "wsi_gin_edge_grad")
        return gx, ge, gb, gs, None, None


def gin_aggregate(x: torch.Tensor, eps: torch.Tensor, plan, mode: str, bias: Optional[torch.Tensor] = None,
                  edge_scale: Optional[torch.Tensor] = None, kernels: Optional[bool] = None) -> torch.Tensor:
    """DGL ``GINConv``'s aggregation as one autograd node: out[w] = (1 + eps) x[w] + reduce_{e: u -> w}(s_e x[u]) (+ bias), reduce = ``mode``
    in sum | mean | max.  mean divides by the in-degree; a node without in-edges gets 0 from every reducer; under max the scale multiplies the
    message before the maximum and the first CSR position wins a tie.  ``eps``: one fp32 value on x's device (a Parameter when it is learned:
    it then receives a gradient; a buffer otherwise: nothing is launched for it).  ``plan``: anything with GraphPlan's rowptr / src / colptr /
    csc_eid / csc_dst / num_nodes / num_edges (``HomoPlan``, ``EdgeCSR``).  ``edge_scale`` [E] in the plan's CSR order (None: the plain
    aggregation) receives a gradient (GNNExplainer's sigmoid(edge_mask): ``graph.message_scale``).  g_x is skipped when x needs none.
    ``kernels=False`` or a CPU tensor: ``gin_aggregate_reference``."""
    _gin_check(x, eps, plan, mode, bias, edge_scale)
    use = x.is_cuda if kernels is None else bool(kernels)
    if not use:
        return gin_aggregate_reference(x, eps, plan, mode, bias, edge_scale)
    return _GinAggregate.apply(x, eps, bias, edge_scale, plan, GIN_MODES[mode])


# ------------------------------------------------------------------------------------------------
# ASAPPooling edge kernels (pooling/ASAP.py:158-179)
# ------------------------------------------------------------------------------------------------
class EdgeCSR:
    """An edge list grouped by the node that aggregates it (CSR: ``rowptr``/``src`` = gathered node per edge) and by the
    gathered node (CSC over the same edge numbering), plus ``perm`` (CSR position -> original edge).  Attribute names
    follow GraphPlan so that ``graph_conv_aggregate`` accepts it; ``in_norm``/``out_norm`` (may stay None = 1) scale the
    aggregating / gathered node."""

    def __init__(self, group: torch.Tensor, other: torch.Tensor, n: int):
        from .graph import _count
        dev = group.device
        E = int(group.numel())
        self.num_nodes, self.num_edges = int(n), E
        perm = torch.sort(group, stable=True).indices if E else group
        g_s, o_s = group[perm], other[perm]
        rowptr = torch.zeros(n + 1, dtype=torch.int64, device=dev)
        colptr = torch.zeros(n + 1, dtype=torch.int64, device=dev)
        if E:
            rowptr[1:] = torch.cumsum(_count(g_s, n), 0)
            colptr[1:] = torch.cumsum(_count(o_s, n), 0)
        cperm = torch.sort(o_s, stable=True).indices if E else o_s
        self.perm = perm
        self.rowptr = rowptr.to(torch.int32).contiguous()
        self.src = o_s.to(torch.int32).contiguous()
        self.colptr = colptr.to(torch.int32).contiguous()
        self.csc_eid = cperm.to(torch.int32).contiguous()
        self.csc_dst = g_s[cperm].to(torch.int32).contiguous() if E else g_s.to(torch.int32)
        self.in_norm = None
        self.out_norm = None
        self.edge_w = None          # optional per-edge weights in CSR order (``with_weights``) ...
        self.edge_w_csc = None      # ... and in CSC order (the backward gathers along it)

    def with_weights(self, w: Optional[torch.Tensor]) -> "EdgeCSR":
        """A shallow copy carrying per-edge weights ``w`` (ORIGINAL edge order; constants: no gradient flows to them) for
        ``graph_conv_aggregate`` (``wsi_spmm_sum``'s edge_w) and ``wsi_stas``."""
        import copy
        if w is not None and w.requires_grad:
            raise RuntimeError("EdgeCSR.with_weights: edge weights are treated as constants (ASAPPooling only ever passes detached values, pooling/ASAP.py:97)")
        c = copy.copy(self)
        if w is None:
            c.edge_w = c.edge_w_csc = None
        else:
            c.edge_w = w.detach().reshape(-1).to(torch.float32)[self.perm].contiguous()
            c.edge_w_csc = c.edge_w[self.csc_eid.long()].contiguous()
        return c


class _CsrGatherMax(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, ec: EdgeCSR):
        N.require_cuda(x)
        x = x.contiguous()
        n, D = ec.num_nodes, x.shape[1]
        out = torch.empty((n, D), dtype=torch.float32, device=x.device)
        arg = torch.empty((n, D), dtype=torch.int32, device=x.device)
        N.check(N.load().wsi_csr_gather_max_fwd(N.ptr(x), D, n, D, N.ptr(ec.rowptr), N.ptr(ec.src), N.ptr(out), D, N.ptr(arg), N.stream()),
                "wsi_csr_gather_max_fwd")
        ctx.ec, ctx.rows = ec, x.shape[0]
        ctx.save_for_backward(arg)
        return out

    @staticmethod
    def backward(ctx, g):
        (arg,) = ctx.saved_tensors
        ec = ctx.ec
        g = g.contiguous()
        D = g.shape[1]
        gx = torch.empty((ctx.rows, D), dtype=torch.float32, device=g.device)
        N.check(N.load().wsi_csr_gather_max_bwd(N.ptr(g), D, N.ptr(arg), ctx.rows, D, N.ptr(ec.colptr), N.ptr(ec.csc_eid), N.ptr(ec.csc_dst),
                                                N.ptr(gx), D, N.stream()), "wsi_csr_gather_max_bwd")
        return gx, None


def csr_gather_max(x: torch.Tensor, ec: EdgeCSR) -> torch.Tensor:
    """out[i] = max over the edges grouped at i of x[j]   (torch_scatter.scatter_max of pooling/ASAP.py:163; 0 for empty groups)."""
    return _CsrGatherMax.apply(x, ec)


class _AsapAttend(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a, b, x, ec: EdgeCSR, slope: float):
        N.require_cuda(a, b, x)
        a_shape, b_shape = a.shape, b.shape
        a, b, x = a.contiguous().view(-1), b.contiguous().view(-1), x.contiguous()
        n, D = ec.num_nodes, x.shape[1]
        out = torch.empty((n, D), dtype=torch.float32, device=x.device)
        score = torch.empty(max(ec.num_edges, 1), dtype=torch.float32, device=x.device)
        N.check(N.load().wsi_asap_attend_fwd(N.ptr(a), N.ptr(b), N.ptr(x), D, n, D, N.ptr(ec.rowptr), N.ptr(ec.src), float(slope),
                                             N.ptr(score), N.ptr(out), D, N.stream()), "wsi_asap_attend_fwd")
        ctx.ec, ctx.slope = ec, float(slope)
        ctx.shapes = (a_shape, b_shape)
        ctx.save_for_backward(a, b, x, score)
        score_orig = torch.empty(ec.num_edges, dtype=torch.float32, device=x.device)
        score_orig[ec.perm] = score[:ec.num_edges]
        ctx.mark_non_differentiable(score_orig)        # the reference detaches it where it is reused (ASAP.py:97)
        return out, score_orig

    @staticmethod
    def backward(ctx, g_out, _g_score):
        a, b, x, score = ctx.saved_tensors
        ec = ctx.ec
        g_out = g_out.contiguous()
        n, D = ec.num_nodes, x.shape[1]
        dev = x.device
        gpre = torch.empty(max(ec.num_edges, 1), dtype=torch.float32, device=dev)
        g_a = torch.empty(n, dtype=torch.float32, device=dev)
        g_b = torch.empty(n, dtype=torch.float32, device=dev)
        gx = torch.empty((n, D), dtype=torch.float32, device=dev)
        N.check(N.load().wsi_asap_attend_bwd(N.ptr(a), N.ptr(b), N.ptr(x), D, n, D, N.ptr(ec.rowptr), N.ptr(ec.src),
                                             N.ptr(ec.colptr), N.ptr(ec.csc_eid), N.ptr(ec.csc_dst), ctx.slope,
                                             N.ptr(score), N.ptr(g_out), D, N.ptr(gpre), N.ptr(g_a), N.ptr(g_b), N.ptr(gx), D, N.stream()),
                "wsi_asap_attend_bwd")
        return g_a.view(ctx.shapes[0]), g_b.view(ctx.shapes[1]), gx, None, None


def asap_attend(a: torch.Tensor, b: torch.Tensor, x: torch.Tensor, ec: EdgeCSR, negative_slope: float):
    """(out [n,D], score [E] in the ORIGINAL edge order) of pooling/ASAP.py:167-179; ``a`` [n] already holds the bias."""
    return _AsapAttend.apply(a, b, x, ec, negative_slope)


# ------------------------------------------------------------------------------------------------
# GAT (DGL GATConv, models/GAT.py:17-92): counter-based feat_drop and the multi-head edge attention
# ------------------------------------------------------------------------------------------------
class _CounterDropoutFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, drop: CounterDropout):
        ctx.drop = drop
        return dropout_apply(x, drop)

    @staticmethod
    def backward(ctx, g):
        return dropout_apply(g, ctx.drop), None


def counter_dropout(x: torch.Tensor, drop: CounterDropout) -> torch.Tensor:
    """nn.Dropout's forward and backward as ``drop``'s counter-based mask (``wsi_dropout_apply`` both ways: no mask tensor)."""
    return _CounterDropoutFn.apply(x, drop)


GAT_ACTIVATIONS = {None: 0, "none": 0, "relu": 1, "leaky_relu": 2}


def _gat_drop_args(drop: Optional[CounterDropout]):
    if drop is None:
        return 0, None, 0, 1.0
    return drop.seed, N.ptr(drop.seed_base), drop.threshold, drop.scale


class _GatAttention(torch.autograd.Function):
    """``edge_scale`` None: wsi_gat_attn_fwd / _bwd.  ``edge_scale`` [E] (CSR order), a per-edge message scale applied after the softmax,
    out = act(sum_e a~_e s_e ft[u] + bias): wsi_gat_attn_fwd_scaled / _bwd_scaled, which take the scale as one more pointer, save it and
    return its gradient as well."""

    @staticmethod
    def forward(ctx, ft, attn_l, attn_r, bias, edge_scale, plan, slope: float, act: int, act_slope: float, drop: Optional[CounterDropout]):
        N.require_cuda(ft, attn_l, attn_r, bias, edge_scale)
        H, D = attn_l.shape[-2], attn_l.shape[-1]
        n = plan.num_nodes
        if ft.dim() != 2 or ft.shape[0] != n or ft.shape[1] != H * D:
            raise ValueError(f"gat_attention: ft must be [{n}, {H * D}], got {tuple(ft.shape)}")
        ft = ft.contiguous()
        al, ar = attn_l.detach().contiguous().view(-1), attn_r.detach().contiguous().view(-1)
        b = bias.detach().contiguous() if bias is not None else None
        s = (edge_scale.detach().to(torch.float32).contiguous(),) if edge_scale is not None else ()
        dev = ft.device
        lib = N.load()
        eler = torch.empty((n, 2 * H), dtype=torch.float32, device=dev)
        N.check(lib.wsi_gat_scores(N.ptr(ft), H * D, n, H, D, N.ptr(al), N.ptr(ar), N.ptr(eler), N.stream()), "wsi_gat_scores")
        out = torch.empty((n, H * D), dtype=torch.float32, device=dev)
        lse = torch.empty((n, 2 * H), dtype=torch.float32, device=dev)       # max | log of the shifted sum, per head
        seed, seed_base, thr, scale = _gat_drop_args(drop)
        fwd, what = (lib.wsi_gat_attn_fwd_scaled, "wsi_gat_attn_fwd_scaled") if s else (lib.wsi_gat_attn_fwd, "wsi_gat_attn_fwd")
        N.check(fwd(N.ptr(ft), H * D, N.ptr(eler), n, H, D, N.ptr(plan.rowptr), N.ptr(plan.src), N.ptr(plan.order_dst),
                    float(slope), seed, seed_base, thr, scale, N.ptr(b), int(act), float(act_slope), *map(N.ptr, s),
                    N.ptr(out), H * D, N.ptr(lse), N.stream()), what)
        ctx.plan, ctx.slope, ctx.act, ctx.act_slope, ctx.drop, ctx.hd = plan, float(slope), int(act), float(act_slope), drop, (H, D)
        ctx.has_bias = bias is not None
        ctx.save_for_backward(ft, al, ar, eler, lse, *s, out if act else None)
        return out

    @staticmethod
    def backward(ctx, g_out):
        ft, al, ar, eler, lse, *s, out = ctx.saved_tensors
        plan = ctx.plan
        H, D = ctx.hd
        n, E, F = plan.num_nodes, plan.num_edges, H * D
        g_out = g_out.contiguous()
        dev = ft.device
        lib = N.load()
        ws_bytes = lib.wsi_gat_attn_bwd_workspace_bytes(n, E, H, D, ctx.act)
        if ws_bytes < 0:
            raise RuntimeError("wsi_gat_attn_bwd_workspace_bytes: bad arguments")
        ws = torch.empty(max(int(ws_bytes), 1), dtype=torch.uint8, device=dev)
        g_ft = torch.empty((n, F), dtype=torch.float32, device=dev)
        g_al = torch.empty(F, dtype=torch.float32, device=dev)
        g_ar = torch.empty(F, dtype=torch.float32, device=dev)
        g_b = torch.empty(F, dtype=torch.float32, device=dev) if ctx.has_bias else None
        g_s = tuple(torch.empty(max(E, 1), dtype=torch.float32, device=dev)[:E] for _ in s)
        seed, seed_base, thr, scale = _gat_drop_args(ctx.drop)
        bwd, what = (lib.wsi_gat_attn_bwd_scaled, "wsi_gat_attn_bwd_scaled") if s else (lib.wsi_gat_attn_bwd, "wsi_gat_attn_bwd")
        N.check(bwd(N.ptr(ft), F, N.ptr(eler), N.ptr(lse), N.ptr(out), F, N.ptr(g_out), F, n, E, H, D,
                    N.ptr(plan.rowptr), N.ptr(plan.src), N.ptr(plan.colptr), N.ptr(plan.csc_eid), N.ptr(plan.csc_dst),
                    N.ptr(plan.order_src), N.ptr(al), N.ptr(ar), ctx.slope, seed, seed_base, thr, scale, ctx.act, ctx.act_slope,
                    *map(N.ptr, s), N.ptr(ws), int(ws_bytes), N.ptr(g_ft), F, N.ptr(g_al), N.ptr(g_ar), N.ptr(g_b), *map(N.ptr, g_s),
                    N.stream()), what)
        return g_ft, g_al.view(1, H, D), g_ar.view(1, H, D), g_b, (g_s[0] if s else None), None, None, None, None, None


def gat_attention(ft: torch.Tensor, attn_l: torch.Tensor, attn_r: torch.Tensor, bias: Optional[torch.Tensor], plan,
                  negative_slope: float, activation: Optional[str] = None, attn_drop: Optional[CounterDropout] = None,
                  act_slope: float = 0.01, edge_scale: Optional[torch.Tensor] = None) -> torch.Tensor:
    """DGL GATConv after its projection: ``ft`` [N, H*D] (head-major rows), ``attn_l`` / ``attn_r`` [1, H, D], ``bias`` [H*D] or None;
    ``plan`` = the graph's homogeneous GraphPlan (CSR by destination, CSC by source, walk orders).  Returns act(sum_e a_e ft[src] + bias)
    [N, H*D] where a = edge softmax of leaky_relu(el[src] + er[dst], negative_slope) over each destination's in-edges, dropped by
    ``attn_drop`` (a CounterDropout over the [E, H] scores: row = CSR edge id, column = head; None = no dropout).  ``activation``:
    None, "relu" or "leaky_relu" (slope ``act_slope``), fused into the kernel.  ``edge_scale`` [E] (CSR edge order; None = the plain
    attention, unchanged): every message a_e ft[src] is multiplied by it AFTER the softmax and it receives a gradient (GNNExplainer's
    sigmoid(edge_mask): ``graph.message_scale``)."""
    if activation not in GAT_ACTIVATIONS:
        raise ValueError(f"gat_attention: activation {activation!r} is not one of {sorted(k for k in GAT_ACTIVATIONS if k)}")
    if attn_l.dim() != 3 or attn_l.shape[0] != 1 or attn_r.shape != attn_l.shape:
        raise ValueError("gat_attention: attn_l / attn_r must be [1, H, D]")
    if edge_scale is not None:
        _check_edge_scale("gat_attention", edge_scale, plan)
    return _GatAttention.apply(ft, attn_l, attn_r, bias, edge_scale, plan, float(negative_slope), GAT_ACTIVATIONS[activation], float(act_slope), attn_drop)


# ------------------------------------------------------------------------------------------------
# train-time graph augmentation (wsi_augment_* / wsi_gather_rows_masked; the draw contract is in include/wsi_hgnn.h)
# ------------------------------------------------------------------------------------------------
AUG_TILE = 1024
AUG_KINDS = ("drop_node", "drop_edge", "node_shuffle", "feat_mask")


def _fmix32(h: int) -> int:
    h &= 0xffffffff
    h ^= h >> 16
    h = (h * 0x85EBCA6B) & 0xffffffff
    h ^= h >> 13
    h = (h * 0xC2B2AE35) & 0xffffffff
    h ^= h >> 16
    return h


def augment_subseed(seed: int, k: int, j: int) -> int:
    """sub(seed, k, j) of the draw contract: transform number ``k`` of the pipeline acting on stream ``j`` (host integers)."""
    return _fmix32(_fmix32(int(seed) + (int(k) + 1) * 0x9E3779B1) + (int(j) + 1) * 0x85EBCA6B)


def augment_threshold(p: float) -> int:
    if not 0.0 <= p <= 1.0:
        raise ValueError("probability must be in [0, 1]")
    return int(round(float(p) * 65536.0))


def augment_hash(n: int, sub: int, device="cpu") -> torch.Tensor:
    """h(i) = fmix32(i * 0x9E3779B1 + sub) for i < n as an int64 tensor of 32-bit values: the contract replayed with integer tensor arithmetic
    (any device; independent of the kernels)."""
    i = torch.arange(int(n), dtype=torch.int64, device=device)
    h = (_mul32(i & 0xffffffff, 0x9E3779B1) + int(sub)) & 0xffffffff
    h = h ^ (h >> 16)
    h = _mul32(h, 0x85EBCA6B)
    h = h ^ (h >> 13)
    h = _mul32(h, 0xC2B2AE35)
    return h ^ (h >> 16)


def augment_drawn(n: int, sub: int, threshold: int, device="cpu") -> torch.Tensor:
    """Boolean [n]: element i is removed / zeroed by a Bernoulli(threshold / 65536) draw of stream ``sub``."""
    return (augment_hash(n, sub, device) & 0xffff) < int(threshold)


def mask_columns(x: torch.Tensor, sub: int, threshold: int) -> torch.Tensor:
    """FeatMask on one field as tensor operations: a copy of ``x`` with the drawn columns (last dimension) set to 0."""
    if x.dim() < 2:
        raise ValueError("FeatMask needs a field with a feature dimension (at least 2-D)")
    out = x.clone()
    if threshold:
        out[..., augment_drawn(x.shape[-1], sub, threshold, x.device)] = 0
    return out


def gather_rows_masked(x: torch.Tensor, row_of: Optional[torch.Tensor], mask_seed: int = 0, mask_threshold: int = 0) -> torch.Tensor:
    """out[i, c] = zeroed(c) ? 0 : x[row_of[i], c] (``wsi_gather_rows_masked``): x fp32 [n, F] with unit column stride, row_of int64 [rows] or
    None (= every row in place)."""
    N.require_cuda(x, row_of)
    if x.dim() != 2 or x.dtype != torch.float32 or (x.shape[1] > 1 and x.stride(1) != 1):
        raise ValueError("gather_rows_masked: an fp32 [n, F] table with contiguous rows")
    rows = x.shape[0] if row_of is None else int(row_of.numel())
    if row_of is not None:
        row_of = row_of.to(torch.int64).contiguous()
    out = torch.empty((rows, x.shape[1]), dtype=torch.float32, device=x.device)
    with _Timed("augment_gather"):
        N.check(N.load().wsi_gather_rows_masked(N.ptr(x), x.stride(0) if x.shape[0] > 1 else max(x.shape[1], 1), x.shape[0], N.ptr(row_of), N.ptr(out),
                                                max(x.shape[1], 1), rows, x.shape[1], int(mask_seed) & 0xffffffff, int(mask_threshold), N.stream()),
                "wsi_gather_rows_masked")
    return out


def _segment_rows(counts: Sequence[int], extra) -> Tuple[List[int], int, List[int]]:
    """Descriptor rows [n, off, first_tile, *extra(j)] of consecutive segments; returns (words, tiles, offsets)."""
    words, off, tiles, offs = [], 0, 0, []
    for j, n in enumerate(counts):
        words += [int(n), off, tiles] + list(extra(j))
        offs.append(off)
        off += int(n)
        tiles += (int(n) + AUG_TILE - 1) // AUG_TILE
    return words, tiles, offs


def _shuffle_perms(counts: Sequence[int], subs: Sequence[int], dev) -> List[torch.Tensor]:
    """NodeShuffle's permutation of every node type: the 32-bit hash keys of all types in one table ((type << 32) | key), ONE stable sort."""
    idx, offs = segment_hash_order(counts, subs, dev)
    return [idx[a:a + c] - a for a, c in zip(offs, counts)]


def segment_hash_order(counts: Sequence[int], subs: Sequence[int], dev) -> Tuple[torch.Tensor, List[int]]:
    """(order, offsets): the elements of consecutive segments (``counts`` each, segment j starting at offsets[j]) in the stable ascending order
    of their draw ``augment_hash(i, subs[j])`` - order[offsets[j] + r] is the position in the whole table of segment j's r-th element."""
    total = sum(counts)
    words, tiles, offs = _segment_rows(counts, lambda j: (subs[j], 0, 0))
    keys = torch.empty(total, dtype=torch.int64, device=dev)
    if total:
        desc = host_to_device(words, torch.int64, dev)
        N.check(N.load().wsi_augment_keys(N.ptr(desc), len(counts), tiles, N.ptr(keys), N.stream()), "wsi_augment_keys")
    return torch.sort(keys, stable=True).indices, offs


def augment_graph(g, stages, seed: int):
    """The fused device path of ``transforms``: at most one each of DropNode, DropEdge, NodeShuffle and FeatMask, in ANY order, applied to a
    single graph on the GPU with a launch count that does not depend on how many of them there are.  ``stages``: tuples
    ``(kind, k, p, node_names, edge_names)`` in pipeline order, ``kind`` one of ``AUG_KINDS``, ``k`` the transform's number in the pipeline.
    The result equals the members applied one after another (transforms.py's tensor formulation) bit for bit.

    Node ids come from one flag + scan pass over all node types, the surviving edges from two over all relations (endpoints, then DropEdge by
    rank), every fp32 [n, F] node field from ONE gather through the composed row index with the column mask applied on the way; the other
    fields follow by indexing.  One device->host read-back per call: the [T] node and [R] edge counts together (HeteroGraph keeps counts on the
    host); none when neither DropNode nor DropEdge is present."""
    from collections import OrderedDict
    from .graph import HeteroGraph
    kinds = [s[0] for s in stages]
    if any(k not in AUG_KINDS for k in kinds) or len(set(kinds)) != len(kinds):
        raise ValueError(f"augment_graph fuses at most one each of {AUG_KINDS}; got {kinds}")
    if g._batch_num_nodes is not None and g.batch_size > 1:
        raise ValueError("graph transforms work on single graphs (augment the slides, then batch them)")
    dev = g.device
    if dev.type != "cuda":
        raise RuntimeError("ops.augment_graph runs on the GPU only (HIP kernels); transforms.py holds the CPU formulation")
    g = g.to(dev)
    lib = N.load()
    order = {s[0]: i for i, s in enumerate(stages)}
    st = {s[0]: s for s in stages}
    ntypes, rels = g.ntypes, g.canonical_etypes
    T, R = len(ntypes), len(rels)
    tindex = {t: i for i, t in enumerate(ntypes)}
    n = [g.num_nodes(t) for t in ntypes]
    edges = g._edges
    e = [int(edges[r][0].numel()) for r in rels]
    Ntot, Etot = sum(n), sum(e)
    if Ntot >= 2 ** 31 - 1 or Etot >= 2 ** 31 - 1:
        raise ValueError("graph too large for the int32 augmentation kernels")
    dn, de, ns, fm = (st.get(k) for k in AUG_KINDS)
    dn_thr = augment_threshold(dn[2]) if dn is not None else 0
    de_thr = augment_threshold(de[2]) if de is not None else 0
    fm_thr = augment_threshold(fm[2]) if fm is not None else 0
    node_changed, edge_changed = dn_thr > 0, dn_thr > 0 or de_thr > 0
    counts_dev = torch.zeros(T + R, dtype=torch.int32, device=dev)
    i32 = lambda m: torch.empty(max(int(m), 1), dtype=torch.int32, device=dev)
    i64 = lambda m: torch.empty(max(int(m), 1), dtype=torch.int64, device=dev)
    with _Timed("augment_index"):
        new_id = kept = None
        if node_changed:
            words, tiles, noff = _segment_rows(n, lambda j: (augment_subseed(seed, dn[1], j), dn_thr, 0))
            desc_n = host_to_device(words, torch.int64, dev)
            new_id, kept, tsum_n = i32(Ntot), i64(Ntot), i32(tiles + 1)
            N.check(lib.wsi_augment_nodes(N.ptr(desc_n), T, tiles, N.ptr(tsum_n), N.ptr(new_id), N.ptr(kept), N.ptr(counts_dev), N.stream()),
                    "wsi_augment_nodes")
        else:
            _, _, noff = _segment_rows(n, lambda j: ())
        sim_in_kernel = {}
        if edge_changed and R > 0:
            by_rank = 1 if (node_changed and de_thr > 0 and order["drop_edge"] > order["drop_node"]) else 0
            uv = [(edges[r][0].contiguous(), edges[r][1].contiguous()) for r in rels]
            sims = []
            for r, m in zip(rels, e):
                x = g._eframes[r].get("sim")
                ok = x is not None and x.dtype == torch.float32 and x.dim() == 1 and x.numel() == m and x.is_contiguous()
                sims.append(x if ok else None)
                sim_in_kernel[r] = ok

            def extra(j):
                s, _, d = rels[j]
                return (uv[j][0].data_ptr(), uv[j][1].data_ptr(), 0 if sims[j] is None else sims[j].data_ptr(), noff[tindex[s]], noff[tindex[d]],
                        augment_subseed(seed, de[1], j) if de is not None else 0, de_thr, by_rank, n[tindex[s]], n[tindex[d]], 0)

            words, tiles, eoff = _segment_rows(e, extra)
            desc_e = host_to_device(words, torch.int64, dev)
            out_u, out_v, out_eid = i64(Etot), i64(Etot), i64(Etot)
            out_sim = torch.empty(max(Etot, 1), dtype=torch.float32, device=dev)
            tsum_e, rank1 = i32(2 * (tiles + 1)), i32(Etot)             # (scratch held in names: two temporaries could share one block)
            N.check(lib.wsi_augment_edges(N.ptr(desc_e), R, tiles, N.ptr(new_id), N.ptr(tsum_e), N.ptr(rank1), N.ptr(out_u), N.ptr(out_v),
                                          N.ptr(out_sim), N.ptr(out_eid), N.ptr(counts_dev[T:]), N.stream()), "wsi_augment_edges")
        shuffle_first = ns is not None and (not node_changed or order["node_shuffle"] < order["drop_node"])
        perms = None
        if shuffle_first:
            perms = _shuffle_perms(n, [augment_subseed(seed, ns[1], j) for j in range(T)], dev)
        if node_changed or (edge_changed and R > 0):
            got = counts_dev.tolist()           # THE read-back: [T] node counts and [R] edge counts in one copy
        n2 = got[:T] if node_changed else n
        e2 = got[T:] if (edge_changed and R > 0) else e
        if ns is not None and not shuffle_first:
            perms = _shuffle_perms(n2, [augment_subseed(seed, ns[1], j) for j in range(T)], dev)
        row_of = []
        for j in range(T):
            kj = kept[noff[j]:noff[j] + n2[j]] if node_changed else None
            if perms is None:
                row_of.append(kj)
            elif kj is None:
                row_of.append(perms[j])
            else:
                row_of.append(perms[j][kj] if shuffle_first else kj[perms[j]])
    new_edges = OrderedDict()
    for j, r in enumerate(rels):
        if edge_changed:
            new_edges[r] = (out_u[eoff[j]:eoff[j] + e2[j]], out_v[eoff[j]:eoff[j] + e2[j]])
        else:
            new_edges[r] = edges[r]
    out = HeteroGraph(OrderedDict(zip(ntypes, n2)), new_edges)
    node_names = list(fm[3] or []) if fm is not None else []
    edge_names = list(fm[4] or []) if fm is not None else []
    for j, t in enumerate(ntypes):
        for key, x in g._nframes[t].items():
            if key == "_pos" and ns is not None:
                continue                        # the locality positions describe the topology, not the rows that now sit on it
            masked = key in node_names and fm_thr > 0
            sub = augment_subseed(seed, fm[1], 65536 * node_names.index(key) + j) if masked else 0
            if masked and x.dim() < 2:
                raise ValueError("FeatMask needs a field with a feature dimension (at least 2-D)")
            if row_of[j] is None and not masked:
                out._nframes[t][key] = x
            elif x.dim() == 2 and x.dtype == torch.float32 and (x.shape[1] <= 1 or x.stride(1) == 1):
                out._nframes[t][key] = gather_rows_masked(x, row_of[j], sub, fm_thr if masked else 0)
            else:
                y = x if row_of[j] is None else x[row_of[j]]
                out._nframes[t][key] = mask_columns(y, sub, fm_thr) if masked else y
    for j, r in enumerate(rels):
        for key, x in g._eframes[r].items():
            masked = key in edge_names and fm_thr > 0
            if not edge_changed:
                y = x
            elif key == "sim" and sim_in_kernel.get(r):
                y = out_sim[eoff[j]:eoff[j] + e2[j]]
            else:
                y = x[out_eid[eoff[j]:eoff[j] + e2[j]]]
            out._eframes[r][key] = mask_columns(y, augment_subseed(seed, fm[1], 65536 * edge_names.index(key) + 32768 + j), fm_thr) if masked else y
    return out


# ------------------------------------------------------------------------------------------------
# leave-one-node-out batches (csrc/loo.hip; graph.leave_one_out_batch)
# ------------------------------------------------------------------------------------------------
_LOO_NEVER = 2 ** 63 - 1        # "no node of this side is removed": never equal to an id, never below one


def leave_one_out_batch(g, nids: Sequence[int], ntype: str, tables, check: bool = False):
    """The device path of ``graph.leave_one_out_batch`` (which validates the arguments): B = len(nids) copies of the single graph ``g``, copy b
    without node ``nids[b]`` of ``ntype``, as ONE block-diagonal ``HeteroGraph`` equal to ``batch([remove_nodes(g, [i], ntype) for i in nids])``.

    Edges: one ``wsi_loo_edges`` call over a descriptor row per (relation, copy) writes the renumbered survivors of every copy straight into the
    batch's relation-major, copy-major edge arrays (+ ``sim`` and the original edge index for the other edge fields); every row's offset and
    capacity comes from ``tables``.  Nodes: one ``wsi_loo_rows`` launch writes the source row of every node of the batch; fp32 [n, F] fields go
    through ``gather_rows_masked``, the rest through indexing.  One small upload, no device->host read (``check=True``: one, of the counts)."""
    from collections import OrderedDict
    from .graph import HeteroGraph
    dev = g.device
    if dev.type != "cuda":
        raise RuntimeError("ops.leave_one_out_batch runs on the GPU only (HIP kernels); graph.leave_one_out_batch composes CPU graphs")
    g = g.to(dev)
    lib = N.load()
    ntypes, rels = g.ntypes, g.canonical_etypes
    T, R, B = len(ntypes), len(rels), len(nids)
    n = [g.num_nodes(t) for t in ntypes]
    per = [m - (1 if t == ntype else 0) for t, m in zip(ntypes, n)]             # nodes of every type in ONE copy
    tindex = {t: i for i, t in enumerate(ntypes)}
    edges = g._edges
    e = [int(edges[r][0].numel()) for r in rels]
    surv = [tables.surviving_edges(i) for i in nids]                            # [B][R]
    etot = [sum(surv[b][j] for b in range(B)) for j in range(R)]
    Etot, Ntot = sum(etot), B * sum(per)
    tiles_e = B * sum((m + AUG_TILE - 1) // AUG_TILE for m in e)
    if Ntot >= 2 ** 31 - 1 or Etot >= 2 ** 31 - 1 or B * sum(e) >= 2 ** 31 - 1 or tiles_e >= 2 ** 31 - 1:
        raise ValueError("batch too large for the int32 leave-one-out kernels")
    uv = [(edges[r][0].contiguous(), edges[r][1].contiguous()) for r in rels]
    sims = []
    for r, m in zip(rels, e):
        x = g._eframes[r].get("sim")
        sims.append(x if (x is not None and x.dtype == torch.float32 and x.dim() == 1 and x.numel() == m and x.is_contiguous()) else None)
    # ---- descriptor tables: edge rows, node rows and the removed ids in one upload
    words, roff, off, tiles = [], [], 0, 0
    for j, (s, _, d) in enumerate(rels):
        roff.append(off)
        for b in range(B):
            words += [e[j], off, tiles, uv[j][0].data_ptr(), uv[j][1].data_ptr(), 0 if sims[j] is None else sims[j].data_ptr(),
                      nids[b] if s == ntype else _LOO_NEVER, nids[b] if d == ntype else _LOO_NEVER,
                      b * per[tindex[s]], b * per[tindex[d]], surv[b][j], 0]
            off += surv[b][j]
            tiles += (e[j] + AUG_TILE - 1) // AUG_TILE
    nwords, noff, no, ntiles_n = [], [], 0, 0
    for j, t in enumerate(ntypes):
        nwords += [B * per[j], no, ntiles_n, per[j], 1 if t == ntype else 0, 0]
        noff.append(no)
        no += B * per[j]
        ntiles_n += (B * per[j] + AUG_TILE - 1) // AUG_TILE
    desc = host_to_device(words + nwords + list(nids), torch.int64, dev)
    desc_n, removed = desc[len(words):], desc[len(words) + len(nwords):]
    i64 = lambda m: torch.empty(max(int(m), 1), dtype=torch.int64, device=dev)
    with _Timed("loo_index"):
        out_u, out_v, out_eid = i64(Etot), i64(Etot), i64(Etot)
        out_sim = torch.empty(max(Etot, 1), dtype=torch.float32, device=dev)
        tsum = torch.empty(tiles + 1, dtype=torch.int32, device=dev)
        counts = torch.empty(max(R * B, 1), dtype=torch.int32, device=dev)
        if R > 0:
            N.check(lib.wsi_loo_edges(N.ptr(desc), R * B, tiles, N.ptr(tsum), N.ptr(out_u), N.ptr(out_v), N.ptr(out_sim), N.ptr(out_eid),
                                      N.ptr(counts), N.stream()), "wsi_loo_edges")
        row_of = i64(Ntot)
        N.check(lib.wsi_loo_rows(N.ptr(desc_n), T, ntiles_n, N.ptr(removed), B, N.ptr(row_of), N.stream()), "wsi_loo_rows")
    if check and R > 0:
        got, want = counts[:R * B].tolist(), [surv[b][j] for j in range(R) for b in range(B)]
        if got != want:
            bad = [(rels[k // B], nids[k % B], want[k], got[k]) for k in range(R * B) if got[k] != want[k]]
            raise RuntimeError(f"leave_one_out_batch: the kernel's surviving edge counts differ from the tables' prediction "
                               f"(relation, removed node, predicted, found): {bad[:8]}")
    out = HeteroGraph(OrderedDict((t, B * per[j]) for j, t in enumerate(ntypes)),
                      OrderedDict((r, (out_u[roff[j]:roff[j] + etot[j]], out_v[roff[j]:roff[j] + etot[j]])) for j, r in enumerate(rels)),
                      {t: torch.full((B,), per[j], dtype=torch.int64) for j, t in enumerate(ntypes)})
    for j, t in enumerate(ntypes):
        rows = row_of[noff[j]:noff[j] + B * per[j]]
        for key, x in g._nframes[t].items():
            if x.dim() == 2 and x.dtype == torch.float32 and (x.shape[1] <= 1 or x.stride(1) == 1):
                out._nframes[t][key] = gather_rows_masked(x, rows, 0, 0)
            else:
                out._nframes[t][key] = x[rows]
    for j, r in enumerate(rels):
        for key, x in g._eframes[r].items():
            if key == "sim" and sims[j] is not None:
                out._eframes[r][key] = out_sim[roff[j]:roff[j] + etot[j]]
            else:
                out._eframes[r][key] = x[out_eid[roff[j]:roff[j] + etot[j]]]
    out._loo_desc = desc                # (the descriptor table must outlive the launches that read it: held by the graph)
    return out


# ------------------------------------------------------------------------------------------------
# GTNMIL (wsi_hgnn_amd.gtn): the mincut assignment over a sparse adjacency (wsi_mincut_*), the pooled products s^T [x | s] on the grouped
# GEMMs, and the attention of the short-sequence transformer (wsi_seq_attn_*)
# ------------------------------------------------------------------------------------------------
SEQ_ATTN_MAX_N = 128
SEQ_ATTN_HEAD_DIMS = (8, 16)


def _mincut_check(logits: torch.Tensor, ec: "EdgeCSR", rp: ReducePlan) -> None:
    if logits.dim() != 2 or logits.dtype != torch.float32 or logits.shape[1] < 1:
        raise ValueError(f"mincut_assign: logits are an fp32 [rows, K >= 1] table, got {tuple(logits.shape)} {logits.dtype}")
    if rp.first_row != 0 or rp.num_rows != logits.shape[0] or ec.num_nodes != logits.shape[0]:
        raise ValueError(f"mincut_assign: {logits.shape[0]} rows of logits, a plan over {rp.num_rows} rows, an adjacency over {ec.num_nodes}")


class _MincutAssign(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, ec: "EdgeCSR", rp: ReducePlan):
        N.require_cuda(logits)
        _mincut_check(logits, ec, rp)
        z = logits if (logits.shape[1] == 1 or logits.stride(1) == 1) and logits.stride(0) >= logits.shape[1] else logits.contiguous()
        n, K = z.shape
        dev = z.device
        lib = N.load()
        s = torch.empty((n, K), dtype=torch.float32, device=dev)
        t = torch.empty((n, K), dtype=torch.float32, device=dev)
        deg = torch.empty(max(n, 1), dtype=torch.float32, device=dev)
        num = torch.empty(rp.num_segs, dtype=torch.float32, device=dev)
        den = torch.empty(rp.num_segs, dtype=torch.float32, device=dev)
        partial = torch.empty(max(lib.wsi_mincut_partials(rp.num_chunks), 1), dtype=torch.float32, device=dev)
        with _Timed("mincut_fwd"):
            N.check(lib.wsi_mincut_fwd(N.ptr(z), z.stride(0) if n > 1 else K, n, K, N.ptr(ec.rowptr), N.ptr(ec.src), N.ptr(ec.edge_w),
                                       N.ptr(rp.chunk_row), rp.num_chunks, N.ptr(rp.seg_chunk), rp.num_segs, N.ptr(s), N.ptr(t), N.ptr(deg),
                                       N.ptr(partial), N.ptr(num), N.ptr(den), N.stream()), "wsi_mincut_fwd")
        ctx.ec, ctx.rp, ctx.deg = ec, rp, deg
        ctx.save_for_backward(s, t)
        ctx.mark_non_differentiable(t)
        return s, num, den, t

    @staticmethod
    def backward(ctx, g_s, g_num, g_den, _g_t):
        if not ctx.needs_input_grad[0]:
            return None, None, None
        s, t = ctx.saved_tensors
        ec, rp = ctx.ec, ctx.rp
        n, K = s.shape
        if g_s is not None and not ((K == 1 or g_s.stride(1) == 1) and g_s.stride(0) >= K):
            g_s = g_s.contiguous()
        g_num = g_num.contiguous() if g_num is not None else None
        g_den = g_den.contiguous() if g_den is not None else None
        g_z = torch.empty((n, K), dtype=torch.float32, device=s.device)
        with _Timed("mincut_bwd"):
            N.check(N.load().wsi_mincut_bwd(N.ptr(g_s), (g_s.stride(0) if n > 1 else K) if g_s is not None else 0, N.ptr(g_num), N.ptr(g_den),
                                            N.ptr(s), N.ptr(t), N.ptr(ctx.deg), n, K, N.ptr(ec.colptr), N.ptr(ec.csc_dst), N.ptr(ec.edge_w_csc),
                                            N.ptr(rp.chunk_row), N.ptr(rp.chunk_seg), rp.num_chunks, N.ptr(g_z), N.stream()), "wsi_mincut_bwd")
        return g_z, None, None


def mincut_assign_t(logits: torch.Tensor, ec: "EdgeCSR", rp: ReducePlan):
    """``mincut_assign`` together with t = A s [rows, K] (not differentiable): what ``gtn.dense_mincut_pool`` forms s^T A s = s^T t from."""
    return _MincutAssign.apply(logits, ec, rp)


def mincut_assign(logits: torch.Tensor, ec: "EdgeCSR", rp: ReducePlan):
    """(s, num, den) of torch_geometric's dense_mincut_pool over a SPARSE adjacency in the packed layout: ``logits`` [rows, K <= 128] fp32, the
    rows of all graphs one after the other (``rp``: one segment per graph); ``ec`` = ``EdgeCSR(group=row, other=column, n=rows)``, optionally
    ``with_weights`` (constants; repeated entries add up, rows may be empty, nothing is assumed symmetric).
    s = softmax(logits, -1);  num[g] = trace(s^T A s) and den[g] = trace(s^T D s) over the rows of graph g, D = diag(A.sum(-1)).  All three are
    differentiable in ``logits`` through one backward launch; identical calls give identical bits."""
    return _MincutAssign.apply(logits, ec, rp)[:3]


class _PoolTN(torch.autograd.Function):
    """out[g] = s_g^T [x_g | s_g] ([K, D + K]) for every graph g of the plan: one grouped TN GEMM in exact fp32; the backward is one grouped NT
    GEMM (the gradient through the left factor) and one grouped NN GEMM (through the right one)."""

    @staticmethod
    def forward(ctx, s, x, rp: ReducePlan):
        N.require_cuda(s, x)
        s = s.contiguous()
        xs = torch.cat([x, s], 1)
        K, W, dev = s.shape[1], xs.shape[1], s.device
        out = torch.zeros((rp.num_segs, K, W), dtype=torch.float32, device=dev) if rp.has_empty() else \
            torch.empty((rp.num_segs, K, W), dtype=torch.float32, device=dev)
        gemm_tn_fp32([dict(A=N.ptr(s, a * K * 4), lda=K, B=N.ptr(xs, a * W * 4), ldb=W, C=N.ptr(out, g * K * W * 4), ldc=W, M=K, N=W, K=b - a)
                      for g, (a, b) in enumerate(rp.ranges) if b > a], dev)
        ctx.rp, ctx.D = rp, x.shape[1]
        ctx.save_for_backward(s, xs)
        return out

    @staticmethod
    def backward(ctx, g_out):
        s, xs = ctx.saved_tensors
        rp, D = ctx.rp, ctx.D
        g_out = g_out.contiguous()
        K, W, dev = s.shape[1], xs.shape[1], s.device
        live = [(g, a, b) for g, (a, b) in enumerate(rp.ranges) if b > a]
        # through the right factor: g_xs_g = s_g g_out_g   ([n_g, K] x [K, W])
        g_xs = torch.empty_like(xs)
        _gemm(N.WSI_GEMM_NN, 0, [dict(A=N.ptr(s, a * K * 4), lda=K, B=N.ptr(g_out, g * K * W * 4), ldb=W, C=N.ptr(g_xs, a * W * 4), ldc=W,
                                      M=b - a, N=W, K=K) for g, a, b in live], dev)
        # through the left factor: g_s_g = xs_g g_out_g^T   ([n_g, W] x [K, W]^T)
        g_s = torch.empty_like(s)
        _gemm(N.WSI_GEMM_NT, 0, [dict(A=N.ptr(xs, a * W * 4), lda=W, B=N.ptr(g_out, g * K * W * 4), ldb=W, C=N.ptr(g_s, a * K * 4), ldc=K,
                                      M=b - a, N=K, K=W) for g, a, b in live], dev)
        g_s = g_s + g_xs[:, D:]
        return g_s, (g_xs[:, :D] if ctx.needs_input_grad[1] else None), None


def mincut_pool_products(s: torch.Tensor, x: torch.Tensor, rp: ReducePlan):
    """(s^T x [G, K, D], s^T s [G, K, K]) per graph of the plan from ONE grouped TN GEMM over [x | s] in exact fp32 (``gemm_tn_fp32``)."""
    if rp.first_row != 0 or rp.num_rows != s.shape[0] or x.shape[0] != s.shape[0]:
        raise ValueError(f"mincut_pool_products: a plan over {rp.num_rows} rows, s has {s.shape[0]}, x has {x.shape[0]}")
    out = _PoolTN.apply(s, x, rp)
    return out[:, :, :x.shape[1]], out[:, :, x.shape[1]:]


# ------------------------------------------------------------------------------------------------
# BatchNorm1d over the live rows of a padded table (wsi_masked_bn_fwd / _bwd: gtn.GCNBlock on a gtn.GraphSlot)
# ------------------------------------------------------------------------------------------------
_FUSED_BN_RELU = {"enabled": True}


def set_fused_bn_relu(on: bool) -> None:
    """On (default): ``masked_batch_norm(relu=True)`` on the GPU is ``wsi_masked_bn_relu_fwd`` / ``_bwd`` - the ReLU inside the normalise,
    gradient-sum and dx passes.  Off: the composite, ``wsi_masked_bn_fwd`` followed by ``F.relu`` - the same bits, one more read
    and write of the table forward, two reads and one write backward; for A/B measurements.  Host state, no environment variable."""
    _FUSED_BN_RELU["enabled"] = bool(on)


def fused_bn_relu() -> bool:
    return _FUSED_BN_RELU["enabled"]


class _MaskedBatchNorm(torch.autograd.Function):
    @staticmethod
    def forward(ctx, y, live, live_rows, weight, bias, running_mean, running_var, training: bool, momentum: float, eps: float,
                relu: bool = False):
        N.require_cuda(y, live, live_rows, weight, bias, running_mean, running_var)
        x = y if y.dtype == torch.float32 and (y.shape[1] == 1 or y.stride(1) == 1) and y.stride(0) >= y.shape[1] else y.to(torch.float32).contiguous()
        rows, C = x.shape
        dev, lib = x.device, N.load()
        w = None if weight is None else weight.detach().contiguous()
        b = None if bias is None else bias.detach().contiguous()
        out = torch.empty((rows, C), dtype=torch.float32, device=dev)
        stats = torch.empty((2, C), dtype=torch.float32, device=dev)
        partial = torch.empty(max(3 * lib.wsi_masked_bn_chunks(rows) * C, 1), dtype=torch.float32, device=dev) if training else None
        fwd = lib.wsi_masked_bn_relu_fwd if relu else lib.wsi_masked_bn_fwd
        N.check(fwd(N.ptr(x), x.stride(0) if rows > 1 else C, rows, C, N.ptr(live), N.ptr(live_rows), N.ptr(w), N.ptr(b),
                    N.ptr(running_mean), N.ptr(running_var), 1 if training else 0, float(momentum), float(eps), N.ptr(partial),
                    N.ptr(stats), N.ptr(out), C, N.stream()), "wsi_masked_bn_relu_fwd" if relu else "wsi_masked_bn_fwd")
        ctx.training, ctx.has_w, ctx.has_b, ctx.relu = training, weight is not None, bias is not None, relu
        ctx.save_for_backward(x, live, live_rows, w, stats, b if relu else None)      # (relu: the backward recomputes y's sign, which needs beta)
        return out

    @staticmethod
    def backward(ctx, g):
        x, live, live_rows, w, stats, b = ctx.saved_tensors
        rows, C = x.shape
        dev, lib = x.device, N.load()
        g = g if (C == 1 or g.stride(1) == 1) and g.stride(0) >= C else g.contiguous()
        dx = torch.empty((rows, C), dtype=torch.float32, device=dev)
        dgamma = torch.empty(C, dtype=torch.float32, device=dev)
        dbeta = torch.empty(C, dtype=torch.float32, device=dev)
        partial = torch.empty(max(2 * lib.wsi_masked_bn_chunks(rows) * C, 1), dtype=torch.float32, device=dev)
        head = (N.ptr(g), g.stride(0) if rows > 1 else C, N.ptr(x), x.stride(0) if rows > 1 else C, rows, C, N.ptr(live), N.ptr(live_rows), N.ptr(w))
        tail = (N.ptr(stats), 1 if ctx.training else 0, N.ptr(partial), N.ptr(dgamma), N.ptr(dbeta), N.ptr(dx), C, N.stream())
        if ctx.relu:
            N.check(lib.wsi_masked_bn_relu_bwd(*head, N.ptr(b), *tail), "wsi_masked_bn_relu_bwd")
        else:
            N.check(lib.wsi_masked_bn_bwd(*head, *tail), "wsi_masked_bn_bwd")
        return dx, None, None, (dgamma if ctx.has_w else None), (dbeta if ctx.has_b else None), None, None, None, None, None, None


def masked_batch_norm_tensor(y, live, live_rows, weight, bias, running_mean, running_var, training: bool, momentum: float, eps: float):
    """``masked_batch_norm`` with tensor operations, in y's dtype on y's device: what the kernels are held against (and the CPU path)."""
    m = live.to(y.dtype).view(-1, 1)
    if training:
        n = live_rows.to(y.dtype).reshape(())
        mean = (y * m).sum(0) / n
        d = (y - mean) * m
        var = (d * d).sum(0) / n
        if running_mean is not None:
            with torch.no_grad():
                running_mean.mul_(1 - momentum).add_(momentum * mean.detach().to(running_mean.dtype))
                running_var.mul_(1 - momentum).add_(momentum * (var.detach() * (n / (n - 1))).to(running_var.dtype))
    else:
        mean, var = running_mean.to(y.dtype), running_var.to(y.dtype)
        d = (y - mean) * m
    out = d / torch.sqrt(var + eps)
    if weight is not None:
        out = out * weight
    if bias is not None:
        out = out + bias
    return out * m


def masked_batch_norm(y: torch.Tensor, live: torch.Tensor, live_rows: torch.Tensor, weight: Optional[torch.Tensor], bias: Optional[torch.Tensor],
                      running_mean: Optional[torch.Tensor], running_var: Optional[torch.Tensor], training: bool, momentum: Optional[float] = 0.1,
                      eps: float = 1e-5, num_batches_tracked: Optional[torch.Tensor] = None, kernels: Optional[bool] = None,
                      relu: bool = False) -> torch.Tensor:
    """``torch.nn.functional.batch_norm`` of the rows of ``y`` [rows, C] with ``live`` [rows] = 1 - and 0 in the others, which enter no
    statistic and receive no gradient.  ``live_rows``: a one-element tensor on y's device holding the number of live rows (at least 2 in
    training - the caller checks: the device cannot raise); no host value of the batch enters, so the call can be recorded.  In training the
    running statistics are updated in place as torch updates them (unbiased variance) and ``num_batches_tracked`` (if given) is incremented;
    in eval mode the running statistics normalise.  ``momentum=None`` (torch's cumulative average) is refused: it needs a host count.
    On the GPU two small launches and one streaming pass each way (``wsi_masked_bn_fwd`` / ``_bwd``; identical calls give identical bits);
    ``kernels=False`` or a CPU tensor: ``masked_batch_norm_tensor``.

    ``relu=True``: ``F.relu`` of the above - on the GPU inside the same passes (``wsi_masked_bn_relu_fwd`` / ``_bwd``: the backward
    recomputes the sign from y's own expression, no mask and no pre-activation is kept), with the bits of the composite, which
    ``set_fused_bn_relu(False)`` restores; on the CPU or with ``kernels=False`` the composite itself."""
    if momentum is None:
        raise ValueError("masked_batch_norm: momentum=None (a cumulative moving average) needs a host count of the batches; pass a number")
    if y.dim() != 2 or live.shape != y.shape[:1] or live_rows.numel() != 1:
        raise ValueError(f"masked_batch_norm: y [rows, C], live [rows] and a one-element live_rows; got {tuple(y.shape)}, {tuple(live.shape)}, {tuple(live_rows.shape)}")
    if (running_mean is None) != (running_var is None) or (not training and running_mean is None):
        raise ValueError("masked_batch_norm: running_mean and running_var come together, and eval mode needs them")
    if training and num_batches_tracked is not None:
        num_batches_tracked.add_(1)
    use = y.is_cuda if kernels is None else bool(kernels)
    if not use:
        out = masked_batch_norm_tensor(y, live, live_rows, weight, bias, running_mean, running_var, training, momentum, eps)
        return torch.relu(out) if relu else out
    if live.dtype != torch.float32 or live_rows.dtype != torch.float32:
        raise ValueError("masked_batch_norm: live and live_rows are fp32 tensors")
    fuse = bool(relu) and fused_bn_relu()
    out = _MaskedBatchNorm.apply(y, live.contiguous(), live_rows, weight, bias, running_mean, running_var, bool(training), float(momentum),
                                 float(eps), fuse)
    return torch.relu(out) if relu and not fuse else out


def seq_attention_supported(n: int, head_dim: int) -> bool:
    """The range the compiled kernels cover (anything else: ``wsi_seq_attn_*`` answer WSI_ENOSYS and the caller uses tensor operations)."""
    return 1 <= int(n) <= SEQ_ATTN_MAX_N and int(head_dim) in SEQ_ATTN_HEAD_DIMS


class _SeqAttention(torch.autograd.Function):
    @staticmethod
    def forward(ctx, qkv, heads: int):
        N.require_cuda(qkv)
        if qkv.dim() != 3 or qkv.dtype != torch.float32 or heads < 1 or qkv.shape[2] % (3 * heads):
            raise ValueError(f"seq_attention: qkv is an fp32 [B, n, 3 * heads * d] tensor, got {tuple(qkv.shape)} {qkv.dtype} with {heads} heads")
        qkv = qkv.contiguous()
        B, n, W = qkv.shape
        d = W // (3 * heads)
        out = torch.empty((B, n, heads * d), dtype=torch.float32, device=qkv.device)
        lse = torch.empty((B, heads, n), dtype=torch.float32, device=qkv.device)
        with _Timed("seq_attn_fwd"):
            N.check(N.load().wsi_seq_attn_fwd(N.ptr(qkv), B, n, heads, d, float(d) ** -0.5, N.ptr(out), N.ptr(lse), N.stream()), "wsi_seq_attn_fwd")
        ctx.heads = heads
        ctx.save_for_backward(qkv, lse)
        ctx.mark_non_differentiable(lse)
        return out, lse

    @staticmethod
    def backward(ctx, g_out, _g_lse):
        if not ctx.needs_input_grad[0]:
            return None, None
        qkv, lse = ctx.saved_tensors
        B, n, W = qkv.shape
        d = W // (3 * ctx.heads)
        g_out = g_out.contiguous()
        g_qkv = torch.empty_like(qkv)
        with _Timed("seq_attn_bwd"):
            N.check(N.load().wsi_seq_attn_bwd(N.ptr(g_out), N.ptr(qkv), N.ptr(lse), B, n, ctx.heads, d, float(d) ** -0.5, N.ptr(g_qkv), N.stream()),
                    "wsi_seq_attn_bwd")
        return g_qkv, None


def seq_attention_lse(qkv: torch.Tensor, heads: int):
    """(out, lse): ``seq_attention`` with the saved row log-sum-exp [B, heads, n] (not differentiable)."""
    return _SeqAttention.apply(qkv, int(heads))


def seq_attention(qkv: torch.Tensor, heads: int) -> torch.Tensor:
    """softmax(q k^T / sqrt(d)) v per head over a short sequence: ``qkv`` [B, n, 3 * heads * d] in the (qkv h d) column order of the
    reference's ``rearrange`` (models/ViT.py:186) -> [B, n, heads * d] in (h d) order.  1 <= n <= 128, d in {8, 16}; anything else raises
    (``seq_attention_supported`` tells beforehand).  No dropout: the reference runs attn_drop_rate = 0."""
    return _SeqAttention.apply(qkv, int(heads))[0]


# ------------------------------------------------------------------------------------------------
# GraphCAM of GTNMIL (wsi_hgnn_amd.gtn.graphcam): the relevance-propagation rules of models/layers.py at alpha = 1 (wsi_lrp_*), batched over
# slides and classes.  Not differentiable; every wrapper raises on a shape the kernels do not cover (the ``*_supported`` functions tell
# beforehand and the caller then runs the tensor-operation form).
# ------------------------------------------------------------------------------------------------
LRP_MAX_WIDTH = 256


def lrp_linear_supported(fan_in: int, fan_out: int) -> bool:
    return 4 <= int(fan_in) <= LRP_MAX_WIDTH and int(fan_in) % 4 == 0 and 1 <= int(fan_out) <= LRP_MAX_WIDTH


def lrp_residual_supported(width: int) -> bool:
    return int(width) >= 4 and int(width) % 4 == 0


def _lrp_rel(t: torch.Tensor, like: torch.Tensor, what: str) -> torch.Tensor:
    if t.dim() != 4 or t.dtype != torch.float32 or t.shape[0] != like.shape[0] or t.shape[2] != like.shape[1]:
        raise ValueError(f"{what}: relevance is fp32 [G, C, n, width] over tensors [G, n, width], got {tuple(t.shape)} over {tuple(like.shape)}")
    return t.contiguous()


def lrp_linear(X: torch.Tensor, W: torch.Tensor, R: torch.Tensor) -> torch.Tensor:
    """The Linear rule at alpha = 1 for all classes: X [G, n, in], W [out, in], R [G, C, n, out] -> [G, C, n, in] =
    X+ * (S W+) + X- * (S W-) with S = sd(R, X+ W+^T + X- W-^T); the bias plays no part.  in a multiple of 4, in and out <= 256."""
    N.require_cuda(X, W, R)
    if X.dim() != 3 or X.dtype != torch.float32 or W.dim() != 2 or W.dtype != torch.float32 or W.shape[1] != X.shape[2]:
        raise ValueError(f"lrp_linear: X fp32 [G, n, in], W fp32 [out, in], got {tuple(X.shape)} and {tuple(W.shape)}")
    R = _lrp_rel(R, X, "lrp_linear")
    if R.shape[3] != W.shape[0]:
        raise ValueError(f"lrp_linear: R has {R.shape[3]} columns, W {W.shape[0]} rows")
    X, W = X.contiguous(), W.contiguous()
    G, n, fin = X.shape
    C = R.shape[1]
    out = torch.empty((G, C, n, fin), dtype=torch.float32, device=X.device)
    with _Timed("lrp_linear"):
        N.check(N.load().wsi_lrp_linear(N.ptr(X), N.ptr(W), N.ptr(R), G, C, n, fin, W.shape[0], N.ptr(out), N.stream()), "wsi_lrp_linear")
    return out


def lrp_residual(X: Optional[torch.Tensor], r1: torch.Tensor, r2: Optional[torch.Tensor], A: torch.Tensor, B: torch.Tensor):
    """(a, b) = add(A, B, R) with R = clone(X, r1, r2) = X * (sd(r1, X) + sd(r2, X)), or R = r1 when r2 is None (X is then not read): the Clone
    rule of a tensor's two uses followed by the Add rule of the residual below it, in one launch.  X, A, B [G, n, E]; r1, r2 [G, C, n, E]; the
    Add rule's three sums run over the [n, E] tensor of every (slide, class), in a fixed order.  E a multiple of 4."""
    N.require_cuda(r1, r2, A, B)
    if A.dim() != 3 or A.dtype != torch.float32 or B.shape != A.shape or B.dtype != torch.float32:
        raise ValueError(f"lrp_residual: A and B fp32 [G, n, E], got {tuple(A.shape)} and {tuple(B.shape)}")
    r1 = _lrp_rel(r1, A, "lrp_residual")
    if r1.shape[3] != A.shape[2]:
        raise ValueError(f"lrp_residual: relevance of width {r1.shape[3]} over tensors of width {A.shape[2]}")
    if r2 is not None:
        r2 = _lrp_rel(r2, A, "lrp_residual")
        if r2.shape != r1.shape or X is None or X.shape != A.shape or X.dtype != torch.float32:
            raise ValueError("lrp_residual: r2 has r1's shape, and X the shape of A")
        N.require_cuda(X)
        X = X.contiguous()
    A, B = A.contiguous(), B.contiguous()
    G, n, E = A.shape
    a, b = torch.empty_like(r1), torch.empty_like(r1)
    with _Timed("lrp_residual"):
        N.check(N.load().wsi_lrp_residual(N.ptr(X) if r2 is not None else None, N.ptr(r1), N.ptr(r2), N.ptr(A), N.ptr(B), G, r1.shape[1], n, E,
                                          N.ptr(a), N.ptr(b), N.stream()), "wsi_lrp_residual")
    return a, b


def lrp_attention(qkv: torch.Tensor, lse: torch.Tensor, R: torch.Tensor, g_out: Optional[torch.Tensor], heads: int):
    """The attention rule of ViT.Attention.relprop and the block's layer map: qkv [G, n, 3 H d] and lse [G, H, n] as ``seq_attention_lse``
    leaves them, R [G, C, n, H d] (the relevance of the attention output), g_out [G, C, n, H d] (d / d attention output of the class
    score; None: the rollout map) -> (cam_qkv [G, C, n, 3 H d], M [G, C, n, n] = mean_h max(d attn * cam_attn, 0) with d attn = g_out v^T).
    1 <= n <= 128, d in {8, 16}."""
    N.require_cuda(qkv, lse, R, g_out)
    heads = int(heads)
    if qkv.dim() != 3 or qkv.dtype != torch.float32 or heads < 1 or qkv.shape[2] % (3 * heads):
        raise ValueError(f"lrp_attention: qkv is an fp32 [G, n, 3 * heads * d] tensor, got {tuple(qkv.shape)} {qkv.dtype} with {heads} heads")
    G, n, W = qkv.shape
    d = W // (3 * heads)
    R = _lrp_rel(R, qkv, "lrp_attention")
    C = R.shape[1]
    if R.shape[3] != heads * d or lse.shape != (G, heads, n) or lse.dtype != torch.float32:
        raise ValueError(f"lrp_attention: R [G, C, n, {heads * d}] and lse fp32 [G, {heads}, n], got {tuple(R.shape)} and {tuple(lse.shape)}")
    if g_out is not None:
        g_out = _lrp_rel(g_out, qkv, "lrp_attention")
        if g_out.shape != R.shape:
            raise ValueError("lrp_attention: g_out has R's shape")
    qkv, lse = qkv.contiguous(), lse.contiguous()
    cam = torch.empty((G, C, n, W), dtype=torch.float32, device=qkv.device)
    M = torch.empty((G, C, n, n), dtype=torch.float32, device=qkv.device)
    partial = torch.empty(G * C * heads * n * n if heads > 1 else 1, dtype=torch.float32, device=qkv.device)
    with _Timed("lrp_attention"):
        N.check(N.load().wsi_lrp_attention(N.ptr(qkv), N.ptr(lse), N.ptr(R), N.ptr(g_out), G, C, n, heads, d, float(d) ** -0.5, N.ptr(partial),
                                           N.ptr(cam), N.ptr(M), N.stream()), "wsi_lrp_attention")
    return cam, M


# ------------------------------------------------------------------------------------------------
# H2MIL (wsi_hgnn_amd/h2mil): RAConv's two-level attention (csrc/ra_attn.hip) and IHPool's cluster assignment (csrc/ihpool.hip)
# ------------------------------------------------------------------------------------------------
RA_NODE_TYPES = 3


def edge_csr_by_source_type(src: torch.Tensor, dst: torch.Tensor, node_type: torch.Tensor, n: int) -> EdgeCSR:
    """The edge layout of ``ra_attention``: an ``EdgeCSR`` grouped by destination whose rows are ordered by the SOURCE'S type (two stable
    sorts, on the edges' own device), so that the groups (destination, source type) of a destination are contiguous runs.  ``perm`` maps a CSR
    position to the original edge; ``node_type`` (int32) is kept on the plan."""
    if src.dim() != 1 or src.shape != dst.shape or node_type.dim() != 1 or node_type.shape[0] != int(n):
        raise ValueError(f"edge_csr_by_source_type: src and dst are 1-D tensors of one length and node_type is [{int(n)}], got "
                         f"{tuple(src.shape)}, {tuple(dst.shape)}, {tuple(node_type.shape)}")
    src, dst = src.to(torch.int64), dst.to(torch.int64)
    first = torch.sort(node_type.to(torch.int64)[src], stable=True).indices if src.numel() else src
    ec = EdgeCSR(dst[first], src[first], n)
    ec.perm = first[ec.perm] if src.numel() else first
    ec.node_type = node_type.to(torch.int32).contiguous()
    ec.by_source_type = True
    return ec


def _ra_check(ft, sc, bias, ec, node_type) -> None:
    if not getattr(ec, "by_source_type", False):
        raise ValueError("ra_attention: the edge plan must come from ops.edge_csr_by_source_type (rows ordered by the source's type)")
    n = ec.num_nodes
    if ft.dim() != 2 or ft.shape[0] != n or not 1 <= ft.shape[1] <= 4096 or ft.dtype != torch.float32:
        raise ValueError(f"ra_attention: ft is an fp32 [{n}, 1 <= C <= 4096] tensor, got {tuple(ft.shape)} {ft.dtype}")
    if sc.shape != (n, 4) or sc.dtype != torch.float32:
        raise ValueError(f"ra_attention: sc is an fp32 [{n}, 4] tensor (el | er | pl | pr), got {tuple(sc.shape)} {sc.dtype}")
    if bias is not None and (bias.shape != (ft.shape[1],) or bias.dtype != torch.float32):
        raise ValueError(f"ra_attention: bias is an fp32 [{ft.shape[1]}] tensor or None, got {tuple(bias.shape)} {bias.dtype}")
    if node_type.shape != (n,) or node_type.dtype not in (torch.int32, torch.int64):
        raise ValueError(f"ra_attention: node_type is an integer [{n}] tensor, got {tuple(node_type.shape)} {node_type.dtype}")


def _ra_edges(ec):
    """The plan's per-edge arrays as the C ABI takes them: an empty tensor has no address and the entry points refuse NULL, so a graph
    without edges passes one unread element each."""
    if ec.num_edges:
        return ec.src, ec.csc_eid, ec.csc_dst
    one = torch.zeros(1, dtype=torch.int32, device=ec.rowptr.device)
    return one, one, one


class _RaAttention(torch.autograd.Function):
    @staticmethod
    def forward(ctx, ft, sc, bias, ec, node_type, slope: float):
        N.require_cuda(ft, sc, bias, node_type, ec.rowptr)
        n, C = ft.shape
        if not (ft.stride(1) == 1 and ft.stride(0) >= C) and n > 1:
            ft = ft.contiguous()
        ldf = ft.stride(0) if n > 1 else C
        sc = sc.detach().contiguous()
        b = bias.detach().contiguous() if bias is not None else None
        out = torch.empty((n, C), dtype=torch.float32, device=ft.device)
        stat = torch.empty((n, RA_NODE_TYPES, 4), dtype=torch.float32, device=ft.device)
        with _Timed("ra_attn_fwd"):
            N.check(N.load().wsi_ra_attn_fwd(N.ptr(ft), ldf, N.ptr(sc), N.ptr(node_type), n, C, N.ptr(ec.rowptr), N.ptr(_ra_edges(ec)[0]), float(slope),
                                             N.ptr(b), N.ptr(out), C, N.ptr(stat), N.stream()), "wsi_ra_attn_fwd")
        ctx.ec, ctx.slope, ctx.has_bias, ctx.ldf = ec, float(slope), bias is not None, ldf
        ctx.save_for_backward(ft, sc, stat, node_type)
        return out

    @staticmethod
    def backward(ctx, g_out):
        ft, sc, stat, node_type = ctx.saved_tensors
        ec = ctx.ec
        n, C = ft.shape
        E = ec.num_edges
        g_out = g_out.contiguous()
        dev = ft.device
        edge_ws = torch.empty(max(E, 1), dtype=torch.float32, device=dev)
        group_ws = torch.empty(max(RA_NODE_TYPES * n, 1), dtype=torch.float32, device=dev)
        bias_ws = torch.empty(N.WSI_RA_BIAS_PARTS * C, dtype=torch.float32, device=dev) if ctx.has_bias else None
        g_ft = torch.empty((n, C), dtype=torch.float32, device=dev)
        g_sc = torch.empty((n, 4), dtype=torch.float32, device=dev)
        g_b = torch.empty(C, dtype=torch.float32, device=dev) if ctx.has_bias else None
        src, csc_eid, csc_dst = _ra_edges(ec)
        with _Timed("ra_attn_bwd"):
            N.check(N.load().wsi_ra_attn_bwd(N.ptr(ft), ctx.ldf, N.ptr(sc), N.ptr(node_type), N.ptr(stat), N.ptr(g_out), C, n, E, C,
                                             N.ptr(ec.rowptr), N.ptr(src), N.ptr(ec.colptr), N.ptr(csc_eid), N.ptr(csc_dst), ctx.slope,
                                             N.ptr(edge_ws), N.ptr(group_ws), N.ptr(bias_ws), N.ptr(g_ft), C, N.ptr(g_sc), N.ptr(g_b), N.stream()),
                    "wsi_ra_attn_bwd")
        return g_ft, g_sc, g_b, None, None, None


def ra_attention(ft: torch.Tensor, sc: torch.Tensor, bias: Optional[torch.Tensor], ec: EdgeCSR, node_type: torch.Tensor,
                 negative_slope: float = 0.2) -> torch.Tensor:
    """RAConv after its projection (``baselines/H2MIL/code/RAConv.py`` at heads = 1): ``ft`` [n, C] fp32 (unit column stride; a row stride
    is taken as it is), ``sc`` [n, 4] = el | er | pl | pr, ``bias`` [C] or None, ``ec`` from ``edge_csr_by_source_type``, ``node_type`` [n]
    in {0, 1, 2}.  With the group of an edge u -> v being (v, node_type[u]):

        a_e = softmax over the group of leaky_relu(el[u] + er[v]);   q_vt = leaky_relu(mean over the group of pl[u] + pr[v])
        beta_vt = softmax of q over the groups present at v;           out[v] = sum_e beta a_e ft[u] + bias

    One autograd function: the gradient of ``ft`` is the aggregation term alone (``sc`` carries the rest), and ``sc`` and ``bias`` receive
    theirs.  Identical calls give identical bits."""
    _ra_check(ft, sc, bias, ec, node_type)
    nt = node_type if node_type.dtype == torch.int32 and node_type.is_contiguous() else node_type.to(torch.int32).contiguous()
    return _RaAttention.apply(ft, sc, bias, ec, nt, float(negative_slope))


def ihpool_assign(xyf: torch.Tensor, member_node: torch.Tensor, member_seg: torch.Tensor, seed_ptr: torch.Tensor, seed_node: torch.Tensor) -> torch.Tensor:
    """``wsi_ihpool_assign``: ``xyf`` [nodes, 3] fp32 = x | y | fitness; the members of all segments grouped by segment (``member_node`` rows of
    xyf, ``member_seg`` non-decreasing), the seeds of segment s = ``seed_node[seed_ptr[s]:seed_ptr[s + 1]]`` (all int32).  Returns for every
    member the position, within its segment's seeds, of the nearest one in |xy_s - xy_n|_2 + |f_s - f_n| (int32; ties to the lowest
    position, a seed to itself, -1 without seeds).  One launch, no read-back."""
    if xyf.dim() != 2 or xyf.shape[1] != 3 or xyf.dtype != torch.float32:
        raise ValueError(f"ihpool_assign: xyf is an fp32 [nodes, 3] tensor, got {tuple(xyf.shape)} {xyf.dtype}")
    if member_node.dim() != 1 or member_node.shape != member_seg.shape or seed_ptr.dim() != 1 or seed_ptr.numel() < 1 or seed_node.dim() != 1:
        raise ValueError("ihpool_assign: member_node and member_seg are 1-D tensors of one length, seed_ptr is [segments + 1], seed_node 1-D")
    if any(t.dtype != torch.int32 for t in (member_node, member_seg, seed_ptr, seed_node)):
        raise ValueError("ihpool_assign: member_node, member_seg, seed_ptr and seed_node are int32")
    N.require_cuda(xyf, member_node, member_seg, seed_ptr, seed_node)
    xyf, member_node, member_seg, seed_ptr, seed_node = (t.contiguous() for t in (xyf, member_node, member_seg, seed_ptr, seed_node))
    m = member_node.shape[0]
    out = torch.empty(max(m, 1), dtype=torch.int32, device=xyf.device)[:m]
    with _Timed("ihpool_assign"):
        N.check(N.load().wsi_ihpool_assign(N.ptr(xyf), xyf.shape[0], N.ptr(member_node), N.ptr(member_seg), m, N.ptr(seed_ptr), N.ptr(seed_node),
                                           seed_ptr.numel() - 1, seed_node.numel(), N.ptr(out), N.stream()), "wsi_ihpool_assign")
    return out


# ------------------------------------------------------------------------------------------------
# Slide graphs from patch grids (csrc/grid_graph.hip; the host layer is construct.grid_adjacency / construct.slide_trees)
# ------------------------------------------------------------------------------------------------
GRID_COORD_LIMIT = 1 << 24
GRID_MAX_SETS = 1 << 13
GRID_MODES = {"adjacency": N.WSI_GRID_ADJACENCY, "tree": N.WSI_GRID_TREE}
GRID_FLAGS = ((N.WSI_GRID_BAD_COORD, "a coordinate outside 0 <= c < 2^24"),
              (N.WSI_GRID_REPEATED, "a coordinate pair repeated within one slide and level"),
              (N.WSI_GRID_TABLE_FULL, "the look-up table is full"),
              (N.WSI_GRID_UNCOVERED, "a level-2 node that no level-1 node covers"))


def grid_capacity(num_points: int) -> int:
    """The smallest power of two >= 2 x ``num_points`` (at least 2): the table size ``wsi_grid_index`` asks for."""
    return 1 << max(1, (2 * int(num_points) - 1).bit_length())


class GridIndex:
    """What ``grid_index`` leaves on the device: the table (``keys`` int64 / ``rows`` int32 [capacity]), ``set_max`` int32 [S, 2], ``flags``
    int32 [2], and the tables it was built from."""

    def __init__(self, coords, set_ptr, keys, rows, set_max, flags):
        self.coords, self.set_ptr, self.keys, self.rows, self.set_max, self.flags = coords, set_ptr, keys, rows, set_max, flags

    @property
    def num_points(self) -> int:
        return self.coords.shape[0]

    @property
    def num_sets(self) -> int:
        return self.set_ptr.shape[0] - 1

    @property
    def capacity(self) -> int:
        return self.keys.shape[0]


def _grid_tables(what: str, coords: torch.Tensor, set_ptr: torch.Tensor) -> None:
    if coords.dim() != 2 or coords.shape[1] != 2 or coords.dtype != torch.int32:
        raise ValueError(f"{what}: coords is an int32 [P, 2] tensor, got {tuple(coords.shape)} {coords.dtype}")
    if set_ptr.dim() != 1 or set_ptr.dtype != torch.int32 or not 2 <= set_ptr.shape[0] <= GRID_MAX_SETS + 1:
        raise ValueError(f"{what}: set_ptr is an int32 [S + 1] tensor with 1 <= S <= {GRID_MAX_SETS}")
    N.require_cuda(coords, set_ptr)


def grid_index(coords: torch.Tensor, set_ptr: torch.Tensor) -> GridIndex:
    """``wsi_grid_index``: one open-addressing table over (set, x, y) -> point for the packed point sets ``coords`` [P, 2] int32 / ``set_ptr``
    [S + 1] int32 (non-decreasing from 0 to P: the caller's), the per-set coordinate maxima and the flag words.  No read-back."""
    _grid_tables("grid_index", coords, set_ptr)
    coords, set_ptr = coords.contiguous(), set_ptr.contiguous()
    P, S, dev = coords.shape[0], set_ptr.shape[0] - 1, coords.device
    cap = grid_capacity(P)
    keys = torch.empty(cap, dtype=torch.int64, device=dev)
    rows = torch.empty(cap, dtype=torch.int32, device=dev)
    set_max = torch.empty((S, 2), dtype=torch.int32, device=dev)
    flags = torch.empty(2, dtype=torch.int32, device=dev)
    with _Timed("grid_index"):
        N.check(N.load().wsi_grid_index(N.ptr(coords), P, N.ptr(set_ptr), S, N.ptr(keys), N.ptr(rows), cap, N.ptr(set_max), N.ptr(flags), N.stream()),
                "wsi_grid_index")
    return GridIndex(coords, set_ptr, keys, rows, set_max, flags)


def _grid_tree_args(what: str, index: GridIndex, mode: str, n1: int, cover: Optional[torch.Tensor]):
    if mode not in GRID_MODES:
        raise ValueError(f"{what}: mode is 'adjacency' or 'tree', got {mode!r}")
    if mode == "adjacency":
        return 0, None
    n1 = int(n1)
    if index.num_sets % 2 or not 0 <= n1 <= index.num_points:
        raise ValueError(f"{what}: a tree call has the sets [level 1 of every slide | level 2 of every slide] and 0 <= n1 <= P")
    if cover is None or cover.dtype != torch.int32 or tuple(cover.shape) != (n1, 4):
        raise ValueError(f"{what}: cover is an int32 [n1, 4] tensor")
    N.require_cuda(cover)
    return n1, cover.contiguous()


def grid_count(index: GridIndex, mode: str, n1: int = 0, cover: Optional[torch.Tensor] = None):
    """``wsi_grid_count``: ``counts`` int32, the items every node will emit - [P] entries for ``mode='adjacency'``, [2 n1 + n2] edges in
    [slide][section][node] order for ``mode='tree'`` - and, for a tree, ``parent`` int32 [n2] (else None).  No read-back."""
    n1, cover = _grid_tree_args("grid_count", index, mode, n1, cover)
    P, dev = index.num_points, index.coords.device
    counts = torch.empty(P + n1, dtype=torch.int32, device=dev)
    parent = torch.empty(P - n1, dtype=torch.int32, device=dev) if mode == "tree" else None
    with _Timed("grid_count"):
        N.check(N.load().wsi_grid_count(GRID_MODES[mode], N.ptr(index.coords), P, N.ptr(index.set_ptr), index.num_sets, n1, N.ptr(cover),
                                        N.ptr(index.keys), N.ptr(index.rows), index.capacity, N.ptr(counts), N.ptr(parent), N.stream()),
                "wsi_grid_count")
    return counts, parent


def grid_write(index: GridIndex, mode: str, counts: torch.Tensor, offsets_incl: torch.Tensor, n1: int = 0, cover: Optional[torch.Tensor] = None,
               parent: Optional[torch.Tensor] = None):
    """``wsi_grid_write``: the items at ``offsets_incl - counts`` (``offsets_incl`` int64 = ``cumsum(counts)``), in buffers of the largest
    possible size - the caller cuts them at the total.  ``mode='adjacency'``: ``(row, col)`` int64 [8 P].  ``mode='tree'``: ``(edge_index``
    int64 [2, 18 n1 + 8 n2], ``node_type`` int64 [N], ``node_tree`` int64 [N], ``x_y_index`` fp64 [N, 2]) over the N = B + P rows of the
    batch, ``index.flags[1]`` raised for an uncovered level-2 node.  No atomics, no read-back."""
    n1, cover = _grid_tree_args("grid_write", index, mode, n1, cover)
    P, dev = index.num_points, index.coords.device
    if counts.dtype != torch.int32 or offsets_incl.dtype != torch.int64 or counts.shape != (P + n1,) or offsets_incl.shape != counts.shape:
        raise ValueError("grid_write: counts int32 and offsets_incl int64, one entry per counted node")
    N.require_cuda(counts, offsets_incl)
    counts, offsets_incl = counts.contiguous(), offsets_incl.contiguous()
    lib, st = N.load(), N.stream()
    if mode == "adjacency":
        row = torch.empty(8 * P, dtype=torch.int64, device=dev)
        col = torch.empty(8 * P, dtype=torch.int64, device=dev)
        with _Timed("grid_write"):
            N.check(lib.wsi_grid_write(GRID_MODES[mode], N.ptr(index.coords), P, N.ptr(index.set_ptr), index.num_sets, 0, None, N.ptr(index.keys),
                                       N.ptr(index.rows), index.capacity, N.ptr(counts), N.ptr(offsets_incl), None, None, N.ptr(row), N.ptr(col),
                                       None, None, None, None, st), "wsi_grid_write")
        return row, col
    if parent is None or parent.dtype != torch.int32 or parent.shape != (P - n1,):
        raise ValueError("grid_write: parent is the int32 [n2] tensor grid_count returned")
    N.require_cuda(parent)
    rows = index.num_sets // 2 + P
    edges = torch.empty((2, 18 * n1 + 8 * (P - n1)), dtype=torch.int64, device=dev)
    node_type = torch.empty(rows, dtype=torch.int64, device=dev)
    node_tree = torch.empty(rows, dtype=torch.int64, device=dev)
    xy = torch.empty((rows, 2), dtype=torch.float64, device=dev)
    with _Timed("grid_write"):
        N.check(lib.wsi_grid_write(GRID_MODES[mode], N.ptr(index.coords), P, N.ptr(index.set_ptr), index.num_sets, n1, N.ptr(cover), N.ptr(index.keys),
                                   N.ptr(index.rows), index.capacity, N.ptr(counts), N.ptr(offsets_incl), N.ptr(parent.contiguous()),
                                   N.ptr(index.set_max), N.ptr(edges), N.ptr(edges, edges.shape[1] * 8), N.ptr(node_type), N.ptr(node_tree),
                                   N.ptr(xy), N.ptr(index.flags), st), "wsi_grid_write")
    return edges, node_type, node_tree, xy


# ------------------------------------------------------------------------------------------------
# Explanations scored against annotations (csrc/localization.hip; the host layer is localization.patch_labels / score / heat_image)
# ------------------------------------------------------------------------------------------------
LOC_TILE = N.WSI_LOC_TILE
LOC_CHUNK = 512                                   # edges per chunk unless the caller of localization.AnnotationBatch says otherwise
LOC_CHUNK_MAX = N.WSI_LOC_CHUNK_MAX
LOC_MAX_SCRATCH_WORDS = 1 << 28                   # 1 GiB of (chunk, centre) words: patch_labels refuses a batch that needs more


def loc_tables(sizes: Sequence[int], chunks_per_slide: Optional[Sequence[int]] = None):
    """The host tables of a packed batch (include/wsi_hgnn.h): ``tiles`` rows (slide, first row, rows, position within the slide), ``slides``
    rows (first scratch word, rows, first tile) as flat lists, and the scratch words needed (0 without ``chunks_per_slide``)."""
    tiles, slides, row, word = [], [], 0, 0
    for s, n in enumerate(sizes):
        slides += [word, n, len(tiles) // 4]
        for at in range(0, n, LOC_TILE):
            tiles += [s, row + at, min(LOC_TILE, n - at), at]
        row += n
        word += n * (chunks_per_slide[s] if chunks_per_slide is not None else 0)
    return tiles, slides, word


def _loc_device_tables(sizes, chunks_per_slide, device):
    tiles, slides, words = loc_tables(sizes, chunks_per_slide)
    t = host_to_device(tiles, torch.int32, device).reshape(len(tiles) // 4, 4)
    s = host_to_device(slides, torch.int64, device).reshape(len(slides) // 3, 3)
    return t, s, words


def loc_labels(centres: torch.Tensor, sizes: Sequence[int], vertices: torch.Tensor, ring_ptr: torch.Tensor, ring_box: torch.Tensor,
               chunks: torch.Tensor, slide_chunk_ptr: torch.Tensor, chunks_per_slide: Sequence[int], chunk_edges: int,
               max_scratch_words: int = LOC_MAX_SCRATCH_WORDS) -> torch.Tensor:
    """``wsi_loc_labels``: int32 [N], 1 where centre i (fp64 [N, 2], the slides one after the other, ``sizes`` rows each) lies strictly inside a
    ring of its slide.  The ring tables are those of ``localization.AnnotationBatch`` on the device.  ``ValueError`` when the (chunk, centre)
    scratch would exceed ``max_scratch_words``.  No read-back."""
    N.require_cuda(centres, vertices, ring_ptr, ring_box, chunks, slide_chunk_ptr)
    if centres.dim() != 2 or centres.shape[1] != 2 or centres.dtype != torch.float64:
        raise ValueError(f"loc_labels: centres is an fp64 [N, 2] tensor, got {tuple(centres.shape)} {centres.dtype}")
    sizes = [int(n) for n in sizes]
    if len(sizes) != len(chunks_per_slide) or any(n < 0 for n in sizes) or sum(sizes) != centres.shape[0]:
        raise ValueError(f"loc_labels: the sizes {sizes} do not match {centres.shape[0]} centres in {len(chunks_per_slide)} annotated slides")
    if (vertices.dtype, ring_ptr.dtype, ring_box.dtype, chunks.dtype, slide_chunk_ptr.dtype) != (torch.float64, torch.int64, torch.float64,
                                                                                                 torch.int32, torch.int32):
        raise ValueError("loc_labels: vertices / ring_box fp64, ring_ptr int64, chunks / slide_chunk_ptr int32")
    centres = centres.contiguous()
    dev, n = centres.device, centres.shape[0]
    tiles, slides, words = _loc_device_tables(sizes, chunks_per_slide, dev)
    if words > max_scratch_words:
        raise ValueError(f"loc_labels: {words} (chunk, centre) words of scratch exceed the limit of {max_scratch_words}; label fewer slides per call")
    scratch = torch.empty(max(words, 1), dtype=torch.int32, device=dev)
    labels = torch.empty(n, dtype=torch.int32, device=dev)
    with _Timed("loc_labels"):
        N.check(N.load().wsi_loc_labels(N.ptr(centres), n, N.ptr(tiles), tiles.shape[0], N.ptr(slides), len(sizes), N.ptr(vertices), vertices.shape[0],
                                        N.ptr(ring_ptr), N.ptr(ring_box), ring_box.shape[0], N.ptr(chunks), chunks.shape[0], N.ptr(slide_chunk_ptr),
                                        max(chunks_per_slide, default=0), int(chunk_edges), N.ptr(scratch), words, N.ptr(labels), N.stream()),
                "wsi_loc_labels")
    return labels


def loc_score(scores: torch.Tensor, labels: torch.Tensor, sizes: Sequence[int]):
    """``wsi_loc_score``: (auc fp64 [B, C], counts int64 [B, C, 4] = (P, N, gt, eq), flags int32 [B, C], mean fp64 [C]) of fp32 ``scores`` [N, C]
    against int32 ``labels`` [N], per slide of ``sizes`` rows.  No read-back."""
    N.require_cuda(scores, labels)
    if scores.dim() != 2 or scores.dtype != torch.float32 or labels.dtype != torch.int32 or labels.shape != scores.shape[:1]:
        raise ValueError(f"loc_score: scores fp32 [N, C] and labels int32 [N], got {tuple(scores.shape)} {scores.dtype} / {tuple(labels.shape)} {labels.dtype}")
    sizes = [int(n) for n in sizes]
    if any(n < 0 for n in sizes) or sum(sizes) != scores.shape[0]:
        raise ValueError(f"loc_score: the sizes {sizes} do not add up to the {scores.shape[0]} rows given")
    scores, labels = scores.contiguous(), labels.contiguous()
    dev, (n, C), B = scores.device, scores.shape, len(sizes)
    tiles, slides, _ = _loc_device_tables(sizes, None, dev)
    T = tiles.shape[0]
    partial = torch.empty(max(C * T * 5, 1), dtype=torch.int64, device=dev)
    counts = torch.empty((B, C, 4), dtype=torch.int64, device=dev)
    flags = torch.empty((B, C), dtype=torch.int32, device=dev)
    auc = torch.empty((B, C), dtype=torch.float64, device=dev)
    mean = torch.empty(C, dtype=torch.float64, device=dev)
    with _Timed("loc_score"):
        N.check(N.load().wsi_loc_score(N.ptr(scores), n, C, N.ptr(labels), N.ptr(tiles), T, N.ptr(slides), B, N.ptr(partial), N.ptr(counts),
                                       N.ptr(flags), N.ptr(auc), N.ptr(mean), N.stream()), "wsi_loc_score")
    return auc, counts, flags, mean


def loc_owner(grid_xy: torch.Tensor, patch: int, height: int, width: int) -> torch.Tensor:
    """``wsi_loc_owner``: int32 [height, width], the highest patch index whose square x .. x + patch, y .. y + patch covers the pixel, -1 for none."""
    N.require_cuda(grid_xy)
    if grid_xy.dim() != 2 or grid_xy.shape[1] != 2 or grid_xy.dtype != torch.int32:
        raise ValueError(f"loc_owner: grid_xy is an int32 [n, 2] tensor, got {tuple(grid_xy.shape)} {grid_xy.dtype}")
    grid_xy = grid_xy.contiguous()
    owner = torch.full((int(height), int(width)), -1, dtype=torch.int32, device=grid_xy.device)
    with _Timed("loc_owner"):
        N.check(N.load().wsi_loc_owner(N.ptr(grid_xy), grid_xy.shape[0], int(patch), int(height), int(width), N.ptr(owner), N.stream()), "wsi_loc_owner")
    return owner
