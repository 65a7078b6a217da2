"""The skinny GEMM kernels of csrc/gemm_f32.hip (launches of at most 32 rows, or at most 32 reduction rows for TN), the paired launch
wsi_gemm_small_pair, the split-K reduction and wsi_row_absmax on the GPU, against float64 on the SAME fp32 inputs.  Shapes, inputs, the float64
restatement and the derived componentwise bound come from tests/gemm_small_cases.py; tests/test_gemm_small_cases.py shows without a GPU that
the bound holds for the kernels' summation order and fails for three seeded faults.
  a. every table row through wsi_gemm_grouped in fp32 mode, within the bound; the 1e30 padding, the sentinel columns behind C and everything
     else in the buffer bit for bit as before;
  b. the same rows under bf16x6, fp16x3 and auto: identical bits (the skinny kernels run "whatever the precision argument"); at M = 33
     (NT / NN) and K = 33 (TN) the bf16x6 bits differ from the fp32 ones - so (b) is not vacuous - and every mode meets the tiled kernels'
     existing tolerance;
  c. launches of 24 descriptors: M mixed up to 8 / 16 / 32, N from 1 to 130, a gate and a bias per group, two groups on one A, empty groups in
     between; and the same launch with one group of 33 rows, which takes the tiles as a whole;
  d. wsi_gemm_small_pair: every dX epilogue set with dW ACCUMULATE / SCALE_GATE and colsum_out, bit-equal to the two wsi_gemm_grouped launches and
     within the bound; 16 descriptors accepted and 17 refused; empty groups skipped; M = 33 or K = 33 answers WSI_ENOSYS and writes nothing;
  e. WSI_EPI_ADD_R without R: WSI_EINVAL at M = 32 and M = 33 from both entry points, nothing written, the next valid call works; likewise a
     negative dimension in a paired launch (the tiled path refuses it, the paired launch used to skip the group);
  f. the split-K reduction behind TN launches of K = 256 .. 2100 (1, 3, 4, 5 and 9 slabs of 256 rows; under fp16x3 the column-scaled kernel
     plans 128-row slabs: 2, 6, 8, 9, 17), in its vector form, its scalar form and with three groups, the workspace size held against the plan;
  g. wsi_row_absmax == torch, exactly, over vector and scalar paths, padded rows, signed zeros, denormals, inf and NaN.

Bound (a, c, d): |err| <= (ceil(K / 64) + 16) u S for NT / NN, (K + 8) u S for TN and its column sums, u = 2^-24 - see gemm_small_cases.
The device sigmoid stayed inside its share of 5 u: no term of the bound was widened.

Measured on an MI355X (largest error / bound, printed at the end of the module's run):
  NT x8 0.177, x16 0.159, x32 0.188; NN x8 0.200, x16 0.172, x32 0.208 (all on the 5 x 130 x 3 group of the 24-group launches; the table rows
  alone: 0.141 at most, NT 32 x 3 x 1 with all five epilogues); TN 0.267 (300 x 7, K = 1, SCALE_GATE | ACCUMULATE, column sums);
  paired launch: dX x8 0.109, x16 0.097, x32 0.106, dW 0.288 (300 x 7, K = 1, SCALE_GATE).
  One past the limit, error over the largest float64 entry: NT fp32 8.3e-7, bf16x6 5.7e-7, fp16x3 1.9e-7; NN 4.8e-7, 6.6e-7, 2.1e-7;
  TN 1.2e-7, 5.9e-8, 1.1e-7 (auto = bf16x6 at these sizes).
"""
import functools

import numpy as np
import pytest
import torch

import gemm_small_cases as GC

pytestmark = pytest.mark.gpu

DEV = "cuda"
POISON, SENTINEL = 1e30, 777.0
MODES = ("fp32", "bf16x6", "fp16x3", "auto")
OPS = {"NT": 0, "NN": 1, "TN": 2}
RATIOS = {}                          # kernel -> (largest error / bound over the module's run, case)


@pytest.fixture(scope="module", autouse=True)
def _report_ratios():
    yield
    for name, (r, case) in sorted(RATIOS.items()):
        print(f"\nlargest error / bound, {name}: {r:.3f} ({case})", end="")
    if RATIOS:
        print(f"\nlargest error / bound of the module: {max(r for r, _ in RATIOS.values()):.3f}")


def _relerr(a, b):
    """tests/test_kernels_gpu.py's measure: largest error over the largest float64 entry."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


@functools.lru_cache(maxsize=None)
def _problem(case, a_from=None):
    """(inputs, float64 reference) of a case: made once, shared, never written.  ``a_from``: the case whose A this one reads instead of its own."""
    inp = GC.make_inputs(case)
    if a_from is not None:
        inp["A"] = _problem(a_from)[0]["A"]
    ref = GC.reference(case, inp)
    for v in list(inp.values()) + list(ref.values()):
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return inp, ref


# ------------------------------------------------------------------------------------------------ one buffer per launch
class Handle:
    def __init__(self, start, rows, cols, ld):
        self.start, self.rows, self.cols, self.ld = start, rows, cols, ld


class Arena:
    """Every tensor of a launch as a view carved from ONE buffer, staged on the host and uploaded at once.  Layouts (gemm_small_cases.LAYOUTS):
    dense - ld = columns, 16-byte aligned starts; padded - ld = columns + 1 or + 3 in turn; offset - every start 4 bytes past a 16-byte
    boundary.  Gaps and the padding of inputs hold 1e30, the padding of outputs SENTINEL.  ``unchanged`` compares everything but the logical
    elements of the outputs, bit for bit, with what was uploaded."""

    def __init__(self, layout):
        self.layout, self.chunks, self.n, self.outs, self.k = layout, [], 0, [], 0
        self.host = self.dev = None

    def put(self, arr, out=False):
        arr = np.asarray(arr, np.float32)
        arr = arr.reshape(1, -1) if arr.ndim < 2 else arr
        rows, cols = arr.shape
        ld = cols + ((1, 3)[self.k % 2] if self.layout == "padded" else 0)
        self.k += 1
        lead = (-self.n) % 4 + 4 + (1 if self.layout == "offset" else 0)
        block = np.full((rows, ld), SENTINEL if out else POISON, np.float32)
        block[:, :cols] = arr
        self.chunks += [np.full(lead, POISON, np.float32), block.ravel()]
        h = Handle(self.n + lead, rows, cols, ld)
        self.n = h.start + rows * ld
        if out:
            self.outs.append(h)
        return h

    def upload(self):
        self.host = np.concatenate(self.chunks + [np.full(8, POISON, np.float32)])
        self.dev = torch.from_numpy(self.host).to(DEV)
        assert self.dev.data_ptr() % 16 == 0
        return self

    def ptr(self, h):
        return None if h is None else self.dev.data_ptr() + 4 * h.start

    def fetch(self):
        torch.cuda.synchronize()
        return self.dev.cpu().numpy()

    @staticmethod
    def read(after, h):
        return after[h.start:h.start + h.rows * h.ld].reshape(h.rows, h.ld)[:, :h.cols]

    def unchanged(self, after, written=True):
        """Nothing but the outputs' logical elements has changed (``written=False``: nothing at all)."""
        keep = np.ones(self.host.size, bool)
        if written:
            for h in self.outs:
                keep[h.start:h.start + h.rows * h.ld].reshape(h.rows, h.ld)[:, :h.cols] = False
        return np.array_equal(after.view(np.uint32)[keep], self.host.view(np.uint32)[keep])


class Launch:
    """The groups of one launch (or of the two halves of a paired launch) in one Arena."""

    def __init__(self, layout):
        self.arena, self.specs = Arena(layout), []

    def add(self, case, share_a=None, prefill=None, drop=()):
        """Stage one group; ``share_a``: the spec whose A this group reads; ``prefill``: what C and the column sums hold instead of C_old;
        ``drop``: pointer fields left NULL although the epilogue asks for them."""
        spec = dict(case=case, h={}, problem=None)
        if case.M > 0 and case.N > 0:
            spec["problem"] = _problem(case, share_a["case"] if share_a is not None else None)
            inp, _ = spec["problem"]
            ar, h, epi = self.arena, spec["h"], case.epi
            h["A"] = share_a["h"]["A"] if share_a is not None else ar.put(inp["A"])
            h["B"] = ar.put(inp["B"])
            h["C"] = ar.put(inp["C_old"] if prefill is None else np.full_like(inp["C_old"], prefill), out=True)
            if epi & GC.BIAS:
                h["bias"] = ar.put(inp["bias"])
            if epi & GC.ADD_R:
                h["R"] = ar.put(inp["R"])
            if GC.uses_gate(epi):
                h["gate"] = ar.put(np.array([inp["gate"]], np.float32))
            if case.colsum:
                h["colsum_out"] = ar.put(inp["cs_old"] if prefill is None else np.full_like(inp["cs_old"], prefill), out=True)
            for name in drop:
                h.pop(name)
        self.specs.append(spec)
        return spec

    def upload(self):
        self.arena.upload()
        return self

    def groups(self, specs=None):
        out = []
        for spec in (self.specs if specs is None else specs):
            c, h = spec["case"], spec["h"]
            g = dict(M=c.M, N=c.N, K=c.K)
            for name, hh in h.items():
                g[name] = self.arena.ptr(hh)
            for name, ld in (("A", "lda"), ("B", "ldb"), ("C", "ldc"), ("R", "ldr")):
                if name in h:
                    g[ld] = h[name].ld
            out.append(g)
        return out

    def results(self, after):
        """Per spec: dict(C[, cs]) read from the fetched buffer (None for an empty group)."""
        out = []
        for spec in self.specs:
            h = spec["h"]
            if not h:
                out.append(None)
                continue
            r = dict(C=Arena.read(after, h["C"]))
            if "colsum_out" in h:
                r["cs"] = Arena.read(after, h["colsum_out"])[0]
            out.append(r)
        return out


def _grouped_raw(op, epi, groups, mode="fp32"):
    """wsi_gemm_grouped through the C ABI with its workspace, as ops._gemm makes the call - but with every descriptor (ops._gemm drops the
    empty ones) and the return code instead of an exception."""
    from wsi_hgnn_amd import ops, _native as N
    lib, prec = N.load(), ops._GEMM_MODES[mode]
    arr, n = ops._group_array(groups), len(groups)
    ws_bytes = lib.wsi_gemm_workspace_bytes(OPS[op], prec, arr, n)
    ws = torch.empty(max(ws_bytes // 4, 1), dtype=torch.float32, device=DEV)
    rc = lib.wsi_gemm_grouped(OPS[op], epi, prec, arr, n, ws.data_ptr(), ws_bytes, N.stream())
    torch.cuda.synchronize()
    return rc


def _pair_raw(dx_groups, dx_epi, dw_groups, dw_epi):
    from wsi_hgnn_amd import ops, _native as N
    rc = N.load().wsi_gemm_small_pair(ops._group_array(dx_groups) if dx_groups else None, len(dx_groups), dx_epi,
                                      ops._group_array(dw_groups) if dw_groups else None, len(dw_groups), dw_epi, N.stream())
    torch.cuda.synchronize()
    return rc


def _grouped_ops(op, epi, groups, mode="fp32"):
    from wsi_hgnn_amd import ops
    before = ops.gemm_precision()
    ops.set_gemm_precision(mode)
    try:
        ops._gemm(OPS[op], epi, groups, torch.device(DEV))
    finally:
        ops.set_gemm_precision(before)


def _last_error():
    from wsi_hgnn_amd import _native as N
    return (N.load().wsi_last_error() or b"").decode()


def _hold_to_bound(kernel, case, got, problem=None):
    """Assert the derived bound on C (and the column sums) of one group and keep the module's worst figure per kernel."""
    _, ref = problem or _problem(case)
    r = GC.worst_ratio(case, got["C"], ref)
    if case.colsum:
        r = max(r, GC.worst_ratio(case, got["cs"], ref, "cs"))
    if r >= RATIOS.get(kernel, (-1.0, None))[0]:
        RATIOS[kernel] = (r, GC.case_id(case))
    assert r <= 1.0, (kernel, GC.case_id(case), r)


def _kernel_name(case, mb=None):
    return "TN" if case.op == "TN" else f"{case.op} x{mb or GC.accumulators(case)}"


# ------------------------------------------------------------------------------------------------ a, b: the tables
@functools.lru_cache(maxsize=None)
def _table_run(case, mode):
    L = Launch(case.layout)
    L.add(case)
    L.upload()
    _grouped_ops(case.op, case.epi, L.groups(), mode)
    after = L.arena.fetch()
    assert L.arena.unchanged(after), (GC.case_id(case), mode, "padding, sentinels or inputs were written")
    return L.results(after)[0]


@pytest.mark.parametrize("case", GC.all_cases(), ids=GC.case_id)
def test_table_row_meets_the_derived_bound(case):
    _hold_to_bound(_kernel_name(case), case, _table_run(case, "fp32"))


@pytest.mark.parametrize("case", GC.all_cases(), ids=GC.case_id)
def test_table_row_has_the_same_bits_under_every_precision_mode(case):
    want = _table_run(case, "fp32")
    for mode in MODES[1:]:
        got = _table_run(case, mode)
        assert all(np.array_equal(_bits(got[k]), _bits(want[k])) for k in want), (GC.case_id(case), mode)


@pytest.mark.parametrize("op", ["NT", "NN", "TN"])
def test_one_past_the_limit_takes_the_tiles(op):
    """M = 33 (K = 33 for TN), same generator: bf16x6 no longer equals fp32 bit for bit - the witness that the equality of the test above
    says something - and every mode meets the tiled kernels' own tolerance (test_gemm_nt_bias: 2e-6; test_gemm_backward: 5e-6 for TN)."""
    case = (GC.Case("TN", 300, 7, GC.SKINNY_K + 1, 0, True, "dense", 401) if op == "TN" else
            GC.Case(op, GC.SKINNY_M + 1, 130, 515, GC.BIAS | GC.SCALE_GATE, False, "dense", 400 + OPS[op]))
    _, ref = _problem(case)
    tol = 5e-6 if op == "TN" else 2e-6
    runs = {mode: _table_run(case, mode) for mode in MODES}
    for mode, got in runs.items():
        print(f"\n{op} {mode}: relerr {_relerr(got['C'], ref['C']):.3e}", end="")
        assert _relerr(got["C"], ref["C"]) < tol, (op, mode)
        if case.colsum:
            assert _relerr(got["cs"], ref["cs"]) < tol, (op, mode, "colsum")
    assert not np.array_equal(_bits(runs["bf16x6"]["C"]), _bits(runs["fp32"]["C"]))


# ------------------------------------------------------------------------------------------------ c: several groups
def _stage_multi(cases, prefill=None):
    L = Launch(cases[0].layout)
    for i, c in enumerate(cases):
        L.add(c, share_a=L.specs[GC.MULTI_SHARED_A[0]] if i == GC.MULTI_SHARED_A[1] else None, prefill=prefill)
    return L.upload()


@pytest.mark.parametrize("maxm", [8, 16, 32])
@pytest.mark.parametrize("op", ["NT", "NN"])
def test_launch_of_24_unequal_groups(op, maxm):
    for epi in (GC.BIAS | GC.SCALE_GATE, GC.ALL_FIVE):
        cases = GC.multi_rows_groups(op, maxm, epi)
        L = _stage_multi(cases)
        assert _grouped_raw(op, epi, L.groups()) == 0, _last_error()
        after = L.arena.fetch()
        assert L.arena.unchanged(after)
        for spec, got in zip(L.specs, L.results(after)):
            if got is not None:
                _hold_to_bound(_kernel_name(spec["case"], maxm), spec["case"], got, spec["problem"])


def test_launch_of_24_unequal_groups_tn():
    for epi in (0, GC.ACCUMULATE | GC.SCALE_GATE):
        cases = GC.multi_tn_groups(epi)
        L = _stage_multi(cases)
        assert _grouped_raw("TN", epi, L.groups()) == 0, _last_error()
        after = L.arena.fetch()
        assert L.arena.unchanged(after)
        for spec, got in zip(L.specs, L.results(after)):
            if got is not None:
                _hold_to_bound("TN", spec["case"], got, spec["problem"])


@pytest.mark.parametrize("op", ["NT", "NN", "TN"])
def test_one_group_past_the_limit_moves_the_whole_launch_to_the_tiles(op, gemm_mode):
    """Group 0 grows to 33 rows (TN: 33 reduction rows): wsi_gemm_grouped decides per CALL, so all 24 take the 128 x 128 tiles - and each still
    meets the existing tolerance of those kernels."""
    epi = GC.ACCUMULATE | GC.SCALE_GATE if op == "TN" else GC.ALL_FIVE
    cases = GC.multi_tn_groups(epi) if op == "TN" else GC.multi_rows_groups(op, 32, epi)
    cases[0] = cases[0]._replace(K=GC.SKINNY_K + 1, seed=77) if op == "TN" else cases[0]._replace(M=GC.SKINNY_M + 1, seed=77)
    L = _stage_multi(cases)
    assert _grouped_raw(op, epi, L.groups(), gemm_mode) == 0, _last_error()
    after = L.arena.fetch()
    assert L.arena.unchanged(after)
    tol = 5e-6 if op == "TN" else 2e-6
    for spec, got in zip(L.specs, L.results(after)):
        if got is None:
            continue
        c, (_, ref) = spec["case"], spec["problem"]
        assert _relerr(got["C"], ref["C"]) < tol, (GC.case_id(c), gemm_mode, _relerr(got["C"], ref["C"]))
        if c.colsum:
            assert _relerr(got["cs"], ref["cs"]) < tol, (GC.case_id(c), gemm_mode, "colsum")


# ------------------------------------------------------------------------------------------------ d: the paired launch
def _stage_pair(dx, dw, prefill=None):
    L = Launch(dx[0].layout if dx else dw[0].layout)
    sx = [L.add(c, prefill=prefill) for c in dx]
    sw = [L.add(c, prefill=prefill) for c in dw]
    return L.upload(), sx, sw


@pytest.mark.parametrize("mb", [8, 16, 32])
def test_small_pair_equals_the_two_launches_for_every_epilogue(mb):
    from wsi_hgnn_amd import ops
    for i, dx_epi in enumerate(GC.ROWS_EPILOGUES):
        dw_epi = GC.TN_EPILOGUES[i % 4]
        dx, dw = GC.pair_groups(mb, dx_epi, dw_epi, GC.LAYOUTS[i % 3])
        L, sx, sw = _stage_pair(dx, dw)
        assert ops._gemm_small_pair(L.groups(sx), dx_epi, L.groups(sw), dw_epi, torch.device(DEV))
        paired = L.arena.fetch()
        assert L.arena.unchanged(paired)
        L.upload()                                            # the same bytes again, for the two grouped launches
        _grouped_ops("NN", dx_epi, L.groups(sx))
        _grouped_ops("TN", dw_epi, L.groups(sw))
        two = L.arena.fetch()
        assert np.array_equal(paired.view(np.uint32), two.view(np.uint32)), (mb, dx_epi, dw_epi)
        for c, got in zip(dx + dw, L.results(paired)):
            _hold_to_bound(f"pair {'dW' if c.op == 'TN' else f'dX x{mb}'}", c, got)


def _sixteen(extra=0):
    """10 + extra dX and 6 dW descriptors, an empty one in each half."""
    dx = [GC.Case("NN", (0 if i == 4 else GC.PAIR_DX_M[i % 6]), 3 + i, (1, 7, 64, 65)[i % 4], GC.BIAS, False, "padded", 9900 + i) for i in range(10 + extra)]
    dw = [GC.Case("TN", 5 + i, (0 if i == 2 else 2 + i), GC.PAIR_DW_K[i % 3], GC.ACCUMULATE, True, "padded", 9950 + i) for i in range(6)]
    return dx, dw


def test_small_pair_takes_16_descriptors_skips_the_empty_ones_and_refuses_17():
    from wsi_hgnn_amd import _native as N
    dx, dw = _sixteen()
    L, sx, sw = _stage_pair(dx, dw)
    assert _pair_raw(L.groups(sx), GC.BIAS, L.groups(sw), GC.ACCUMULATE) == 0, _last_error()
    after = L.arena.fetch()
    assert L.arena.unchanged(after)
    for c, got in zip(dx + dw, L.results(after)):
        if got is not None:
            _hold_to_bound("pair dW" if c.op == "TN" else "pair dX x32", c, got)
    dx, dw = _sixteen(extra=1)
    L, sx, sw = _stage_pair(dx, dw, prefill=np.nan)
    assert _pair_raw(L.groups(sx), GC.BIAS, L.groups(sw), GC.ACCUMULATE) == N.WSI_EINVAL
    assert L.arena.unchanged(L.arena.fetch(), written=False)


@pytest.mark.parametrize("which", ["dX of 33 rows", "dW over 33 rows"])
def test_small_pair_refuses_a_group_that_is_not_small_and_writes_nothing(which):
    from wsi_hgnn_amd import _native as N
    dx, dw = GC.pair_groups(32, GC.BIAS, 0)
    if which.startswith("dX"):
        dx[-1] = dx[-1]._replace(M=GC.SKINNY_M + 1, seed=1)
    else:
        dw[-1] = dw[-1]._replace(K=GC.SKINNY_K + 1, seed=2)
    L, sx, sw = _stage_pair(dx, dw, prefill=np.nan)
    assert _pair_raw(L.groups(sx), GC.BIAS, L.groups(sw), 0) == N.WSI_ENOSYS
    after = L.arena.fetch()
    assert L.arena.unchanged(after, written=False)
    assert all(np.isnan(v).all() for got in L.results(after) for v in got.values())


# ------------------------------------------------------------------------------------------------ e: ADD_R without R
@pytest.mark.parametrize("M", [GC.SKINNY_M, GC.SKINNY_M + 1])
@pytest.mark.parametrize("op", ["NT", "NN"])
def test_add_r_without_r_is_refused_on_both_sides_of_the_limit(op, M):
    """The tiled path always answered WSI_EINVAL ("ADD_R needs R"); the skinny path dropped the term and answered OK, so the same call
    changed its answer between M = 32 and M = 33.  Also with a first group that has its R: nothing of the launch may run."""
    from wsi_hgnn_amd import _native as N
    for epi in (GC.ADD_R, GC.ALL_FIVE):
        good = GC.Case(op, 8, 5, 65, epi, False, "dense", 600)
        bad = GC.Case(op, M, 7, 64, epi, False, "dense", 601 + M)
        for cases in ([bad], [good, bad]):
            L = Launch("dense")
            for c in cases:
                L.add(c, prefill=np.nan, drop=("R",) if c is bad else ())
            L.upload()
            assert _grouped_raw(op, epi, L.groups()) == N.WSI_EINVAL, (epi, len(cases))
            assert "ADD_R needs R" in _last_error()
            assert L.arena.unchanged(L.arena.fetch(), written=False)
        L = Launch("dense")                                   # the next valid call works
        L.add(bad)
        L.upload()
        assert _grouped_raw(op, epi, L.groups()) == 0, _last_error()
        after = L.arena.fetch()
        assert L.arena.unchanged(after)
        got = L.results(after)[0]
        if M <= GC.SKINNY_M:
            _hold_to_bound(_kernel_name(bad), bad, got)
        else:
            assert _relerr(got["C"], _problem(bad)[1]["C"]) < 2e-6


@pytest.mark.parametrize("M", [GC.SKINNY_M, GC.SKINNY_M + 1])
def test_small_pair_refuses_add_r_without_r_and_negative_dimensions(M):
    from wsi_hgnn_amd import _native as N
    epi = GC.ADD_R | GC.R_1MG
    good = GC.Case("NN", 8, 5, 65, epi, False, "dense", 700)
    bad = GC.Case("NN", M, 7, 64, epi, False, "dense", 701 + M)
    dw = GC.Case("TN", 5, 3, 8, 0, True, "dense", 703)
    L = Launch("dense")
    sx = [L.add(good, prefill=np.nan), L.add(bad, prefill=np.nan, drop=("R",))]
    sw = [L.add(dw, prefill=np.nan)]
    L.upload()
    assert _pair_raw(L.groups(sx), epi, L.groups(sw), 0) == N.WSI_EINVAL
    assert "ADD_R needs R" in _last_error()
    assert L.arena.unchanged(L.arena.fetch(), written=False)
    # a negative dimension: WSI_EINVAL as from wsi_gemm_grouped, in either half
    for half in (0, 1):
        gx, gw = L.groups(sx[:1]), L.groups(sw)
        (gx, gw)[half][0]["M"] = -1
        assert _pair_raw(gx, epi, gw, 0) == N.WSI_EINVAL
        assert "negative dimension" in _last_error()
        assert L.arena.unchanged(L.arena.fetch(), written=False)
    # the next valid call works
    ok = bad._replace(M=GC.SKINNY_M)
    L = Launch("dense")
    sx, sw = [L.add(good), L.add(ok)], [L.add(dw)]
    L.upload()
    assert _pair_raw(L.groups(sx), epi, L.groups(sw), 0) == 0, _last_error()
    after = L.arena.fetch()
    assert L.arena.unchanged(after)
    for c, got in zip((good, ok, dw), L.results(after)):
        _hold_to_bound("pair dW" if c.op == "TN" else "pair dX x32", c, got)


# ------------------------------------------------------------------------------------------------ f: the split-K reduction
SPLITK_K = (256, 700, 1024, 1100, 2100)
SPLITK_SHAPES = {"vector": ((12, 8),), "scalar": ((7, 5),), "three groups, odd offset": ((3, 5), (4, 8), (6, 4))}


def _pad4(x):
    return (x + 3) // 4 * 4


@pytest.mark.parametrize("form", list(SPLITK_SHAPES))
def test_splitk_reduction_over_one_to_nine_slabs(form, gemm_mode):
    """TN launches of one output tile per group and K rows: the exact-fp32 and bf16x6 kernels (modes fp32, bf16x6, auto) cut K into slabs of
    256 rows - 1, 3, 4, 5 and 9 of them - and the column-scaled kernel of fp16x3 into slabs of 128 - 2, 6, 8, 9 and 17; the workspace size
    says so, and if a plan ever changes this fails and the K are picked again.  N % 4 == 0 alone: splitk_reduce_kernel<true>; N = 5: <false>;
    three groups whose second starts at flat element 15: <false> for all.  Tolerance: test_gemm_backward's."""
    from wsi_hgnn_amd import ops, _native as N
    lib, prec = N.load(), ops._GEMM_MODES[gemm_mode]
    shapes = SPLITK_SHAPES[form]
    assert all(M <= 128 and Nn <= 128 for M, Nn in shapes) and (len(shapes) == 1 or shapes[0][0] * shapes[0][1] % 2 == 1)
    for K in SPLITK_K:
        for epi, colsum in ((0, False), (GC.SCALE_GATE | GC.ACCUMULATE, True)):
            cases = [GC.Case("TN", M, Nn, K, epi, colsum, "dense", 8000 + K + i) for i, (M, Nn) in enumerate(shapes)]
            L = Launch("dense")
            for c in cases:
                L.add(c)
            L.upload()
            groups = L.groups()
            arr = ops._group_array(groups)
            if lib.wsi_gemm_kernel_precision(N.WSI_GEMM_TN, prec, arr, len(groups)) == N.WSI_GEMM_FP16X3:
                slabs, chunks = -(-K // 128), -(-K // 256)
                floats = _pad4(sum(slabs * M * Nn for M, Nn in shapes)) + sum(
                    (_pad4(M) + _pad4(Nn)) * (1 + chunks) + (_pad4(M) * chunks if colsum else 0) for M, Nn in shapes)
            else:
                slabs = -(-K // 256)
                assert slabs == {256: 1, 700: 3, 1024: 4, 1100: 5, 2100: 9}[K]
                floats = sum(slabs * M * Nn + (slabs * _pad4(M) if colsum else 0) for M, Nn in shapes)
            assert lib.wsi_gemm_workspace_bytes(N.WSI_GEMM_TN, prec, arr, len(groups)) == 4 * floats, (form, gemm_mode, K, colsum)
            ops._gemm(N.WSI_GEMM_TN, epi, groups, torch.device(DEV))
            after = L.arena.fetch()
            assert L.arena.unchanged(after)
            for c, got in zip(cases, L.results(after)):
                _, ref = _problem(c)
                assert _relerr(got["C"], ref["C"]) < 5e-6, (form, gemm_mode, K, GC.case_id(c), _relerr(got["C"], ref["C"]))
                if colsum:
                    assert _relerr(got["cs"], ref["cs"]) < 5e-6, (form, gemm_mode, K, GC.case_id(c), "colsum")


# ------------------------------------------------------------------------------------------------ g: wsi_row_absmax
ABSMAX_COLS = (1, 3, 4, 5, 255, 256, 257, 1023, 1024)


def _absmax_input(rows, cols, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(rows, cols, generator=g) * torch.exp2(torch.randint(-20, 20, (rows, 1), generator=g).float())
    special = torch.tensor([-0.0, 1e-40, -3e-42, 0.0, float("nan")])
    pick = torch.rand(rows, cols, generator=g) < 0.1
    x[pick] = special[torch.randint(0, 5, (int(pick.sum()),), generator=g)]
    x[0, 0] = float("nan")                                   # a NaN element is dropped, also in front of a row
    if rows > 1:
        x[1] = 0.0
        x[1, ::2] = -0.0                                     # a row of zeros of both signs: bits 0
    if rows > 2:
        x[2, cols // 2] = float("-inf")
    if rows > 3:
        x[3] = torch.randn(cols, generator=g) * 1e-41        # a row of denormals alone: its maximum is one
    for r in range(7, rows, 10):
        x[r, (r * 7) % cols] = float("inf")
    return x


@pytest.mark.parametrize("rows", [1, 4, 5, 1000])
def test_row_absmax_equals_torch_exactly(rows):
    """``wsi_row_absmax`` serves as the expected value of five other tests; here it is held against torch: every bit of every row, the vector
    path (16-byte aligned rows), the scalar path (ld = cols + 3, or a base 4 bytes in), cols from one lane's worth to several trips."""
    from wsi_hgnn_amd import _native as N
    lib = N.load()
    for cols in ABSMAX_COLS:
        x = _absmax_input(rows, cols, 100 * rows + cols)
        want = torch.where(x.isnan(), torch.zeros_like(x), x.abs()).max(1).values.view(torch.int32)
        if rows > 1:
            assert want[1] == 0
        for pad in (0, 3):
            for base in (0, 1):
                ld = cols + pad
                buf = torch.full((base + rows * ld + 4,), POISON)
                buf[base:base + rows * ld].view(rows, ld)[:, :cols] = x
                dbuf = buf.to(DEV)
                out = torch.full((rows + 16,), -7777, dtype=torch.int32, device=DEV)
                assert lib.wsi_row_absmax(dbuf.data_ptr() + 4 * base, ld, rows, cols, out.data_ptr() + 4 * 8, N.stream()) == 0, _last_error()
                got = out.cpu()
                assert torch.equal(got[8:8 + rows], want), (rows, cols, pad, base)
                assert (got[:8] == -7777).all() and (got[8 + rows:] == -7777).all()
                assert torch.equal(dbuf.cpu().view(torch.int32), buf.view(torch.int32))
    # a single row of zeros
    z = torch.zeros(1, 5, device=DEV)
    out = torch.full((1,), -1, dtype=torch.int32, device=DEV)
    assert lib.wsi_row_absmax(z.data_ptr(), 5, 1, 5, out.data_ptr(), N.stream()) == 0
    assert out.item() == 0
