"""What the segment-tail tests share (no test functions, no GPU, no library): the cases and float64 references for the segment dots
(``wsi_segment_dot_diff``, ``wsi_gate_grad``), the weighted sums (``wsi_segment_weighted_sums``, ``wsi_pool_factors``) and the loss kernel
(``wsi_cross_entropy``) of csrc/segment.hip and csrc/loss.hip.

Segments.  ``SEG_SIZES`` in chunks of 128 rows: empty segments at the start, in the middle and at the end, segments with fewer rows than the
workgroup's four waves, 127 / 128 / 129 rows around a chunk edge, one segment of three chunks; 695 rows.  ``PLAN7`` is the same list starting at
row 7 with rows behind the last segment; ``PLAN_LONG`` holds one segment of 71 chunks, more partials than the 64 lanes of the second stage.

Layouts.  ``LAYOUTS`` gives (offset of the first element in floats, row stride) of a D-wide table; csrc/common.h's ``vec_ok`` (16-byte base,
row stride a multiple of 4) is restated as ``vec_ok``.  ``embed`` puts a table into a NaN-filled buffer: padding columns, the float(s) in front
of an offset base and the rows outside the plan read NaN.

Two families of inputs.
  integers   small nonzero integers: every product and every partial sum is an integer below 2^24, so fp32 is exact in ANY order of summation
             and the check is equality with the float64 reference (``exact_condition`` is what the CPU test asserts for every case);
  gaussian   randn (for the dots also ``cancelling``: a = b + 1e-3 randn).  Every output entry is judged against ITS OWN scale - the float64
             sum of the absolute values of its terms - with the bound  n_chain * 2^-24 * scale,  n_chain = the longest chain of roundings into
             the entry, read off the kernels (``n_chain_dot``, ``n_chain_wsum``).  A derived worst case; no measured margin goes into it."""
import functools

import torch

U = 2.0 ** -24                       # unit roundoff of fp32
CHUNK = 128                          # rows per chunk (ReducePlan.from_ranges' default)
SEG_SIZES = (0, 1, 2, 3, 5, 127, 128, 129, 0, 300, 0)
NAN = float("nan")


def cdiv(a, b):
    return -(-a // b)


# ---------------------------------------------------------------------------------------------------- plans
class Plan:
    """Host chunk tables of contiguous segments (what ops.ReducePlan.from_ranges builds): chunk c covers rows [chunk_row[c], chunk_row[c+1]),
    the chunks of segment s are [seg_chunk[s], seg_chunk[s+1]).  ``tail_rows`` rows behind the last segment belong to no segment."""

    def __init__(self, name, sizes, first_row=0, tail_rows=0):
        self.name, self.sizes, self.first_row = name, tuple(int(n) for n in sizes), first_row
        self.ranges, pos = [], first_row
        for n in self.sizes:
            self.ranges.append((pos, pos + n))
            pos += n
        self.end_row, self.total_rows = pos, pos + tail_rows
        self.chunk_row, self.chunk_seg, self.seg_chunk = [], [], [0]
        for s, (a, b) in enumerate(self.ranges):
            for r in range(a, b, CHUNK):
                self.chunk_row.append(r)
                self.chunk_seg.append(s)
            self.seg_chunk.append(len(self.chunk_row))
        self.chunk_row.append(pos)
        self.num_segs, self.num_chunks = len(self.sizes), len(self.chunk_seg)

    def live(self):
        m = torch.zeros(self.total_rows, dtype=torch.bool)
        m[self.first_row:self.end_row] = True
        return m


PLAN = Plan("base", SEG_SIZES)
PLAN7 = Plan("row7", SEG_SIZES, first_row=7, tail_rows=5)
PLAN_LONG = Plan("long", (0, 70 * CHUNK + 3, 1))           # 71 chunks in one segment: the second stage's lanes take more than one partial
PLAN_EMPTY = Plan("empty", (0, 0, 0))                       # num_chunks == 0
MAX_ROWS = max(p.total_rows for p in (PLAN, PLAN7, PLAN_LONG))


@functools.lru_cache(maxsize=None)
def pool_plan(T, Bg, variant=0):
    """The T * Bg source segments of a wsi_pool_factors case: SEG_SIZES repeated or cut.  A single segment cannot be empty AND hold one row:
    S = 1 runs as three variants (empty, one row, 129 rows)."""
    S = T * Bg
    if S == 1:
        return Plan(f"pool1v{variant}", ((0,), (1,), (129,))[variant])
    return Plan(f"pool{S}", (SEG_SIZES * cdiv(S, len(SEG_SIZES)))[:S])


def pool_variants(T, Bg):
    return (0, 1, 2) if T * Bg == 1 else (0,)


# ---------------------------------------------------------------------------------------------------- layouts
def ceil4(D):
    return cdiv(D, 4) * 4


LAYOUTS = {                                   # name -> (first element, in floats from the 16-byte aligned start of the buffer; row stride)
    "plain": lambda D: (0, D),                # 16-byte accesses exactly when D % 4 == 0
    "pad4": lambda D: (0, ceil4(D) + 4),      # 16-byte accesses, a scalar tail when D % 4 != 0, at least four padding columns
    "pad1": lambda D: (0, D + 1),             # scalar (but for D % 4 == 3, where D + 1 is a multiple of 4), one padding column
    "offset": lambda D: (1, ceil4(D)),        # base 4 bytes into the buffer under a stride that would allow 16-byte accesses: scalar
}
X_LAYOUTS = ("plain", "pad4", "pad1", "offset")
DOT_LAYOUTS = X_LAYOUTS + ("mixed",)


def vec_ok(off, ld):
    """csrc/common.h: the base is 16-byte aligned and the row stride a multiple of four floats."""
    return (off * 4) % 16 == 0 and ld % 4 == 0


def dot_layouts(layout, D):
    """(layout of g, of a, of b).  ``mixed``: ONE operand offset (which one turns with D), the others plain - all three must go scalar."""
    if layout != "mixed":
        return (layout,) * 3
    return tuple("offset" if i == D % 3 else "plain" for i in range(3))


def dot_vec(layout, D):
    """What the dot kernels' ``vec`` comes to: every operand must allow 16-byte accesses."""
    return all(vec_ok(*LAYOUTS[name](D)) for name in dot_layouts(layout, D))


def embed(table, layout, live=None):
    """(flat NaN-filled buffer, offset, row stride): ``table`` [rows, D] at the layout's place; rows outside ``live`` NaN as well."""
    rows, D = table.shape
    off, ld = LAYOUTS[layout](D)
    buf = torch.full((off + rows * ld + 3,), NAN, dtype=torch.float32)
    view = buf[off:off + rows * ld].view(rows, ld)
    view[:, :D] = table
    if live is not None:
        view[~live] = NAN
    return buf, off, ld


def embed_ld(table, ld):
    """``table`` [rows, J] under row stride ld >= J at offset 0, NaN padding."""
    rows, J = table.shape
    buf = torch.full((rows, ld), NAN, dtype=torch.float32)
    buf[:, :J] = table
    return buf.reshape(-1)


# ---------------------------------------------------------------------------------------------------- the dots
DOT_D = (1, 3, 4, 5, 67, 255, 256, 257, 260, 513, 1027)
DOT_D_ROW7 = (5, 260)
DOT_D_LONG = (5, 8, 67)               # 8: no scalar tail, so only the second stage can go wrong there
GATE_D = (3, 256, 257, 1027)
DOT_FAMILIES = ("integers", "gaussian", "cancelling")
DMAX = max(DOT_D)


def _pick(values, shape, gen):
    v = torch.tensor(values, dtype=torch.float32)
    return v[torch.randint(0, len(values), shape, generator=gen)]


@functools.lru_cache(maxsize=None)
def dot_tables(family, rows, width):
    """g, a, b [rows, width] of a family; a case takes the first rows / columns it needs."""
    gen = torch.Generator().manual_seed({"integers": 101, "gaussian": 102, "cancelling": 103}[family] + rows)
    if family == "integers":                 # g (a - b): a - b in {1, 2, 3, 4}, no term is zero, |term| <= 8
        return _pick((-2, -1, 1, 2), (rows, width), gen), _pick((1, 2, 3), (rows, width), gen), _pick((-1, 0), (rows, width), gen)
    g, b = torch.randn(rows, width, generator=gen), torch.randn(rows, width, generator=gen)
    if family == "cancelling":
        return g, b + 1e-3 * torch.randn(rows, width, generator=gen), b
    return g, torch.randn(rows, width, generator=gen), b


def dot_inputs(family, plan, D):
    """g, a, b [plan.total_rows, D] fp32 (rows outside the plan are poisoned by ``embed``)."""
    rows, width = (MAX_ROWS, max(DOT_D_LONG)) if plan.total_rows > 1024 else (1024, DMAX)
    return tuple(t[:plan.total_rows, :D] for t in dot_tables(family, rows, width))


def n_chain_dot(n_rows, D):
    """Roundings on the longest path into one segment dot (csrc/segment.hip).  Stage 1, per chunk and 256-column tile: a thread runs ONE fma
    chain over its (up to) four columns of every fourth row of the chunk; six wave_sum steps; two levels (sh[0] + sh[1]) + (sh[2] + sh[3]).
    Stage 2 (seg_dot_stage2 and gate_grad_stage2 alike): a lane adds every 64th partial of the segment, then six wave_sum steps.  One more
    for the rounding of a - b inside each term."""
    if n_rows == 0:
        return 0
    fmas = min(4, D) * cdiv(min(n_rows, CHUNK), 4)
    partials = cdiv(n_rows, CHUNK) * cdiv(D, 256)
    return 1 + fmas + 6 + 2 + cdiv(partials, 64) + 6


@functools.lru_cache(maxsize=None)
def _dot_reference(family, plan, D):
    g, a, b = (t.double() for t in dot_inputs(family, plan, D))
    terms = g * (a - b)
    ref, scale = torch.zeros(plan.num_segs, dtype=torch.float64), torch.zeros(plan.num_segs, dtype=torch.float64)
    for s, (r0, r1) in enumerate(plan.ranges):
        ref[s], scale[s] = terms[r0:r1].sum(), terms[r0:r1].abs().sum()
    chain = torch.tensor([n_chain_dot(n, D) for n in plan.sizes], dtype=torch.float64)
    return ref, scale, chain * U * scale


def dot_reference(family, plan, D):
    """(float64 dots [S], their scales = sum of |term|, the bound n_chain * 2^-24 * scale).  Shared: do not write into them."""
    return _dot_reference(family, plan, D)


def exact_condition(scale):
    """Every partial sum of integer terms is an integer of magnitude <= sum of |term|: below 2^24 fp32 holds it exactly, in any order."""
    return float(scale.max()) < 2.0 ** 24 if scale.numel() else True


# ---------------------------------------------------------------------------------------------------- the gate gradient
GATE_MAPS = {              # n_gates -> seg_gate over the 11 segments (sizes 0 1 2 3 5 127 128 129 0 300 0)
    1: (0, 0, -1, 0, 0, 0, -1, 0, 0, 0, 0),             # every gated segment on the one gate
    3: (1, 0, -1, 2, 0, 2, -1, 0, 1, 2, 1),             # gate 1 is fed by the three EMPTY segments only; gates 0 and 2 by three segments each
    300: (1, 0, -1, 299, 0, 257, -1, 0, 1, 299, 257),   # gates beyond the first 256 (the second turn of the gate loop); 295 gates nobody feeds
}
SKIP_KINDS = ("randn", "saturated", "zero")


def gate_skip(kind, n_gates):
    if kind == "randn":
        return torch.randn(n_gates, generator=torch.Generator().manual_seed(7 + n_gates))
    if kind == "saturated":                             # the factor 1 - sigmoid saturates to 0 (+30) and to 1 (-30)
        return torch.tensor([30.0, -30.0] * cdiv(n_gates, 2))[:n_gates].clone()
    if kind == "zero":
        return torch.zeros(n_gates)
    return torch.full((n_gates,), float(kind))          # a number: that value everywhere (-100: the factor is exactly 1.0 in fp32)


def gate_reference(dots, dot_bounds, seg_gate, skip, n_gates):
    """(g_skip [n_gates] float64, its bound) from float64 segment dots:  g_skip[gate] = (1 - sigmoid(skip[gate])) * sum of the dots of the
    segments mapped to it.  Bound: the members' dot bounds times the factor, plus 4 * 2^-24 * |sum of dots| for the sigmoid arithmetic
    (expf, 1 + e, the division, 1 - q: four roundings of a factor that is at most 1)."""
    sums, bsum = torch.zeros(n_gates, dtype=torch.float64), torch.zeros(n_gates, dtype=torch.float64)
    for s, gt in enumerate(seg_gate):
        if gt >= 0:
            sums[gt] += dots[s]
            bsum[gt] += dot_bounds[s]
    factor = 1.0 - torch.sigmoid(skip.double())
    return sums * factor, bsum * factor + 4 * U * sums.abs(), sums


def many_segments(num_segs, n_gates=3):
    """One row per segment at D = 4, integers: (plan, seg_gate) for the num_segs limit of wsi_gate_grad."""
    return Plan(f"segs{num_segs}", (1,) * num_segs), tuple((s % (n_gates + 1)) - 1 for s in range(num_segs))


# ---------------------------------------------------------------------------------------------------- the weighted sums
WSUM_D = (1, 3, 4, 5, 255, 256, 257, 260)
WSUM_J = (1, 15, 16, 17, 32, 33)
WSUM_FAMILIES = ("integers", "gaussian")
POOL_SHAPES = ((1, 1, 1), (2, 8, 1), (4, 4, 2), (3, 5, 3), (16, 2, 1))      # (T, H, Bg): T * H = 1, 16, 16, 15, 32
POOL_D = (3, 256, 260)
WSUM_ROWS = 720                              # >= the rows of every weighted-sum plan


@functools.lru_cache(maxsize=None)
def wsum_tables(family, J=max(WSUM_J)):
    """x [WSUM_ROWS, 260], w [WSUM_ROWS, J]; a case takes the first rows / columns it needs."""
    gen = torch.Generator().manual_seed({"integers": 201, "gaussian": 202}[family] + J)
    if family == "integers":
        return _pick((-3, -2, -1, 1, 2, 3), (WSUM_ROWS, max(WSUM_D)), gen), _pick((-2, -1, 1, 2), (WSUM_ROWS, J), gen)
    return torch.randn(WSUM_ROWS, max(WSUM_D), generator=gen), torch.randn(WSUM_ROWS, J, generator=gen)


def wsum_inputs(family, plan, D, J):
    x, w = wsum_tables(family, max(J, max(WSUM_J)))
    return x[:plan.total_rows, :D], w[:plan.total_rows, :J]


def n_chain_wsum(n_rows):
    """Roundings on the longest path into one weighted sum.  seg_wsum_stage1: a thread runs one fma per row over every fourth row of the
    chunk; two levels across the four waves.  Stage 2 (seg_stage2<SUM>, pool_factors_stage2): one chain over the segment's chunks.  The sums
    of the weights alone (csum) take the same path with adds for fmas."""
    if n_rows == 0:
        return 0
    return cdiv(min(n_rows, CHUNK), 4) + 2 + cdiv(n_rows, CHUNK)


def weighted_sums_reference(x, w, plan):
    """float64 out [S, J, D] = w[rows].T @ x[rows], its scale |w|.T @ |x|, the bound; and the same for the sums of the weights [S, J]."""
    x, w = x.double(), w.double()
    S, J, D = plan.num_segs, w.shape[1], x.shape[1]
    out, scale = torch.zeros(S, J, D, dtype=torch.float64), torch.zeros(S, J, D, dtype=torch.float64)
    ws, wscale = torch.zeros(S, J, dtype=torch.float64), torch.zeros(S, J, dtype=torch.float64)
    for s, (r0, r1) in enumerate(plan.ranges):
        out[s], scale[s] = w[r0:r1].t() @ x[r0:r1], w[r0:r1].abs().t() @ x[r0:r1].abs()
        ws[s], wscale[s] = w[r0:r1].sum(dim=0), w[r0:r1].abs().sum(dim=0)
    chain = torch.tensor([n_chain_wsum(n) for n in plan.sizes], dtype=torch.float64)
    return dict(out=out, scale=scale, bound=chain.view(S, 1, 1) * U * scale, ws=ws, wscale=wscale, wbound=chain.view(S, 1) * U * wscale)


@functools.lru_cache(maxsize=None)
def wsum_reference(family, plan, D, J):
    """Shared: do not write into it."""
    return weighted_sums_reference(*wsum_inputs(family, plan, D, J), plan)


def permute_hp(t, T, H, Bg):
    """[source seg = tau * Bg + g][j = b * H + hh][D] -> hp [seg = b * Bg + g][hh][tau][D]."""
    return t.view(T, Bg, T, H, -1).permute(2, 1, 3, 0, 4).reshape(T * Bg, H, T, -1)


def permute_csum(t, T, H, Bg):
    """[source seg = tau * Bg + g][j = b * H + hh] -> csum [tau][seg = b * Bg + g][hh]."""
    return t.view(T, Bg, T, H).permute(0, 2, 1, 3).reshape(T, T * Bg, H)


def pool_reference(x, w, plan, T, H, Bg):
    """float64 hp [S][H][T][D], csum [T][S][H], x_mean [S][D] (0 for an empty segment) of wsi_pool_factors, each with its bound.  x_mean: the
    sum's chain and one more rounding for the division, against the scale sum |x| / rows."""
    r = weighted_sums_reference(x, w, plan)
    x = x.double()
    S, D = plan.num_segs, x.shape[1]
    mean, mbound = torch.zeros(S, D, dtype=torch.float64), torch.zeros(S, D, dtype=torch.float64)
    for s, (r0, r1) in enumerate(plan.ranges):
        if r1 > r0:
            mean[s] = x[r0:r1].mean(dim=0)
            mbound[s] = (n_chain_wsum(r1 - r0) + 1) * U * x[r0:r1].abs().sum(dim=0) / (r1 - r0)
    return dict(hp=permute_hp(r["out"], T, H, Bg), hp_bound=permute_hp(r["bound"], T, H, Bg), hp_scale=permute_hp(r["scale"], T, H, Bg),
                csum=permute_csum(r["ws"], T, H, Bg), csum_bound=permute_csum(r["wbound"], T, H, Bg), csum_scale=permute_csum(r["wscale"], T, H, Bg),
                x_mean=mean, x_mean_bound=mbound)


def integer_mean_bound(mean, plan):
    """The integers family: the sum is exact, the division rounds once - exact where the row count is a power of two (the quotient of an
    integer below 2^24 by it is a float), elsewhere 2 * 2^-24 * |mean|."""
    pow2 = torch.tensor([n > 0 and n & (n - 1) == 0 for n in plan.sizes]).view(-1, 1)
    return torch.where(pow2, torch.zeros_like(mean), 2 * U * mean.abs())


# ---------------------------------------------------------------------------------------------------- cross entropy
CE_LOSS_TOL, CE_GRAD_TOL = 2e-6, 1e-6        # the project's tolerances for this kernel: loss 2e-6 * max(1, |ref|), gradient 1e-6 absolute
CE_IGNORE = -100
CE_LIMIT = 65536                             # B * C of the one-workgroup kernel


def _ce_large(mag, B, C, gen):
    """|logit| in [mag, 1.2 mag] with random signs, one entry of +1.2 mag in every row (96 for mag = 80: expf of the raw logit overflows
    fp32 above 88.7)."""
    x = mag * (1 + 0.2 * torch.rand(B, C, generator=gen)) * (torch.randint(0, 2, (B, C), generator=gen) * 2 - 1).float()
    x[torch.arange(B), torch.randint(0, C, (B,), generator=gen)] = 1.2 * mag
    return x


@functools.lru_cache(maxsize=None)
def ce_cases():
    """name -> (logits [B, C] fp32, labels [B] int64)."""
    gen = torch.Generator().manual_seed(301)
    cases = {}
    for mag in (80.0, 1e4):
        x = _ce_large(mag, 67, 7, gen)
        cases[f"large{mag:g}"] = (x, torch.randint(0, 7, (67,), generator=gen))
        cases[f"large{mag:g}_target_is_max"] = (x, x.argmax(dim=1))
    x, y = torch.randn(9, 5, generator=gen) * 3, torch.randint(0, 5, (9,), generator=gen)
    x[2] = float("-inf")
    x[2, y[2]] = 1.5                         # a row whose non-target entries are -inf
    x[5] = float("-inf")
    x[5, y[5]] = -1e4
    cases["neg_inf"] = (x, y)
    x = torch.randn(6, 4, generator=gen)
    x[1, 0] = x[1, 3] = 5.0                  # two equal maxima, the target one of them / neither
    x[4, 1] = x[4, 2] = 7.0
    cases["equal_maxima"] = (x, torch.tensor([0, 0, 1, 2, 0, 3]))
    for B, C in ((256, 256), (65536, 1), (1, 65536), (257, 255)):
        cases[f"limit{B}x{C}"] = (torch.randn(B, C, generator=gen) * 3, torch.randint(0, C, (B,), generator=gen))
    for B in (255, 256, 257):                # ignored labels where a thread's first and second row meet
        y = torch.randint(0, 3, (B,), generator=gen)
        for r in (0, 255, 256):
            if r < B:
                y[r] = CE_IGNORE
        cases[f"ignored{B}"] = (torch.randn(B, 3, generator=gen) * 3, y)
    return cases


CE_OVER_LIMIT = ((65537, 1), (1, 65537))


def ce_reference(logits, labels):
    """F.cross_entropy with default arguments on float64 copies: (loss, d loss / d logits)."""
    x = logits.double().requires_grad_(True)
    loss = torch.nn.functional.cross_entropy(x, labels)
    loss.backward()
    return loss.detach(), x.grad


def ce_closed_form(logits, labels):
    """The header's statement in float64: the mean over the valid rows of logsumexp - the target's logit; (softmax - onehot) / #valid, 0 on
    the ignored rows."""
    x = logits.double()
    valid = labels != CE_IGNORE
    n = int(valid.sum())
    y = labels.clamp(min=0)
    lse = torch.logsumexp(x, dim=1)
    loss = ((lse - x.gather(1, y.view(-1, 1)).view(-1))[valid]).sum() / n
    grad = torch.exp(x - lse.view(-1, 1))
    grad[torch.arange(x.shape[0]), y] -= 1.0
    return loss, grad * valid.view(-1, 1) / n
