"""Shape tables, float64 restatement, error bound and an fp32 emulation for the "skinny" GEMM kernels of csrc/gemm_f32.hip
(gemm_skinny_kernel<NT|NN, 8|16|32>, gemm_skinny_kernel<TN, 1>, gemm_skinny_pair_kernel<8|16|32>).  No test functions, no GPU: numpy only.
tests/test_gemm_small_cases.py proves on the CPU that the tables reach what they are here for and that the bound separates the kernels'
arithmetic from three seeded faults; tests/test_gemm_small_gpu.py runs the tables on the device.

The operation (include/wsi_hgnn.h), with s = sigmoid(*gate), gs = s under SCALE_GATE else 1, rs = 1 - s under R_1MG else 1:
    NT  x[m, n] = sum_k A[m, k] B[n, k]        NN  x[m, n] = sum_k A[m, k] B[k, n]        TN  x[m, n] = sum_k A[k, m] B[k, n]
    C = (x + bias[n]) * gs + R[m, n] * rs + C_old[m, n]            (each term only under its epilogue flag; bias and R: NT / NN only)
    TN with colsum_out:  cs[m] = gs * sum_k A[k, m] + cs_old[m]    (cs_old under ACCUMULATE)

The bound, componentwise, u = 2^-24 (first order; the constants round the sums below up):
    NT / NN   |err[m, n]| <= (ceil(K / 64) + 16) u S[m, n],   S = gs (sum_k |a| |b| + |bias|) + |R| + |C_old|
        a lane makes at most ceil(K / 64) fmas, the butterfly adds 6 sums, the epilogue makes at most 5 operations, and the fp32 sigmoid
        (expf, one sum, one division; it enters through gs and through 1 - s) has a share of 5 u;
    TN        |err[m, n]| <= (K + 8) u S[m, n]  (one chain of K fmas, two epilogue operations, the sigmoid), and the same for colsum_out
        with S[m] = gs sum_k |a| + |cs_old|.
Every output row of A carries its own power of two between 2^-6 and 2^6 (R and C_old follow it), so a bound relative to the tensor's largest
entry would let a wrong small row pass; this one does not.
"""
from collections import namedtuple

import numpy as np

U = 2.0 ** -24

# the header's WSI_EPI_* values (tests/test_gemm_small_cases.py holds them against the binding)
BIAS, ACCUMULATE, SCALE_GATE, ADD_R, R_1MG = 1, 2, 4, 16, 32
ALL_FIVE = BIAS | ACCUMULATE | SCALE_GATE | ADD_R | R_1MG
ROWS_EPILOGUES = (0, BIAS, BIAS | SCALE_GATE, ADD_R, ADD_R | R_1MG, ACCUMULATE, ALL_FIVE)      # NT / NN (ADD_R | R_1MG comes with a gate)
TN_EPILOGUES = (0, ACCUMULATE, SCALE_GATE, ACCUMULATE | SCALE_GATE)                               # TN, each with and without colsum_out

ROWS_M = (1, 8, 9, 16, 17, 31, 32)          # both sides of each accumulator count (8 / 16 / 32)
ROWS_N = (1, 3, 4, 5, 130)                  # 130: more than one workgroup of four waves
ROWS_K = (1, 63, 64, 65, 200, 515)          # a lane with no term, exactly one term each, a ragged last trip
TN_K = (1, 8, 31, 32)
TN_MN = ((1, 1), (5, 3), (16, 16), (300, 7))   # 16 x 16 = 256 threads: exactly one workgroup; 300 x 7: several
LAYOUTS = ("dense", "padded", "offset")     # padded: every leading dimension + 1 or + 3; offset: every tensor 4 bytes into its 16-byte line
SKINNY_M = SKINNY_K = 32                    # the kernels' limits: the boundary cases of the GPU tests sit at 33

# one group of a launch.  M, N, K: the GEMM's (TN: K = the reduction rows); colsum: TN with colsum_out
Case = namedtuple("Case", "op M N K epi colsum layout seed")

# NT / NN: chosen rows, not a product.  (M, N, K, index into ROWS_EPILOGUES, layout)
_ROWS = (
    (1, 1, 1, 0, "dense"), (8, 3, 63, 1, "padded"), (9, 4, 64, 2, "offset"), (16, 5, 65, 3, "dense"),
    (17, 130, 200, 4, "padded"), (31, 1, 515, 5, "offset"), (32, 3, 1, 6, "dense"), (1, 130, 64, 6, "padded"),
    (8, 5, 515, 2, "dense"), (9, 130, 65, 5, "padded"), (16, 4, 200, 0, "offset"), (17, 3, 63, 1, "dense"),
    (31, 4, 64, 4, "offset"), (32, 130, 515, 2, "padded"), (32, 5, 200, 3, "offset"), (8, 1, 65, 6, "offset"),
    (16, 130, 515, 6, "dense"), (2, 5, 64, 2, "padded"),
)


def rows_cases():
    out = []
    for op in ("NT", "NN"):
        for i, (M, N, K, e, layout) in enumerate(_ROWS):
            out.append(Case(op, M, N, K, ROWS_EPILOGUES[e], False, layout, 1000 * (1 + (op == "NN")) + i))
    return out


def tn_cases():
    out = []
    for ki, K in enumerate(TN_K):
        for mi, (M, N) in enumerate(TN_MN):
            i = 4 * ki + mi
            out.append(Case("TN", M, N, K, TN_EPILOGUES[(ki + mi) % 4], mi % 2 == 1, LAYOUTS[i % 3], 3000 + i))
    return out


def all_cases():
    return rows_cases() + tn_cases()


def accumulators(case):
    """The MB the launch of this case alone is compiled for (TN: 1)."""
    return 1 if case.op == "TN" else (8 if case.M <= 8 else 16 if case.M <= 16 else 32)


def case_id(case):
    return f"{case.op}-{case.M}x{case.N}x{case.K}-epi{case.epi}{'-cs' if case.colsum else ''}-{case.layout}"


# ------------------------------------------------------------------------------------------------ launches of several groups
_MULTI_M = (32, 1, 17, 8, 9, 16, 31, 0, 2, 24, 5, 32, 13, 1, 7, 4, 20, 3, 30, 11, 6, 0, 27, 4)        # 24 = WSI_GEMM_MAX_GROUPS
_MULTI_N = (130, 1, 3, 64, 4, 5, 17, 5, 129, 2, 130, 1, 33, 7, 4, 0, 65, 3, 8, 100, 1, 0, 5, 12)
_MULTI_K = (200, 1, 63, 64, 65, 7, 128, 9, 515, 515, 3, 64, 31, 130, 1, 5, 66, 192, 2, 63, 65, 4, 64, 1)
MULTI_SHARED_A = (8, 9)                      # group 9 reads group 8's A (same M and K)
MULTI_EMPTY = (7, 15, 21)                    # M = 0, N = 0, both


def multi_rows_groups(op, maxm, epi, layout="padded"):
    """24 descriptors of one NT / NN launch: M mixed over 1 .. maxm (the launch is compiled for the largest), N from 1 to 130 (narrow groups
    leave early), groups without rows or columns in between, group 9 on group 8's A.  None of the Cases is in the tables."""
    out = []
    for i in range(24):
        M = 0 if _MULTI_M[i] == 0 else (_MULTI_M[i] - 1) % maxm + 1
        K = _MULTI_K[i]
        if i == MULTI_SHARED_A[1]:
            M, K = out[MULTI_SHARED_A[0]].M, out[MULTI_SHARED_A[0]].K
        out.append(Case(op, M, _MULTI_N[i], K, epi, False, layout, 5000 + 100 * maxm + i + (50 if op == "NN" else 0)))
    return out


_MULTI_TN_K = (1, 8, 31, 32, 5, 16)
_MULTI_TN_MN = ((1, 1), (5, 3), (16, 16), (300, 7), (2, 9), (7, 1), (33, 5))


def multi_tn_groups(epi, layout="padded"):
    """24 descriptors of one TN launch: K over 1 .. 32, 1 to 2100 output elements (the grid is sized by the widest), every other one with
    colsum_out, empty groups in between, group 9 on group 8's A."""
    out = []
    for i in range(24):
        K = _MULTI_TN_K[i % 6]
        M, N = _MULTI_TN_MN[i % 7]
        if i in MULTI_EMPTY:
            M, N = (0, N) if i == 7 else (M, 0) if i == 15 else (0, 0)
        if i == MULTI_SHARED_A[1]:
            M, K = out[MULTI_SHARED_A[0]].M, out[MULTI_SHARED_A[0]].K
        out.append(Case("TN", M, N, K, epi, i % 2 == 0, layout, 7000 + i))
    return out


# ------------------------------------------------------------------------------------------------ wsi_gemm_small_pair
PAIR_DX_M = (1, 8, 9, 16, 17, 32)
PAIR_DW_K = (1, 8, 32)
PAIR_MAX_GROUPS = 16
# per accumulator count of the paired kernel: the dX groups (M, N, K) and the dW groups (K, M, N); unequal N throughout
PAIR_SETS = {
    8: (((1, 5, 200), (8, 130, 64)), ((1, 5, 3), (8, 16, 16), (32, 300, 7))),
    16: (((9, 3, 65), (16, 130, 63), (1, 4, 1)), ((1, 16, 16), (8, 300, 7), (32, 1, 1))),
    32: (((17, 130, 515), (32, 4, 64), (8, 1, 7)), ((1, 300, 7), (8, 5, 3), (32, 16, 16))),
}


def pair_groups(mb, dx_epi, dw_epi, layout="padded"):
    dx, dw = PAIR_SETS[mb]
    return ([Case("NN", M, N, K, dx_epi, False, layout, 9000 + 10 * mb + i) for i, (M, N, K) in enumerate(dx)],
            [Case("TN", M, N, K, dw_epi, True, layout, 9500 + 10 * mb + i) for i, (K, M, N) in enumerate(dw)])


# ------------------------------------------------------------------------------------------------ inputs
def make_inputs(case):
    """fp32 operands of one group, from the case's seed alone.  A: [M, K] (TN: [K, M]); B: [N, K] (NT) or [K, N]; bias [N]; R, C_old [M, N];
    gate: one fp32 value; cs_old [M].  Output row m of everything that has rows is scaled by 2^e[m], e[m] in -6 .. 6."""
    rng = np.random.default_rng(case.seed)
    M, N, K = case.M, case.N, case.K
    f = np.float32
    scale = (2.0 ** rng.integers(-6, 7, size=M)).astype(f)
    A = rng.standard_normal((M, K)).astype(f) * scale[:, None]
    if case.op == "TN":
        A = np.ascontiguousarray(A.T)
    B = rng.standard_normal((N, K) if case.op == "NT" else (K, N)).astype(f)
    return dict(A=A, B=B, bias=rng.standard_normal(N).astype(f), R=rng.standard_normal((M, N)).astype(f) * scale[:, None],
                C_old=rng.standard_normal((M, N)).astype(f) * scale[:, None], gate=f(rng.uniform(-2.0, 2.0)),
                cs_old=rng.standard_normal(M).astype(f) * scale)


def uses_gate(epi):
    return bool(epi & (SCALE_GATE | R_1MG))


# ------------------------------------------------------------------------------------------------ float64
def _ab(case, inp, dtype):
    """A as [M, K] and B as [K, N] in ``dtype``."""
    A, B = inp["A"].astype(dtype), inp["B"].astype(dtype)
    return (A.T if case.op == "TN" else A), (B.T if case.op == "NT" else B)


def reference(case, inp):
    """float64 of the same operation on the same fp32 inputs: dict(C, S[, cs, cs_S]); S: the magnitudes the bound is relative to."""
    d = np.float64
    A, B = _ab(case, inp, d)
    epi = case.epi
    s = 1.0 / (1.0 + np.exp(-d(inp["gate"])))
    gs = s if epi & SCALE_GATE else 1.0
    x, S = A @ B, np.abs(A) @ np.abs(B)
    if epi & BIAS:
        x, S = x + inp["bias"].astype(d), S + np.abs(inp["bias"].astype(d))
    x, S = x * gs, S * gs
    if epi & ADD_R:
        x, S = x + inp["R"].astype(d) * ((1.0 - s) if epi & R_1MG else 1.0), S + np.abs(inp["R"].astype(d))
    if epi & ACCUMULATE:
        x, S = x + inp["C_old"].astype(d), S + np.abs(inp["C_old"].astype(d))
    out = dict(C=x, S=S)
    if case.colsum:
        cs, cs_S = A.sum(1) * gs, np.abs(A).sum(1) * gs
        if epi & ACCUMULATE:
            cs, cs_S = cs + inp["cs_old"].astype(d), cs_S + np.abs(inp["cs_old"].astype(d))
        out.update(cs=cs, cs_S=cs_S)
    return out


def bound_factor(case):
    """err <= bound_factor(case) * S, componentwise."""
    return ((case.K + 8) if case.op == "TN" else (-(-case.K // 64) + 16)) * U


def worst_ratio(case, got, ref, key="C"):
    """Largest |got - ref| / bound over the tensor (a zero bound with a zero error counts as 0, with an error as inf)."""
    err = np.abs(np.asarray(got, dtype=np.float64) - ref[key])
    lim = bound_factor(case) * ref["S" if key == "C" else "cs_S"]
    if err.size == 0:
        return 0.0
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0.0, 0.0, err / lim)
    return float(np.nan_to_num(r, nan=np.inf).max())


# ------------------------------------------------------------------------------------------------ fp32 emulation of the kernels' order
FAULTS = ("last_row", "lane63", "bias_after_gate")


def fault_applies(case, fault):
    if fault == "last_row":
        return case.M >= 2
    if fault == "lane63":
        return case.op != "TN" and case.K >= 64
    return case.op != "TN" and (case.epi & (BIAS | SCALE_GATE)) == (BIAS | SCALE_GATE)


def _fma(a, b, c):
    """fp32 fma: the product of two fp32 is exact in float64; the sum is rounded to float64, then to fp32 (a double rounding moves the
    result by at most one fp32 ulp in rare ties - an emulation for a bound, not for bits)."""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def _sigmoid32(g):
    f = np.float32
    return f(1.0) / (f(1.0) + np.exp(-f(g), dtype=f))


def emulate(case, inp, fault=None):
    """The kernels' arithmetic in numpy fp32, vectorised over (m, n).  NT / NN: lane l sums k = l, l + 64, ...; the xor butterfly 32 .. 1;
    (x + bias) * gs; fma(R, rs, x); + C_old.  TN: one chain over k.  ``fault``: one of FAULTS, seeded into that order.
    Returns dict(C[, cs]) in fp32."""
    f = np.float32
    A, B = _ab(case, inp, f)                        # [M, K], [K, N]
    M, N, K, epi = case.M, case.N, case.K, case.epi
    if fault == "last_row":                         # the last output row reads the row of A before it
        A = A.copy()
        A[M - 1] = A[M - 2]
    s = _sigmoid32(inp["gate"]) if uses_gate(epi) else f(1.0)
    gs = s if epi & SCALE_GATE else f(1.0)
    if case.op == "TN":
        x = np.zeros((M, N), f)
        cs = np.zeros(M, f)
        for k in range(K):
            x = _fma(A[:, k, None], B[None, k, :], x)
            cs = cs + A[:, k]
        x = x * gs
        if epi & ACCUMULATE:
            x = x + inp["C_old"]
        out = dict(C=x)
        if case.colsum:
            cs = cs * gs
            if epi & ACCUMULATE:
                cs = cs + inp["cs_old"]
            out["cs"] = cs
        return out
    trips = -(-K // 64)
    Ap = np.zeros((M, trips * 64), f)
    Bp = np.zeros((trips * 64, N), f)
    Ap[:, :K], Bp[:K] = A, B                        # (a term beyond K is an fma with zeros: exact, the lane's sum unchanged)
    acc = np.zeros((M, N, 64), f)
    for t in range(trips):
        acc = _fma(Ap[:, None, 64 * t:64 * t + 64], Bp[64 * t:64 * t + 64].T[None, :, :], acc)
    if fault == "lane63":
        acc[:, :, 63] = 0.0
    lanes = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        acc = acc + acc[:, :, lanes ^ o]
    x = acc[:, :, 0]
    bias = inp["bias"] if epi & BIAS else np.zeros(N, f)
    x = (x * gs + bias) if fault == "bias_after_gate" else (x + bias) * gs
    if epi & ADD_R:
        x = _fma(inp["R"], (f(1.0) - s) if epi & R_1MG else f(1.0), x)
    if epi & ACCUMULATE:
        x = x + inp["C_old"]
    return dict(C=x.astype(f))
