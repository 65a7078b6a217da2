"""What tests/gemm_small_cases.py promises, shown without a GPU: the tables reach every skinny-kernel instantiation and every boundary they
name; an fp32 emulation of the kernels' summation order stays inside the derived bound on every table row; and each of three seeded faults
leaves it on every row where the fault can act - so the bound is neither vacuous nor out of the kernels' reach.

Measured here (printed by the tests): emulation, largest error / bound 0.271 over the tables (C and column sums; TN 300 x 7, K = 1); smallest
largest-element ratio of a seeded fault over the rows where it applies: wrong last row 4.6e4 (44 rows), lane 63 dropped 4.5e3 (28 rows),
bias after gate 266 (16 rows).
"""
import numpy as np
import pytest

import gemm_small_cases as GC

CASES = GC.all_cases()


def test_epilogue_values_are_the_headers():
    from wsi_hgnn_amd import _native as N
    assert (GC.BIAS, GC.ACCUMULATE, GC.SCALE_GATE, GC.ADD_R, GC.R_1MG) == (
        N.WSI_EPI_BIAS, N.WSI_EPI_ACCUMULATE, N.WSI_EPI_SCALE_GATE, N.WSI_EPI_ADD_R, N.WSI_EPI_R_1MG)
    assert N.WSI_GEMM_MAX_GROUPS == 24 == len(GC.multi_rows_groups("NT", 32, 0)) == len(GC.multi_tn_groups(0))


def test_tables_reach_every_instantiation_and_boundary():
    rows, tn = GC.rows_cases(), GC.tn_cases()
    assert len(CASES) == len(set(CASES)) and 24 <= len(CASES) <= 60            # a few dozen, none twice
    assert {(c.op, GC.accumulators(c)) for c in CASES} == {(op, mb) for op in ("NT", "NN") for mb in (8, 16, 32)} | {("TN", 1)}
    for op in ("NT", "NN"):
        mine = [c for c in rows if c.op == op]
        assert {c.M for c in mine} >= set(GC.ROWS_M) and max(c.M for c in mine) == GC.SKINNY_M
        assert {c.N for c in mine} >= set(GC.ROWS_N)
        assert {c.K for c in mine} >= set(GC.ROWS_K)
        assert {c.epi for c in mine} == set(GC.ROWS_EPILOGUES)
        assert {c.layout for c in mine} == set(GC.LAYOUTS)
        assert not any(c.colsum for c in mine)
    assert {c.K for c in tn} == set(GC.TN_K) and max(c.K for c in tn) == GC.SKINNY_K
    assert {(c.K, c.M, c.N) for c in tn} == {(K, M, N) for K in GC.TN_K for M, N in GC.TN_MN}
    assert {(c.epi, c.colsum) for c in tn} == {(e, cs) for e in GC.TN_EPILOGUES for cs in (False, True)}
    assert {c.layout for c in tn} == set(GC.LAYOUTS)
    # every fault has rows to act on
    for fault in GC.FAULTS:
        assert sum(GC.fault_applies(c, fault) for c in CASES) >= 6, fault


def test_multi_group_and_pair_tables():
    for op in ("NT", "NN"):
        for maxm in (8, 16, 32):
            g = GC.multi_rows_groups(op, maxm, GC.ALL_FIVE)
            live = [c for c in g if c.M > 0 and c.N > 0]
            assert len(g) == 24 and max(c.M for c in g) == maxm and min(c.M for c in live) == 1
            assert min(c.N for c in live) == 1 and max(c.N for c in live) == 130
            assert [(g[i].M == 0, g[i].N == 0) for i in GC.MULTI_EMPTY] == [(True, False), (False, True), (True, True)]
            assert len(live) == 21
            a, b = (g[i] for i in GC.MULTI_SHARED_A)
            assert (a.M, a.K) == (b.M, b.K) and a.N != b.N
    g = GC.multi_tn_groups(0)
    live = [c for c in g if c.M > 0 and c.N > 0]
    assert len(live) == 21 and {c.K for c in live} >= {1, 32} and max(c.K for c in live) == 32
    assert min(c.M * c.N for c in live) == 1 and max(c.M * c.N for c in live) == 2100
    assert {c.colsum for c in live} == {False, True}
    dx_m, dw_k = set(), set()
    for mb in (8, 16, 32):
        dx, dw = GC.pair_groups(mb, 0, 0)
        assert max(c.M for c in dx) == mb and (mb == 8 or min(c.M for c in dx if c.M > mb // 2) == mb // 2 + 1)
        assert len({c.N for c in dx + dw}) >= 5 and len(dx) + len(dw) <= GC.PAIR_MAX_GROUPS
        assert all(c.colsum for c in dw)
        dx_m |= {c.M for c in dx}
        dw_k |= {c.K for c in dw}
    assert dx_m >= set(GC.PAIR_DX_M) and dw_k == set(GC.PAIR_DW_K)


def test_inputs_have_row_scales_and_are_reproducible():
    c = next(c for c in CASES if c.M == 32 and c.K == 515)
    a, b = GC.make_inputs(c), GC.make_inputs(c)
    assert all(np.array_equal(a[k], b[k]) for k in a)
    rowmax = np.abs(a["A"]).max(1)
    assert rowmax.max() / rowmax.min() >= 2.0 ** 6           # rows of very different size in one tensor
    ref = GC.reference(c, a)
    assert ref["C"].shape == ref["S"].shape == (c.M, c.N) and (ref["S"] >= np.abs(ref["C"]) * (1 - 1e-12)).all()


def test_emulation_stays_within_the_bound():
    worst = (0.0, None)
    for c in CASES:
        inp = GC.make_inputs(c)
        ref, got = GC.reference(c, inp), GC.emulate(c, inp)
        r = GC.worst_ratio(c, got["C"], ref)
        if c.colsum:
            r = max(r, GC.worst_ratio(c, got["cs"], ref, "cs"))
        assert r <= 1.0, (GC.case_id(c), r)
        worst = max(worst, (r, GC.case_id(c)))
    print(f"\nemulation, largest error / bound: {worst[0]:.3f} ({worst[1]})")
    assert worst[0] > 1e-3                                   # ... and the bound is not orders of magnitude away from fp32 arithmetic


@pytest.mark.parametrize("fault", GC.FAULTS)
def test_seeded_fault_exceeds_the_bound_wherever_it_applies(fault):
    least = (np.inf, None)
    n = 0
    for c in CASES:
        if not GC.fault_applies(c, fault):
            continue
        inp = GC.make_inputs(c)
        ref, got = GC.reference(c, inp), GC.emulate(c, inp, fault)
        r = GC.worst_ratio(c, got["C"], ref)
        assert r > 1.0, (fault, GC.case_id(c), r)
        least = min(least, (r, GC.case_id(c)))
        n += 1
    assert n >= 6
    print(f"\n{fault}: smallest error / bound over {n} cases: {least[0]:.3g} ({least[1]})")
