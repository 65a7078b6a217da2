"""The three graph-construction kernels of csrc/knn.hip (wsi_row_sqnorm, wsi_knn_select, wsi_pair_stats) called directly on
hand-built inputs, and construct.knn_pearson at the settings where it branches (several row blocks, the 32-candidate
instantiation, pad 0, n = radius, exact duplicates, a tight cluster away from the origin), each against a float64 restatement on
the CPU and scipy.stats.pearsonr.

Tolerances are those of tests/test_kernels_gpu.py::test_knn_pearson_matches_bruteforce: distances 2e-5 relative, Pearson r 2e-5
absolute, and two neighbours may swap only where their exact distances agree to 2e-6 relative.  The selection kernel is compared
integer-exact.
"""
import functools
import warnings

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

EINVAL = -22
D2_RTOL, R_ATOL, TIE_RTOL = 2e-5, 2e-5, 2e-6


def _dev():
    return torch.device("cuda:0")


def _lib():
    from wsi_hgnn_amd import _native as N
    return N, N.load()


def _pearson(a, b):
    """scipy.stats.pearsonr on the fp32 rows, as the reference calls it (a constant row gives nan and a warning)."""
    from scipy.stats import pearsonr
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return float(pearsonr(a, b)[0])


@pytest.fixture(params=["fp32", "fp16x3", "auto"])
def mode(request):
    from wsi_hgnn_amd import ops
    ops.set_gemm_precision(request.param)
    try:
        yield request.param
    finally:
        ops.set_gemm_precision("fp32")


# ---------------------------------------------------------------------------------------------------- A. wsi_knn_select
SEL_KC = (1, 8, 16, 17, 32)                 # both instantiations (<= 16, <= 32) and their boundary
SEL_N = (3, 17, 64, 255, 256, 257, 1030)
SEL_ROWS = (1, 5, 9)                        # 4 rows per workgroup: a partial last workgroup every time
SEL_LAYOUTS = ("tight", "padded", "shifted", "sqn_shifted")
SEL_PATTERNS = ("random", "random_ties", "descending", "ascending", "equal", "one_lane", "inf")
PAD_DOT = 1e30                              # fills the gaps between rows: key -2e30, would win every selection if it were read


def _layout_ldd(layout, N):
    return N if layout in ("tight", "sqn_shifted") else (N + 3) // 4 * 4 + 4


def _row_is_vector(layout, ldd, w):
    """Does row w take the float4 path: its pointer and sqnorm's are both 16-byte aligned (buffers are allocated aligned)."""
    if layout in ("shifted", "sqn_shifted"):
        return False
    return (w * ldd) % 4 == 0


def _lane_columns(N, lane, vector):
    """The columns one lane of knn_select_kernel streams."""
    if not vector:
        return [j for j in range(N) if j % 64 == lane]
    n4 = N & ~3
    cols = [j for j in range(n4) if (j % 256) // 4 == lane]
    if n4 + lane < N:
        cols.append(n4 + lane)
    return cols


def _select_inputs(pattern, rng, rows, N, kc, row0, layout, ldd):
    """(dots [rows, N], sqnorm [N]) as fp32 arrays, or None when the pattern cannot be built at this size."""
    if pattern in ("random", "inf"):
        d = rng.standard_normal((rows, N)).astype(np.float32)
        s = (4 * rng.random(N)).astype(np.float32)
        if pattern == "inf":
            s[rng.choice(N, size=max(1, min(3, N // 2)), replace=False)] = np.inf
        return d, s
    cols = np.arange(N)
    if pattern == "random_ties":
        key = rng.integers(0, 6, size=(rows, N))                       # many equal keys: the smaller column must win
    elif pattern == "descending":
        key = np.broadcast_to(N - cols, (rows, N))                     # every offer inserts at the head of its lane's list
    elif pattern == "ascending":
        key = np.broadcast_to(cols, (rows, N))
    elif pattern == "equal":
        key = np.full((rows, N), 3)
    else:                                                              # one_lane
        key = np.empty((rows, N), dtype=np.int64)
        for w in range(rows):
            lane = (0, 13, 63, 2)[w % 4]
            mine = [j for j in _lane_columns(N, lane, _row_is_vector(layout, ldd, w)) if j != row0 + w]
            if len(mine) < kc:
                return None
            key[w] = 100 + rng.permutation(N)
            key[w, rng.choice(mine, size=kc, replace=False)] = rng.permutation(kc)
    # integer keys from integer norms: d = (s - key) / 2 is exact in fp32, so the kernel's fmaf gives exactly `key`
    s = rng.integers(0, 64, size=N).astype(np.float32)
    d = ((s[None, :] - key) / 2).astype(np.float32)
    return d, s


def _select_reference(d, s, row0, kc):
    """key = -2 d + s in float64 rounded once to fp32 (= fmaf); sort by (key, column); drop column row0 + w; first kc, -1 pads."""
    key = (-2.0 * d.astype(np.float64) + s.astype(np.float64)[None, :]).astype(np.float32)
    out = np.full((d.shape[0], kc), -1, dtype=np.int32)
    for w in range(d.shape[0]):
        order = np.argsort(key[w], kind="stable")
        order = order[order != row0 + w][:kc]
        out[w, :order.size] = order
    return out, key


def _run_select(d, s, row0, kc, layout):
    N_, lib = _lib()
    rows, N = d.shape
    ldd = _layout_ldd(layout, N)
    doff = 1 if layout == "shifted" else 0
    soff = 1 if layout == "sqn_shifted" else 0
    dbuf = np.full(rows * ldd + 8, PAD_DOT, dtype=np.float32)
    dbuf[doff:doff + rows * ldd].reshape(rows, ldd)[:, :N] = d
    sbuf = np.zeros(N + 8, dtype=np.float32)
    sbuf[soff:soff + N] = s
    dg, sg = torch.from_numpy(dbuf).to(_dev()), torch.from_numpy(sbuf).to(_dev())
    assert dg.data_ptr() % 16 == 0 and sg.data_ptr() % 16 == 0
    cand = torch.full((rows + 2, kc), -7, dtype=torch.int32, device=_dev())          # a guard row on either side
    rc = lib.wsi_knn_select(N_.ptr(dg, 4 * doff), ldd, N_.ptr(sg, 4 * soff), row0, rows, N, kc, N_.ptr(cand, 4 * kc), N_.stream())
    assert rc == 0, lib.wsi_last_error()
    got = cand.cpu().numpy()
    assert (got[0] == -7).all() and (got[-1] == -7).all(), "wsi_knn_select wrote outside its rows"
    return got[1:-1]


@pytest.mark.parametrize("layout", SEL_LAYOUTS)
@pytest.mark.parametrize("pattern", SEL_PATTERNS)
def test_knn_select_direct(pattern, layout):
    """wsi_knn_select on hand-built dots / sqnorm, integer-exact against the sorted (key, column) list.  Layouts: `tight` (ldd = N:
    with N odd the rows alternate between the float4 and the scalar path), `padded` (every row aligned: float4 path with a scalar
    tail when N % 4 != 0), `shifted` (dots starts one float into its buffer) and `sqn_shifted` (sqnorm does): scalar path.
    With `inf` keys and fewer finite keys than kc, the finite ones must come first in order; what follows them may be the +inf
    columns or -1 (a +inf key is an overflowed norm, not a neighbour)."""
    rng = np.random.default_rng(SEL_PATTERNS.index(pattern) * 16 + SEL_LAYOUTS.index(layout))
    ran = 0
    sizes = SEL_N + ((2100,) if pattern == "one_lane" else ())        # 32 columns of one lane need N >= 2048
    for N in sizes:
        ldd = _layout_ldd(layout, N)
        for kc in SEL_KC:
            for rows in SEL_ROWS:
                for row0 in sorted({0, 7, max(N - rows, 0)}):
                    built = _select_inputs(pattern, rng, rows, N, kc, row0, layout, ldd)
                    if built is None:
                        continue
                    d, s = built
                    want, key = _select_reference(d, s, row0, kc)
                    got = _run_select(d, s, row0, kc, layout)
                    ran += 1
                    where = f"{pattern}/{layout} N={N} kc={kc} rows={rows} row0={row0}"
                    if pattern != "inf":
                        assert np.array_equal(got, want), f"{where}\n got {got}\nwant {want}"
                        continue
                    for w in range(rows):
                        others = np.delete(np.arange(N), row0 + w) if row0 + w < N else np.arange(N)
                        nfin = int(np.isfinite(key[w, others]).sum())
                        m = min(nfin, kc)
                        assert np.array_equal(got[w, :m], want[w, :m]), f"{where} row {w}\n got {got[w]}\nwant {want[w]}"
                        tail = got[w, m:]
                        tail = tail[tail >= 0]
                        assert len(set(tail.tolist())) == tail.size and (tail != row0 + w).all(), where
                        assert np.isposinf(key[w, tail]).all(), f"{where} row {w}: {got[w]}"
    assert ran >= (20 if pattern == "one_lane" else 200)


def test_knn_select_argument_checks():
    N_, lib = _lib()
    d = torch.zeros(4, 8, device=_dev())
    s = torch.zeros(8, device=_dev())
    cand = torch.zeros(4, 32, dtype=torch.int32, device=_dev())
    st = N_.stream()
    assert lib.wsi_knn_select(N_.ptr(d), 8, N_.ptr(s), 0, 4, 8, 0, N_.ptr(cand), st) == EINVAL
    assert lib.wsi_knn_select(N_.ptr(d), 8, N_.ptr(s), 0, 4, 8, 33, N_.ptr(cand), st) == EINVAL
    assert lib.wsi_knn_select(N_.ptr(d), 8, N_.ptr(s), 0, 0, 8, 4, N_.ptr(cand), st) == 0
    assert lib.wsi_knn_select(None, 8, None, 0, 0, 8, 4, None, st) == 0
    assert lib.wsi_knn_select(None, 8, N_.ptr(s), 0, 4, 8, 4, N_.ptr(cand), st) == EINVAL
    torch.cuda.synchronize()
    assert (cand == 0).all()


# ---------------------------------------------------------------------------------- B. wsi_row_sqnorm and wsi_pair_stats
@pytest.mark.parametrize("F", [1, 3, 64, 65, 1024])
@pytest.mark.parametrize("n", [1, 4, 5])
def test_row_sqnorm_direct(n, F):
    N_, lib = _lib()
    rng = np.random.default_rng(n * 2000 + F)
    for ldx in (F, F + 3):
        buf = np.full((n, ldx), 1e18, dtype=np.float32)               # the gap between rows would show at once
        buf[:, :F] = rng.standard_normal((n, F)).astype(np.float32)
        x = torch.from_numpy(buf).to(_dev())
        out = torch.full((n + 2,), -7.0, device=_dev())
        assert lib.wsi_row_sqnorm(N_.ptr(x), ldx, n, F, N_.ptr(out, 4), N_.stream()) == 0, lib.wsi_last_error()
        got = out.cpu().numpy().astype(np.float64)
        assert got[0] == -7.0 and got[-1] == -7.0
        want = (buf[:, :F].astype(np.float64) ** 2).sum(1)
        np.testing.assert_allclose(got[1:-1], want, rtol=2e-5, atol=0)
    assert lib.wsi_row_sqnorm(None, F, 0, F, None, N_.stream()) == 0
    assert lib.wsi_row_sqnorm(None, F, n, F, None, N_.stream()) == EINVAL


def _run_pair_stats(xbuf, F, cand, keep, fill=-5):
    """xbuf [n, ldx] fp32 (columns >= F are padding), cand [n, kc] int32 -> (nbr, dist2, corr) as numpy arrays."""
    N_, lib = _lib()
    n, ldx = xbuf.shape
    kc = cand.shape[1]
    x = torch.from_numpy(xbuf).to(_dev())
    cg = torch.from_numpy(cand).to(_dev())
    nbr = torch.full((n + 2, keep), fill, dtype=torch.int32, device=_dev())
    d2 = torch.full((n + 2, keep), -7.0, device=_dev())
    r = torch.full((n + 2, keep), -7.0, device=_dev())
    rc = lib.wsi_pair_stats(N_.ptr(x), ldx, n, F, N_.ptr(cg), kc, keep, N_.ptr(nbr, 4 * keep), N_.ptr(d2, 4 * keep), N_.ptr(r, 4 * keep),
                            N_.stream())
    assert rc == 0, lib.wsi_last_error()
    nbr, d2, r = nbr.cpu().numpy(), d2.cpu().numpy(), r.cpu().numpy()
    for a, v in ((nbr, fill), (d2, -7.0), (r, -7.0)):
        assert (a[0] == v).all() and (a[-1] == v).all(), "wsi_pair_stats wrote outside its rows"
    return nbr[1:-1], d2[1:-1], r[1:-1]


def _pair_reference(x64, cand, keep):
    """Per row the float64 (d2, column) ranking of its valid candidates: (columns [n, keep] padded with -1, d2 [n, keep], counts)."""
    n = cand.shape[0]
    nbr = np.full((n, keep), -1, dtype=np.int64)
    d2o = np.full((n, keep), np.nan)
    cnt = np.zeros(n, dtype=np.int64)
    for i in range(n):
        valid = cand[i][cand[i] >= 0].astype(np.int64)
        d2 = ((x64[valid] - x64[i]) ** 2).sum(1)
        order = np.lexsort((valid, d2))[:keep]
        cnt[i] = order.size
        nbr[i, :order.size] = valid[order]
        d2o[i, :order.size] = d2[order]
    return nbr, d2o, cnt


def _build_cand(rng, n, kc, keep):
    """Distinct candidates other than the row itself at scattered slots, some slots -1; row 0 has fewer than `keep` valid ones."""
    cand = np.full((n, kc), -1, dtype=np.int32)
    for i in range(n):
        others = rng.permutation(np.delete(np.arange(n), i))
        m = min(kc, others.size)
        if i == 0:
            m = min(m, keep - 1)
        elif m > 1 and rng.random() < 0.5:
            m -= int(rng.integers(0, max(1, m // 4) + 1))              # knock a few out
        cand[i, np.sort(rng.choice(kc, size=m, replace=False))] = others[:m]
    return cand


@pytest.mark.parametrize("F", [2, 3, 10, 96, 1024])
@pytest.mark.parametrize("n", [1, 6, 130])
def test_pair_stats_direct(n, F):
    """wsi_pair_stats on candidate lists built here: the kept neighbours against the float64 (d2, column) ranking, dist2 at 2e-5
    relative, corr against scipy.stats.pearsonr (sampled rows) and a float64 Pearson (every kept pair) at 2e-5 absolute.  Slots
    past the number of valid candidates keep the caller's fill in nbr."""
    rng = np.random.default_rng(n * 5000 + F)
    xs = rng.random((n, F)).astype(np.float32)
    x64 = xs.astype(np.float64)
    xc = x64 - x64.mean(1, keepdims=True)
    norm = np.sqrt((xc * xc).sum(1))
    for kc in (1, 9, 16, 32, 64):
        for keep in sorted({1, max(kc // 2, 1), kc}):
            for ldx in (F, F + 5):
                xbuf = np.full((n, ldx), 1e18, dtype=np.float32)
                xbuf[:, :F] = xs
                cand = _build_cand(rng, n, kc, keep)
                nbr, d2, r = _run_pair_stats(xbuf, F, cand, keep)
                ref_nbr, ref_d2, cnt = _pair_reference(x64, cand, keep)
                where = f"n={n} F={F} kc={kc} keep={keep} ldx={ldx}"
                assert cnt[0] < keep, where
                sample = set(rng.choice(n, size=min(n, 6), replace=False).tolist())
                for i in range(n):
                    m = int(cnt[i])
                    assert (nbr[i, m:] == -5).all(), f"{where} row {i}: {nbr[i]}"
                    mine = nbr[i, :m].astype(np.int64)
                    assert ((mine >= 0) & (mine < n)).all() and len(set(mine.tolist())) == m, f"{where} row {i}: {nbr[i]}"
                    assert np.isin(mine, cand[i]).all(), f"{where} row {i}"
                    np.testing.assert_allclose(d2[i, :m], ref_d2[i, :m], rtol=D2_RTOL, atol=0, err_msg=f"{where} row {i}")
                    for c in np.nonzero(mine != ref_nbr[i, :m])[0]:    # a swap only between neighbours fp32 cannot tell apart
                        exact = ((x64[i] - x64[mine[c]]) ** 2).sum()
                        assert abs(exact - ref_d2[i, c]) <= TIE_RTOL * ref_d2[i, c], f"{where} row {i} slot {c}"
                    r64 = (xc[mine] * xc[i]).sum(1) / (norm[mine] * norm[i])
                    assert np.abs(r[i, :m] - r64).max(initial=0.0) < R_ATOL, f"{where} row {i}"
                    if i in sample:
                        for c in range(m):
                            assert abs(float(r[i, c]) - _pearson(xs[i], xs[mine[c]])) < R_ATOL, f"{where} row {i} slot {c}"


CONST_VALUES = (0.0, 0.5, 0.1, 0.7, 1.1)


def _rows_with_constants(F, n_random, seed):
    """One constant row per value of CONST_VALUES (rows 0..4), then n_random rows of uniform noise."""
    rng = np.random.default_rng(seed)
    xs = rng.random((len(CONST_VALUES) + n_random, F)).astype(np.float32)
    for k, v in enumerate(CONST_VALUES):
        xs[k] = np.float32(v)
    return xs


@pytest.mark.parametrize("F", [1024, 96])
def test_pair_stats_constant_rows_give_nan(F):
    """scipy.stats.pearsonr returns nan when either vector is constant ((x == x[0]).all()), and the reference then types the edge
    'neg'.  Row i constant, row j constant and both constant, for 0.0, 0.5, 0.1, 0.7 and 1.1.  The centred fp32 sum of squares of
    1024 copies of 0.7f, 0.1f or 1.1f is not 0 (the fp32 mean of the row is not the value), so constancy cannot be read off sxx:
    before the kernel voted on `every element equals the first`, those rows gave a finite r of arbitrary sign here."""
    xs = _rows_with_constants(F, 7, seed=F)
    n = xs.shape[0]
    nconst = len(CONST_VALUES)
    cand = np.stack([np.delete(np.arange(n, dtype=np.int32), i) for i in range(n)])
    nbr, _, r = _run_pair_stats(xs, F, cand, n - 1)
    assert (nbr >= 0).all()
    for i in range(n):
        for c in range(n - 1):
            j = int(nbr[i, c])
            want = _pearson(xs[i], xs[j])
            if i < nconst or j < nconst:
                assert np.isnan(want)
                assert np.isnan(r[i, c]), f"F={F}: r({i}, {j}) = {r[i, c]!r}, scipy gives nan (constant row)"
            else:
                assert abs(float(r[i, c]) - want) < R_ATOL, (i, j)


def test_construct_graph_types_constant_row_edges_neg():
    """Through construct_graph: every edge that touches a constant row has sim = nan and sits in a 'neg' relation."""
    from wsi_hgnn_amd import construct
    F, radius, T = 1024, 9, 2
    xs = _rows_with_constants(F, 59, seed=7)
    n = xs.shape[0]
    const = np.zeros(n, dtype=bool)
    const[:len(CONST_VALUES)] = True
    node_type = [i % T for i in range(n)]
    het, homo, _ = construct.construct_graph(torch.from_numpy(xs).to(_dev()), node_type, radius, T)
    touched = 0
    for rel in het.canonical_etypes:
        u, v = het.edges(rel)
        gu = het.nodes[rel[0]].data["_ID"][u].cpu().numpy()
        gv = het.nodes[rel[2]].data["_ID"][v].cpu().numpy()
        sim = het.edata["sim"][rel].cpu().numpy()
        hit = const[gu] | const[gv]
        touched += int(hit.sum())
        assert np.isnan(sim[hit]).all(), rel
        assert not np.isnan(sim[~hit]).any(), rel
        if rel[1] == "pos":
            assert not hit.any(), f"{int(hit.sum())} edges of {rel} touch a constant row"
    assert touched >= len(CONST_VALUES) * (radius - 1)                 # at least the constant rows' own out-edges


def test_pair_stats_argument_checks():
    N_, lib = _lib()
    x = torch.rand(4, 8, device=_dev())
    cand = torch.zeros(4, 64, dtype=torch.int32, device=_dev())
    nbr = torch.full((4, 64), -1, dtype=torch.int32, device=_dev())
    d2 = torch.zeros(4, 64, device=_dev())
    r = torch.zeros(4, 64, device=_dev())
    st = N_.stream()
    p = N_.ptr
    assert lib.wsi_pair_stats(p(x), 8, 4, 8, p(cand), 4, 5, p(nbr), p(d2), p(r), st) == EINVAL          # keep > kc
    assert lib.wsi_pair_stats(p(x), 8, 4, 8, p(cand), 65, 4, p(nbr), p(d2), p(r), st) == EINVAL         # kc > 64
    assert lib.wsi_pair_stats(p(x), 8, 4, 0, p(cand), 4, 4, p(nbr), p(d2), p(r), st) == EINVAL          # F = 0
    assert lib.wsi_pair_stats(p(x), 8, 4, 8, p(cand), 4, 0, p(nbr), p(d2), p(r), st) == EINVAL          # keep = 0
    for missing in range(5):
        args = [p(x), p(cand), p(nbr), p(d2), p(r)]
        args[missing] = None
        assert lib.wsi_pair_stats(args[0], 8, 4, 8, args[1], 4, 4, args[2], args[3], args[4], st) == EINVAL
    assert lib.wsi_pair_stats(None, 8, 0, 8, None, 4, 4, None, None, None, st) == 0
    torch.cuda.synchronize()
    assert (nbr == -1).all()


# ------------------------------------------------------------------------------------------ C. knn_pearson end to end
def _wsi_like_features(n, F, seed, clusters=12):
    """Non-negative, clustered features, as in tests/test_kernels_gpu.py."""
    g = torch.Generator().manual_seed(seed)
    centres = torch.rand(clusters, F, generator=g)
    assign = torch.randint(0, clusters, (n,), generator=g)
    return (centres[assign] + 0.15 * torch.randn(n, F, generator=g)).clamp_(min=0).float()


@functools.lru_cache(maxsize=None)
def _case(kind, n, F, radius):
    """(features, brute-force neighbours, their exact d2) of one case; computed once, shared by the GEMM modes, never modified."""
    from oracle import construct as OC
    if kind == "wsi":
        x = _wsi_like_features(n, F, seed=n + radius)
    elif kind == "integer":               # small integers: every dot product is exact, neighbour gaps are 0 (index order) or >= 1
        x = torch.randint(0, 4, (n, F), generator=torch.Generator().manual_seed(n + F)).float()
    else:
        raise ValueError(kind)
    ref_nbr, ref_d2 = OC.knn_bruteforce(x.numpy(), radius)
    ref_nbr.flags.writeable = False
    ref_d2.flags.writeable = False
    return x, ref_nbr, ref_d2


def _check_against_bruteforce(x, nbr, corr, d2, radius, ref_nbr, ref_d2, pearson_rows=60):
    """The comparison of test_knn_pearson_matches_bruteforce: shapes, no self loop, distances at 2e-5 relative, identical lists
    except where two candidates are closer than fp32 can tell apart (and on fewer than 1 % of the slots), Pearson r of the emitted
    edges against scipy on the fp32 rows."""
    n = x.shape[0]
    nbr_c, d2_c = nbr.cpu().numpy(), d2.cpu().numpy().astype(np.float64)
    corr_c = corr.cpu().numpy()
    assert nbr_c.shape == (n, radius - 1) and (nbr_c >= 0).all() and (nbr_c < n).all()
    assert (nbr_c != np.arange(n)[:, None]).all()                       # never the patch itself
    np.testing.assert_allclose(d2_c, ref_d2, rtol=D2_RTOL, atol=1e-9)
    diff = nbr_c != ref_nbr
    if diff.any():
        xd = x.double().numpy()
        for r, c in zip(*np.nonzero(diff)):
            mine = ((xd[r] - xd[nbr_c[r, c]]) ** 2).sum()
            assert abs(mine - ref_d2[r, c]) <= TIE_RTOL * ref_d2[r, c], (r, c)
        assert diff.mean() < 0.01
    xs = x.numpy()
    rng = np.random.default_rng(0)
    for r in rng.choice(n, size=min(n, pearson_rows), replace=False):
        for c in range(radius - 1):
            assert abs(float(corr_c[r, c]) - _pearson(xs[r], xs[nbr_c[r, c]])) < R_ATOL, (r, c)


@pytest.mark.parametrize("n,block_rows", [(257, 100), (257, 64), (130, 100), (130, 64)])
def test_knn_pearson_several_row_blocks(n, block_rows, mode):
    """row0 > 0: the self column row0 + w, the offset cand pointer and a ragged last block (257 = 100 + 100 + 57, 130 = 64 + 64 + 2)."""
    from wsi_hgnn_amd import construct
    F, radius = 96, 9
    x, ref_nbr, ref_d2 = _case("wsi", n, F, radius)
    nbr, corr, d2 = construct.knn_pearson(x.to(_dev()), radius, block_rows=block_rows)
    assert (nbr.cpu() != torch.arange(n)[:, None]).all(), "a row lists itself"
    _check_against_bruteforce(x, nbr, corr, d2, radius, ref_nbr, ref_d2, pearson_rows=30)


@pytest.mark.parametrize("F", [96, 1024])
@pytest.mark.parametrize("n", [64, 300])
@pytest.mark.parametrize("radius", [10, 17, 25])
def test_knn_pearson_wide_radius(radius, n, F, mode):
    """radius >= 10: kc = 17, 24, 32, the 32-slot instantiation of the selection kernel."""
    from wsi_hgnn_amd import construct
    x, ref_nbr, ref_d2 = _case("wsi", n, F, radius)
    nbr, corr, d2 = construct.knn_pearson(x.to(_dev()), radius)
    _check_against_bruteforce(x, nbr, corr, d2, radius, ref_nbr, ref_d2, pearson_rows=12)


def test_knn_pearson_pad_zero_on_separated_data(mode):
    """pad = 0: nothing is re-ranked in, the shortlist alone must hold the right neighbours.  Small-integer features: the dot
    products and norms are exact in every GEMM mode that keeps fp32-class error, exact distances are integers, so two neighbours
    are either tied (the smaller index first, the rule of both kernels) or a whole unit apart."""
    from wsi_hgnn_amd import construct
    n, F, radius = 130, 96, 9
    x, ref_nbr, ref_d2 = _case("integer", n, F, radius)
    nbr, corr, d2 = construct.knn_pearson(x.to(_dev()), radius, pad=0)
    _check_against_bruteforce(x, nbr, corr, d2, radius, ref_nbr, ref_d2, pearson_rows=30)


@pytest.mark.parametrize("n,radius", [(9, 9), (25, 25), (2, 2)])
def test_knn_pearson_smallest_legal_size(n, radius, mode):
    """n = radius: kc = n - 1, every other row is a neighbour."""
    from wsi_hgnn_amd import construct
    x, ref_nbr, ref_d2 = _case("wsi", n, 16, radius)
    nbr, corr, d2 = construct.knn_pearson(x.to(_dev()), radius)
    _check_against_bruteforce(x, nbr, corr, d2, radius, ref_nbr, ref_d2)


def test_knn_pearson_exact_duplicates(mode):
    """40 identical rows scattered in n = 200: each one's neighbours are duplicates at d2 == 0.0 and r == 1.0, ascending in index,
    and they are the 8 smallest indices of the group other than the row itself (ties -> smaller index, as the docstring says)."""
    from wsi_hgnn_amd import construct
    n, F, radius, ndup = 200, 96, 9, 40
    g = torch.Generator().manual_seed(40)
    x = _wsi_like_features(n, F, seed=200).clone()
    group = torch.sort(torch.randperm(n, generator=g)[:ndup]).values
    x[group] = x[group[0]].clone()
    assert x[group[0]].min() < x[group[0]].max()                        # not a constant row
    nbr, corr, d2 = construct.knn_pearson(x.to(_dev()), radius)
    nbr, corr, d2 = nbr.cpu(), corr.cpu(), d2.cpu()
    for i in group.tolist():
        want = [j for j in group.tolist() if j != i][:radius - 1]
        assert nbr[i].tolist() == want, (i, nbr[i].tolist(), want)
        assert (d2[i] == 0.0).all(), (i, d2[i])
        assert (corr[i] == 1.0).all(), (i, corr[i])
    from oracle import construct as OC
    ref_nbr, ref_d2 = OC.knn_bruteforce(x.numpy(), radius)
    _check_against_bruteforce(x, nbr, corr, d2, radius, ref_nbr, ref_d2, pearson_rows=20)


# ------------------------------------------------------------------------------------------ D. the resolution limit
RES_N, RES_F, RES_BLOB, RES_RADIUS, RES_KC = 264, 1024, 64, 9, 16


@functools.lru_cache(maxsize=None)
def _resolution_case(sigma):
    """Features with a tight blob away from the origin, the exact kc + 1 nearest neighbours of every row, and per row the key
    error e of the CPU restatement of the shortlist key |x_j|^2 - 2 x_i.x_j (fp32 matmul and norms against float64)."""
    from oracle import construct as OC
    g = torch.Generator().manual_seed(RES_N)
    centre = torch.rand(RES_F, generator=g)
    x = torch.rand(RES_N, RES_F, generator=g)
    blob = torch.randperm(RES_N, generator=g)[:RES_BLOB]
    x[blob] = (centre + sigma * torch.randn(RES_BLOB, RES_F, generator=g)).clamp_(min=0)
    x = x.float().contiguous()
    key32 = (x * x).sum(1)[None, :] - 2 * (x @ x.T)
    xd = x.double()
    key64 = (xd * xd).sum(1)[None, :] - 2 * (xd @ xd.T)
    e = (key32.double() - key64).abs().max(1).values.numpy()
    ref_nbr, ref_d2 = OC.knn_bruteforce(x.numpy(), RES_KC + 2)          # kc + 1 neighbours: the last one bounds the shortlist
    for a in (e, ref_nbr, ref_d2):
        a.flags.writeable = False
    return x, np.sort(blob.numpy()), e, ref_nbr, ref_d2


@pytest.mark.parametrize("sigma", [1e-2, 1e-3, 1e-4])
def test_resolution_limit(sigma, mode):
    """What knn_pearson guarantees for a tight cluster away from the origin (64 rows centre + sigma randn among 264, F = 1024,
    |x|^2 = 347, radius 9, kc 16).  The shortlist ranks by an fp32 key with absolute error e; a true neighbour can lose its place
    to a row whose exact distance is at most slack = 8 e larger (2: a swap takes two key errors; 2: the emulated GEMM modes are
    bounded at twice the fp32 path by test_gemm_emulated_error_vs_fp32_mfma; 2: another accumulation order than the CPU's).  So
        d2_ref[c] (1 - 2e-5) <= d2[c] <= d2_ref[c] + slack          for every row and slot c,
    and the list equals the exact one (up to fp32 ties) wherever the exact d2 of the keep-th and the (kc+1)-th neighbour are more
    than slack apart.  e comes from the CPU restatement (torch fp32 x @ x.T and row norms against float64), per row, never from
    the kernels.  It depends on the host's BLAS: max over rows 4.0e-4, 4.4e-4, 4.4e-4 for sigma 1e-2, 1e-3, 1e-4 (median 2.7e-4)
    on one host, 2.5e-4 (median 1.7e-4) at sigma 1e-4 on the host of the MI355X run, so slack is 2e-3 to 3.5e-3.
    Measured on an MI355X, fp32 mode, sigma 1e-4: 486 of the blob's 512 slots differ from the exact list, in all 64 blob rows
    and in no other; largest d2 - d2_ref 2.0e-5 = 0.017 slack; lowest d2 / d2_ref 0.99999989.  At sigma 1e-2 and 1e-3 the
    contract held in fp32 mode; the first sigma at which the lists differ on the GPU, and the fp16x3 and auto modes, are not
    measured yet; the line printed below reports them (a numpy fp32 simulation of the shortlist puts the first difference
    between 1e-2 and 3e-3)."""
    from wsi_hgnn_amd import construct
    keep = RES_RADIUS - 1
    x, blob, e, ref_nbr, ref_d2 = _resolution_case(sigma)
    nbr, corr, d2 = construct.knn_pearson(x.to(_dev()), RES_RADIUS)
    nbr_c, d2_c = nbr.cpu().numpy(), d2.cpu().numpy().astype(np.float64)
    assert nbr_c.shape == (RES_N, keep) and (nbr_c >= 0).all() and (nbr_c != np.arange(RES_N)[:, None]).all()
    slack = 8.0 * e
    want_nbr, want_d2 = ref_nbr[:, :keep], ref_d2[:, :keep]
    certified = (ref_d2[:, RES_KC] - ref_d2[:, keep - 1]) > slack
    xd = x.double().numpy()
    exact_mine = ((xd[:, None, :] - xd[nbr_c]) ** 2).sum(2)
    differs = (nbr_c != want_nbr) & (np.abs(exact_mine - want_d2) > TIE_RTOL * want_d2)      # beyond an fp32 tie
    excess = d2_c - want_d2
    print(f"\nresolution sigma={sigma:g} mode={mode}: e max {e.max():.3e} median {np.median(e):.3e} blob max {e[blob].max():.3e}; "
          f"slack max {slack.max():.3e}; certified rows {int(certified.sum())}/{RES_N} (blob {int(certified[blob].sum())}/{RES_BLOB}); "
          f"slots that differ from the exact list {int(differs.sum())} in {int(differs.any(1).sum())} rows "
          f"(blob rows {int(differs[blob].any(1).sum())}); largest d2 - d2_ref {excess.max():.3e} "
          f"(largest / slack {np.max(excess / slack[:, None]):.3f}); lowest d2 / d2_ref {np.min(d2_c / want_d2):.8f}")
    assert (d2_c >= want_d2 * (1 - D2_RTOL)).all()
    assert (d2_c <= want_d2 + slack[:, None]).all(), f"largest d2 - d2_ref over slack: {np.max(excess / slack[:, None]):.3f}"
    assert not differs[certified].any(), f"rows {np.nonzero(differs.any(1) & certified)[0].tolist()} differ although certified"
    # The fixture's own sanity: an unrelated row whose kc + 1 exact neighbours are all unrelated has gaps of order 1 and is always
    # certified.  (A few unrelated rows have the blob among their nearest; at small sigma its 64 rows are all equally far from
    # them, closer together than slack, so those rows are uncertified like the blob's own.)
    away = ~np.isin(np.arange(RES_N), blob) & ~np.isin(ref_nbr, blob).any(1)
    assert away.sum() >= RES_N - RES_BLOB - 8 and certified[away].all()
