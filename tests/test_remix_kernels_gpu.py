"""The ReMix kernels (wsi_bag_kmeans_step, wsi_remix_nearest, wsi_remix_rows) on the GPU against float64 on the SAME fp32 inputs
(tests/remix_cases.py), through ``ops`` and through the raw ABI.

One plan: bags of 0, 5, 8, 9, 127, 128, 129, 293 and 1061 rows with the default chunk of 128 rows - at K = 8 two bags with fewer rows than
clusters, a bag of exactly K rows, the chunk boundary from both sides and combines of 3 and 9 chunks.

Labels must equal float64's except on rows whose float64 best and second-best squared distance differ by <= 1e-5 (unit rows: d^2 in [0, 4];
an fp32 sum of 1024 terms errs by about 1e-6); float64 alone must put <= 1 % of the rows there.  Counts are exact for the kernel's own labels;
new centroids and objective (means taken over the kernel's labels) lie within 1e-4 x the largest float64 entry."""
import numpy as np
import pytest
import torch

import remix_cases as rc
from test_remix import FIX, check_mixed_rows, fixture_case

pytestmark = pytest.mark.gpu

DEV = "cuda"
TOL = 1e-4
SIZES = rc.KERNEL_SIZES
OFF = rc.offsets(SIZES)
NROWS = OFF[-1]
S = len(SIZES)
R = rc.Ratios(TOL)


@pytest.fixture(scope="module", autouse=True)
def _report_ratios():
    yield
    R.report()


@pytest.fixture(scope="module")
def rp():
    from wsi_hgnn_amd import mil
    return mil.bag_plan(SIZES, DEV)


def _rows(kind, K, D, seed):
    return rc.gaussian_rows(SIZES, D, seed) if kind == "gaussian" else rc.blob_rows(SIZES, D, max(K, 2), seed)


def _centroids(x, K, seed, normalize=True):
    """Per bag K of its own (normalised) rows plus a little noise: distinct centroids near the data; zeros for a bag with fewer than K rows.
    (At D <= 3 the noise is ten times larger: normalised rows of one column are +-1, so centroids 0.05 apart would tie half the rows.)"""
    rs = np.random.RandomState(seed)
    D = x.shape[1]
    noise = 0.05 if D > 3 else 0.5
    cen = np.zeros((S, K, D), dtype=np.float32)
    for s, n in enumerate(SIZES):
        if n >= K:
            rows = x[OFF[s] + rs.permutation(n)[:K]].astype(np.float64)
            cen[s] = ((rc.normalize64(rows) if normalize else rows) + noise * rs.standard_normal((K, D))).astype(np.float32)
    return cen


def _check_step(got, x, cen, K, normalize, case, update=True):
    """``got`` = (labels, counts, objective, new) of the kernel against float64."""
    labels, counts, objective, new = (None if t is None else t.cpu() for t in got)
    lab64, _, _, _, gap = rc.step64(x, SIZES, cen, normalize, update=False)
    valid = np.concatenate([np.full(n, n >= K) for n in SIZES])
    near = (gap <= rc.BAND) & valid
    assert near.sum() <= 0.01 * max(valid.sum(), 1), f"{case}: float64 puts {near.sum()} of {valid.sum()} rows within {rc.BAND} of a tie"
    mine = labels.numpy().astype(np.int64)
    differ = (mine != lab64) & ~near
    assert not differ.any(), f"{case}: {differ.sum()} labels differ outside the band (first row {np.argmax(differ)})"
    assert (mine[~valid] == 0).all() and mine.min() >= 0 and mine.max() < K
    _, cnt64, obj64, new64, _ = rc.step64(x, SIZES, cen, normalize, update=update, labels=mine)
    assert np.array_equal(counts.numpy(), cnt64), f"{case}: counts"
    assert counts.sum(1).tolist() == [n if n >= K else 0 for n in SIZES]
    R.check(objective, torch.from_numpy(obj64), "objective", case)
    if update:
        R.check(new, torch.from_numpy(new64), "new_centroids", case)
    else:
        assert new is None
        for s in range(S):
            assert counts[s].tolist() == np.bincount(mine[OFF[s]:OFF[s + 1]], minlength=K).tolist() or SIZES[s] < K
    for s, n in enumerate(SIZES):
        if n < K:
            assert not counts[s].any() and objective[s] == 0 and (new is None or not new[s].any()), f"{case}: small bag {s}"


@pytest.mark.parametrize("kind", ["gaussian", "blobs"])
@pytest.mark.parametrize("D", rc.KERNEL_DS)
@pytest.mark.parametrize("K", rc.KERNEL_KS)
def test_step_sweep_against_float64(rp, K, D, kind):
    from wsi_hgnn_amd import ops
    x = _rows(kind, K, D, seed=100 * K + D)
    cen = _centroids(x, K, seed=7 * K + D)
    xd, cd = torch.from_numpy(x).to(DEV), torch.from_numpy(cen).to(DEV)
    case = f"K={K} D={D} {kind}"
    got = ops.bag_kmeans_step(xd, rp, cd, True, True)
    _check_step(got, x, cen, K, True, case)
    only = ops.bag_kmeans_step(xd, rp, cd, True, False)
    assert torch.equal(only[0], got[0]) and torch.equal(only[2], got[2])
    _check_step(only, x, cen, K, True, case + " assign", update=False)


@pytest.mark.parametrize("D", [50, 1024, 1500])
def test_strided_and_misaligned_rows_and_the_wide_path(rp, D):
    """Rows inside a wider table at a 4-byte offset (no 16-byte loads possible) give the bits of the aligned layout; D = 1500 takes the
    kernel for rows wider than 1024 columns."""
    from wsi_hgnn_amd import ops
    K = 8
    x = rc.gaussian_rows(SIZES, D, seed=3)
    cen = _centroids(x, K, seed=4)
    cd = torch.from_numpy(cen).to(DEV)
    wide = torch.zeros(NROWS, D + 7, device=DEV)
    wide[:, 1:1 + D] = torch.from_numpy(x).to(DEV)
    view = wide[:, 1:1 + D]
    assert view.data_ptr() % 16 == 4 and view.stride(0) == D + 7
    a = ops.bag_kmeans_step(view, rp, cd, True, True)
    _check_step(a, x, cen, K, True, f"strided D={D}")
    b = ops.bag_kmeans_step(torch.from_numpy(x).to(DEV), rp, cd, True, True)
    assert all(torch.equal(p, q) for p, q in zip(a, b))


def test_raw_abi(rp):
    from wsi_hgnn_amd import _native as N
    from wsi_hgnn_amd import ops
    lib = N.load()
    K, D = 8, 50
    x = rc.blob_rows(SIZES, D, K, seed=5)
    cen = _centroids(x, K, seed=6)
    xd, cd = torch.from_numpy(x).to(DEV), torch.from_numpy(cen).to(DEV)
    labels = torch.full((NROWS,), -1, dtype=torch.int32, device=DEV)
    counts = torch.full((S, K), -1, dtype=torch.int32, device=DEV)
    objective = torch.full((S,), -1.0, device=DEV)
    new = torch.full((S, K, D), -1.0, device=DEV)
    partial = torch.empty(rp.num_chunks * K * (D + 2), device=DEV)
    args = lambda k, out: (N.ptr(xd), D, D, N.ptr(cd), k, 1, N.ptr(rp.chunk_row), N.ptr(rp.chunk_seg), rp.num_chunks, N.ptr(rp.seg_chunk),
                           rp.num_segs, N.ptr(partial), N.ptr(labels), N.ptr(counts), N.ptr(objective), out, N.stream())
    assert lib.wsi_bag_kmeans_step(*args(K, N.ptr(new))) == 0
    got = (labels, counts, objective, new)
    _check_step(got, x, cen, K, True, "raw ABI")
    assert all(torch.equal(p, q) for p, q in zip(got, ops.bag_kmeans_step(xd, rp, cd, True, True)))
    kept = new.clone()
    assert lib.wsi_bag_kmeans_step(*args(K, None)) == 0 and torch.equal(new, kept)          # NULL: assign only, nothing written there
    assert lib.wsi_bag_kmeans_step(*args(17, N.ptr(new))) == N.WSI_ENOSYS and b"17 clusters" in lib.wsi_last_error()
    assert lib.wsi_bag_kmeans_step(*args(0, N.ptr(new))) == N.WSI_EINVAL
    assert lib.wsi_remix_nearest(N.ptr(cd), S, 17, D, None, None, 1, None, N.stream()) == N.WSI_ENOSYS
    assert lib.wsi_remix_rows(N.ptr(cd), None, S, K, 0, D, None, 0, None, 3, None, N.stream()) == N.WSI_EINVAL


@pytest.mark.parametrize("D", [50, 1024])
def test_exact_arithmetic_ties_go_to_the_smaller_index(rp, D):
    """Small-integer rows without normalisation: every product and sum is exact in float32, so labels equal float64's everywhere - with two
    identical centroids (2 and 5) and with rows constructed at the same distance from centroids 0 and 1."""
    from wsi_hgnn_amd import ops
    K = 8
    x = rc.integer_rows(SIZES, D, seed=9)
    cen = np.zeros((S, K, D), dtype=np.float32)
    rs = np.random.RandomState(10)
    for s, n in enumerate(SIZES):
        if n >= K:
            cen[s] = rs.randint(-3, 4, size=(K, D))
            cen[s, 5] = cen[s, 2]
            cen[s, 0] = 0
            cen[s, 1] = 0
            cen[s, 1, 0] = 2
            x[OFF[s]:OFF[s] + 3] = 0
            x[OFF[s]:OFF[s] + 3, 0] = 1                         # |x - c0|^2 = |x - c1|^2 = 1
    lab64, cnt64, obj64, _, gap = rc.step64(x, SIZES, cen, normalize=False)
    assert (gap == 0).sum() >= 3 * sum(n >= K for n in SIZES)
    labels, counts, objective, new = ops.bag_kmeans_step(torch.from_numpy(x).to(DEV), rp, torch.from_numpy(cen).to(DEV), False, True)
    assert np.array_equal(labels.cpu().numpy(), lab64)
    assert not (labels == 5).any() and all(int(labels[OFF[s]]) == 0 for s, n in enumerate(SIZES) if n >= K)
    if D == 50:                                                 # (at D = 1024 the objective of 1061 rows passes 2^24)
        assert np.array_equal(objective.cpu().numpy().astype(np.float64), obj64)
    R.check(new, torch.from_numpy(rc.step64(x, SIZES, cen, normalize=False)[3]), "new_centroids", f"integers D={D}")


@pytest.mark.parametrize("far", [(3,), (3, 6)])
def test_empty_clusters_are_split_off_the_largest(rp, far):
    from wsi_hgnn_amd import ops
    K, D = 8, 50
    x = rc.blob_rows(SIZES, D, K, seed=21)
    cen = _centroids(x, K, seed=22)
    for k in far:
        cen[:, k] = 5.0                                          # far from every unit row: the cluster stays empty
    labels, counts, objective, new = ops.bag_kmeans_step(torch.from_numpy(x).to(DEV), rp, torch.from_numpy(cen).to(DEV), True, True)
    mine = labels.cpu().numpy().astype(np.int64)
    assert not np.isin(mine, far).any()
    _, cnt64, _, new64, _ = rc.step64(x, SIZES, cen, labels=mine)
    assert np.array_equal(counts.cpu().numpy(), cnt64)
    R.check(new, torch.from_numpy(new64), "new_centroids", f"empty {far}")
    s = SIZES.index(1061)
    raw = np.bincount(mine[OFF[s]:OFF[s + 1]], minlength=K)
    donor = int(np.argmax(raw))
    assert int(counts[s, far[0]]) == raw[donor] // 2 and int(counts[s].sum()) == 1061
    ratio = (new[s, far[0]] / new[s, donor]).cpu().numpy()       # (1 + e) / (1 - e) on even columns, the inverse on odd ones
    e = rc.SPLIT_EPS
    if len(far) == 1:
        assert np.allclose(ratio[0::2], (1 + e) / (1 - e), rtol=1e-5) and np.allclose(ratio[1::2], (1 - e) / (1 + e), rtol=1e-5)


def test_zero_row_under_normalisation_gives_no_nan(rp):
    from wsi_hgnn_amd import ops
    K, D = 8, 512
    x = rc.gaussian_rows(SIZES, D, seed=31)
    zero = [OFF[s] + 2 for s, n in enumerate(SIZES) if n >= K]
    x[zero] = 0
    cen = _centroids(x, K, seed=32)
    got = ops.bag_kmeans_step(torch.from_numpy(x).to(DEV), rp, torch.from_numpy(cen).to(DEV), True, True)
    assert all(torch.isfinite(t.float()).all() for t in got)
    _check_step(got, x, cen, K, True, "zero rows")
    want = np.argmin((cen.astype(np.float64) ** 2).sum(-1), 1)     # a zero row goes to the centroid closest to the origin
    assert [int(got[0][r]) for r in zero] == [int(want[s]) for s, n in enumerate(SIZES) if n >= K]


@pytest.mark.parametrize("K,D", [(8, 1024), (16, 50), (2, 3)])
def test_reproducible_and_independent_of_the_other_bags(rp, K, D):
    from wsi_hgnn_amd import mil, ops
    x = rc.gaussian_rows(SIZES, D, seed=41)
    cen = _centroids(x, K, seed=42)
    xd, cd = torch.from_numpy(x).to(DEV), torch.from_numpy(cen).to(DEV)
    a = ops.bag_kmeans_step(xd, rp, cd, True, True)
    b = ops.bag_kmeans_step(xd, rp, cd, True, True)
    assert all(torch.equal(p, q) for p, q in zip(a, b))
    for s in (SIZES.index(1061), SIZES.index(129)):
        alone = ops.bag_kmeans_step(xd[OFF[s]:OFF[s + 1]].clone(), mil.bag_plan([SIZES[s]], DEV), cd[s:s + 1].clone(), True, True)
        assert torch.equal(alone[0], a[0][OFF[s]:OFF[s + 1]]) and torch.equal(alone[1][0], a[1][s])
        assert torch.equal(alone[2][0], a[2][s]) and torch.equal(alone[3][0], a[3][s])


def _bank(Sb, K, D, V, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(Sb, K, D, generator=g), torch.randn(Sb, K, V, D, generator=g) * 0.3


@pytest.mark.parametrize("K,D", [(3, 3), (8, 50), (8, 512), (16, 1030)])
def test_nearest_and_rows_kernels_equal_the_tensor_formulation(K, D):
    from wsi_hgnn_amd import ops
    from wsi_hgnn_amd.mil import remix
    Sb, V = 5, 6
    protos, shifts = _bank(Sb, K, D, V, seed=K * D)
    labels = [0, 1, 0, 0, 1]
    rng = np.random.RandomState(K + D)
    draws = [remix.draw_mix(rng, labels, i % Sb, K, mode, 0.6, V) for i, mode in enumerate(remix.MODES + (None, "joint"))]
    bank = remix.PrototypeBank(protos.to(DEV), shifts.to(DEV), labels)
    src = torch.tensor([d.idx for d in draws], dtype=torch.int32, device=DEV)
    tgt = torch.tensor([d.partner for d in draws], dtype=torch.int32, device=DEV)
    near = ops.remix_nearest(bank.prototypes, src, tgt)
    assert torch.equal(near.cpu(), remix.nearest_tensor(protos, src.cpu(), tgt.cpu()))
    d64 = ((protos[src.cpu().long()].double().unsqueeze(2) - protos[tgt.cpu().long()].double().unsqueeze(1)) ** 2).sum(-1)
    assert torch.equal(near.cpu().long(), d64.argmin(2))
    got, sizes = remix.mix(bank, draws)
    want, sizes_t = remix.mix(remix.PrototypeBank(protos, shifts, labels), draws, kernels=False)
    assert sizes == sizes_t == [d.num_rows for d in draws] and got.shape == want.shape
    ops_col = np.concatenate([d.desc[:, 0] for d in draws])
    copies = torch.from_numpy((ops_col == remix.KEEP) | (ops_col == remix.APPEND))
    assert torch.equal(got.cpu()[copies], want[copies])
    assert float((got.cpu() - want).abs().max()) <= 1e-6 * float(want.abs().max())
    assert (~copies).sum() > 0


def test_a_descriptor_outside_the_bank_gives_a_zero_row_and_reads_nothing():
    from wsi_hgnn_amd import ops
    protos, shifts = _bank(2, 4, 8, 3, seed=1)
    near = torch.zeros((1, 4), dtype=torch.int32, device=DEV)
    one = int(np.float32(0.5).view(np.int32))
    desc = torch.tensor([[0, 0, 1, 0, 0, 0, one, one], [0, 0, 99, 0, 0, 0, one, one], [1, 0, 1, 7, 0, 0, one, one], [3, 0, 1, 1, 0, 9, one, one],
                         [2, 44, 1, 1, 0, 0, one, one], [9, 0, 1, 1, 0, 0, one, one]], dtype=torch.int32, device=DEV)
    out = ops.remix_rows(protos.to(DEV), shifts.to(DEV), near, desc).cpu()
    assert torch.equal(out[0], protos[0, 1]) and not out[1:].any()


@pytest.mark.parametrize("name", ["replace.0.5", "append.1.0", "interpolate.0.5", "cov.0.5", "cov.1.0", "joint.0.5", "joint.1.0"])
def test_fixture_cases_on_the_device(name):
    f = np.load(FIX)
    Sb, K, V, D = (int(v) for v in f["shift_shape"])
    shifts = (np.random.RandomState(int(f["shift_seed"])).standard_normal((Sb, K, V, D)) * float(f["shift_scale"])).astype(np.float32)
    rows, want, draw, sizes = fixture_case(f, shifts, name, device=DEV)
    assert rows.is_cuda and sizes == [want.shape[0]]
    check_mixed_rows(rows, want, draw, name)
