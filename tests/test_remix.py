"""ReMix on the CPU: the draw order and the tensor formulation of the mixing against the reference's own ``mix_aug`` (tests/golden/mil/
reference_remix.npz, made by tests/golden/make_reference_remix_fixture.py), the shift formula against ``np.cov``, the bank's files, and
the restated reduction (tests/remix_cases.py)."""
import os

import numpy as np
import pytest
import torch

import remix_cases as rc
from wsi_hgnn_amd.mil import remix

FIX = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mil", "reference_remix.npz")


@pytest.fixture(scope="module")
def fixture():
    f = np.load(FIX)
    S, K, V, D = (int(v) for v in f["shift_shape"])
    shifts = (np.random.RandomState(int(f["shift_seed"])).standard_normal((S, K, V, D)) * float(f["shift_scale"])).astype(np.float32)
    return f, shifts


def fixture_case(f, shifts, name, device="cpu", kernels=None):
    """(got rows, reference rows, the draw) of one fixture case, from the same seed the reference ran under."""
    mode = name.split(".")[0]
    protos = f["prototypes"]
    bank = remix.PrototypeBank(torch.from_numpy(protos).to(device), torch.from_numpy(shifts).to(device), f["labels"])
    np.random.seed(int(f[name + ".seed"]))
    draw = remix.draw_mix(np.random, f["labels"], int(f[name + ".idx"]), protos.shape[1], mode, float(name.split(".", 1)[1]), shifts.shape[2])
    rows, sizes = remix.mix(bank, [draw], kernels=kernels)
    return rows, f[name + ".out"], draw, sizes


def check_mixed_rows(got, want, draw, name):
    """Copied rows bit for bit; interpolated and shifted rows within 1e-6 x the largest entry (two float32 roundings and a possible fused
    multiply-add against the reference's float64 for the shifted rows)."""
    got = got.detach().cpu().numpy()
    assert got.shape == want.shape and got.dtype == np.float32, (name, got.shape, want.shape)
    K = len(draw.perm)
    copied = [True] * K + [op == remix.APPEND for op, _, _, _ in draw.appended]
    for r, is_copy in enumerate(copied):
        if is_copy:
            assert np.array_equal(got[r], want[r]), f"{name}: copied row {r} differs"
        else:
            err = np.abs(got[r].astype(np.float64) - want[r]).max()
            print(f"{name} row {r}: error / bound {err / (1e-6 * np.abs(want).max()):.3e}")
            assert err <= 1e-6 * np.abs(want).max(), f"{name}: row {r} off by {err}"


def test_fixture_covers_every_mode_at_both_rates(fixture):
    f, _ = fixture
    assert sorted(f["cases"]) == sorted(f"{m}.{r}" for m in remix.MODES for r in (0.5, 1.0))
    assert f["prototypes"].shape[1:] == (8, 512) and f["prototypes"].dtype == np.float32
    assert sum(int(f[n + ".partner"]) != int(f[n + ".idx"]) for n in f["cases"]) >= 5


@pytest.mark.parametrize("name", [f"{m}.{r}" for m in remix.MODES for r in (0.5, 1.0)])
def test_draws_and_tensor_formulation_reproduce_the_reference(fixture, name):
    f, shifts = fixture
    rows, want, draw, sizes = fixture_case(f, shifts, name)
    assert draw.partner == int(f[name + ".partner"]) and draw.lam == float(f[name + ".strength"])
    assert sizes == [want.shape[0]] == [draw.num_rows]
    check_mixed_rows(rows, want, draw, name)


@pytest.mark.parametrize("name", ["joint.0.5", "cov.1.0", "interpolate.0.5"])
def test_restated_row_semantics_match_the_reference(fixture, name):
    """tests/remix_cases.mix_aug_rows (what the GPU tests restate with) is the reference's mix_aug too."""
    f, shifts = fixture
    _, want, draw, _ = fixture_case(f, shifts, name)
    src = f["prototypes"][draw.idx][draw.perm]
    got = rc.mix_aug_rows(src, f["prototypes"][draw.partner], shifts[draw.partner].astype(np.float64), draw.lam, draw.replaced, draw.appended)
    assert np.array_equal(got.astype(np.float32), want)


def test_draw_order_is_the_reference_order():
    """permutation(K), choice(same-class bags), uniform(0, 1), then the per-row draws - against np.random calls made by hand."""
    labels = np.asarray([0, 1, 1, 0, 1])
    for mode, per_row in (("replace", 1), ("cov", 1), ("joint", 4)):
        a, b = np.random.RandomState(77), np.random.RandomState(77)
        d = remix.draw_mix(a, labels, 2, 8, mode, 0.4, V=50)
        perm = b.permutation(8)
        partner = b.choice(np.argwhere(labels == labels[2]).reshape(-1))
        lam = b.uniform(0, 1)
        assert np.array_equal(d.perm, perm) and d.partner == partner and d.lam == lam
        fired = []
        for i in range(8):
            for j in range(per_row):
                hit = b.rand() <= 0.4
                fired.append(hit)
                if hit and (mode == "cov" or j == 3):
                    v = int(b.choice(50, 1)[0])
                    assert (remix.COV, i, bool(d.replaced[i]), v) in d.appended
        assert a.rand() == b.rand(), f"{mode}: the two streams are at different positions"
        if mode == "replace":
            assert list(d.replaced) == fired and d.num_rows == 8
        if mode == "joint":
            assert list(d.replaced) == fired[0::4] and d.num_rows == 8 + sum(fired) - sum(fired[0::4])
    a, b = np.random.RandomState(5), np.random.RandomState(5)
    d = remix.draw_mix(a, labels, 0, 8, None, 0.5)              # mode None: the shuffle alone
    assert np.array_equal(d.perm, b.permutation(8)) and a.rand() == b.rand() and d.num_rows == 8 and d.partner == 0
    with pytest.raises(ValueError):
        remix.draw_mix(a, labels, 0, 8, "mixup", 0.5)


def test_joint_uses_the_replaced_row_and_keeps_generation_order():
    protos = torch.arange(2 * 3 * 2, dtype=torch.float32).view(2, 3, 2) * 1.5
    shifts = torch.ones(2, 3, 4, 2)
    bank = remix.PrototypeBank(protos, shifts, [0, 0])
    rng = np.random.RandomState(1)
    d = remix.draw_mix(rng, bank.labels, 0, 3, "joint", 1.0, V=4)          # rate 1: every draw fires
    rows, sizes = remix.mix(bank, [d])
    assert sizes == [3 + 9] and [op for op, _, _, _ in d.appended] == [remix.APPEND, remix.INTERPOLATE, remix.COV] * 3
    want = rc.mix_aug_rows(protos[0].numpy()[d.perm], protos[d.partner].numpy(), shifts[d.partner].numpy().astype(np.float64), d.lam,
                           d.replaced, d.appended)
    assert np.abs(rows.numpy() - want).max() <= 1e-6 * np.abs(want).max()
    near = remix.nearest_tensor(protos, torch.tensor([0]), torch.tensor([d.partner]))[0].numpy()
    for i in range(3):                                                       # interpolating a replaced row with its target gives the target
        assert np.allclose(rows[3 + 3 * i + 1].numpy(), protos[d.partner, near[d.perm[i]]].numpy(), rtol=1e-6)


def test_cov_rows_need_the_shift_bank():
    bank = remix.PrototypeBank(torch.randn(2, 4, 3), None, [1, 1])
    d = remix.draw_mix(np.random.RandomState(0), bank.labels, 0, 4, "cov", 1.0, V=5)
    with pytest.raises(ValueError, match="shift bank"):
        remix.mix(bank, [d])


def test_prototype_bank_round_trip_keeps_the_reference_file_names(tmp_path):
    protos, shifts = torch.randn(3, 8, 16), torch.randn(3, 8, 5, 16)
    bank = remix.PrototypeBank(protos, shifts, [1, 0, 1])
    bank.save(str(tmp_path), 8)
    assert sorted(os.listdir(tmp_path)) == ["train_bag_feats_proto_8_base.npy", "train_bag_feats_shift_8_base.npy", "train_bag_labels_base.npy"]
    assert np.load(tmp_path / "train_bag_feats_proto_8_base.npy").shape == (3, 8, 16)
    assert np.load(tmp_path / "train_bag_feats_shift_8_base.npy").shape == (3, 8, 5, 16)
    assert np.load(tmp_path / "train_bag_labels_base.npy").tolist() == [1, 0, 1]
    back = remix.PrototypeBank.load(str(tmp_path), 8)
    assert torch.equal(back.prototypes, protos) and torch.equal(back.shifts, shifts) and back.labels.tolist() == [1, 0, 1]
    with pytest.raises(ValueError):
        bank.save(str(tmp_path), 4)


def test_from_reduced_drops_the_bags_that_are_not_ok():
    sizes = [40, 3, 60]
    x = torch.from_numpy(rc.blob_rows(sizes, 6, 4, seed=7)).double()
    red = remix.reduce_bags(x, sizes, num_prototypes=4, niter=5, num_shift_vectors=3)
    assert red.ok.tolist() == [n >= 4 and int(red.counts[s].min()) >= 2 for s, n in enumerate(sizes)]
    assert red.ok.tolist() == [True, False, True] and red.shifts.shape == (3, 4, 3, 6)
    bank = remix.PrototypeBank.from_reduced(red, [0, 1, 1])
    assert bank.prototypes.shape == (2, 4, 6) and bank.shifts.shape == (2, 4, 3, 6) and bank.labels.tolist() == [0, 1]
    assert torch.equal(bank.prototypes[1], red.prototypes[2])


def test_shift_formula_has_the_cluster_covariance():
    """With z = sqrt(n) Q (Q orthogonal, V = n) the V shifts of a cluster have exactly the sample covariance np.cov of its rows."""
    rs = np.random.RandomState(11)
    n, D, K = 24, 7, 2
    sizes = [2 * n]
    x = rs.standard_normal((2 * n, D)) * rs.uniform(0.5, 2.0, size=D)
    labels = np.asarray([0, 1] * n)
    q, _ = np.linalg.qr(rs.standard_normal((n, n)))
    z = np.zeros((2 * n, n))
    z[labels == 0] = np.sqrt(n) * q
    z[labels == 1] = np.sqrt(n) * q[::-1]
    counts = torch.tensor([[n, n]], dtype=torch.int32)
    protos = torch.from_numpy(np.stack([x[labels == k].mean(0) for k in range(K)])[None])
    got = remix.shift_bank(torch.from_numpy(x), sizes, torch.from_numpy(labels).to(torch.int32), counts, protos, torch.from_numpy(z)).numpy()
    assert np.abs(got - rc.shift64(x, sizes, labels, K, z)).max() <= 1e-12 * np.abs(got).max()
    for k in range(K):
        cov = np.cov(x[labels == k].T)
        emp = got[0, k].T @ got[0, k] / n
        assert np.abs(emp - cov).max() <= 1e-4 * np.abs(cov).max()


def test_clusters_of_one_row_give_zero_shifts_and_not_ok():
    x = torch.tensor([[1.0, 0.0], [0.9, 0.1], [1.0, 0.05], [0.0, 1.0]], dtype=torch.float64)          # the last row is a cluster of its own
    red = remix.reduce_bags(x, [4], num_prototypes=2, niter=4, num_shift_vectors=3, initial=torch.tensor([[0, 3]]))
    assert red.counts.tolist() == [[3, 1]] and red.ok.tolist() == [False]
    assert torch.count_nonzero(red.shifts[0, 1]) == 0 and torch.count_nonzero(red.shifts[0, 0]) > 0
    again = remix.reduce_bags(x, [4], num_prototypes=2, niter=4, num_shift_vectors=0, initial=torch.tensor([[0, 3]]))
    assert again.shifts is None and again.ok.tolist() == [True]


def test_step_tensor_formulation_is_the_restated_step():
    sizes = (0, 5, 8, 9, 40)
    x = rc.gaussian_rows(sizes, 6, seed=5)
    cen = np.random.RandomState(6).standard_normal((len(sizes), 8, 6))
    cen[4, 3] = 50.0                                                        # an empty cluster: the split rule runs
    want = rc.step64(x, sizes, cen)
    got = remix.kmeans_step_tensor(torch.from_numpy(x).double(), list(sizes), torch.from_numpy(cen))
    assert np.array_equal(got[0].numpy(), want[0]) and np.array_equal(got[1].numpy(), want[1])
    assert want[1][4, 3] > 0 and want[1].sum(1).tolist() == [0, 0, 8, 9, 40]
    assert np.allclose(got[2].numpy(), want[2], rtol=1e-12) and np.allclose(got[3].numpy(), want[3], rtol=1e-12, atol=1e-14)


def test_restated_reduction_objective_never_increases():
    sizes = (293, 5, 64)
    for x in (rc.gaussian_rows(sizes, 16, seed=1), rc.blob_rows(sizes, 16, 8, seed=2)):
        init = remix.initial_rows(sizes, 8, 66).numpy()
        lab, counts, protos, objs, _, _ = rc.reduce64(x, sizes, init, 8, niter=20)
        assert (np.diff(objs, axis=0) <= 1e-12 * objs[:-1] + 1e-300).all()
        assert counts.sum(1).tolist() == [293, 0, 64] and objs[:, 1].max() == 0
        red = remix.reduce_bags(torch.from_numpy(x).double(), list(sizes), niter=20, num_shift_vectors=0)
        assert np.array_equal(red.labels.numpy(), lab) and rc.rel_err(red.prototypes, torch.from_numpy(protos)) <= 1e-12
        assert np.allclose(red.objective.numpy(), objs, rtol=1e-10)


def test_initial_rows_are_distinct_rows_of_their_bag():
    sizes = [0, 5, 8, 200]
    rows = remix.initial_rows(sizes, 8, 66)
    assert rows.shape == (4, 8) and rows[:2].abs().sum() == 0
    assert sorted(rows[2].tolist()) == list(range(5, 13))
    assert len(set(rows[3].tolist())) == 8 and all(13 <= r < 213 for r in rows[3].tolist())
    assert not torch.equal(rows, remix.initial_rows(sizes, 8, 67))
