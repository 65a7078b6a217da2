"""ReMix end to end on the GPU: ``remix.reduce_bags`` against the float64 restatement from the same initial rows (tests/remix_cases.py), the
shift bank against float64, and ``remix.train_one_step`` against ``mil.train_one_step`` fed the rows the tensor formulation mixes.
Tolerance (the MIL tests' norm): error <= 1e-4 x the largest float64 entry of each tensor."""
import copy

import numpy as np
import pytest
import torch

import remix_cases as rc

pytestmark = pytest.mark.gpu

DEV = "cuda"
TOL = 1e-4
K = 8
SIZES = (1061, 5, 293, 128, 0)
OFF = rc.offsets(SIZES)
R = rc.Ratios(TOL)


@pytest.fixture(scope="module", autouse=True)
def _report_ratios():
    yield
    R.report()


@pytest.mark.parametrize("D", [64, 1024])
def test_reduce_bags_on_separated_blobs_equals_float64(D):
    """Centres N(0, 9), noise 0.5: the 20 iterations take the same labels in float32 as in float64 from the same initial rows."""
    from wsi_hgnn_amd.mil import remix
    x = rc.blob_rows(SIZES, D, K, seed=50 + D)
    red = remix.reduce_bags(torch.from_numpy(x).to(DEV), list(SIZES), num_prototypes=K, niter=20, seed=66, num_shift_vectors=0)
    init = remix.initial_rows(SIZES, K, 66, DEV).cpu().numpy()
    lab, counts, protos, objs, _, _ = rc.reduce64(x, SIZES, init, K, niter=20)
    differ = int((red.labels.cpu().numpy() != lab).sum())
    print(f"D={D}: {differ} labels differ after 20 iterations")
    assert differ == 0
    assert np.array_equal(red.counts.cpu().numpy(), counts)
    R.check(red.prototypes, torch.from_numpy(protos), "prototypes", f"blobs D={D}")
    R.check(red.objective[-1], torch.from_numpy(objs[-1]), "objective", f"blobs D={D}")
    assert red.ok.tolist() == [True, False, True, True, False] and red.shifts is None


def test_reduce_bags_on_gaussian_noise_keeps_its_invariants():
    from wsi_hgnn_amd.mil import remix
    D = 64
    x = rc.gaussian_rows(SIZES, D, seed=61)
    red = remix.reduce_bags(torch.from_numpy(x).to(DEV), list(SIZES), num_prototypes=K, niter=20, num_shift_vectors=0)
    mine = red.labels.cpu().numpy().astype(np.int64)
    cen = red.centroids.cpu().numpy()
    # the final labels are the assignment to the final centroids (outside the band of float32 ties)
    lab64, _, _, _, gap = rc.step64(x, SIZES, cen, update=False)
    assert not ((mine != lab64) & (gap > rc.BAND)).any()
    # prototypes are the means of the raw rows of the labels
    want = np.zeros((len(SIZES), K, D))
    for s, n in enumerate(SIZES):
        for k in range(K):
            m = mine[OFF[s]:OFF[s + 1]] == k
            if n >= K and m.any():
                want[s, k] = x[OFF[s]:OFF[s + 1]][m].astype(np.float64).mean(0)
    R.check(red.prototypes, torch.from_numpy(want), "prototypes", "gaussian")
    assert red.counts.sum(1).tolist() == [n if n >= K else 0 for n in SIZES]
    obj = red.objective.double().cpu().numpy()
    assert obj.shape == (21, len(SIZES)) and (np.diff(obj, axis=0) <= 1e-5 * obj[:-1]).all(), "the objective rose"


def test_reduce_bags_reads_nothing_back():
    """The whole reduction - initial rows, 5 iterations, prototypes, shifts, ok - queues without a synchronising call."""
    from wsi_hgnn_amd import mil
    from wsi_hgnn_amd.mil import remix
    x = torch.from_numpy(rc.blob_rows(SIZES, 64, K, seed=91)).to(DEV)
    plan = mil.bag_plan(SIZES, DEV)
    remix.reduce_bags(x, plan, num_prototypes=K, niter=1, num_shift_vectors=4)            # (first use: code objects, the plan's row table)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        red = remix.reduce_bags(x, plan, num_prototypes=K, niter=5, num_shift_vectors=4)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert red.ok.is_cuda and red.ok.tolist() == [True, False, True, True, False]
    with pytest.raises(ValueError, match="host values"):
        remix.reduce_bags(x, torch.tensor(SIZES, device=DEV))


def test_initial_rows_equal_the_cpu_formulation():
    from wsi_hgnn_amd.mil import remix
    for seed in (66, 7):
        dev = remix.initial_rows(SIZES, K, seed, DEV)
        assert dev.is_cuda and torch.equal(dev.cpu(), remix.initial_rows(SIZES, K, seed, "cpu"))


@pytest.mark.parametrize("V", [200, 5])
def test_shifts_from_a_given_z_against_float64(V):
    from wsi_hgnn_amd.mil import remix
    D = 64
    x = rc.blob_rows(SIZES, D, K, seed=71)
    z = np.random.RandomState(72).standard_normal((OFF[-1], V)).astype(np.float32)
    red = remix.reduce_bags(torch.from_numpy(x).to(DEV), list(SIZES), num_prototypes=K, niter=5, num_shift_vectors=V, z=torch.from_numpy(z).to(DEV))
    mine = red.labels.cpu().numpy()
    want = rc.shift64(x, SIZES, mine, K, z)
    small = red.counts.cpu().numpy() < 2
    want[small] = 0
    for s, n in enumerate(SIZES):
        if n < K:
            want[s] = 0
    R.check(red.shifts, torch.from_numpy(want), "shifts", f"V={V}")
    assert red.ok.tolist() == [n >= K and not small[s].any() for s, n in enumerate(SIZES)]
    again = remix.reduce_bags(torch.from_numpy(x).to(DEV), list(SIZES), num_prototypes=K, niter=5, num_shift_vectors=V)
    assert again.shifts.shape == (len(SIZES), K, V, D) and torch.isfinite(again.shifts).all()       # z drawn on the device from the seed


@pytest.mark.parametrize("model", ["abmil", "dsmil"])
def test_train_one_step_equals_the_step_on_the_tensor_formulations_rows(model):
    from wsi_hgnn_amd import mil
    from wsi_hgnn_amd.mil import abmil, dsmil, remix
    Sb, D, V, C = 6, 64, 10, 2
    g = torch.Generator().manual_seed(81)
    protos, shifts = torch.randn(Sb, K, D, generator=g), torch.randn(Sb, K, V, D, generator=g) * 0.3
    labels = np.asarray([0, 1, 1, 0, 1, 0])
    idxs = [4, 0, 3, 1]
    torch.manual_seed(82)
    m = (dsmil.MILNet(dsmil.FCLayer(D, C), dsmil.BClassifier(D, C, dropout_v=0.0)) if model == "dsmil" else abmil.BClassifier(D, C)).to(DEV)
    m2 = copy.deepcopy(m)
    bank = remix.PrototypeBank(protos.to(DEV), shifts.to(DEV), labels)
    loss = remix.train_one_step(m, torch.optim.SGD(m.parameters(), lr=0.0), bank, idxs, "joint", 0.5, np.random.RandomState(83))
    rng = np.random.RandomState(83)
    draws = [remix.draw_mix(rng, labels, i, K, "joint", 0.5, V) for i in idxs]
    rows, sizes = remix.mix(remix.PrototypeBank(protos, shifts, labels), draws, kernels=False)
    assert sum(sizes) > 4 * K
    want = mil.train_one_step(m2, torch.optim.SGD(m2.parameters(), lr=0.0), rows.to(DEV), mil.bag_plan(sizes, DEV), labels[idxs])
    R.check(loss.view(1), want.view(1), "loss", model)
    for (k, p), (_, q) in zip(m.named_parameters(), m2.named_parameters()):
        if k == "attention.2.bias":            # zero in exact arithmetic (a softmax ignores a shift): held against the weight gradient's scale
            assert float((p.grad - q.grad).abs().max()) <= TOL * float(m2.attention[2].weight.grad.abs().max())
            continue
        R.check(p.grad, q.grad, "g." + k, model)
    plain = remix.train_one_step(m, torch.optim.SGD(m.parameters(), lr=0.0), bank, idxs, None, 0.5, np.random.RandomState(84))
    assert torch.isfinite(plain)
