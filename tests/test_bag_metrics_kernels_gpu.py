"""``wsi_bag_metrics_update`` / ``wsi_bag_metrics_finalize`` on the GPU, from logits: the stored scores against a float64 sigmoid (1e-6), then the
CPU formulation of ``mil.BagEpochMetrics`` applied to the scores READ BACK from the device - thresholds, every integer, the AUCs and the flag word
must be equal exactly (the ranking consumes the same bits) - and the loss sum against float64 BCE (1e-5).  The cases of the reference fixture
(tests/bag_metrics_cases.py), the sizes around a wave and around the update's tile of 256, the supported capacity, C = 1 and C = 32, every flag,
sentinels behind the cursor and behind the capacity, and two identical runs bit for bit."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import bag_metrics_cases as BM

pytestmark = pytest.mark.gpu

DEV = "cuda"
SENTINEL = -7.0
PAD = 5                      # sentinel rows behind the capacity
WORST = {"score": 0.0, "loss": 0.0}


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    print(f"\nlargest error / bound: scores {WORST['score'] / 1e-6:.3e}, loss sum {WORST['loss'] / 1e-5:.3e}")


def _guarded(C, capacity):
    """A device accumulator whose row buffers and result block are views into larger sentinel-filled ones."""
    from wsi_hgnn_amd import mil
    m = mil.BagEpochMetrics(C, capacity, DEV)
    m._big = [torch.full((capacity + PAD, C), SENTINEL, device=DEV), torch.full((capacity + PAD, C), SENTINEL, device=DEV),
              torch.full((m.result.numel() + PAD,), -7, dtype=torch.int64, device=DEV)]
    m.score_rows, m.target_rows, m.result = m._big[0][:capacity], m._big[1][:capacity], m._big[2][:m.result.numel()]
    return m


def _run(m, bag, mx, y, w=None, piece=None):
    n = bag.shape[0]
    piece = piece or n
    for lo in range(0, n, piece):
        sl = slice(lo, lo + piece)
        m.update(torch.from_numpy(bag[sl]).to(DEV), torch.from_numpy(y[sl]).to(DEV), None if w is None else torch.from_numpy(w[sl]).to(DEV),
                 None if mx is None else torch.from_numpy(mx[sl]).to(DEV))
    return m


def _check(m, bag, mx, y, counted, flags_expected=0):
    """``counted``: bool [n], the rows the update must have stored (in order)."""
    from wsi_hgnn_amd import mil
    C, cap = m.num_classes, m.capacity
    stored = counted.copy()
    stored[np.nonzero(counted)[0][cap:]] = False
    n = int(stored.sum())
    block = m.result_block(check=False)
    torch.cuda.synchronize()
    assert int(m.state[0]) == n == block[0]
    scores = m._big[0].cpu().numpy()
    # sentinels: nothing behind the cursor, nothing behind the capacity
    assert (scores[n:] == SENTINEL).all() and (m._big[1].cpu().numpy()[n:] == SENTINEL).all()
    assert (m._big[2][-PAD:] == -7).all()
    assert np.array_equal(m._big[1].cpu().numpy()[:n], y[stored])
    s64 = torch.sigmoid(torch.from_numpy(bag[stored]).double()).numpy()
    err = float(np.abs(scores[:n].astype(np.float64) - s64).max()) if n else 0.0
    WORST["score"] = max(WORST["score"], err)
    assert err <= 1e-6
    # the CPU formulation over the device's own scores
    ref = mil.BagEpochMetrics(C, cap, "cpu")
    ref.score_rows[:n] = torch.from_numpy(scores[:n])
    ref.target_rows[:n] = torch.from_numpy(y[stored])
    ref.state[0] = n
    ref.state[1] = int(m.state[1])
    want = ref.result_block(check=False)
    assert block[1] == want[1] == flags_expected
    assert block[:2] == want[:2] and block[3:] == want[3:], [(i, a, b) for i, (a, b) in enumerate(zip(block, want)) if a != b and i != 2][:8]
    t64 = torch.from_numpy(y[stored]).double()
    bce = lambda x: F.binary_cross_entropy_with_logits(torch.from_numpy(x[stored]).double(), t64, reduction="none").mean(1)
    loss64 = float((bce(bag) if mx is None else 0.5 * bce(bag) + 0.5 * bce(mx)).sum()) if n else 0.0
    got = float(np.array(block[2:3], dtype=np.int64).view(np.float64)[0])
    WORST["loss"] = max(WORST["loss"], abs(got - loss64))
    assert abs(got - loss64) <= 1e-5
    return block


_FIXTURE_CASES = BM.case_list()


@pytest.mark.parametrize("n", BM.NS)
def test_fixture_cases_from_logits(n):
    """Every case of the reference fixture with this n (all C, all families), logits in, one accumulator per C reset between cases."""
    acc = {}
    for name, cn, C, family, seed, absent in _FIXTURE_CASES:
        if cn != n:
            continue
        scores, y = BM.build(cn, C, family, seed, absent)
        bag = BM.logits_for(scores)
        rng = np.random.RandomState(seed)
        mx = (bag + rng.rand(*bag.shape).astype(np.float32)) if seed % 2 else None          # DSMIL's second term / ABMIL
        m = acc.setdefault(C, _guarded(C, n))
        m.reset()
        for t in m._big[:2]:
            t.fill_(SENTINEL)
        _run(m, bag, mx, y, piece=(None, 1 if n <= 7 else 29, 64)[seed % 3])
        _check(m, bag, mx, y, np.ones(scores.shape[0], dtype=bool))


def _mixed(n, C, seed):
    """Logits whose columns take the families in turn (continuous, five levels, two levels), labels with both values in every class."""
    rng = np.random.RandomState(seed)
    y = BM.labels_for(rng, n, C)
    fam = ("continuous", "levels5", "levels2", "separable")
    s = np.stack([BM.scores_for(rng, fam[c % 4], y[:, c]) for c in range(C)], 1)
    bag = BM.logits_for(s)
    return bag, (bag - rng.rand(n, C).astype(np.float32)), y.astype(np.float32)


@pytest.mark.parametrize("n,C,piece", [(63, 3, None), (64, 3, None), (65, 3, None), (256, 2, None), (257, 2, None), (257, 32, 100), (300, 1, 7),
                                       (1000, 32, 2048), (4096, 1, 1500), (4096, 2, None), (4095, 5, 4095)])
def test_sizes_classes_and_capacity(n, C, piece):
    bag, mx, y = _mixed(n, C, 40 + n + C)
    m = _run(_guarded(C, n), bag, mx, y, piece=piece)
    _check(m, bag, mx, y, np.ones(n, dtype=bool))


def test_flags_weights_and_overflow():
    from wsi_hgnn_amd import _native as N
    n, C = 300, 2
    bag, mx, y = _mixed(n, C, 9)
    w = np.ones(n, dtype=np.float32)
    w[[0, 77, 255, 256, 299]] = 0
    bag[77] = np.nan                                              # (weight 0: never looked at)
    y[255] = 3.0
    counted = w > 0
    m = _run(_guarded(C, n), bag, mx, y, w)
    _check(m, bag, mx, y, counted)
    b2, m2, y2 = bag.copy(), mx.copy(), y.copy()
    b2[5, 1], m2[260, 0], y2[100, 0] = np.inf, np.nan, 0.5
    bad = counted.copy()
    bad[[5, 260, 100]] = False
    m = _run(_guarded(C, n), b2, m2, y2, w)
    _check(m, b2, m2, y2, bad, N.WSI_BAG_METRICS_NONFINITE | N.WSI_BAG_METRICS_BAD_TARGET)
    # overflow: the capacity holds exactly the counted rows, or one fewer - across two updates, the second one crossing it
    k = int(counted.sum())
    m = _run(_guarded(C, k), bag, mx, y, w, piece=200)
    _check(m, bag, mx, y, counted)
    m = _run(_guarded(C, k - 1), bag, mx, y, w, piece=200)
    _check(m, bag, mx, y, counted, N.WSI_BAG_METRICS_OVERFLOW)
    with pytest.raises(RuntimeError, match="capacity"):
        m.compute()
    # a class with one label value; n = 1; n = 0
    y1 = y.copy()
    y1[:, 1] = 1.0
    m = _run(_guarded(C, n), bag, mx, y1, w)
    _check(m, bag, mx, y1, counted, N.WSI_BAG_METRICS_ONE_LABEL)
    with pytest.raises(RuntimeError, match="without a positive or without a negative"):
        m.compute()
    m = _run(_guarded(C, 4), bag[1:2], mx[1:2], y[1:2])
    _check(m, bag[1:2], mx[1:2], y[1:2], np.ones(1, dtype=bool), N.WSI_BAG_METRICS_ONE_LABEL)
    m = _guarded(C, 4)
    _check(m, bag[:0], mx[:0], y[:0], np.zeros(0, dtype=bool), N.WSI_BAG_METRICS_ONE_LABEL)


def test_identical_calls_give_identical_bits():
    n, C = 700, 5
    bag, mx, y = _mixed(n, C, 21)
    runs = []
    for _ in range(2):
        m = _run(_guarded(C, n), bag, mx, y, piece=256)
        m.result_block()
        torch.cuda.synchronize()
        runs.append([m.state.clone()] + [t.clone() for t in m._big])
    for a, b in zip(*runs):
        assert torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a, b.view(torch.int32) if b.dtype == torch.float32 else b)
    first = runs[0][3].clone()
    m.result_block()                                              # finalize again over the same rows
    assert torch.equal(m._big[2], first)


def test_constructor_limits_on_the_device():
    from wsi_hgnn_amd import mil
    with pytest.raises(ValueError, match="capacity"):
        mil.BagEpochMetrics(2, 4097, DEV)
    with pytest.raises(ValueError, match="num_classes"):
        mil.BagEpochMetrics(33, 64, DEV)
    m = mil.BagEpochMetrics(2, 8, DEV)
    with pytest.raises(RuntimeError, match="lives on"):
        m.update(torch.zeros(2, 2), torch.zeros(2, 2))
