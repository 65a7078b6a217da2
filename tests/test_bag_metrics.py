"""The bag metrics without a GPU: the CPU formulation of ``mil.BagEpochMetrics`` fed the scores and labels of tests/bag_metrics_cases.py against
the fixture recorded from the reference's own ``multi_label_roc`` / ``optimal_thresh`` / ``inverse_convert_label`` and sklearn
(tests/golden/mil/reference_bag_metrics.json): thresholds bit-equal, every integer equal, AUCs and every score of the two scripts within 1e-12;
updates in pieces, reset, every flag, weights of 0, scores and loss against float64 (the bounds of tests/test_epoch_metrics.py: 1e-6 / 1e-5), and
``mil.evaluate`` on the CPU against a per-bag loop."""
import json
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import bag_metrics_cases as BM
import mil_cases as MC

HERE = os.path.dirname(os.path.abspath(__file__))
FIX = json.load(open(os.path.join(HERE, "golden", "mil", "reference_bag_metrics.json")))
CASES = {c["name"]: c for c in FIX["cases"]}
TOL = 1e-12


def _metrics(C, capacity):
    from wsi_hgnn_amd import mil
    return mil.BagEpochMetrics(C, capacity, "cpu")


def _feed(m, scores, labels):
    """Put fp32 scores straight into the accumulator (the fixture's scores, bit for bit: a sigmoid of logits would round them again)."""
    n = scores.shape[0]
    m.reset()
    m.score_rows[:n] = torch.from_numpy(scores)
    m.target_rows[:n] = torch.from_numpy(labels)
    m.state[0] = n
    return m


def _bits(x):
    return int(np.array([x], dtype=np.float64).view(np.int64)[0])


def check_against_fixture(case, block, got):
    """``block``: the int64 result block; ``got``: the dict derived from it."""
    from wsi_hgnn_amd.mil import metrics as M
    C, n = case["C"], case["n"]
    K = C if C > 1 else 2
    assert block[0] == n and block[1] == 0 and got["n"] == n
    assert block[3] == case["exact"]
    for c in range(C):
        w = block[M.HEAD + 8 * c:M.HEAD + 8 * c + 8]
        assert w[0] == case["threshold_bits"][c], (case["name"], c, got["thresholds"][c])
        assert list(w[1:7]) == [case[k][c] for k in ("tp", "fp", "P", "N", "gt", "eq")], (case["name"], c)
        assert abs(got["auc"][c] - case["auc"][c]) <= TOL, (case["name"], c)
        assert _bits(got["thresholds"][c]) == case["threshold_bits"][c]
    conf = [list(block[M.HEAD + 8 * C + r * K:M.HEAD + 8 * C + (r + 1) * K]) for r in range(K)]
    assert conf == case["confusion"], case["name"]
    for script in ("tcga", "remix"):
        for k, want in case[script].items():
            assert abs(got[script][k] - want) <= TOL, (case["name"], script, k, got[script][k], want)


def test_fixture_covers_what_the_issue_lists():
    assert FIX["sklearn"] == "1.7.2" and len(CASES) == len(BM.case_list())
    fams = {c["family"] for c in CASES.values()}
    assert fams == set(BM.FAMILIES)
    assert {c["n"] for c in CASES.values()} >= {2, 3, 7, 64, 65, 257, 300, 256} and {c["C"] for c in CASES.values()} == {1, 2, 3, 5}
    inf = _bits(math.inf)
    assert all(all(b == inf for b in c["threshold_bits"]) for c in CASES.values() if c["family"] == "anti")
    assert any(p < d + 1 for c in CASES.values() if c["family"] == "runs" for p, d in zip(c["roc_points"], c["distinct_scores"]))     # step 3 drops points
    assert all(c["P"][k] > 0 and c["N"][k] > 0 for c in CASES.values() for k in range(c["C"]))
    absent = [c for c in CASES.values() if c["absent"] is not None]
    assert len(absent) >= 4 and all(c["absent"] not in c["labels_present"] and len(c["labels_present"]) < c["C"] for c in absent)


@pytest.mark.parametrize("name", sorted(CASES))
def test_cpu_formulation_against_the_reference(name):
    from wsi_hgnn_amd.mil import metrics as M
    case = CASES[name]
    scores, labels = BM.build(case["n"], case["C"], case["family"], case["seed"], case["absent"])
    assert scores.shape == (case["n"], case["C"])
    assert int(scores.view(np.int32).astype(np.int64).sum()) == case["score_bits_sum"] and [int(v) for v in labels.sum(0)] == case["label_sum"]
    m = _feed(_metrics(case["C"], case["n"]), scores, labels)
    block = m.result_block()
    check_against_fixture(case, block, M.derive(block, case["C"]))
    assert m.compute() == M.derive(block, case["C"])                  # (no flag is set: nothing in it is NaN)


def _logit_case(n, C, seed, dsmil=True):
    rng = np.random.RandomState(seed)
    bag = (3 * rng.randn(n, C)).astype(np.float32)
    mx = (3 * rng.randn(n, C)).astype(np.float32) if dsmil else None
    y = BM.labels_for(rng, n, C).astype(np.float32)
    return bag, mx, y


def _t(a):
    return None if a is None else torch.from_numpy(a)


@pytest.mark.parametrize("C,dsmil", [(1, True), (2, False), (5, True)])
def test_update_in_pieces_scores_and_loss(C, dsmil):
    n = 65
    bag, mx, y = _logit_case(n, C, 7 + C, dsmil)
    whole = _metrics(C, n)
    whole.update(_t(bag), _t(y), None, _t(mx))
    want_block = whole.result_block()
    for piece in (1, 3):
        m = _metrics(C, n)
        for lo in range(0, n, piece):
            m.update(_t(bag[lo:lo + piece]), _t(y[lo:lo + piece]), None, _t(None if mx is None else mx[lo:lo + piece]))
        assert torch.equal(m.scores(), whole.scores()) and torch.equal(m.targets(), whole.targets())
        block = m.result_block()
        assert block[:2] == want_block[:2] and block[3:] == want_block[3:]
        assert abs(m.compute()["loss"] - whole.compute()["loss"]) <= 1e-12
    s64 = torch.sigmoid(torch.from_numpy(bag).double())
    assert float((whole.scores().double() - s64).abs().max()) <= 1e-6
    t64 = torch.from_numpy(y).double()
    bce = lambda x: F.binary_cross_entropy_with_logits(torch.from_numpy(x).double(), t64, reduction="none").mean(1)
    loss64 = float((0.5 * bce(bag) + 0.5 * bce(mx) if dsmil else bce(bag)).mean())
    assert abs(whole.compute()["loss"] - loss64) <= 1e-5
    assert whole.compute()["n"] == n
    first = whole.scores()[:9].clone()
    whole.reset()
    assert whole.scores().shape[0] == 0 and int(whole.state[1]) == 0 and float(whole._loss_sum) == 0.0
    whole.update(_t(bag[:9]), _t(y[:9]), None, _t(None if mx is None else mx[:9]))
    assert whole.scores().shape[0] == 9 and torch.equal(whole.scores(), first)


def test_flags_and_weights():
    C, n = 2, 8
    bag, mx, y = _logit_case(n, C, 3)
    # non-finite logits (either prediction), a bad target: the row is skipped and the flag named
    for spoil, why in ((lambda b, m_, t: b.__setitem__((2, 1), np.inf), "non-finite"), (lambda b, m_, t: m_.__setitem__((3, 0), np.nan), "non-finite"),
                       (lambda b, m_, t: t.__setitem__((4, 1), 0.5), "target other than 0 or 1")):
        b2, m2, y2 = bag.copy(), mx.copy(), y.copy()
        spoil(b2, m2, y2)
        m = _metrics(C, n)
        m.update(_t(b2), _t(y2), None, _t(m2))
        assert m.scores().shape[0] == n - 1
        with pytest.raises(RuntimeError, match=why):
            m.compute()
    # a weight of 0 skips the row before it is looked at
    w = np.ones(n, dtype=np.float32)
    w[[1, 5]] = 0
    b2 = bag.copy()
    b2[1] = np.nan
    m = _metrics(C, n)
    m.update(_t(b2), _t(y), _t(w).view(-1, 1), _t(mx))
    keep = w > 0
    assert m.scores().shape[0] == 6 and int(m.state[1]) == 0
    assert torch.equal(m.targets(), torch.from_numpy(y[keep]))
    ref = _metrics(C, n)
    ref.update(_t(bag[keep]), _t(y[keep]), None, _t(mx[keep]))
    assert torch.equal(m.scores(), ref.scores()) and m.result_block(check=False) == ref.result_block(check=False)
    # overflow: capacity n holds the rows, n - 1 drops the last and nothing is written past it
    full = _metrics(C, n)
    full.update(_t(bag), _t(y), None, _t(mx))
    assert int(full.state[1]) == 0 and full.scores().shape[0] == n
    short = _metrics(C, n - 1)
    short.update(_t(bag[:5]), _t(y[:5]), None, _t(mx[:5]))
    short.update(_t(bag[5:]), _t(y[5:]), None, _t(mx[5:]))
    assert short.scores().shape[0] == n - 1 and torch.equal(short.scores(), full.scores()[:n - 1])
    with pytest.raises(RuntimeError, match="capacity"):
        short.compute()
    # a class with one label value (also n = 1, and n = 0)
    y1 = y.copy()
    y1[:, 1] = 0
    one = _metrics(C, n)
    one.update(_t(bag), _t(y1), None, _t(mx))
    with pytest.raises(RuntimeError, match="without a positive or without a negative"):
        one.compute()
    from wsi_hgnn_amd import _native as N
    blk = one.result_block(check=False)
    assert blk[1] == N.WSI_BAG_METRICS_ONE_LABEL and math.isnan(np.array(blk[4 + 8:4 + 9], dtype=np.int64).view(np.float64)[0])
    single = _metrics(C, 4)
    single.update(_t(bag[:1]), _t(y[:1]), None, _t(mx[:1]))
    with pytest.raises(RuntimeError, match="without a positive"):
        single.compute()
    with pytest.raises(RuntimeError, match="without a positive"):
        _metrics(C, 4).compute()


def test_argument_errors():
    from wsi_hgnn_amd import mil
    with pytest.raises(ValueError, match="num_classes"):
        mil.BagEpochMetrics(33, 10, "cpu")
    with pytest.raises(ValueError, match="capacity"):
        mil.BagEpochMetrics(2, 4097, "cpu")
    m = mil.BagEpochMetrics(2, 4096, "cpu")
    with pytest.raises(ValueError, match="contiguous"):
        m.update(torch.zeros(3, 3), torch.zeros(3, 3))
    with pytest.raises(ValueError, match="contiguous"):
        m.update(torch.zeros(3, 2), torch.zeros(4, 2))
    with pytest.raises(ValueError, match="weights"):
        m.update(torch.zeros(3, 2), torch.zeros(3, 2), torch.ones(2))
    assert {"BagEpochMetrics", "CapturedBagEval", "evaluate"} <= set(mil.__all__)


def test_library_exports_and_refuses_without_a_gpu():
    from wsi_hgnn_amd import _native as N
    lib = N.load()
    assert lib.wsi_bag_metrics_update(None, None, None, None, 4, 33, None, None, None, 8, None) == N.WSI_ENOSYS
    assert lib.wsi_bag_metrics_update(None, None, None, None, 4, 2, None, None, None, N.WSI_BAG_METRICS_MAX_ROWS + 1, None) == N.WSI_ENOSYS
    assert lib.wsi_bag_metrics_update(None, None, None, None, 4, 2, None, None, None, 8, None) == N.WSI_EINVAL
    assert lib.wsi_bag_metrics_finalize(None, None, None, 2, N.WSI_BAG_METRICS_MAX_ROWS + 1, None, None) == N.WSI_ENOSYS
    assert lib.wsi_bag_metrics_finalize(None, None, None, 2, 8, None, None) == N.WSI_EINVAL and b"null" in lib.wsi_last_error()


class _TorchDsmil(torch.nn.Module):
    """The float32 restatement of tests/mil_cases.py behind the package's call signature ``(rows, plan)``: a model the CPU can run."""

    def __init__(self, sd, model):
        super().__init__()
        self.sd, self.model = {k: v.detach().float() for k, v in sd.items()}, model

    def forward(self, x, bags):
        sizes = [b - a for a, b in bags.ranges]
        if self.model == "dsmil":
            return MC.dsmil_forward(self.sd, x, sizes)
        return MC.abmil_forward(self.sd, x, sizes)


@pytest.mark.parametrize("model", ["dsmil", "abmil"])
def test_evaluate_on_the_cpu_against_a_per_bag_loop(model):
    from wsi_hgnn_amd import mil
    from wsi_hgnn_amd.mil import abmil, dsmil
    feats, C = 20, 2
    torch.manual_seed(5)
    net = dsmil.MILNet(dsmil.FCLayer(feats, C), dsmil.BClassifier(feats, C)) if model == "dsmil" else abmil.BClassifier(feats, C)
    with torch.no_grad():
        for p in net.parameters():
            p.mul_(3.0)
    twin = _TorchDsmil(dict(net.state_dict()), model)
    sizes, labels = (5, 40, 13, 7, 22, 31, 9), (0, 1, 1, 0, 2, 1, 0)                 # (2: past the last class - the all-zero target row)
    g = torch.Generator().manual_seed(11)
    bags = [torch.randn(n, feats, generator=g) for n in sizes]
    twin.train()
    got = mil.evaluate(twin, bags, labels, batch_size=3)
    assert twin.training                                                             # the flag is restored
    # the reference's loop: one bag per forward
    m = mil.BagEpochMetrics(C, len(bags), "cpu")
    total = 0.0
    for x, lab in zip(bags, labels):
        t = MC.target_row(lab, C).view(1, -1)
        out = twin(x, mil.bag_plan([x.shape[0]], "cpu"))
        bag = (out[1] if model == "dsmil" else out).view(1, -1)
        mx = out[0].max(0)[0].view(1, -1) if model == "dsmil" else None
        loss = F.binary_cross_entropy_with_logits(bag.double(), t.double())
        if mx is not None:
            loss = 0.5 * loss + 0.5 * F.binary_cross_entropy_with_logits(mx.double(), t.double())
        total += float(loss)
        m.update(bag.contiguous(), t.contiguous(), None, mx)
    want = m.compute()
    assert got["n"] == want["n"] == len(bags)
    assert abs(got["loss"] - total / len(bags)) <= 1e-5
    for k in ("auc", "thresholds"):
        assert np.allclose(got[k], want[k], rtol=0, atol=1e-5), k
    assert got["tcga"] == want["tcga"] and got["remix"] == want["remix"]
    again = mil.evaluate(twin, bags, labels, metrics=m, batch_size=7)                # a passed accumulator is reset first
    assert again["n"] == len(bags) and again["tcga"] == want["tcga"]
