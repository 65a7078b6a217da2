"""Case builders shared by tests/golden/make_reference_bag_metrics_fixture.py, tests/test_bag_metrics.py and the GPU tests of the bag metrics:
score families in fp32 with labels in which every class has both values, and the logits whose fp32 sigmoid they come from.

Families (per class column): 'continuous' random; 'levels2' / 'levels3' / 'levels5' quantised to that many values (heavy ties); 'equal' all the
same; 'separable' every positive above every negative; 'anti' every positive below every negative - the first minimum of fpr - tpr is then the
prepended (0, 0) point, the threshold +inf and every prediction 0; 'collinear' strictly descending scores with alternating labels, P = N - a ROC
staircase whose upper corners all lie on one line of slope 1, so fpr - tpr is tied there but for fp64 rounding; 'runs' the same scores with the
labels in runs of three - the interior points of every run are collinear with their neighbours and sklearn's drop_intermediate removes them."""
import numpy as np

NS = (2, 3, 7, 64, 65, 257, 300)
CS = (1, 2, 3, 5)
FAMILIES = ("continuous", "levels2", "levels3", "levels5", "equal", "separable", "anti", "collinear", "runs")


def labels_for(rng, n, C, absent=None):
    """bool [n, C]: every class has both values.  C > 1: one-hot rows of a drawn class, some rows all zero (a label past the last class);
    ``absent``: a class no row DECODES to is still given positives only in rows an earlier class owns (multi-label rows)."""
    if C == 1:
        y = rng.rand(n) < 0.4
        y[0], y[1] = True, False
        return y.reshape(n, 1)
    cls = rng.randint(0, C + 1, size=n)                   # C: the all-zero row
    cls[:2] = (0, 1)
    y = cls[:, None] == np.arange(C)[None, :]
    for c in range(C):
        if y[:, c].all():
            y[rng.randint(n), c] = False
        if not y[:, c].any():                             # (a multi-label row: the class is there, argmax decodes the row to an earlier one if any)
            y[rng.randint(n), c] = True
    if absent is not None and n > 2:
        y[:, absent] = False
        first = np.nonzero(y[:, :absent].any(axis=1))[0] if absent > 0 else []
        y[first[0] if len(first) else 0, absent] = True   # one positive, in a row that decodes to an earlier class (or: absent == 0 is present)
    return y


def scores_for(rng, family, y):
    """fp32 [n] in (0, 1) for the bool labels ``y`` [n] (both values occur)."""
    n = len(y)
    if family == "continuous":
        s = rng.rand(n) * 0.6 + 0.3 * y
    elif family.startswith("levels"):
        L = int(family[6:])
        s = (np.floor(rng.rand(n) * L) + 0.5) / L
    elif family == "equal":
        s = np.full(n, 0.375)
    elif family == "separable":
        s = np.where(y, 0.6 + 0.3 * rng.rand(n), 0.1 + 0.3 * rng.rand(n))
    elif family == "anti":
        s = np.where(y, 0.1 + 0.3 * rng.rand(n), 0.6 + 0.3 * rng.rand(n))
    else:
        raise ValueError(family)
    return np.clip(s, 1e-6, 1 - 1e-6).astype(np.float32)


def collinear_case(n, run=1):
    """(scores fp32 [n], labels bool [n]): strictly descending scores, labels in runs of ``run`` from a positive one (run = 1, n even: P = N)."""
    order = np.arange(n)
    s = (0.9 - 0.8 * order / n).astype(np.float32)
    assert (np.diff(s) < 0).all()
    return s, (order // run) % 2 == 0


def build(n, C, family, seed, absent=None):
    """(scores fp32 [n, C], labels fp32 [n, C]) of one case; 'collinear' / 'runs' round n down to an even number and give every column the staircase (shifted)."""
    rng = np.random.RandomState(seed)
    if family in ("collinear", "runs"):
        n -= n % 2
        cols, labs = [], []
        for c in range(C):
            s, y = collinear_case(n, 1 if family == "collinear" else 3)
            cols.append(np.roll(s, 2 * c)); labs.append(np.roll(y, 2 * c))       # (an even shift keeps score and label together)
        return np.stack(cols, 1).astype(np.float32), np.stack(labs, 1).astype(np.float32)
    y = labels_for(rng, n, C, absent)
    s = np.stack([scores_for(rng, family, y[:, c]) for c in range(C)], 1)
    return s.astype(np.float32), y.astype(np.float32)


def case_list():
    """[(name, n, C, family, seed, absent)]: every n and C over the families, plus cases where a decoded class is absent from y_true and y_pred."""
    out, seed = [], 1000
    for n in NS:
        for C in CS:
            for family in FAMILIES:
                if family in ("collinear", "runs") and n < 4:
                    continue
                seed += 1
                out.append((f"{family}-n{n}-C{C}", n, C, family, seed, None))
    for n, C, absent in ((7, 3, 2), (64, 5, 3), (65, 5, 4), (257, 3, 1)):
        seed += 1
        out.append((f"absent{absent}-n{n}-C{C}", n, C, "anti", seed, absent))        # 'anti': every prediction is 0, so no row is PREDICTED as it either
    return out


def logits_for(scores):
    """fp32 logits whose sigmoid is ``scores`` up to rounding (the tests read the stored scores back rather than assume the bits)."""
    s = scores.astype(np.float64)
    return np.log(s / (1.0 - s)).astype(np.float32)
