"""What the BatchNorm + ReLU tests share (no test functions): the shapes, live patterns and parameter sets of DESIGN 3.33's test plan, and a
restatement of ``ops.masked_batch_norm(relu=True)`` - forward, running statistics and every gradient - in numpy, in float64 or (to measure
what fp32 itself costs) in float32.

Inputs.  Column j of x is ``offset + scale * randn`` with (scale, offset) = ((0.01, 0.002), (1, -0.7), (0.01, -0.003), (3, -2))[j % 4]: in the
columns of scale 0.01 the variance (1e-4) is of the order of eps (1e-5), so that dx is not a pure cancellation there - at two live rows and
scale 1, dx = gamma rstd (g1 - g2) / 2 * eps / (var + eps) is 1e-5 of its terms, nothing fp32 can hold to 1e-4 of ITS size.  Dead rows
of x hold values around 1000: whatever leaks into a statistic shows.  With C >= 4 the first four columns are special: gamma = beta = 0 (y is
exactly 0: the zero side), beta = -50 (every y < 0), beta = +50 (every y > 0), gamma = 0 with a random beta; the other gammas are normal
draws (both signs).  The incoming gradient g is 0.5 + randn: with C = 1 a block such as dbeta is ONE sum, and a sum of zero-mean terms
that happens to cancel has no size of its own to hold an error against."""
import numpy as np

ROWS = (2, 127, 128, 129, 300)                # one chunk edge (128 rows per workgroup), three chunks
COLS = (1, 4, 64, 67, 132)                    # 67: scalar path; 132: 16-byte path unless the layout breaks it
# "stride": row stride C + 1;  "offset": every tensor starts 4 bytes into its buffer - both send C = 132 down the scalar path
SHAPES = [(r, c, "plain") for r in ROWS for c in COLS] + [(r, 132, lay) for r in ROWS for lay in ("stride", "offset")]
SHAPE_IDS = [f"{r}x{c}-{lay}" for r, c, lay in SHAPES]
# (affine, running statistics, training); eval mode needs running statistics
VARIANTS = [(a, r, t) for a in (True, False) for r in (True, False) for t in (True, False) if t or r]
MOMENTUM, EPS = 0.1, 1e-5
TOL = 1e-4                                    # of the block's largest float64 entry
SIDE_BAND, SIDE_SHARE = 1e-5, 0.01            # a ReLU side may differ from float64's within this band of the column's largest |y|, on this share


def live_patterns(rows):
    """name -> float32 [rows] of 0 / 1, each with at least two live rows."""
    out = {"all": np.ones(rows, dtype=np.float32)}
    if rows > 2:
        k = max(2, rows // 3)
        out["dead suffix"] = (np.arange(rows) < k).astype(np.float32)                  # the slot's shape: the filler's rows last
        out["interleaved"] = (np.arange(rows) % 3 != 1).astype(np.float32)
        two = np.zeros(rows, dtype=np.float32)
        two[[rows // 2, rows - 1]] = 1
        out["two live rows"] = two
    if rows > 256:
        chunk = np.ones(rows, dtype=np.float32)
        chunk[128:256] = 0
        out["a dead chunk"] = chunk                                                    # one whole workgroup's rows
    return out


def make(rows, C, pattern, seed=0):
    """dict of float32 arrays: x, g [rows, C], live [rows], gamma, beta, rm, rv [C]; n = the number of live rows."""
    rng = np.random.default_rng([rows, C, sorted(live_patterns(rows)).index(pattern), seed])
    live = live_patterns(rows)[pattern]
    scale = np.array([0.01, 1.0, 0.01, 3.0])[np.arange(C) % 4]
    offset = np.array([0.002, -0.7, -0.003, -2.0])[np.arange(C) % 4]
    x = offset + scale * rng.standard_normal((rows, C))
    x = np.where(live[:, None] != 0, x, 1000.0 + rng.standard_normal((rows, C)))
    gamma, beta = rng.standard_normal(C), 0.5 * rng.standard_normal(C)
    if C >= 4:
        gamma[:4] = (0.0, 1.0, 1.0, 0.0)
        beta[:3] = (0.0, -50.0, 50.0)
    f = lambda a: np.ascontiguousarray(a, dtype=np.float32)
    return dict(x=f(x), g=f(0.5 + rng.standard_normal((rows, C))), live=live, n=float(live.sum()), gamma=f(gamma), beta=f(beta),
                rm=f(offset + 0.1 * rng.standard_normal(C)), rv=f(scale ** 2 * (0.5 + rng.random(C))))


def restate(case, affine, running, train, g=True, sides=None, dtype=np.float64):
    """``relu(masked_batch_norm(x))`` and its gradients by the definition, in ``dtype``.  ``sides`` [rows, C] 0 / 1: replay these ReLU sides
    instead of deciding them here.  Returns y (before the ReLU), out, side, mean, rstd, running_mean, running_var (None when not tracked;
    unchanged in eval mode) and, with ``g``, dx, dgamma, dbeta."""
    f = dtype
    x, m = case["x"].astype(f), case["live"].astype(f)[:, None]
    C = x.shape[1]
    ga = case["gamma"].astype(f) if affine else np.ones(C, dtype=f)
    be = case["beta"].astype(f) if affine else np.zeros(C, dtype=f)
    rm, rv = (case["rm"].astype(f), case["rv"].astype(f)) if running else (None, None)
    n, mom, eps = f(case["n"]), f(MOMENTUM), f(EPS)
    if train:
        mean = (x * m).sum(0) / n
        d = (x - mean) * m
        var = (d * d).sum(0) / n
        if running:
            rm = (f(1) - mom) * rm + mom * mean
            rv = (f(1) - mom) * rv + mom * (var * (n / (n - f(1))))
    else:
        mean, var = rm, rv
    rstd = f(1) / np.sqrt(var + eps)
    xhat = (x - mean) * rstd
    y = (xhat * ga + be) * m
    side = ((y > 0) if sides is None else (np.asarray(sides) != 0)).astype(f) * m
    res = dict(y=y, out=y * side, side=side, mean=mean, rstd=rstd, running_mean=rm, running_var=rv)
    if g:
        ge = case["g"].astype(f) * side
        res["dbeta"], res["dgamma"] = ge.sum(0), (ge * xhat).sum(0)
        res["dx"] = ga * rstd * (ge - res["dbeta"] / n - xhat * (res["dgamma"] / n)) * m if train else ga * rstd * ge
    assert all(v is None or v.dtype == f for v in res.values())
    return res


KEYS = ("out", "mean", "rstd", "running_mean", "running_var", "dx", "dgamma", "dbeta")


def bounds(ref64):
    """key -> TOL * the largest float64 entry of that block (None where the block does not exist)."""
    return {k: None if ref64.get(k) is None else TOL * float(np.abs(ref64[k]).max()) for k in KEYS}


def worst_ratio(got, ref64, limit=1.0, what=""):
    """max over the blocks of |got - ref64| / bound; asserts every block is finite and stays within ``limit`` of its bound."""
    worst = 0.0
    for k, b in bounds(ref64).items():
        if b is None:
            continue
        a = np.asarray(got[k], dtype=np.float64)
        assert np.isfinite(a).all(), (what, k)
        err = float(np.abs(a - ref64[k]).max())
        if b == 0.0:
            assert err == 0.0, (what, k, err)
            continue
        assert err <= limit * b, (what, k, err, b)
        worst = max(worst, err / b)
    return worst


def check_sides(side, ref64, what=""):
    """The ReLU sides ``side`` against float64's own: they may differ only where |y64| <= SIDE_BAND * the column's largest |y64|, and on at
    most SIDE_SHARE of the entries.  Returns the number that differ."""
    y = ref64["y"]
    bad = (np.asarray(side) != 0) != (y > 0)                   # (dead rows: y is 0 there, both sides 0)
    if bad.any():
        band = SIDE_BAND * np.abs(y).max(0, keepdims=True)
        assert (np.abs(y)[bad] <= np.broadcast_to(band, y.shape)[bad]).all(), what
        assert bad.sum() <= SIDE_SHARE * y.size, (what, int(bad.sum()))
    return int(bad.sum())


def all_cases():
    """(rows, C, pattern, affine, running, train) of every case the shapes, patterns and variants give (plain layout: once per (rows, C))."""
    for rows in ROWS:
        for C in COLS:
            for pattern in live_patterns(rows):
                for affine, running, train in VARIANTS:
                    yield rows, C, pattern, affine, running, train
