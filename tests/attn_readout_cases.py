"""Cases of the attention readout (ops.attention_readout, wsi_attn_readout_fwd / _bwd) and its restatement in numpy, shared by
tests/test_attn_readout.py (CPU) and tests/test_attn_readout_kernels_gpu.py.

One segment layout for every case, chunk = 128 rows: an empty segment first, one row, 127 rows, two empty segments in a row, 128 rows (a chunk
edge that lands on a segment edge), 129 rows, 300 rows (three chunks), an empty segment last.

Gates (gate = <x, w> + b):
  ordinary  x, w standard normal, w / sqrt(D)
  peaked    the same w x 30: one or two rows carry a segment.  In every segment of two rows or more a second row is moved along w until its
            gate lies 0.3 under the largest: with ONE row carrying a segment the gate's weight gradient - a covariance under p - is what
            float32 rounding of (<g_out, x> - delta) leaves (measured: the float32 restatement alone then misses the bound on g_w fourfold at
            D = 4), and an error relative to the block's largest entry says nothing.  Not at D = 1: there the gate IS the row, rows with
            competing gates are equal rows, and g_w = g_out Var_p(x) stays such a residue whatever the rows (float32 floor: 0.47 of the bound)
  offset    gates near -1e4.  w picks column 0, which holds multiples of 2^-8 within +-4, and b = -1e4: the float32 gate is then EXACT (an
            ordinary dot product offset by -1e4 would be rounded to an ulp of 1e-3 before any kernel sees it - an error of the inputs, not of
            the code under test), and the softmax is the one of the unshifted column
  ties      w = 0: all gates of a segment are equal, out = the mean of its rows
  twomax    ordinary, then in every segment of two rows or more the row of the largest gate is copied over another row: two equal maxima
g_out: standard normal, the row of segment ZERO_SEG (129 rows) exactly zero."""
import numpy as np
import torch

LENS = [0, 1, 127, 0, 0, 128, 129, 300, 0]
OFF = [0]
for _n in LENS:
    OFF.append(OFF[-1] + _n)
ROWS = OFF[-1]
S = len(LENS)
ZERO_SEG = 6
CHUNK = 128
DS = [1, 4, 67, 256, 1028]
GATES = ["ordinary", "peaked", "offset", "ties", "twomax"]
# (D, gate kind, row stride of x): contiguous rows for every (D, kind); a stride of D + 1 - rows that are not 16-byte aligned - once per width
# that could take 16-byte loads.  D = 67 is on the scalar path by itself.
CASES = [(D, k, D) for D in DS for k in GATES if (D, k) != (1, "peaked")] + [(D, "ordinary", D + 1) for D in (4, 256, 1028)]
TOL = 1e-4                      # x the largest float64 entry of the block compared


def case_id(case):
    D, kind, ld = case
    return f"D{D}-{kind}" + ("" if ld == D else f"-ld{ld}")


def inputs(case):
    """(x [ROWS, D] float32 with row stride ld, w [D], b [1], g_out [S, D]) as torch CPU tensors."""
    D, kind, ld = case
    g = torch.Generator().manual_seed(97 * D + 7 * GATES.index(kind) + ld)
    buf = torch.randn(ROWS, ld, generator=g)
    x = buf[:, :D]
    w = torch.randn(D, generator=g) / D ** 0.5
    b = torch.randn(1, generator=g)
    g_out = torch.randn(S, D, generator=g)
    g_out[ZERO_SEG] = 0.0
    if kind == "peaked":
        w = w * 30.0
        gate = x @ w
        for a, e in zip(OFF[:-1], OFF[1:]):
            if e - a >= 2:
                top = a + int(gate[a:e].argmax())
                other = a if top != a else a + 1
                x[other] += (gate[top] - 0.3 - gate[other]) / (w @ w) * w
    elif kind == "offset":
        x[:, 0] = (x[:, 0].clamp(-4, 4) * 256).round() / 256
        w = torch.zeros(D); w[0] = 1.0
        b = torch.tensor([-1.0e4])
    elif kind == "ties":
        w = torch.zeros(D)
    elif kind == "twomax":
        gate = x @ w
        for a, e in zip(OFF[:-1], OFF[1:]):
            if e - a >= 2:
                top = a + int(gate[a:e].argmax())
                x[a if top != a else a + 1] = x[top]
    return x, w, b, g_out


def restate(x, w, b, g_out, dtype=np.float64):
    """The readout and its gradients, segment by segment, in ``dtype``: dict of out, gate, stats, g_x, g_wb.  g_wb [D + 1] = g_w | g_b is ONE
    block, as the kernel writes it: a softmax ignores a shift of its gates, so g_b is 0 up to rounding and has no scale of its own."""
    x, w, g_out = (np.asarray(t, dtype=dtype) for t in (x, w, g_out))
    b = dtype(np.asarray(b).reshape(-1)[0])
    D = x.shape[1]
    gate = (x @ w + b).astype(dtype)
    out, stats = np.zeros((S, D), dtype), np.zeros((S, 2), dtype)
    g_x, g_w, g_b = np.zeros_like(x), np.zeros(D, dtype), dtype(0)
    for s, (a, e) in enumerate(zip(OFF[:-1], OFF[1:])):
        if e == a:
            continue
        m = gate[a:e].max()
        ex = np.exp(gate[a:e] - m)
        L = ex.sum(dtype=dtype)
        p = ex / L
        out[s] = p @ x[a:e]
        stats[s] = (m, np.log(L))
        delta = g_out[s] @ out[s]
        gg = p * (x[a:e] @ g_out[s] - delta)
        g_x[a:e] = p[:, None] * g_out[s][None, :] + gg[:, None] * w[None, :]
        g_w += gg @ x[a:e]
        g_b += gg.sum(dtype=dtype)
    return {"out": out, "gate": gate, "stats": stats, "g_x": g_x, "g_wb": np.concatenate([g_w, np.asarray([g_b], dtype)])}


def error_ratio(got, ref):
    """max |got - ref| / (TOL x max |ref|): <= 1 passes.  A reference block of zeros allows nothing but zeros."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    if ref.size == 0:
        return 0.0
    err, top = float(np.abs(got - ref).max()), float(np.abs(ref).max())
    return err / (TOL * top) if top > 0 else (0.0 if err == 0 else float("inf"))
