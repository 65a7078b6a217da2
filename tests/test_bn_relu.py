"""BatchNorm + ReLU over live rows and the live rows of a slot, without a GPU: ``ops.masked_batch_norm(relu=True)`` through its
tensor path against the numpy restatement of tests/bn_relu_cases.py (float64, 1e-12), ``relu=False`` unchanged, what float32 itself costs
on those cases (a quarter of the GPU tests' bounds at most, ReLU sides inside their cap), and ``graph.derive_live_rows`` on CPU slots against
a Python loop over ``row_seg`` / ``seg_counts``."""
import os
import re

import numpy as np
import pytest
import torch

import bn_relu_cases as B
import gin_slot_cases as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _rel(a, b):
    b = np.asarray(b, dtype=np.float64)
    return float(np.abs(np.asarray(a, dtype=np.float64) - b).max()) / max(float(np.abs(b).max()), 1.0)


def _op(case, affine, running, train, relu, **kw):
    """``ops.masked_batch_norm`` on float64 CPU tensors: dict of out, dx, dgamma, dbeta, running_mean, running_var, tracked."""
    from wsi_hgnn_amd import ops
    t = lambda a: torch.from_numpy(a).double()
    x = t(case["x"]).requires_grad_(True)
    gamma, beta = (t(case["gamma"]).requires_grad_(True), t(case["beta"]).requires_grad_(True)) if affine else (None, None)
    rm, rv = (t(case["rm"]), t(case["rv"])) if running else (None, None)
    tracked = torch.zeros((), dtype=torch.int64)
    out = ops.masked_batch_norm(x, torch.from_numpy(case["live"]), torch.tensor([case["n"]]), gamma, beta, rm, rv, train, B.MOMENTUM, B.EPS,
                                num_batches_tracked=tracked, **({"relu": True} if relu else {}), **kw)
    (out * t(case["g"])).sum().backward()
    return dict(out=out.detach().numpy(), dx=x.grad.numpy(), dgamma=gamma.grad.numpy() if affine else None,
                dbeta=beta.grad.numpy() if affine else None, running_mean=rm.numpy() if running else None,
                running_var=rv.numpy() if running else None, tracked=int(tracked))


@pytest.mark.parametrize("rows", B.ROWS)
def test_tensor_path_equals_the_restatement(rows):
    seen = 0
    for C in B.COLS:
        for pattern in B.live_patterns(rows):
            case = B.make(rows, C, pattern)
            for affine, running, train in B.VARIANTS:
                ref = B.restate(case, affine, running, train)
                got = _op(case, affine, running, train, relu=True)
                what = (rows, C, pattern, affine, running, train)
                for k in ("out", "dx", "dgamma", "dbeta", "running_mean", "running_var"):
                    if got[k] is not None:
                        assert _rel(got[k], ref[k]) <= 1e-12, (what, k)
                assert got["tracked"] == (1 if train else 0)
                dead = case["live"] == 0
                assert not got["out"][dead].any() and not got["dx"][dead].any(), what
                assert (got["out"] >= 0).all()
                seen += 1
    assert seen >= 5 * 6


def test_special_columns_sit_where_the_cases_say():
    case = B.make(300, 64, "interleaved")
    ref = B.restate(case, True, True, True)
    live = case["live"] != 0
    assert not ref["y"][:, 0].any() and not ref["side"][:, 0].any()                    # y == 0 exactly: the zero side
    assert (ref["y"][live, 1] < 0).all() and (ref["y"][live, 2] > 0).all()
    assert np.unique(ref["y"][live, 3]).size == 1                                      # gamma = 0: y = beta
    assert (case["gamma"] < 0).any() and (case["gamma"] > 0).any()
    assert set(B.live_patterns(300)) == {"all", "dead suffix", "interleaved", "two live rows", "a dead chunk"}
    assert B.live_patterns(300)["two live rows"].sum() == 2 and not B.live_patterns(300)["a dead chunk"][128:256].any()
    assert all(p.sum() >= 2 for r in B.ROWS for p in B.live_patterns(r).values())


def test_without_relu_nothing_changes():
    from wsi_hgnn_amd import ops
    case = B.make(129, 67, "interleaved")
    for affine, running, train in B.VARIANTS:
        a = _op(case, affine, running, train, relu=False)
        b = _op(case, affine, running, train, relu=False, kernels=False)
        t = lambda v: torch.from_numpy(v).double()
        want = ops.masked_batch_norm_tensor(t(case["x"]), torch.from_numpy(case["live"]), torch.tensor([case["n"]]),
                                            t(case["gamma"]) if affine else None, t(case["beta"]) if affine else None,
                                            t(case["rm"]) if running else None, t(case["rv"]) if running else None, train, B.MOMENTUM, B.EPS)
        assert np.array_equal(a["out"], want.numpy()) and np.array_equal(a["out"], b["out"]) and np.array_equal(a["dx"], b["dx"])
        assert (a["out"] < 0).any()
        r = _op(case, affine, running, train, relu=True)
        assert np.array_equal(r["out"], np.maximum(a["out"], 0))
    assert ops.fused_bn_relu() is True
    ops.set_fused_bn_relu(False)
    assert ops.fused_bn_relu() is False
    ops.set_fused_bn_relu(True)
    with pytest.raises(RuntimeError, match="GPU only"):
        _op(case, True, True, True, relu=True, kernels=True)


def test_float32_costs_a_quarter_of_the_bounds_at_most():
    """The restatement in float32 against itself in float64, each deciding its own ReLU sides' gradient under float32's sides: every block
    within a quarter of TOL * its largest float64 entry, the sides inside their cap - what the GPU test asserts first, over every case."""
    worst, flipped, n = 0.0, 0, 0
    for rows, C, pattern, affine, running, train in B.all_cases():
        case = B.make(rows, C, pattern)
        what = f"{rows}x{C} {pattern} affine={affine} running={running} train={train}"
        r32 = B.restate(case, affine, running, train, dtype=np.float32)
        r64 = B.restate(case, affine, running, train, sides=r32["side"])
        flipped += B.check_sides(r32["side"], r64, what)
        worst = max(worst, B.worst_ratio(r32, r64, 0.25, what))
        n += 1
    print(f"{n} cases: float32 reaches {worst:.3f} of the bound at most, {flipped} ReLU sides differ from float64's")
    assert n == len(list(B.all_cases())) >= 400


# ---------------------------------------------------------------------------------------------------- the live rows of a slot
def _loop(slot):
    lay = slot.layout
    row_seg, counts = slot.bufs["row_seg"].tolist(), slot.bufs["seg_counts"].reshape(-1).tolist()
    live = [1.0 if s < lay.b_cap else 0.0 for s in row_seg]
    total = 0.0
    for b in range(lay.b_cap):
        total += counts[b]
    return live, total


@pytest.mark.parametrize("idxs", [[0], [0, 5], [1, 3], [6], [4, 2]])
def test_derive_live_rows_against_a_loop(idxs):
    from wsi_hgnn_amd.data import BatchSlot
    from wsi_hgnn_amd.models.GIN import live_rows
    slot = BatchSlot(S.loader("cpu"), S.WIDE)
    assert slot.live_rows is not None and slot.graph.__dict__["_gin_live"] is slot.live_rows
    slot.load([1, 3]).load(idxs)                           # (over a larger batch: nothing of it may stay)
    live, total = _loop(slot)
    n = sum(S.SIZES[i] for i in idxs)
    assert slot.live_rows[0].tolist() == live and slot.live_rows[1].tolist() == [total] == [float(n)]
    assert live == [1.0] * n + [0.0] * (slot.layout.N - n)
    if idxs == [0]:
        assert slot.layout.N - n > 2 * n and len(idxs) < slot.layout.b_cap             # the filler holds most rows; fewer slides than b_cap
    got = live_rows(slot.graph, slot.layout.N, torch.device("cpu"))
    assert got[0] is slot.live_rows[0] and got[1] is slot.live_rows[1]                 # what models.GIN reads


def test_derive_live_rows_refusals():
    from wsi_hgnn_amd import graph as G
    from wsi_hgnn_amd.data import BatchSlot
    import slot_cases as C
    slot = BatchSlot(S.loader("cpu"), S.WIDE).load([0])
    n = slot.layout.N
    with pytest.raises(ValueError, match="contiguous float32"):
        G.derive_live_rows(slot.layout, slot.bufs, torch.zeros(n - 1), torch.zeros(1))
    with pytest.raises(ValueError, match="contiguous float32"):
        G.derive_live_rows(slot.layout, slot.bufs, torch.zeros(n), torch.zeros(1, dtype=torch.float64))
    het = BatchSlot(C.loader("cpu"), C.BIG)
    assert het.live_rows is None and "_gin_live" not in het.graph.__dict__
    with pytest.raises(ValueError, match="homogeneous"):
        G.derive_live_rows(het.layout, het.bufs, torch.zeros(het.layout.N), torch.zeros(1))


def test_new_code_reads_no_environment_variable():
    for rel in ("wsi-hgnn_amd/csrc/masked_bn.hip", "wsi-hgnn_amd/csrc/segment_table.hip", "tools/gin_slot_bench.py"):
        text = open(os.path.join(ROOT, rel)).read()
        assert not re.search(r"os\.environ|\bgetenv\b", text), rel
