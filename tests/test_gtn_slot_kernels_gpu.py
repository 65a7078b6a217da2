"""The graph-slot fill (wsi_graph_slot_fill) on the GPU against the tensor formulation on the CPU, bit for bit, and the masked BatchNorm
kernels (wsi_masked_bn_fwd / _bwd) against float64 ``F.batch_norm`` over the live rows alone: C in {1, 32, 64, 100} (one partial column tile,
the scalar and the 16-byte elementwise path), 127 / 128 / 129 / 293 rows per cell (the 128-row chunk from both sides, several chunks), dead
rows at the cell tails, a whole dead cell, the minimum of two live rows, train and eval, columns of mean 10 and spread 0.1 (which a
sum-of-squares variance cannot pass), and identical calls giving identical bits.  Tolerance: error <= 1e-4 x the largest float64 entry of
each tensor (tests/test_gtn_gpu.py)."""
import pytest
import torch

import gtn_slot_cases as S
from mil_cases import Ratios

pytestmark = pytest.mark.gpu

DEV = "cuda"
R = Ratios(1e-4)


@pytest.fixture(scope="module", autouse=True)
def _report_ratios():
    yield
    R.report()


# ------------------------------------------------------------------------------------------------ the fill
def test_fill_equals_the_cpu_tables_and_leaves_nothing_stale():
    from wsi_hgnn_amd import gtn
    slides = S.table_slides()
    cpu_set, gpu_set = gtn.SlideSet(slides, device="cpu"), gtn.SlideSet(slides, device=DEV)
    cap = 2 * sum(cpu_set.entries) + 37
    make = lambda dev: gtn.GraphSlot(slides[0][0].shape[1], S.TABLE_CELLS, S.TABLE_CELL_ROWS, cap, device=dev)
    slot = make(DEV)
    for idxs, labels in (([0, 1], [2, 0]), ([1], [1]), ([1, 0, 1], [0, 1, 2])):        # a full load, a smaller one into the same slot, every cell used
        slot.load(gpu_set, idxs, labels)
        want = S.slot_tables(make("cpu").load(cpu_set, idxs, labels))
        S.assert_tables_equal(S.slot_tables(slot), want, f"load {idxs}")
        S.assert_tables_equal(want, S.host_tables([slides[i] for i in idxs], labels, S.TABLE_CELLS, S.TABLE_CELL_ROWS), f"host loop {idxs}")


def test_fill_with_a_feature_width_off_the_16_byte_path():
    from wsi_hgnn_amd import gtn
    slides = S.shuffled_slides((5, 70), 7, 40, (False, True))
    cpu_set, gpu_set = gtn.SlideSet(slides, device="cpu"), gtn.SlideSet(slides, device=DEV)
    args = (7, 2, 70, sum(cpu_set.entries))
    got = gtn.GraphSlot(*args, device=DEV).load(gpu_set, [0, 1], [1, 0])
    S.assert_tables_equal(S.slot_tables(got), S.slot_tables(gtn.GraphSlot(*args, device="cpu").load(cpu_set, [0, 1], [1, 0])), "feats 7")


# ------------------------------------------------------------------------------------------------ masked BatchNorm
def _bn_case(C_, cell_rows, live_per_cell, seed, mean=0.0, spread=1.0):
    gen = torch.Generator().manual_seed(seed)
    rows = len(live_per_cell) * cell_rows
    return dict(live=S.live_mask(len(live_per_cell), cell_rows, live_per_cell), n=float(sum(live_per_cell)),
                y=mean + spread * torch.randn(rows, C_, generator=gen), gamma=1 + 0.1 * torch.randn(C_, generator=gen),
                beta=0.1 * torch.randn(C_, generator=gen), rm=0.05 * torch.randn(C_, generator=gen), rv=0.5 + torch.rand(C_, generator=gen),
                g_out=torch.randn(rows, C_, generator=gen))


def _run_kernels(case, train):
    from wsi_hgnn_amd import ops
    y = case["y"].to(DEV).requires_grad_(True)
    gamma, beta = case["gamma"].to(DEV).requires_grad_(True), case["beta"].to(DEV).requires_grad_(True)
    rm, rv, tracked = case["rm"].to(DEV), case["rv"].to(DEV), torch.zeros((), dtype=torch.int64, device=DEV)
    out = ops.masked_batch_norm(y, case["live"].to(DEV), torch.tensor([case["n"]], device=DEV), gamma, beta, rm, rv, train, 0.1, 1e-5,
                                num_batches_tracked=tracked)
    (out * case["g_out"].to(DEV)).sum().backward()
    return dict(out=out.detach(), g_y=y.grad, g_gamma=gamma.grad, g_beta=beta.grad, running_mean=rm, running_var=rv), int(tracked)


def _check_bn(case, train, name):
    got, tracked = _run_kernels(case, train)
    ref = S.masked_bn_reference(case["y"], case["live"], case["gamma"], case["beta"], case["rm"], case["rv"], train, case["g_out"])
    for k in ("out", "g_y", "g_gamma", "g_beta", "running_mean", "running_var"):
        R.check(got[k], ref[k], "bn " + k, name)
    dead = (case["live"] == 0).to(DEV)
    assert bool((got["out"][dead] == 0).all()) and bool((got["g_y"][dead] == 0).all())
    assert tracked == (1 if train else 0)
    if not train:
        assert torch.equal(got["running_mean"].cpu(), case["rm"]) and torch.equal(got["running_var"].cpu(), case["rv"])
    return got


@pytest.mark.parametrize("train", [True, False])
@pytest.mark.parametrize("cell_rows", [127, 128, 129, 293])
@pytest.mark.parametrize("C_", [1, 32, 64, 100])
def test_masked_batch_norm_against_float64(C_, cell_rows, train):
    # cell 0 with a dead tail, cell 1 all dead, cell 2 full
    case = _bn_case(C_, cell_rows, (cell_rows - 5, 0, cell_rows), seed=1000 + 7 * C_ + cell_rows)
    _check_bn(case, train, f"C={C_} rows={cell_rows} {'train' if train else 'eval'}")


@pytest.mark.parametrize("train", [True, False])
def test_masked_batch_norm_at_two_live_rows(train):
    _check_bn(_bn_case(64, 129, (1, 0, 1), seed=77), train, f"two live rows {'train' if train else 'eval'}")


def test_masked_batch_norm_with_a_large_mean():
    """Columns of mean 10 and spread 0.1: E[x^2] - mean^2 in fp32 loses the variance (100.01 - 100 with 6e-6 of rounding in each term); the
    centred form does not.  The float64 reference sees the same fp32 inputs, exactly."""
    _check_bn(_bn_case(64, 293, (280, 0, 293), seed=88, mean=10.0, spread=0.1), True, "mean 10 spread 0.1")


def test_identical_calls_give_identical_bits():
    case = _bn_case(100, 293, (200, 0, 293), seed=99)
    a, _ = _run_kernels(case, True)
    b, _ = _run_kernels(case, True)
    for k in a:
        assert torch.equal(a[k], b[k]), k
