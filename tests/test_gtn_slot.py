"""gtn.GraphSlot, gtn.SlideSet and ops.masked_batch_norm without a GPU: the tables a ``load`` writes on the CPU against a host-loop restatement
and against ``ops.EdgeCSR`` of the unpadded batch, the capacity edges of ``fits`` / ``load``, ``gtn.Classifier(kernels=False)`` on a slot
against the float64 restatement on the UNPADDED slides (tests/gtn_cases.py), and the tensor form of the masked BatchNorm against
``torch.nn.functional.batch_norm`` on the live rows alone.  Tolerance (tests/test_gtn_gpu.py's norm): error <= 1e-4 x the largest float64 entry
of each tensor; the tables are integers and copied floats and must be equal bit for bit."""
import pytest
import torch

import gtn_slot_cases as S
from mil_cases import Ratios
from wsi_hgnn_amd import gtn, ops

R = Ratios(1e-4)


@pytest.fixture(scope="module", autouse=True)
def _report_ratios():
    yield
    R.report()


def _table_slot(entry_cap=None):
    slides = S.table_slides()
    ss = gtn.SlideSet(slides, device="cpu")
    cap = sum(ss.entries) + 37 if entry_cap is None else entry_cap
    return slides, ss, gtn.GraphSlot(slides[0][0].shape[1], S.TABLE_CELLS, S.TABLE_CELL_ROWS, cap, device="cpu")


def test_load_writes_what_a_host_loop_writes():
    slides, ss, slot = _table_slot()
    slot.load(ss, [0, 1], [2, 0])
    S.assert_tables_equal(S.slot_tables(slot), S.host_tables(slides, [2, 0], S.TABLE_CELLS, S.TABLE_CELL_ROWS), "tables")
    assert slot.num_real == 2 and slot.num_graphs == 3 and slot.rp.ranges == [(0, 140), (140, 280), (280, 420)]
    # the slides the other way round, into the same slot: nothing of the first load is left in a referenced entry
    slot.load(ss, [1, 0], [1, 1])
    S.assert_tables_equal(S.slot_tables(slot), S.host_tables([slides[1], slides[0]], [1, 1], S.TABLE_CELLS, S.TABLE_CELL_ROWS), "second load")


def test_live_part_is_the_edge_csr_of_the_unpadded_batch():
    slides, ss, slot = _table_slot()
    slot.load(ss, [0, 1], [0, 1])
    n0, n1 = S.TABLE_SIZES
    unit = S.with_unit_weights(slides)
    row = torch.cat([unit[0][1], unit[1][1] + n0])
    col = torch.cat([unit[0][2], unit[1][2] + n0])
    want = ops.EdgeCSR(row, col, n0 + n1).with_weights(torch.cat([unit[0][3], unit[1][3]]))
    live = slot.live.nonzero().flatten()
    assert live.tolist() == list(range(n0)) + list(range(S.TABLE_CELL_ROWS, S.TABLE_CELL_ROWS + n1))
    E, ec = slot.num_entries, slot.ec
    assert E == want.num_edges
    # entry offsets are those of the packed batch (the slides' entries lie one after the other); row numbers lose the cell padding
    unpad = lambda r: torch.where(r >= S.TABLE_CELL_ROWS, r - (S.TABLE_CELL_ROWS - n0), r)
    assert torch.equal(ec.rowptr[live], want.rowptr[:-1]) and torch.equal(ec.colptr[live], want.colptr[:-1])
    assert int(ec.rowptr[-1]) == E == int(ec.colptr[-1])
    assert torch.equal(unpad(ec.src[:E]), want.src) and torch.equal(unpad(ec.csc_dst[:E]), want.csc_dst)
    assert torch.equal(ec.edge_w[:E], want.edge_w) and torch.equal(ec.edge_w_csc[:E], want.edge_w_csc)
    # every dead row has an empty range in both directions
    dead = (slot.live == 0).nonzero().flatten()
    assert torch.equal(ec.rowptr[dead], ec.rowptr[dead + 1]) and torch.equal(ec.colptr[dead], ec.colptr[dead + 1])


def test_capacities():
    slides, ss, _ = _table_slot()
    e = ss.entries
    slot = gtn.GraphSlot(12, 2, 140, e[0] + e[1], device="cpu")
    assert slot.fits([129, 140], e) and slot.load(ss, [0, 1], [0, 1]).num_real == 2       # a full cell and exactly entry_cap entries
    assert not slot.fits([129, 140, 5], e + [0])                                           # too many slides
    with pytest.raises(ValueError, match="does not fit"):
        slot.load(ss, [0, 1, 0], [0, 1, 0])
    short = gtn.GraphSlot(12, 2, 139, e[0] + e[1], device="cpu")                           # a slide longer than a cell
    assert short.fits([129], e[:1]) and not short.fits([129, 140], e)
    with pytest.raises(ValueError, match="does not fit"):
        short.load(ss, [0, 1], [0, 1])
    tight = gtn.GraphSlot(12, 2, 140, e[0] + e[1] - 1, device="cpu")                       # too many entries
    assert tight.fits([129], e[:1]) and not tight.fits([129, 140], e)
    with pytest.raises(ValueError, match="does not fit"):
        tight.load(ss, [0, 1], [0, 1])
    one = gtn.SlideSet([(torch.randn(1, 12), torch.tensor([0]), torch.tensor([0]), None), (torch.randn(1, 12), torch.tensor([0]), torch.tensor([0]), None)],
                       device="cpu")
    assert not slot.fits([1], [1]) and slot.fits([1, 1], [1, 1])                           # fewer than 2 live rows in all
    with pytest.raises(ValueError, match="does not fit"):
        slot.load(one, [0], [1])
    assert float(slot.load(one, [0, 1], [1, 0]).live_rows) == 2.0
    assert not slot.fits([], []) and not slot.fits([0, 5], [0, 0])
    with pytest.raises(ValueError, match="labels"):
        slot.load(ss, [0, 1], [0])
    with pytest.raises(ValueError, match="feats"):
        gtn.GraphSlot(13, 2, 140, 10, device="cpu").load(ss, [0], [0])


@pytest.mark.parametrize("train", [True, False])
def test_classifier_on_a_slot_against_float64_on_the_unpadded_slides(train):
    cfg = S.SMALL
    slides, labels, base = S.model_case((40, 129), (True, False), seed=121)
    ref, sd = S.reference(slides, labels, base, train)
    ss = gtn.SlideSet(slides, device="cpu")
    slot = gtn.GraphSlot(cfg["in_feats"], 3, 140, sum(ss.entries) + 11, device="cpu").load(ss, [0, 1], labels)      # one cell unused
    m = S.build_model(gtn, cfg, base, "cpu", kernels=False)
    loss, logits = S.run_on_slot(m, slot, train)
    assert torch.isfinite(loss) and torch.isfinite(logits).all() and logits.shape == (3, cfg["n_class"])
    S.check_against_reference(R, m, loss, logits, ref, sd, base, 2, train, f"cpu slot {'train' if train else 'eval'}")


def test_a_graph_batch_still_gives_what_it_gave():
    """The slot branches leave the packed path alone: a ``GraphBatch`` of the same slides against the same float64 reference."""
    cfg = S.SMALL
    slides, labels, base = S.model_case((40, 129), (True, True), seed=131)
    ref, sd = S.reference(slides, labels, base, True)
    ss = gtn.SlideSet(slides, device="cpu")
    m = S.build_model(gtn, cfg, base, "cpu", kernels=False).train()
    _, _, loss, probs = m(ss.batch([0, 1]), torch.tensor(labels))
    R.check(loss.reshape(1), ref["loss"].reshape(1), "loss", "cpu packed")
    R.check(probs, ref["probs"], "probs", "cpu packed")


@pytest.mark.parametrize("train", [True, False])
def test_masked_batch_norm_tensor_form(train):
    C_, cells, rows = 7, 3, 9
    gen = torch.Generator().manual_seed(5)
    live = S.live_mask(cells, rows, (9, 0, 4))
    y = torch.randn(cells * rows, C_, generator=gen, dtype=torch.float64).requires_grad_(True)
    gamma = (1 + 0.1 * torch.randn(C_, generator=gen, dtype=torch.float64)).requires_grad_(True)
    beta = (0.1 * torch.randn(C_, generator=gen, dtype=torch.float64)).requires_grad_(True)
    rm, rv = 0.05 * torch.randn(C_, generator=gen, dtype=torch.float64), 0.5 + torch.rand(C_, generator=gen, dtype=torch.float64)
    g_out = torch.randn(cells * rows, C_, generator=gen, dtype=torch.float64)
    ref = S.masked_bn_reference(y, live, gamma, beta, rm, rv, train, g_out)
    tracked = torch.tensor(0)
    rm1, rv1 = rm.clone(), rv.clone()
    out = ops.masked_batch_norm(y, live, torch.tensor([13.0]), gamma, beta, rm1, rv1, train, 0.1, 1e-5, num_batches_tracked=tracked)
    (out * g_out).sum().backward()
    case = "tensor form " + ("train" if train else "eval")
    R.check(out, ref["out"], "bn out", case)
    R.check(y.grad, ref["g_y"], "bn g_y", case)
    R.check(gamma.grad, ref["g_gamma"], "bn g_gamma", case)
    R.check(beta.grad, ref["g_beta"], "bn g_beta", case)
    R.check(rm1, ref["running_mean"], "bn running_mean", case)
    R.check(rv1, ref["running_var"], "bn running_var", case)
    dead = live == 0
    assert bool((out[dead] == 0).all()) and bool((y.grad[dead] == 0).all())
    assert int(tracked) == (1 if train else 0)
    if not train:
        assert torch.equal(rm1, rm) and torch.equal(rv1, rv)


def test_masked_batch_norm_refusals():
    y, live, n = torch.randn(4, 3), torch.ones(4), torch.tensor([4.0])
    with pytest.raises(ValueError, match="momentum"):
        ops.masked_batch_norm(y, live, n, None, None, torch.zeros(3), torch.ones(3), True, None, 1e-5)
    with pytest.raises(ValueError, match="eval mode needs"):
        ops.masked_batch_norm(y, live, n, None, None, None, None, False, 0.1, 1e-5)
    with pytest.raises(ValueError, match="live"):
        ops.masked_batch_norm(y, torch.ones(5), n, None, None, None, None, True, 0.1, 1e-5)
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.masked_batch_norm(y, live, n, None, None, None, None, True, 0.1, 1e-5, kernels=True)


def test_c_abi_argument_errors_without_a_gpu():
    from wsi_hgnn_amd import _native as N
    lib = N.load()
    P = 1 << 20                                                  # (a pointer that is never dereferenced: every call fails its checks first)
    fill = lambda slides=2, cells=3, rows=140, feats=8, cap=100, total=50, desc=P, x=P: lib.wsi_graph_slot_fill(
        desc, slides, cells, rows, feats, cap, total, 0.5, 2.0, x, P, P, P, P, P, P, P, P, P, P, None)
    assert fill(slides=4) == N.WSI_EINVAL and fill(total=101) == N.WSI_EINVAL and fill(feats=0) == N.WSI_EINVAL and fill(rows=0) == N.WSI_EINVAL
    assert fill(desc=None) == N.WSI_EINVAL and fill(x=None) == N.WSI_EINVAL and fill(cells=1 << 20, rows=1 << 12) == N.WSI_EINVAL
    assert lib.wsi_masked_bn_chunks(0) == 0 and lib.wsi_masked_bn_chunks(128) == 1 and lib.wsi_masked_bn_chunks(129) == 2
    fwd = lambda rows=10, C_=4, ldx=4, x=P, part=P, train=1: lib.wsi_masked_bn_fwd(x, ldx, rows, C_, P, P, None, None, None, None, train, 0.1, 1e-5,
                                                                                   part, P, P, C_, None)
    assert fwd(C_=0) == N.WSI_EINVAL and fwd(ldx=3) == N.WSI_EINVAL and fwd(x=None) == N.WSI_EINVAL and fwd(part=None) == N.WSI_EINVAL
    assert fwd(train=0) == N.WSI_EINVAL and fwd(rows=0) == N.WSI_OK          # (eval needs the running statistics)
    bwd = lambda rows=10, C_=4, ldg=4, g=P, dg=P: lib.wsi_masked_bn_bwd(g, ldg, P, C_, rows, C_, P, P, None, P, 1, P, dg, P, P, C_, None)
    assert bwd(C_=0) == N.WSI_EINVAL and bwd(ldg=3) == N.WSI_EINVAL and bwd(g=None) == N.WSI_EINVAL and bwd(dg=None) == N.WSI_EINVAL
