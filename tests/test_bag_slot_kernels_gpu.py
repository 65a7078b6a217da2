"""The patch-dropout and slot-fill kernels (wsi_bag_dropout_select, wsi_bag_slot_fill) on the GPU against the tensor formulation on the CPU,
bit for bit, over the cases of tests/bag_slot_cases.py; and every bag kernel under a slot's padded plan (trailing empty chunks that no segment
owns) against the unpadded plan of the same segments, bit for bit, forward and backward."""
import array

import pytest
import torch

import bag_slot_cases as BC

pytestmark = pytest.mark.gpu

DEV = "cuda"


def _expected(bags_cpu, sizes, p, draws, key_bits):
    from wsi_hgnn_amd import mil
    return mil.dropout_patches_tensor(torch.cat([t.contiguous() for t in bags_cpu]), sizes, p, draws, key_bits)


@pytest.mark.parametrize("key_bits", [32, 3])
@pytest.mark.parametrize("p", BC.RATES)
@pytest.mark.parametrize("feats", BC.FEATS)
def test_dropout_kernels_through_ops(feats, p, key_bits):
    from wsi_hgnn_amd import mil, ops
    sizes = list(BC.KERNEL_SIZES)
    draws = BC.draws_for(sizes, key_bits)
    bags = BC.make_bags(sizes, feats, 11, DEV)
    assert any(not t.is_contiguous() for t in bags)                                    # one source is a strided view
    counts = [mil.patch_counts(n, p) for n in sizes]
    rows, sel = ops.bag_dropout_rows(bags, counts, draws, key_bits)
    want_rows, new_sizes, want_sel = _expected([t.cpu() for t in bags], sizes, p, draws, key_bits)
    assert rows.shape[0] == sum(new_sizes)
    assert torch.equal(sel.cpu(), want_sel)
    assert torch.equal(rows.cpu(), want_rows)
    rows2, sel2 = ops.bag_dropout_rows(bags, counts, draws, key_bits)                  # the same bits run after run
    assert torch.equal(sel2, sel) and torch.equal(rows2, rows)
    # a bag alone gives the rows it gives among the others
    b = sizes.index(300)
    off = sum(new_sizes[:b])
    alone, sel_alone = ops.bag_dropout_rows([bags[b]], [counts[b]], [draws[b]], key_bits)
    assert torch.equal(sel_alone, sel[off:off + new_sizes[b]]) and torch.equal(alone, rows[off:off + new_sizes[b]])


@pytest.mark.parametrize("p", [0.25, 0.5])
def test_dropout_patches_on_a_plan(p):
    from wsi_hgnn_amd import mil
    sizes = list(BC.KERNEL_SIZES)
    x = torch.randn(sum(sizes), 64, generator=torch.Generator().manual_seed(5)).to(DEV)
    plan = mil.bag_plan(sizes, DEV)
    rows, new_plan = mil.dropout_patches(x, plan, p, seed=12)
    want, want_plan = mil.dropout_patches(x.cpu(), sizes, p, seed=12, kernels=False)
    assert new_plan.ranges == want_plan.ranges and torch.equal(rows.cpu(), want)
    same, same_plan = mil.dropout_patches(x, plan, 0.0)
    assert same is x and same_plan is plan


@pytest.mark.parametrize("key_bits", [32, 3])
@pytest.mark.parametrize("feats", BC.FEATS)
def test_dropout_kernels_through_the_raw_abi(feats, key_bits):
    """The C entry points with a descriptor table built by hand: strided sources, a destination with a row stride of its own."""
    from wsi_hgnn_amd import _native as N, mil
    lib = N.load()
    sizes, p = [129, 0, 300, 3], 0.29
    draws = BC.draws_for(sizes, 9)
    wide = torch.randn(sum(sizes), feats + 8, generator=torch.Generator().manual_seed(6)).to(DEV)
    src = wide[:, 4:4 + feats]                                                          # stride feats + 8, 16 bytes into the row
    odd = wide[:, 1:1 + feats]                                                          # 4 bytes into the row: never 16-byte aligned
    counts = [mil.patch_counts(n, p) for n in sizes]
    words, parts, off, row = [], [], 0, 0
    for b, (n, (k, m), d) in enumerate(zip(sizes, counts, draws)):
        view = (odd if b == 2 else src)[off:off + n]                                    # (one bag falls back to the scalar path on its own)
        parts.append(view.cpu().contiguous())
        words += [view.data_ptr() if n else 0, feats + 8, n, k, m, row, d, 0]
        off, row = off + n, row + k + m
    desc = torch.frombuffer(array.array("q", words), dtype=torch.int64).to(DEV)
    total, ld = row, feats + 4
    sel = torch.full((total + 8,), -7, dtype=torch.int32, device=DEV)
    out = torch.full((total + 2, ld), 3.0, device=DEV)
    N.check(lib.wsi_bag_dropout_select(N.ptr(desc), len(sizes), key_bits, N.ptr(sel), total, N.stream()), "select")
    N.check(lib.wsi_bag_slot_fill(N.ptr(desc), len(sizes), N.ptr(sel), N.ptr(out), ld, feats, total, None, 0, None, None, 0, N.stream()), "fill")
    want_rows, _, want_sel = mil.dropout_patches_tensor(torch.cat(parts), sizes, p, draws, key_bits)
    assert torch.equal(sel[:total].cpu(), want_sel) and int((sel[total:] != -7).sum()) == 0
    assert torch.equal(out[:total, :feats].cpu(), want_rows)
    assert int((out[total:] != 3.0).sum()) == 0 and int((out[:, feats:] != 3.0).sum()) == 0       # nothing beyond the rows and columns asked for


def _slot_and_plans(feats, sizes, filler):
    from wsi_hgnn_amd import mil
    slot = mil.BagSlot(feats, BC.row_cap(sizes, filler), BC.BAG_CAP, num_classes=2, device=DEV)
    slot.load(BC.make_bags(sizes, feats, 21, DEV), BC.LABELS[:len(sizes)])
    segs = list(sizes) + [0] * (BC.BAG_CAP - len(sizes)) + [slot.row_cap - sum(sizes)]
    plain = mil.bag_plan(segs, DEV)
    assert slot.plan.num_chunks > plain.num_chunks                                      # the padded plan ends in chunks that no segment owns
    return slot, plain


@pytest.mark.parametrize("filler", list(BC.FILLERS))
@pytest.mark.parametrize("sizes", BC.BATCHES)
def test_bag_kernels_under_the_padded_plan(sizes, filler):
    """wsi_bag_softmax_pool_fwd / _bwd, wsi_bag_scores_fwd / _bwd, wsi_segment_weighted_sums and wsi_segment_reduce (max, as critical_onehot
    uses it, and its backward): every output under the slot's padded plan equals the output under the unpadded plan of the same segments."""
    from wsi_hgnn_amd import _native as N, ops
    from wsi_hgnn_amd.mil import dsmil
    D, C = 64, 2
    slot, plain = _slot_and_plans(D, sizes, filler)
    g = torch.Generator().manual_seed(31)
    n, S = slot.row_cap, slot.num_segs
    scores0, values0, q0 = torch.randn(n, C, generator=g).to(DEV), torch.randn(n, D, generator=g).to(DEV), torch.randn(n, D, generator=g).to(DEV)
    w_out, w_sc, w_mx = torch.randn(S, C, D, generator=g).to(DEV), torch.randn(n, C, generator=g).to(DEV), torch.randn(S, C, generator=g).to(DEV)
    got = {}
    for name, rp in (("padded", slot.plan), ("plain", plain)):
        r = {}
        scores, values, q = (t.clone().requires_grad_(True) for t in (scores0, values0, q0))
        out, lse, stats = ops.bag_softmax_pool_lse(scores, values, rp, 0.5)
        (out * w_out).sum().backward()
        r.update(out=out, lse=lse, stats=stats, g_scores=scores.grad, g_values=values.grad)
        r["attention"] = ops.bag_attention(scores, stats, rp, 0.5)
        onehot = dsmil.critical_onehot(scores0, rp)
        sc = ops.bag_scores(q, onehot, rp)
        (sc * w_sc).sum().backward()
        r.update(onehot=onehot, bag_scores=sc, g_q=q.grad)
        r["weighted_sums"] = ops.segment_weighted_sums(values0, scores0, rp)
        r["max"], r["argmax"] = ops._segment_reduce_raw(scores0, rp, N.WSI_RED_MAX)
        s2 = scores0.clone().requires_grad_(True)
        (ops.segment_reduce(s2, rp, "max") * w_mx).sum().backward()
        r["g_max"] = s2.grad
        got[name] = r
    torch.cuda.synchronize()
    for k, v in got["padded"].items():
        assert torch.equal(v, got["plain"][k]), k
        assert torch.isfinite(v.to(torch.float32)).all(), k


@pytest.mark.parametrize("filler", list(BC.FILLERS))
@pytest.mark.parametrize("p", [0.0, 0.25, 0.29])
@pytest.mark.parametrize("feats", BC.FEATS)
def test_slot_fill_against_the_cpu_fill(feats, p, filler):
    from wsi_hgnn_amd import mil
    cap = max(BC.row_cap(sizes, filler) for sizes in BC.BATCHES)
    gpu = mil.BagSlot(feats, cap, BC.BAG_CAP, num_classes=2, device=DEV, dropout_patch=p, seed=5)
    cpu = mil.BagSlot(feats, cap, BC.BAG_CAP, num_classes=2, device="cpu", dropout_patch=p, seed=5)
    order = (BC.BATCHES[3], BC.BATCHES[0], BC.BATCHES[2], BC.BATCHES[1], BC.BATCHES[3])   # smaller loads after larger ones: the filler is zeroed again
    for r, sizes in enumerate(order):
        bags = BC.make_bags(sizes, feats, 60 + r, DEV)
        labels = BC.LABELS[:len(sizes)]
        draws = BC.draws_for(sizes, r) if r % 2 else None                                # (None: the slots' own running counters agree)
        gpu.load(bags, labels, draws)
        cpu.load([t.cpu() for t in bags], labels, draws)
        assert torch.equal(gpu.small.cpu(), cpu.small), (r, "small tables")
        assert torch.equal(gpu.row_seg.cpu(), cpu.row_seg), (r, "row_seg")
        assert torch.equal(gpu.rows.cpu(), cpu.rows), (r, "rows")
        assert gpu.plan.ranges == cpu.plan.ranges and gpu.sizes == cpu.sizes and gpu.num_real == cpu.num_real
        BC.check_slot_tables(gpu, cpu.sizes, labels, cpu.rows[:sum(cpu.sizes)])
        real = sum(gpu.sizes)
        assert int(gpu.rows[real:].abs().max()) == 0                                    # the filler's rows are zero after a larger load
