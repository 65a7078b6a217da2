"""The cases the bag-slot tests share (tests/test_bag_slot.py on the CPU, tests/test_bag_slot_kernels_gpu.py and tests/test_bag_slot_gpu.py on
the GPU), and the pure-Python restatement of the draw contract of include/wsi_hgnn.h ("patch dropout of many bags").

Feats 20 and 64 are both multiples of 4, so rows of either take the row kernel's 16-byte path when the pointers and strides allow; feats 22
cannot, its rows always take the scalar path.  The bag sizes sit on the edges of the default chunk of 128 rows and include the empty bag; the
batches below spread them over 1 to 4 real bags of a slot of 4.  A slot's row capacity either leaves the filler exactly one row or several
chunks.  One source of every batch is a strided view of a wider table."""
import torch

FEATS = (20, 22, 64)
SIZES = (0, 1, 2, 3, 127, 128, 129, 300)
KERNEL_SIZES = SIZES + (2500,)            # the selection kernel walks a bag 1024 rows at a time: a bag of more than two such tiles
RATES = (0.0, 0.1, 0.25, 0.29, 0.5)
BAG_CAP = 4
BATCHES = ((300,), (129, 0), (1, 127, 2), (3, 128, 0, 300))          # every size of SIZES, 1 to 4 real bags
FILLERS = {"one_row": 1, "chunks": 3 * 128 + 5}
LABELS = (1, 0, 1, 3)                                                   # (3: past the last of two classes - an all-zero target row)

M32 = 0xffffffff


def row_cap(sizes, filler):
    return sum(sizes) + FILLERS[filler]


def draws_for(sizes, salt=0):
    return [(0x1234567 * (b + 1) + 0x9E37 * n + salt) & M32 for b, n in enumerate(sizes)]


def make_bags(sizes, feats, seed, device="cpu"):
    """The batch's bags as separate tensors; the LAST non-empty one is a strided view (rows of a wider table, columns 4 .. 4 + feats)."""
    g = torch.Generator().manual_seed(seed)
    bags = [torch.randn(n, feats, generator=g) for n in sizes]
    last = max((b for b, n in enumerate(sizes) if n > 0), default=None)
    out = []
    for b, t in enumerate(bags):
        if b == last:
            wide = torch.zeros(t.shape[0], feats + 12)
            wide[:, 4:4 + feats] = t
            wide = wide.to(device)
            out.append(wide[:, 4:4 + feats])
        else:
            out.append(t.to(device))
    return out


def fmix32(h):
    h &= M32
    h ^= h >> 16
    h = (h * 0x85EBCA6B) & M32
    h ^= h >> 13
    h = (h * 0xC2B2AE35) & M32
    h ^= h >> 16
    return h


def python_selection(n, k, m, draw, key_bits=32):
    """The source rows of one bag's output, by the words of the contract: a loop and two sorts on (key, row) tuples."""
    mask = (1 << key_bits) - 1
    s1, s2 = fmix32(draw), fmix32(draw ^ 0x85EBCA6B)
    key1 = lambda i: fmix32((i * 0x9E3779B1 + s1) & M32) & mask
    key2 = lambda i: fmix32((i * 0x9E3779B1 + s2) & M32) & mask
    kept = sorted(i for _, i in sorted((key1(i), i) for i in range(n))[:k])
    pads = sorted(i for _, i in sorted((key2(i), i) for i in kept)[:m])
    return kept + pads


def _expected_plan(slot, new_sizes):
    """``bag_plan`` of the new sizes, the empty bags and the filler: (plan, the segments' row counts)."""
    from wsi_hgnn_amd import mil
    segs = list(new_sizes) + [0] * (slot.bag_cap - len(new_sizes)) + [slot.row_cap - sum(new_sizes)]
    return mil.bag_plan(segs, "cpu", slot.chunk), segs


def check_slot_tables(slot, new_sizes, labels, rows_expected):
    """Every table of a loaded slot (tensors on any device) against ``bag_plan`` of the new sizes plus the filler and the padding."""
    from wsi_hgnn_amd import mil
    plan, segs = _expected_plan(slot, new_sizes)
    nc, S, C = plan.num_chunks, slot.bag_cap + 1, slot.num_classes
    p = slot.plan
    assert (p.num_segs, p.num_chunks, p.num_rows, p.first_row) == (S, slot.chunk_cap, slot.row_cap, 0) and nc <= slot.chunk_cap
    assert p.chunk_row.cpu().tolist() == plan.chunk_row.tolist()[:nc] + [slot.row_cap] * (slot.chunk_cap - nc + 1)
    assert p.chunk_seg.cpu().tolist() == plan.chunk_seg.tolist()[:nc] + [S - 1] * (slot.chunk_cap - nc)
    assert p.seg_chunk.cpu().tolist() == plan.seg_chunk.tolist()
    assert p.ranges == plan.ranges
    assert torch.equal(p.counts().cpu(), plan.counts()) and torch.equal(p.inv_counts().cpu(), plan.inv_counts())
    assert torch.equal(p.nonempty().cpu(), plan.nonempty())
    assert torch.equal(p.row_segment().cpu(), plan.row_segment())
    want_t = torch.zeros(S, C)
    want_t[:len(labels)] = mil.bag_targets(list(labels), C)
    assert torch.equal(slot.targets.cpu(), want_t)
    live = sum(1 for n in new_sizes if n > 0)
    want_w = torch.tensor([1.0 / live if n > 0 else 0.0 for n in new_sizes] + [0.0] * (S - len(new_sizes))).view(-1, 1)
    assert torch.equal(slot.weights.cpu(), want_w)
    if live:
        assert abs(float(slot.weights.sum()) - 1.0) < 1e-6
    real = sum(new_sizes)
    assert torch.equal(slot.rows[:real].cpu(), rows_expected)
    assert int(slot.rows[real:].abs().max()) == 0 and slot.row_cap - real >= 1
    assert slot.num_real == len(new_sizes) and slot.sizes == list(new_sizes)
