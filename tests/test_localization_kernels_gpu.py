"""The kernels of csrc/localization.hip (patch labels, pair counting, the owner image) against the loop restatements of localization_cases.py
and against the tensor formulation (``kernels=False``) on the same GPU.  Lattice coordinates and integer counts: every comparison is an
equality.  Shapes are the smallest that reach every path: 1 / 255 / 256 / 257 centres (one lane, a tile less one, a full tile, two tiles),
rings of chunk - 1 / chunk / chunk + 1 / 2 chunk + 1 edges, a ring whose box misses a whole tile, slides with different chunk counts in one
launch, and 5000 rows of scores so that the positives span several tiles."""
import numpy as np
import pytest
import torch

import localization_cases as C

pytestmark = pytest.mark.gpu

LABEL_CASES = C.label_cases()
AUC_CASES = C.auc_cases()
CHUNK = 64
_CACHE = {}


def _dev():
    return torch.device("cuda:0")


def _both(slides, chunk=None):
    """(labels through the kernels, labels through the tensor formulation on the GPU, the packed batch)."""
    from wsi_hgnn_amd import localization as L
    centres, sizes, ann = C.pack_labels_case(slides, L, chunk)
    centres, ann = centres.to(_dev()), ann.to(_dev())
    got = L.patch_labels(centres, sizes, ann)
    assert got.is_cuda and got.dtype == torch.int32
    return got, L.patch_labels(centres, sizes, ann, kernels=False), ann


def _want(key, slides):
    if key not in _CACHE:
        _CACHE[key] = C.label_loop(slides)
    return _CACHE[key]


@pytest.mark.parametrize("name", sorted(LABEL_CASES))
def test_patch_labels_equal_the_loop(name):
    got, tensor, _ = _both(LABEL_CASES[name])
    assert np.array_equal(got.cpu().numpy(), _want(name, LABEL_CASES[name])) and torch.equal(got, tensor)
    small, _, _ = _both(LABEL_CASES[name], chunk=1)                  # every edge a chunk of its own
    assert torch.equal(small, got)


def test_patch_labels_equal_the_matplotlib_fixture():
    from wsi_hgnn_amd import localization as L
    z = C.labels_fixture()
    ptr, sptr = z["ring_ptr"], z["slide_ring_ptr"]
    anns = [L.Annotation(torch.from_numpy(z["vertices"][ptr[a]:ptr[b]]), torch.from_numpy(ptr[a:b + 1] - ptr[a])) for a, b in zip(sptr, sptr[1:])]
    for chunk in (3, 512):
        got = L.patch_labels(torch.from_numpy(z["points"]).to(_dev()), z["sizes"].tolist(), L.AnnotationBatch(anns, chunk=chunk).to(_dev()))
        assert np.array_equal(got.cpu().numpy(), z["labels"]), chunk


def _stair_slide(edges, n, seed):
    ring = C.staircase(edges, x0=16.0, y0=-8.0)
    hi = max(v[0] for v in ring) + 1.0
    return [ring], C.lattice_points(n, 15.0, -9.0, hi, hi - 24.0 + 1.0, seed)


@pytest.mark.parametrize("n", [1, 255, 256, 257])
@pytest.mark.parametrize("edges,chunks", [(CHUNK - 1, 1), (CHUNK, 1), (CHUNK + 1, 2), (2 * CHUNK + 1, 3)])
def test_ring_cut_into_chunks(edges, chunks, n):
    slides = [_stair_slide(edges, n, seed=edges * 1000 + n)]
    got, tensor, ann = _both(slides, chunk=CHUNK)
    assert ann.chunks_per_slide == [chunks] and ann.chunks[:, 2].sum().item() == edges
    want = _want(("stair", edges, n), slides)
    assert n == 1 or 0 < want.sum() < n
    assert np.array_equal(got.cpu().numpy(), want) and torch.equal(got, tensor)


def test_default_chunk_and_a_long_ring():
    from wsi_hgnn_amd import ops
    slides = [_stair_slide(2 * ops.LOC_CHUNK + 1, 300, seed=5)]
    got, tensor, ann = _both(slides)
    assert ann.chunk == ops.LOC_CHUNK and ann.chunks_per_slide == [3]
    assert np.array_equal(got.cpu().numpy(), _want("long", slides)) and torch.equal(got, tensor)


def test_a_ring_whose_box_misses_the_whole_tile():
    """Two tiles of centres: the first lies far from the second ring's box and the other way round, so each (tile, chunk) pair either rejects
    the tile before reading an edge or walks the edges."""
    near, far = C.staircase(40, x0=0.0, y0=0.0), C.staircase(40, x0=4000.0, y0=4000.0)
    a = C.lattice_points(256, -1.0, -1.0, 6.0, 6.0, seed=1)
    b = [(x + 4000.0, y + 4000.0) for x, y in C.lattice_points(200, -1.0, -1.0, 6.0, 6.0, seed=2)]
    slides = [([near, far], a + b)]
    got, tensor, ann = _both(slides, chunk=CHUNK)
    want = _want("reject", slides)
    assert 0 < want[:256].sum() < 256 and 0 < want[256:].sum() < 200
    assert np.array_equal(got.cpu().numpy(), want) and torch.equal(got, tensor)


def test_slides_with_different_chunk_counts_in_one_batch():
    slides = [_stair_slide(3 * CHUNK + 5, 257, seed=11), ([C.TRIANGLE], C.lattice_points(100, -1.0, -1.0, 9.0, 9.0, seed=12)),
              ([], C.lattice_points(7, 0.0, 0.0, 4.0, 4.0, seed=13)), _stair_slide(CHUNK + 1, 300, seed=14)]
    got, tensor, ann = _both(slides, chunk=CHUNK)
    assert ann.chunks_per_slide == [4, 1, 0, 2]
    want = _want("mixed", slides)
    assert np.array_equal(got.cpu().numpy(), want) and torch.equal(got, tensor) and not want[357:364].any()


def _score_both(name):
    from wsi_hgnn_amd import localization as L
    scores, labels, sizes = AUC_CASES[name]
    s, l = torch.from_numpy(scores).to(_dev()), torch.from_numpy(labels).to(_dev())
    return L.score(s, l, sizes), L.score(s, l, sizes, kernels=False)


@pytest.mark.parametrize("name", sorted(AUC_CASES))
def test_score_equals_the_loop(name):
    """n = 2 / 255 / 256 / 257 / 2000 with heavy ties, one-class, NaN and empty slides, three columns, and 5000 rows (20 tiles of positives)."""
    scores, labels, sizes = AUC_CASES[name]
    dev_score, tensor = _score_both(name)
    assert dev_score.auc.is_cuda and dev_score.mean.is_cuda
    got = dev_score.cpu()
    if name not in _CACHE:
        _CACHE[name] = C.pair_loop(scores, labels, sizes)
    want = _CACHE[name]
    pick = (lambda a: a[:, 0]) if scores.ndim == 1 else (lambda a: a)
    for k, field in enumerate(("pos", "neg", "gt", "eq", "flags")):
        assert np.array_equal(getattr(got, field).numpy(), pick(want[..., k])), field
    auc = C.auc_of(want)
    assert np.array_equal(got.auc.numpy().view(np.int64), pick(auc).view(np.int64))
    assert np.array_equal(got.mean.numpy().reshape(-1).view(np.int64), C.nanmean_columns(auc).view(np.int64))
    t = tensor.cpu()
    for field in ("pos", "neg", "gt", "eq", "flags"):
        assert torch.equal(getattr(t, field), getattr(got, field)), field
    assert torch.equal(t.auc.view(torch.int64), got.auc.view(torch.int64)) and torch.equal(t.mean.view(torch.int64), got.mean.view(torch.int64))
    for s, cols in enumerate(C.auc_fixture()[name]):
        for c, v in enumerate(cols):
            assert (np.isnan(auc[s, c]) if v is None else abs(auc[s, c] - v) <= 1e-12), (s, c)


def test_mean_over_many_slides():
    """150 slides of 3 rows: the mean's pairwise order beyond 128 values, with NaN slides in between."""
    from wsi_hgnn_amd import localization as L
    rng = np.random.RandomState(4)
    labels = np.tile(np.array([0, 1, 0], dtype=np.int32), 150)
    labels[1::60] = 0                                                # every 20th slide has one class only
    scores = (np.floor(rng.rand(450) * 4) / 4).astype(np.float32)
    got = L.score(torch.from_numpy(scores).to(_dev()), torch.from_numpy(labels).to(_dev()), [3] * 150).cpu()
    auc = C.auc_of(C.pair_loop(scores, labels, [3] * 150))
    assert np.isnan(auc).sum() >= 7 and np.array_equal(got.auc.numpy().view(np.int64), auc[:, 0].view(np.int64))
    assert got.mean.item() == C.nanmean_columns(auc)[0]


def test_heat_image_equals_the_loop():
    from wsi_hgnn_amd import localization as L
    grid, values, height, width, patch = C.heat_case()
    base = torch.from_numpy(np.random.RandomState(1).randint(0, 256, size=(height, width, 3)).astype(np.uint8))
    g, v = torch.tensor(grid).to(_dev()), torch.from_numpy(values).to(_dev())
    for b in (None, base):
        got = L.heat_image(g, v, height, width, patch, base=None if b is None else b.to(_dev()))
        want = C.fill_loop(grid, values, height, width, patch, L.WISTIA.numpy(), None if b is None else b.numpy())
        assert got.is_cuda and np.array_equal(got.cpu().numpy(), want)
        assert torch.equal(got, L.heat_image(g, v, height, width, patch, base=None if b is None else b.to(_dev()), kernels=False))


def test_two_runs_give_identical_bits():
    slides = [_stair_slide(3 * CHUNK + 5, 257, seed=11), ([C.BOWTIE, C.OUTER], C.lattice_points(300, -1.0, -1.0, 13.0, 13.0, seed=3))]
    a, _, _ = _both(slides, chunk=CHUNK)
    b, _, _ = _both(slides, chunk=CHUNK)
    assert torch.equal(a, b)
    x, y = _score_both("levels_4")[0].cpu(), _score_both("levels_4")[0].cpu()
    for field in ("pos", "neg", "gt", "eq", "flags"):
        assert torch.equal(getattr(x, field), getattr(y, field))
    assert torch.equal(x.auc.view(torch.int64), y.auc.view(torch.int64)) and torch.equal(x.mean.view(torch.int64), y.mean.view(torch.int64))


def test_ordinary_errors_leave_the_next_call_working():
    from wsi_hgnn_amd import localization as L
    slides = [_stair_slide(2 * CHUNK + 1, 257, seed=21)]
    centres, sizes, ann = C.pack_labels_case(slides, L, CHUNK)
    centres, ann = centres.to(_dev()), ann.to(_dev())
    with pytest.raises(ValueError, match="scratch"):
        L.patch_labels(centres, sizes, ann, max_scratch_words=3 * 257 - 1)
    with pytest.raises(ValueError, match="add up"):
        L.patch_labels(centres, [256], ann)
    with pytest.raises(ValueError, match="annotations"):
        L.patch_labels(centres, [200, 57], ann)
    with pytest.raises(ValueError, match="on cpu|on cuda"):
        L.patch_labels(centres.cpu(), sizes, ann)
    with pytest.raises(ValueError, match="labels"):
        L.score(torch.zeros(4, device=_dev()), torch.zeros(3, dtype=torch.int32, device=_dev()), [4])
    got = L.patch_labels(centres, sizes, ann, max_scratch_words=3 * 257)
    assert np.array_equal(got.cpu().numpy(), C.label_loop(slides))
