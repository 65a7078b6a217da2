"""Scoring explanations against annotations (wsi_hgnn_amd/localization.py) through the tensor formulation on the CPU (``kernels=False``):
patch labels, the localisation AUROC, the heat-map fill, the host helpers and the C ABI's argument checks.  Labelling cases live on the
quarter-integer lattice, where the rule is exact: every comparison with the loop restatements of localization_cases.py is an equality."""
import warnings
from collections import OrderedDict

import numpy as np
import pytest
import torch

import localization_cases as C

LABEL_CASES = C.label_cases()
AUC_CASES = C.auc_cases()


def _labels(slides, **kw):
    from wsi_hgnn_amd import localization as L
    centres, sizes, ann = C.pack_labels_case(slides, L)
    return L.patch_labels(centres, sizes, ann, kernels=False, **kw)


@pytest.mark.parametrize("name", sorted(LABEL_CASES))
def test_patch_labels_equal_the_loop(name):
    slides = LABEL_CASES[name]
    got = _labels(slides)
    assert got.dtype == torch.int32 and got.shape == (sum(len(ps) for _, ps in slides),)
    assert np.array_equal(got.numpy(), C.label_loop(slides)), name


@pytest.mark.parametrize("name", sorted(LABEL_CASES))
def test_off_boundary_labels_equal_matplotlib(name):
    Path = pytest.importorskip("matplotlib.path").Path
    slides = [(rings, [p for p in ps if not C.on_any_boundary(rings, *p)]) for rings, ps in LABEL_CASES[name]]
    want = []
    for rings, ps in slides:
        inside = np.zeros(len(ps), dtype=bool)
        for ring in rings:
            if ps and len(ring) >= 3:
                inside |= Path(np.array(ring + ring[:1]), closed=True).contains_points(np.array(ps))
        want += inside.astype(np.int32).tolist()
    assert _labels(slides).tolist() == want, name


def test_patch_labels_equal_the_matplotlib_fixture():
    from wsi_hgnn_amd import localization as L
    z = C.labels_fixture()
    ptr, sptr = z["ring_ptr"], z["slide_ring_ptr"]
    anns = [L.Annotation(torch.from_numpy(z["vertices"][ptr[a]:ptr[b]]), torch.from_numpy(ptr[a:b + 1] - ptr[a])) for a, b in zip(sptr, sptr[1:])]
    assert len(z["labels"]) >= 300 and 0 < z["labels"].sum() < len(z["labels"])
    got = L.patch_labels(torch.from_numpy(z["points"]), z["sizes"].tolist(), anns, kernels=False)
    assert np.array_equal(got.numpy(), z["labels"])
    one = L.patch_labels(torch.from_numpy(z["points"]), z["sizes"].tolist(), L.AnnotationBatch(anns, chunk=3), kernels=False)      # the chunking changes nothing
    assert torch.equal(one, got)


def test_patch_labels_refusals():
    from wsi_hgnn_amd import localization as L
    centres, sizes, ann = C.pack_labels_case(LABEL_CASES["rings_are_per_slide"], L)
    with pytest.raises(ValueError, match="add up"):
        L.patch_labels(centres, [1, 1], ann, kernels=False)
    with pytest.raises(ValueError, match="annotations"):
        L.patch_labels(centres, [5], ann, kernels=False)
    with pytest.raises(RuntimeError, match="GPU only"):
        L.patch_labels(centres, sizes, ann, kernels=True)
    with pytest.raises(ValueError, match="chunk"):
        L.AnnotationBatch([], chunk=0)
    with pytest.raises(ValueError, match="chunk"):
        L.AnnotationBatch([], chunk=1025)
    with pytest.raises(RuntimeError, match="GPU only"):
        L.score(torch.zeros(2), torch.zeros(2, dtype=torch.int32), [2], kernels=True)
    with pytest.raises(RuntimeError, match="GPU only"):
        L.heat_image(torch.zeros((1, 2), dtype=torch.int64), torch.zeros(1), 4, 4, 1, kernels=True)


def test_annotation_batch_tables():
    from wsi_hgnn_amd import localization as L
    a = L.Annotation.from_rings([C.staircase(9), [], [(0.0, 0.0), (1.0, 1.0)]])
    b = L.AnnotationBatch([a, L.Annotation.from_rings([]), L.Annotation.from_rings([C.TRIANGLE])], chunk=4)
    assert b.chunks.tolist() == [[0, 0, 4, 0], [0, 4, 4, 0], [0, 8, 1, 0], [2, 0, 2, 0], [3, 0, 3, 2]]
    assert b.slide_chunk_ptr.tolist() == [0, 4, 4, 5] and b.chunks_per_slide == [4, 0, 1] and b.rings_per_slide == [3, 0, 1]
    assert b.ring_ptr.tolist() == [0, 9, 9, 11, 14] and b.slide_ring_ptr.tolist() == [0, 3, 3, 4]
    assert b.ring_box[3].tolist() == [0.0, 0.0, 8.0, 8.0] and b.ring_box[1].tolist() == [float("inf")] * 2 + [-float("inf")] * 2
    assert b.to("cpu").chunks is not None and b.vertices.dtype == torch.float64 and b.chunks.dtype == torch.int32


def test_read_annotations(tmp_path):
    from wsi_hgnn_amd import localization as L
    xml = """<?xml version="1.0"?>
<ASAP_Annotations><Annotations>
  <Annotation Name="_0" Type="Polygon" PartOfGroup="_0" Color="#F4FA58"><Coordinates>
      <Coordinate Order="0" X="10.5" Y="20.25" />
      some text between the children
      <Coordinate Order="1" X="30.125" Y="20.25" /><Coordinate Order="2" X="30.1" Y="-40.75" />
  </Coordinates></Annotation>
  <Annotation Name="_1" Type="Polygon" PartOfGroup="_2" Color="#F4FA58"><Coordinates>
      <Coordinate Order="0" X="1" Y="2" /><Coordinate Order="1" X="3" Y="4" />
  </Coordinates></Annotation>
</Annotations><AnnotationGroups /></ASAP_Annotations>"""
    (tmp_path / "a.xml").write_text(xml)
    a = L.read_annotations(tmp_path / "a.xml")
    assert a.vertices.dtype == torch.float64 and a.ring_ptr.dtype == torch.int64 and a.num_rings == 2
    assert a.ring_ptr.tolist() == [0, 3, 5]
    assert a.vertices.tolist() == [[10.5, 20.25], [30.125, 20.25], [float("30.1"), -40.75], [1.0, 2.0], [3.0, 4.0]]


def test_patch_centres_and_tiles_from_names():
    from wsi_hgnn_amd import localization as L
    tiles = L.tiles_from_names(["3_5.jpeg", "some/dir/0_12.jpeg", "7_0.jpeg"])
    assert tiles.dtype == torch.int64 and tiles.tolist() == [[3, 5], [0, 12], [7, 0]]
    # grid = (t * patch_size) // 2 ** (level - 1); centre = grid * 2 ** level + patch_size
    for patch_size, level, grid, centres in ((256, 1, [[768, 1280], [0, 3072], [1792, 0]], [[1792, 2816], [256, 6400], [3840, 256]]),
                                             (256, 2, [[384, 640], [0, 1536], [896, 0]], [[1792, 2816], [256, 6400], [3840, 256]]),
                                             (512, 1, [[1536, 2560], [0, 6144], [3584, 0]], [[3584, 5632], [512, 12800], [7680, 512]]),
                                             (512, 2, [[768, 1280], [0, 3072], [1792, 0]], [[3584, 5632], [512, 12800], [7680, 512]])):
        g, c = L.patch_centres(tiles, patch_size, level)
        assert g.dtype == c.dtype == torch.int64 and g.tolist() == grid and c.tolist() == centres, (patch_size, level)
    assert L.patch_centres(torch.tensor([[3, 1]]), 255, 3)[0].tolist() == [[191, 63]]          # 765 // 4, 255 // 4: the floor


def test_patch_order():
    from wsi_hgnn_amd import localization as L
    from wsi_hgnn_amd.graph import HeteroGraph
    ids = {"0": torch.tensor([4, 0, 6]), "1": torch.tensor([5, 1, 3, 2])}
    g = HeteroGraph.from_coo(OrderedDict((t, len(v)) for t, v in ids.items()),
                             OrderedDict([(("0", "a", "1"), (torch.tensor([0]), torch.tensor([1])))]),
                             feat={t: torch.zeros(len(v), 2) for t, v in ids.items()})
    for t, v in ids.items():
        g.nodes[t].data["_ID"] = v
    mask = {"0": torch.tensor([0.4, 0.0, 0.6]), "1": torch.tensor([0.5, 0.1, 0.3, 0.2])}
    assert torch.equal(L.patch_order(g, mask), torch.tensor([0.0, 0.1, 0.2, 0.3, 0.4, 0.5, 0.6]))
    flat = torch.rand(7)
    assert L.patch_order(g, flat) is flat
    del g.nodes["1"].data["_ID"]
    with pytest.raises(ValueError, match="_ID"):
        L.patch_order(g, mask)


def _check_score(got, scores, labels, sizes):
    """pos / neg / gt / eq equal the loop's integers, auc is bit-equal to the one division in numpy float64, mean to numpy.nanmean."""
    want = C.pair_loop(scores, labels, sizes)
    flat = np.asarray(scores).ndim == 1
    pick = (lambda a: a[:, 0]) if flat else (lambda a: a)
    for k, name in enumerate(("pos", "neg", "gt", "eq")):
        t = getattr(got, name)
        assert t.dtype == torch.int64 and np.array_equal(t.numpy(), pick(want[..., k])), name
    assert got.flags.dtype == torch.int32 and np.array_equal(got.flags.numpy(), pick(want[..., 4]))
    auc = C.auc_of(want)
    assert got.auc.dtype == torch.float64 and np.array_equal(got.auc.numpy().view(np.int64), pick(auc).view(np.int64))
    mean = C.nanmean_columns(auc)
    assert np.array_equal(got.mean.numpy().reshape(-1).view(np.int64), mean.view(np.int64))
    return auc


@pytest.mark.parametrize("name", sorted(AUC_CASES))
def test_score_equals_the_loop_and_the_sklearn_fixture(name):
    from wsi_hgnn_amd import localization as L
    scores, labels, sizes = AUC_CASES[name]
    got = L.score(torch.from_numpy(scores), torch.from_numpy(labels), sizes, kernels=False)
    assert got.cpu() is got
    auc = _check_score(got, scores, labels, sizes)
    recorded = C.auc_fixture()[name]
    assert len(recorded) == auc.shape[0]
    for s, cols in enumerate(recorded):
        for c, v in enumerate(cols):
            if v is None:
                assert np.isnan(auc[s, c]), (s, c)
            else:
                assert abs(auc[s, c] - v) <= 1e-12, (s, c, auc[s, c], v)       # n 2^-53 at n = 2000, x 4 for sklearn's cumulative sums


def test_score_special_values():
    from wsi_hgnn_amd import localization as L
    run = lambda name: L.score(*(torch.from_numpy(a) for a in AUC_CASES[name][:2]), AUC_CASES[name][2], kernels=False)
    assert run("tied_perfect_inverted").auc.tolist() == [0.5, 1.0, 0.0]
    one = run("one_class")
    assert torch.isnan(one.auc[:2]).all() and one.flags.tolist() == [0, 0, 0] and one.mean.item() == one.auc[2].item()
    bad = run("nan_score")
    assert bad.flags.tolist() == [0, 1, 0] and torch.isnan(bad.auc[1]) and bad.auc[0] == bad.auc[2] == one.auc[2]
    assert torch.isnan(run("empty_slide_in_the_middle").auc[1])
    assert run("three_columns").auc.shape == (2, 3) and run("three_columns").mean.shape == (3,)
    every = L.score(torch.zeros(4), torch.zeros(4, dtype=torch.int32), [2, 2], kernels=False)
    assert torch.isnan(every.mean) and torch.isnan(every.auc).all()
    many = np.random.RandomState(3).rand(300)                                   # the mean's summation order beyond 8 and beyond 128 slides
    many[::7] = np.nan
    for n in (7, 8, 9, 100, 129, 300):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)
            assert L._nan_mean(torch.from_numpy(many[:n].copy())[:, None]).item() == np.nanmean(many[:n])


def test_heat_image_equals_the_loop():
    from wsi_hgnn_amd import localization as L
    grid, values, height, width, patch = C.heat_case()
    base = torch.from_numpy(np.random.RandomState(1).randint(0, 256, size=(height, width, 3)).astype(np.uint8))
    for b in (None, base):
        got = L.heat_image(torch.tensor(grid), torch.from_numpy(values), height, width, patch, base=b, kernels=False)
        assert got.dtype == torch.uint8 and got.shape == (height, width, 3)
        want = C.fill_loop(grid, values, height, width, patch, L.WISTIA.numpy(), None if b is None else b.numpy())
        assert np.array_equal(got.numpy(), want)
    assert got[12, 12].tolist() == L.WISTIA[255].tolist() and got[11, 13].tolist() == L.WISTIA[int(0.999 * 256)].tolist()     # the highest index wins
    assert got[22, 0].tolist() == [0, 0, 0] and got[0, 63].tolist() == base[0, 63].tolist()


def test_wistia_table():
    from wsi_hgnn_amd import localization as L
    assert L.WISTIA.dtype == torch.uint8 and L.WISTIA.shape == (256, 3)
    assert [L.WISTIA[i].tolist() for i in (0, 64, 128, 255)] == [[228, 255, 122], [255, 232, 26], [255, 189, 0], [252, 127, 0]]


def test_wistia_table_equals_matplotlib():
    matplotlib = pytest.importorskip("matplotlib")
    from wsi_hgnn_amd import localization as L
    want = np.rint(255 * matplotlib.colormaps["Wistia"](np.arange(256))[:, :3]).astype(np.uint8)
    assert np.array_equal(L.WISTIA.numpy(), want)


def test_c_abi_refuses_bad_localization_arguments_without_a_gpu():
    from wsi_hgnn_amd import _native as N
    lib = N.load()
    err = lambda: lib.wsi_last_error().decode()
    assert lib.wsi_abi_version() == 26 == N.WSI_ABI_VERSION
    labels = lambda **kw: lib.wsi_loc_labels(*[kw.get(k, d) for k, d in (
        ("centres", None), ("num_centres", 4), ("tiles", None), ("num_tiles", 1), ("slides", None), ("num_slides", 1), ("vertices", None),
        ("num_vertices", 3), ("ring_ptr", None), ("ring_box", None), ("num_rings", 1), ("chunks", None), ("num_chunks", 1),
        ("slide_chunk_ptr", None), ("max_slide_chunks", 1), ("chunk_edges", 512), ("scratch", None), ("scratch_words", 4), ("labels", None),
        ("stream", None))])
    assert labels() == N.WSI_EINVAL and "null pointer" in err()
    for name in ("num_centres", "num_tiles", "num_slides", "num_vertices", "num_rings", "num_chunks", "max_slide_chunks", "scratch_words"):
        assert labels(**{name: -1}) == N.WSI_EINVAL and "negative" in err(), name
    for chunk in (0, -5, N.WSI_LOC_CHUNK_MAX + 1):
        assert labels(chunk_edges=chunk) == N.WSI_EINVAL and "chunk_edges" in err()
    assert labels(max_slide_chunks=N.WSI_LOC_MAX_SLIDE_CHUNKS + 1) == N.WSI_EINVAL and "chunks in one slide" in err()
    assert labels(num_tiles=0) == N.WSI_OK
    score = lambda **kw: lib.wsi_loc_score(*[kw.get(k, d) for k, d in (
        ("scores", None), ("num_rows", 4), ("C", 1), ("labels", None), ("tiles", None), ("num_tiles", 1), ("slides", None), ("num_slides", 1),
        ("partial", None), ("counts", None), ("flags", None), ("auc", None), ("mean", None), ("stream", None))])
    assert score() == N.WSI_EINVAL and "null pointer" in err()
    for name in ("num_rows", "num_tiles", "num_slides"):
        assert score(**{name: -1}) == N.WSI_EINVAL and "negative" in err(), name
    for C_ in (0, -1, N.WSI_LOC_MAX_COLUMNS + 1):
        assert score(C=C_) == N.WSI_EINVAL and "score columns" in err()
    owner = lambda n=3, patch=4, h=8, w=8: lib.wsi_loc_owner(None, n, patch, h, w, None, None)
    assert owner() == N.WSI_EINVAL and "null pointer" in err()
    assert owner(n=-1) == N.WSI_EINVAL and owner(h=-1) == N.WSI_EINVAL and owner(w=-1) == N.WSI_EINVAL and "negative" in err()
    assert owner(patch=-1) == N.WSI_EINVAL and owner(patch=N.WSI_LOC_MAX_PATCH + 1) == N.WSI_EINVAL and "patch" in err()
    assert owner(h=1 << 16, w=1 << 15) == N.WSI_EINVAL and "2^31" in err()
    assert owner(n=0) == N.WSI_OK


class _StubExplainer:
    """``GemExplainer``'s surface, returning the mask stored on the graph."""

    def __init__(self, graph, model, label):
        self.graph = graph

    def explain_node(self):
        return self.graph.stub_mask


def test_explain_and_score_on_cpu_with_a_stub_explainer():
    from wsi_hgnn_amd import localization as L, synthetic
    rng = np.random.RandomState(9)
    slides, masks = [], []
    for s, n in enumerate((40, 55)):
        g = synthetic.homogeneous_graph(n, 4, seed=s)
        g.stub_mask = (np.floor(rng.rand(n) * 8) / 8).astype(np.float32)             # a numpy array, as GemExplainer returns
        tiles = torch.stack([torch.arange(n) % 8, torch.arange(n) // 8], 1)
        _, centres = L.patch_centres(tiles, 256, 1)
        ann = L.Annotation.from_rings([[(0.0, 0.0), (1100.0 + 512 * s, 0.0), (1100.0 + 512 * s, 1300.0), (0.0, 1300.0)]])
        slides.append((g, torch.tensor([1]), centres, ann))
        masks.append(torch.from_numpy(g.stub_mask))
    got, got_masks = L.explain_and_score(None, slides, explainer=_StubExplainer)
    sizes = [40, 55]
    labels = L.patch_labels(torch.cat([c for _, _, c, _ in slides]), sizes, [a for _, _, _, a in slides], kernels=False)
    assert 0 < labels[:40].sum() < 40 and 0 < labels[40:].sum() < 55
    want = L.score(torch.cat(masks), labels, sizes, kernels=False)
    for name in L.LocalizationScore._FIELDS:
        assert torch.equal(getattr(got, name), getattr(want, name)) or name in ("auc", "mean"), name
    assert got.auc.tolist() == want.auc.tolist() and got.mean.item() == want.mean.item()
    assert all(torch.equal(a, b) for a, b in zip(got_masks, masks))
    again, _ = L.explain_and_score(None, slides, explainer=None, scores=masks)            # precomputed scores in place of an explainer
    assert again.auc.tolist() == want.auc.tolist()
    with pytest.raises(NotImplementedError):
        L.explain_and_score(None, slides, explainer="SomethingElse")
