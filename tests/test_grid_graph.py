"""The slide graphs of GTNMIL and H2MIL from patch grids, on the CPU: the tensor formulation of construct.grid_adjacency / construct.slide_trees
against the loop restatements of tests/grid_cases.py, and the host layer (gtn.from_grid, gtn.read_coords, h2mil.from_grid,
h2mil.tables_from_names).  Every comparison is exact: integers equal, x_y_index bit-equal to numpy's float64 division (a nan matching a nan)."""
import numpy as np
import pytest
import torch

import grid_cases as G

GTN = G.gtn_cases()


@pytest.mark.parametrize("name", sorted(GTN))
def test_grid_adjacency_equals_the_loops(name):
    from wsi_hgnn_amd import construct
    slides = GTN[name]
    coords, sizes = G.as_tensors(slides)
    want = G.adjacency_loops(slides)
    for c in (coords, coords.to(torch.int32)):
        for kernels in (None, False):
            row, col = construct.grid_adjacency(c, sizes, kernels=kernels)
            assert row.dtype == col.dtype == torch.int64
            assert torch.equal(row, want[0]) and torch.equal(col, want[1])
    if name == "one node":
        assert want[0].numel() == 0
    if name == "full 5 x 7":
        assert want[0].numel() == 212
    if name == "three slides with identical coordinates":             # sets do not see each other: three copies of one slide's entries
        n, e = sizes[0], want[0].numel() // 3
        assert torch.equal(want[0][e:2 * e], want[0][:e] + n) and torch.equal(want[1][2 * e:], want[1][:e] + 2 * n)


def test_the_loops_equal_the_dense_double_loop():
    """The dictionary restatement against the reference's O(n^2) rule, in nonzero() order."""
    for name, slides in GTN.items():
        rows, cols, off = [], [], 0
        for pts in slides:
            nz = torch.from_numpy(G.dense_adjacency(pts)).nonzero()
            rows.append(nz[:, 0] + off), cols.append(nz[:, 1] + off)
            off += len(pts)
        want = G.adjacency_loops(slides)
        assert torch.equal(torch.cat(rows), want[0]) and torch.equal(torch.cat(cols), want[1]), name


@pytest.mark.parametrize("packed", [False, True])
def test_gtn_from_grid_equals_from_dense(packed):
    from wsi_hgnn_amd import gtn
    slides = GTN["unequal slides"][:3]
    g = torch.Generator().manual_seed(5)
    feats = [torch.randn(len(s), 7, generator=g) for s in slides]
    coords = [torch.tensor(s, dtype=torch.int64) for s in slides]
    nmax = max(len(s) for s in slides)
    node_feat, adj, mask = torch.zeros(3, nmax, 7), torch.zeros(3, nmax, nmax, dtype=torch.float64), torch.zeros(3, nmax)
    for b, s in enumerate(slides):
        node_feat[b, :len(s)], mask[b, :len(s)] = feats[b], 1
        adj[b, :len(s), :len(s)] = torch.from_numpy(G.dense_adjacency(s))
    want = gtn.from_dense(node_feat, adj, mask)
    got = gtn.from_grid(torch.cat(feats), torch.cat(coords), sizes=[len(s) for s in slides]) if packed else gtn.from_grid(feats, coords)
    assert got.sizes == want.sizes and got.weight is None and bool((want.weight == 1).all())
    assert torch.equal(got.row, want.row) and torch.equal(got.col, want.col) and torch.equal(got.x, want.x)


def test_read_coords_round_trip(tmp_path):
    from wsi_hgnn_amd import gtn
    pts = GTN["9 x 9 with holes"][0]
    path = tmp_path / "c_idx.txt"
    with open(path, "w") as f:                                   # as the reference's save_coords writes it
        for x, y in pts:
            f.writelines(str(x) + "\t" + str(y) + "\n")
    got = gtn.read_coords(str(path))
    assert got.dtype == torch.int64 and got.tolist() == [list(p) for p in pts]
    (tmp_path / "bad.txt").write_text("1\t2\n3 4\n")
    with pytest.raises(ValueError, match=r"bad\.txt:2"):
        gtn.read_coords(str(tmp_path / "bad.txt"))


TREES = {"small": lambda: [G.small_tree()],
         "unequal batch": lambda: [G.rich_tree(6, 5, seed=0), G.small_tree(seed=1), G.zero_max_tree(), G.random_tree(2, 9, seed=4, origin=(G.LIMIT - 24, 3))]}


@pytest.mark.parametrize("name", sorted(TREES))
def test_h2mil_from_grid_equals_from_slides_of_the_restated_tensors(name):
    from wsi_hgnn_amd import h2mil
    slides = TREES[name]()
    want = h2mil.from_slides([G.restated(s) for s in slides])
    for kernels in (None, False):
        got = h2mil.from_grid(slides, kernels=kernels)
        G.same_batches(got, want)
    if name == "small":
        assert want.sizes == [16] and want.edge_index.shape[1] == 86
    else:
        assert len(set(want.sizes)) == len(want.sizes)


def test_slide_trees_returns_the_batch_tensors():
    from wsi_hgnn_amd import construct, h2mil
    slides = TREES["unequal batch"]()
    want = h2mil.from_slides([G.restated(s) for s in slides])
    cat = lambda k: torch.cat([s[k] for s in slides])
    ei, nt, tree, xy = construct.slide_trees(cat("coords1"), cat("cover"), cat("coords2"), want.n1, want.n2)
    assert torch.equal(ei, want.edge_index) and torch.equal(nt, want.node_type) and torch.equal(tree, want.tree)
    assert xy.dtype == torch.float64 and G.same_doubles(xy, want.x_y_index)
    assert bool(torch.isnan(xy).any()) and bool((xy[~torch.isnan(xy)] <= 1).all())


def test_tables_from_names():
    from wsi_hgnn_amd import h2mil
    s = G.small_tree()
    l1 = ["%d-%d-%d-%d-%d-%d.jpeg" % (*c, *p) for c, p in zip(s["cover"].tolist(), s["coords1"].tolist())]
    l2 = ["%d-%d.jpeg" % tuple(p) for p in s["coords2"].tolist()]
    names = [l2[0], l1[0], l2[1], "-1.jpeg"] + l1[1:] + l2[2:]          # file order mixes the three kinds
    c1, cv, c2, perm = h2mil.tables_from_names(names)
    assert torch.equal(c1, s["coords1"]) and torch.equal(cv, s["cover"]) and torch.equal(c2, s["coords2"])
    assert [names[i] for i in perm.tolist()] == ["-1.jpeg"] + l1 + l2
    assert h2mil.tables_from_names([n.split(".")[0] for n in names])[3].tolist() == perm.tolist()
    for bad, what in ((l1 + l2, "exactly one root"), (names + ["-1"], "exactly one root"), (names + ["1-2-3"], "neither"),
                      (names + ["a-b"], "neither"), (names + ["1--2"], "neither"), (names + ["1-2-3-4-5-6-7"], "neither")):
        with pytest.raises(ValueError, match=what):
            h2mil.tables_from_names(bad)


def _adj(points, sizes=None, **kw):
    from wsi_hgnn_amd import construct
    return construct.grid_adjacency(torch.tensor(points, dtype=torch.int64).reshape(-1, 2), sizes or [len(points)], **kw)


def _tree(coords1, cover, coords2, **kw):
    from wsi_hgnn_amd import construct
    t = lambda rows, w: torch.tensor(rows, dtype=torch.int64).reshape(-1, w)
    return construct.slide_trees(t(coords1, 2), t(cover, 4), t(coords2, 2), kw.pop("n1", [len(coords1)]), kw.pop("n2", [len(coords2)]), **kw)


def test_refusals():
    with pytest.raises(ValueError, match="repeated"):
        _adj([(1, 1), (2, 2), (1, 1)])
    assert _adj([(1, 1), (2, 2), (1, 1)], sizes=[2, 1])[0].tolist() == [0, 1]               # the same pair in two slides is fine
    for bad in (-1, G.LIMIT, 2 ** 40):
        with pytest.raises(ValueError, match="outside 0 <= c < 2\\^24"):
            _adj([(0, 0), (bad, 1)])
        with pytest.raises(ValueError, match="outside 0 <= c < 2\\^24"):
            _adj([(0, 0), (1, bad)])
    assert _adj([(G.LIMIT - 1, 0), (G.LIMIT - 1, 1), (0, G.LIMIT - 1)])[1].tolist() == [1, 0]
    with pytest.raises(ValueError, match="add up"):
        _adj([(0, 0), (1, 1)], sizes=[3])
    with pytest.raises(ValueError, match="integer"):
        from wsi_hgnn_amd import construct
        construct.grid_adjacency(torch.zeros(3, 2), [3])
    ok = ([(0, 0), (1, 0)], [(0, 1, 0, 1), (2, 3, 0, 1)], [(0, 0), (3, 1)])
    assert _tree(*ok)[2].tolist() == [-1, 0, 0, 1, 2]
    with pytest.raises(ValueError, match="no level-1 node covers"):
        _tree(ok[0], ok[1], ok[2] + [(5, 5)])
    with pytest.raises(ValueError, match="repeated"):
        _tree([(0, 0), (0, 0)], ok[1], ok[2])
    with pytest.raises(ValueError, match="repeated"):
        _tree(ok[0], ok[1], [(0, 0), (0, 0)])
    with pytest.raises(ValueError, match="outside 0 <= c < 2\\^24"):
        _tree([(0, 0), (-1, 0)], ok[1], ok[2])
    with pytest.raises(ValueError, match="outside 0 <= c < 2\\^24"):
        _tree(ok[0], ok[1], [(0, 0), (G.LIMIT, 1)])
    assert _tree(ok[0], [(0, 1, 0, 1), (-5, 3, 0, 1)], ok[2])[0].shape[1] == 10               # a cover value outside the range matches nothing
    for n1, n2 in (([2, 0], [1, 1]), ([1, 1], [2, 0])):
        with pytest.raises(ValueError, match="empty level"):
            _tree(*ok, n1=n1, n2=n2)
    with pytest.raises(ValueError, match="empty level"):
        _tree([], [], ok[2])


def test_kernels_true_on_cpu_tensors_is_refused():
    from wsi_hgnn_amd import gtn, h2mil, ops
    with pytest.raises(RuntimeError, match="GPU only"):
        _adj([(0, 0), (1, 1)], kernels=True)
    with pytest.raises(RuntimeError, match="GPU only"):
        _tree([(0, 0)], [(0, 1, 0, 1)], [(0, 0)], kernels=True)
    with pytest.raises(RuntimeError, match="GPU only"):
        gtn.from_grid([torch.zeros(2, 3)], [torch.tensor([[0, 0], [1, 1]])], kernels=True)
    with pytest.raises(RuntimeError, match="GPU only"):
        h2mil.from_grid([G.small_tree()], kernels=True)
    with pytest.raises(RuntimeError, match="GPU only"):                                       # the ops refuse CPU tensors like every other op
        ops.grid_index(torch.zeros((2, 2), dtype=torch.int32), torch.tensor([0, 2], dtype=torch.int32))


def test_c_abi_refuses_bad_grid_arguments_without_a_gpu():
    from wsi_hgnn_amd import _native as N, ops
    lib = N.load()
    err = lambda: lib.wsi_last_error().decode()
    assert [ops.grid_capacity(p) for p in (0, 1, 2, 3, 255, 256, 257)] == [2, 2, 4, 8, 512, 512, 1024]
    assert lib.wsi_grid_index(None, 5, None, 1, None, None, 8, None, None, None) == N.WSI_EINVAL and "capacity" in err()        # < 2 P
    assert lib.wsi_grid_index(None, 5, None, 1, None, None, 12, None, None, None) == N.WSI_EINVAL                                # not a power of two
    assert lib.wsi_grid_index(None, 5, None, 0, None, None, 16, None, None, None) == N.WSI_EINVAL
    assert lib.wsi_grid_index(None, 5, None, 1, None, None, 16, None, None, None) == N.WSI_EINVAL and "null pointer" in err()
    assert lib.wsi_grid_count(7, None, 5, None, 1, 0, None, None, None, 16, None, None, None) == N.WSI_EINVAL and "mode" in err()
    assert lib.wsi_grid_count(N.WSI_GRID_TREE, None, 5, None, 3, 0, None, None, None, 16, None, None, None) == N.WSI_EINVAL and "tree" in err()
    assert lib.wsi_grid_count(N.WSI_GRID_TREE, None, 5, None, 2, 6, None, None, None, 16, None, None, None) == N.WSI_EINVAL
    assert lib.wsi_grid_count(N.WSI_GRID_ADJACENCY, None, 0, None, 1, 0, None, None, None, 2, None, None, None) == 0
    assert lib.wsi_grid_write(N.WSI_GRID_ADJACENCY, None, 5, None, 1, 0, None, None, None, 16, *([None] * 11)) == N.WSI_EINVAL and "null pointer" in err()
