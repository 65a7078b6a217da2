"""The grid-graph kernels (csrc/grid_graph.hip: wsi_grid_index / wsi_grid_count / wsi_grid_write) on the GPU: the cases of tests/test_grid_graph.py
through the kernels, against the loop restatement of tests/grid_cases.py and against the tensor formulation run on the same GPU.  Every
comparison is exact (integers equal, x_y_index bit-equal to numpy's float64 division, a nan matching a nan).  Sizes around the 256-thread block,
a batch dense enough that the table has probe chains, run-to-run identity, and the flag paths (ordinary error returns: the next call works)."""
import pytest
import torch

import grid_cases as G

pytestmark = pytest.mark.gpu

DEV = "cuda"
GTN = G.gtn_cases()


def _adjacency(slides, kernels):
    from wsi_hgnn_amd import construct
    coords, sizes = G.as_tensors(slides)
    return construct.grid_adjacency(coords.to(DEV), sizes, kernels=kernels)


def _same(got, want):
    return all(a.dtype == torch.int64 and torch.equal(a.cpu(), b.cpu()) for a, b in zip(got, want))


@pytest.mark.parametrize("name", sorted(GTN))
def test_adjacency_kernels_equal_the_loops_and_the_tensor_formulation(name):
    want = G.adjacency_loops(GTN[name])
    got = _adjacency(GTN[name], True)
    assert got[0].is_cuda and _same(got, want)
    assert _same(_adjacency(GTN[name], None), want)                       # CUDA tensors: the kernels by default
    assert _same(_adjacency(GTN[name], False), want)


@pytest.mark.parametrize("n", [1, 255, 256, 257])
def test_adjacency_at_sizes_around_the_block(n):
    slides = [G.disc(n, seed=n), G.disc(n, seed=n + 1, x0=G.LIMIT - 40, y0=5)]
    want = G.adjacency_loops(slides)
    assert _same(_adjacency(slides, True), want) and _same(_adjacency(slides, False), want)


@pytest.fixture(scope="module")
def dense_batch():
    """3 slides of about 2 000 nodes in one dense region: 6 000 keys that differ in few bits, so that a table of 16 384 slots has probe chains
    under any hash that spreads them (about 6 000^2 / (2 x 16 384) = 1 100 pairs land in one slot at a uniform hash)."""
    slides = [G.disc(2000, seed=1), G.disc(1999, seed=2), G.disc(2001, seed=3)]
    assert 8 in G.neighbour_counts(slides[0])
    return slides, G.adjacency_loops(slides)


def test_a_dense_batch_with_probe_chains(dense_batch):
    from wsi_hgnn_amd import ops
    slides, want = dense_batch
    assert _same(_adjacency(slides, True), want) and _same(_adjacency(slides, False), want)
    coords, sizes = G.as_tensors(slides)
    ptr = torch.tensor([0, 2000, 3999, 6000], dtype=torch.int32, device=DEV)
    index = ops.grid_index(coords.to(torch.int32).to(DEV), ptr)
    assert index.capacity == 16384 and index.flags.tolist() == [0, 0]
    keys = index.keys.cpu()
    used = keys != -1
    assert int(used.sum()) == 6000 and keys[used].unique().numel() == 6000              # every key stored once
    assert sorted(index.rows.cpu()[used].tolist()) == list(range(6000))                   # ... with its own row
    c = coords.clone()
    assert index.set_max.tolist() == [[int(c[a:b, 0].max()), int(c[a:b, 1].max())] for a, b in ((0, 2000), (2000, 3999), (3999, 6000))]
    set_of = torch.repeat_interleave(torch.arange(3), torch.tensor(sizes))
    key = (set_of << 50) | ((c[:, 0] + 1) << 25) | (c[:, 1] + 1)
    counts, _ = ops.grid_count(index, "adjacency")
    assert counts.sum().item() == want[0].numel() and counts.max().item() == 8
    assert set(keys[used].tolist()) == set(key.tolist())                                  # the documented key layout


def test_identical_calls_give_identical_outputs(dense_batch):
    from wsi_hgnn_amd import h2mil
    slides, _ = dense_batch
    a, b = _adjacency(slides, True), _adjacency(slides, True)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    trees = [_to_dev(G.rich_tree(16, 16, seed=1)), _to_dev(G.small_tree())]
    p, q = h2mil.from_grid(trees, kernels=True), h2mil.from_grid(trees, kernels=True)
    G.same_batches(p, q)


def _to_dev(slide):
    return {k: v.to(DEV) for k, v in slide.items()}


TREES = {"small": lambda: [G.small_tree()],
         "unequal batch": lambda: [G.rich_tree(6, 5, seed=0), G.small_tree(seed=1), G.zero_max_tree(), G.random_tree(2, 9, seed=4, origin=(G.LIMIT - 24, 3))],
         "several blocks": lambda: [G.rich_tree(16, 16, seed=1), G.rich_tree(23, 22, seed=2), G.small_tree(seed=2)]}


@pytest.mark.parametrize("name", sorted(TREES))
def test_tree_kernels_equal_the_loops_and_the_tensor_formulation(name):
    from wsi_hgnn_amd import h2mil
    slides = TREES[name]()
    want = h2mil.from_slides([G.restated(s) for s in slides])
    on_dev = [_to_dev(s) for s in slides]
    for kernels in (True, None, False):
        got = h2mil.from_grid(on_dev, kernels=kernels)
        assert got.edge_index.is_cuda and got.x_y_index.dtype == torch.float64
        G.same_batches(got, want)
    if name == "several blocks":
        assert 2 * sum(want.n1) + sum(want.n2) > 3 * 256


@pytest.mark.parametrize("n1", [1, 255, 256, 257])
def test_trees_at_sizes_around_the_block(n1):
    """A row of ``n1`` level-1 cells in shuffled order; cell i covers the level-2 columns 2i and 2i + 1 in the rows 0 and 1, and row 1 has its
    even columns only: 3 children each."""
    from wsi_hgnn_amd import h2mil
    g = torch.Generator().manual_seed(n1)
    coords1 = [(i, 0) for i in torch.randperm(n1, generator=g).tolist()]
    cover = [(2 * i, 2 * i + 1, 0, 1) for i, _ in coords1]
    cells = [(x, 0) for x in range(2 * n1)] + [(x, 1) for x in range(0, 2 * n1, 2)]
    coords2 = [cells[i] for i in torch.randperm(len(cells), generator=g).tolist()]
    s = G._slide(coords1, cover, coords2, 4, n1)
    assert set(G.children_counts(cover, coords2)) == {3} and set(G.cover_counts(cover, coords2)) == {1}
    other = G.small_tree(feat=4)
    want = h2mil.from_slides([G.restated(s), G.restated(other)])
    G.same_batches(h2mil.from_grid([_to_dev(s), _to_dev(other)], kernels=True), want)


def test_flag_paths_raise_and_leave_the_process_usable():
    from wsi_hgnn_amd import construct
    t = lambda rows, w=2: torch.tensor(rows, dtype=torch.int64, device=DEV).reshape(-1, w)
    good = G.full_grid(5, 7, seed=1)
    want = G.adjacency_loops([good])
    for bad, what in (([(1, 1), (2, 2), (1, 1)], "repeated"), ([(0, 0), (-1, 0)], "outside 0 <= c < 2\\^24"), ([(0, G.LIMIT), (0, 0)], "outside 0 <= c < 2\\^24"),
                      ([(0, 0), (2 ** 40, 0)], "outside 0 <= c < 2\\^24")):
        with pytest.raises(ValueError, match=what):
            construct.grid_adjacency(t(bad), [len(bad)], kernels=True)
        assert _same(construct.grid_adjacency(t(good), [len(good)], kernels=True), want)           # the next call succeeds
    assert construct.grid_adjacency(t([(1, 1), (2, 2), (1, 1)]), [2, 1], kernels=True)[0].tolist() == [0, 1]
    ok = ([(0, 0), (1, 0)], [(0, 1, 0, 1), (2, 3, 0, 1)], [(0, 0), (3, 1)])
    tree = lambda c1, cv, c2: construct.slide_trees(t(c1), t(cv, 4), t(c2), [len(c1)], [len(c2)], kernels=True)
    assert tree(*ok)[2].tolist() == [-1, 0, 0, 1, 2]
    for args, what in (((ok[0], ok[1], ok[2] + [(5, 5)]), "no level-1 node covers"), (([(0, 0), (0, 0)], ok[1], ok[2]), "repeated"),
                       ((ok[0], ok[1], [(0, 0), (0, 0)]), "repeated"), (([(0, 0), (-1, 0)], ok[1], ok[2]), "outside 0 <= c < 2\\^24")):
        with pytest.raises(ValueError, match=what):
            tree(*args)
        assert tree(*ok)[0].shape[1] == 10
    assert tree(ok[0], [(0, 1, 0, 1), (-5, 3, 0, 1)], ok[2])[0].shape[1] == 10
