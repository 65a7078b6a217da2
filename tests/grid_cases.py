"""Cases and loop restatements for the slide graphs built from patch grids (construct.grid_adjacency / construct.slide_trees).

The reference's own scripts cannot be run to record fixtures (build_graphs.py imports torchvision, pandas and cl and calls .cuda();
github_pretreat.py is a script with hard-wired paths, joblib and torch_geometric), so the rules are restated here as plain loops with
dictionaries over integer tuples, written from the statement of the rules (include/wsi_hgnn.h) and not carried over from the
reference's files.  Every builder asserts what makes its case worth running, so a case that loses its point fails the test that uses it.
"""
import numpy as np
import torch

NB8 = ((0, 1), (0, -1), (1, 0), (-1, 0), (1, 1), (-1, 1), (1, -1), (-1, -1))
LIMIT = 1 << 24


# ------------------------------------------------------------------------------------------------ GTNMIL
def dense_adjacency(points):
    """The reference's rule as its double loop: a float64 n x n matrix, 1 where two nodes are at most one step apart in x and in y."""
    n = len(points)
    adj = np.zeros((n, n))
    for i in range(n - 1):
        for j in range(i + 1, n):
            if abs(points[i][0] - points[j][0]) <= 1 and abs(points[i][1] - points[j][1]) <= 1:
                adj[i][j] = 1
                adj[j][i] = 1
    return adj


def adjacency_loops(slides):
    """(row, col) int64 for a batch of slides (each a list of (x, y)): per node the other nodes of its slide at most one step away, rows
    ascending, the columns of a row ascending, global row numbers.  A dictionary per slide; linear in the number of nodes."""
    rows, cols, off = [], [], 0
    for points in slides:
        at = {}
        for i, p in enumerate(points):
            assert tuple(p) not in at, "a repeated coordinate"
            at[tuple(p)] = i
        for i, (x, y) in enumerate(points):
            hits = sorted(at[(x + dx, y + dy)] for dx in (-1, 0, 1) for dy in (-1, 0, 1) if (dx or dy) and (x + dx, y + dy) in at)
            rows += [off + i] * len(hits)
            cols += [off + j for j in hits]
        off += len(points)
    return torch.tensor(rows, dtype=torch.int64), torch.tensor(cols, dtype=torch.int64)


def neighbour_counts(points):
    at = set(map(tuple, points))
    return [sum((x + dx, y + dy) in at for dx, dy in NB8) for x, y in points]


def _shuffled(points, seed):
    g = torch.Generator().manual_seed(seed)
    return [points[i] for i in torch.randperm(len(points), generator=g).tolist()]


def full_grid(w, h, seed=0):
    """Every cell of a w x h grid, shuffled.  It has 2((w-1)h + w(h-1) + 2(w-1)(h-1)) entries."""
    pts = _shuffled([(x, y) for x in range(w) for y in range(h)], seed)
    c = neighbour_counts(pts)
    assert sum(c) == 2 * ((w - 1) * h + w * (h - 1) + 2 * (w - 1) * (h - 1))
    assert (w < 3 or h < 3) or 8 in c, "no node with all 8 neighbours"
    assert any(x == 0 for x, _ in pts) and any(y == 0 for _, y in pts)
    return pts


def holed_grid(w, h, removed, seed):
    """A w x h grid with the fraction ``removed`` of its cells taken out, shuffled; must keep a node with all 8 neighbours, one with none and a
    node at coordinate 0 in x and one in y."""
    g = torch.Generator().manual_seed(seed)
    cells = [(x, y) for x in range(w) for y in range(h)]
    order = torch.randperm(len(cells), generator=g).tolist()
    pts = [cells[i] for i in order[int(round(removed * len(cells))):]]
    c = neighbour_counts(pts)
    assert 8 in c, "no node with all 8 neighbours"
    assert 0 in c, "no node without neighbours"
    assert any(x == 0 for x, _ in pts) and any(y == 0 for _, y in pts), "no node at coordinate 0"
    return pts


def disc(n, seed, x0=0, y0=0):
    """The ``n`` grid cells nearest to a centre (a filled disc), shifted so that the smallest coordinates are (x0, y0), shuffled."""
    r = int(np.ceil(np.sqrt(n / np.pi))) + 2
    cells = sorted(((x * x + y * y, x, y) for x in range(-r, r + 1) for y in range(-r, r + 1)))[:n]
    assert len(cells) == n
    mx, my = min(c[1] for c in cells), min(c[2] for c in cells)
    return _shuffled([(x - mx + x0, y - my + y0) for _, x, y in cells], seed)


HOLED_SEED = 7          # the first seed at which the 9 x 9 grid with 40 % removed keeps all the properties holed_grid asserts


def gtn_cases():
    """{name: list of slides}: the cases of the issue, each slide in shuffled node order."""
    one = [(3, 5)]
    assert neighbour_counts(one) == [0]
    full = full_grid(5, 7, seed=1)
    assert sum(neighbour_counts(full)) == 212
    holed = holed_grid(9, 9, 0.4, seed=HOLED_SEED)
    same = full_grid(4, 3, seed=2)
    return {"one node": [one], "full 5 x 7": [full], "9 x 9 with holes": [holed],
            "three slides with identical coordinates": [same, list(same), list(same)],
            "unequal slides": [one, holed, full, [(0, 0), (LIMIT - 1, LIMIT - 1), (LIMIT - 2, LIMIT - 1), (0, 1)]]}


def as_tensors(slides):
    """(packed int64 [N, 2], sizes)."""
    return torch.tensor([p for s in slides for p in s], dtype=torch.int64).reshape(-1, 2), [len(s) for s in slides]


# ------------------------------------------------------------------------------------------------ H2MIL
def tree_loops(coords1, cover, coords2):
    """One slide's tensors as the reference makes them, with LOCAL rows: the root is row 0, then the level-1 nodes, then the level-2 nodes."""
    n1, n2 = len(coords1), len(coords2)
    at1, at2 = {}, {}
    for r, p in enumerate(coords1):
        assert tuple(p) not in at1, "a repeated level-1 coordinate"
        at1[tuple(p)] = 1 + r
    for r, p in enumerate(coords2):
        assert tuple(p) not in at2, "a repeated level-2 coordinate"
        at2[tuple(p)] = 1 + n1 + r
    src, dst = [], []
    tree = [-1] + [0] * n1 + [-2] * n2
    for r, (a, b, c, d) in enumerate(cover):                   # section A
        me = 1 + r
        src += [me, 0]
        dst += [0, me]
        for child in ((a, c), (b, c), (a, d), (b, d)):
            if child in at2:
                src += [me, at2[child]]
                dst += [at2[child], me]
                tree[at2[child]] = me                          # a later level-1 node overwrites an earlier one
    for points, at in ((coords1, at1), (coords2, at2)):       # sections B and C
        for x, y in points:
            for dx, dy in NB8:
                if (x + dx, y + dy) in at:
                    src.append(at[(x, y)])
                    dst.append(at[(x + dx, y + dy)])
    xy = np.zeros((1 + n1 + n2, 2), dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        for lo, points in ((1, coords1), (1 + n1, coords2)):
            p = np.asarray(points, dtype=np.float64).reshape(-1, 2)
            xy[lo:lo + len(points)] = p / p.max(0)
    return {"edge_index_tree_8nb": torch.tensor([src, dst], dtype=torch.int64).reshape(2, -1),
            "node_type": torch.tensor([0] + [1] * n1 + [2] * n2, dtype=torch.int64), "node_tree": torch.tensor(tree, dtype=torch.int64),
            "x_y_index": torch.from_numpy(xy)}


def children_counts(cover, coords2):
    at2 = set(map(tuple, coords2))
    return [sum(k in at2 for k in ((a, c), (b, c), (a, d), (b, d))) for a, b, c, d in cover]


def cover_counts(cover, coords2):
    """How many level-1 nodes cover every level-2 node."""
    return [sum((x in (a, b)) and (y in (c, d)) for a, b, c, d in cover) for x, y in coords2]


def _slide(coords1, cover, coords2, feat, seed):
    g = torch.Generator().manual_seed(1000 + seed)
    t = lambda rows, w: torch.tensor(rows, dtype=torch.int64).reshape(-1, w)
    return {"x": torch.randn(1 + len(coords1) + len(coords2), feat, generator=g), "coords1": t(coords1, 2), "cover": t(cover, 4),
            "coords2": t(coords2, 2)}


def small_tree(feat=6, seed=0):
    """A 3 x 2 level-1 grid with a hole, covers of 2 x 2 level-2 cells with some cells missing: a level-1 node with 4 children, one with none,
    a name with a == b (its child is emitted twice), level-2 nodes covered twice (the last level-1 node in order wins), a level-2 node
    without neighbours.  (Nodes with all 8 neighbours: ``rich_tree``.)"""
    level1 = {(0, 0): (0, 1, 0, 1), (1, 0): (2, 3, 0, 1), (2, 0): (6, 6, 0, 1), (0, 1): (1, 2, 1, 2), (2, 1): (8, 9, 8, 9)}
    coords2 = [(0, 0), (1, 0), (0, 1), (1, 1), (2, 0), (3, 0), (2, 1), (6, 0), (1, 2), (2, 2)]
    coords1 = _shuffled(sorted(level1), 10 + seed)
    cover = [level1[p] for p in coords1]
    coords2 = _shuffled(coords2, 20 + seed)
    kids, covered = children_counts(cover, coords2), cover_counts(cover, coords2)
    assert 0 in kids and 4 in kids, kids
    assert max(covered) >= 2 and min(covered) >= 1, covered
    assert any(a == b for a, b, _, _ in cover)
    assert (1, 1) not in level1 and len(coords1) == 5, "the level-1 grid has a hole"
    assert 0 in neighbour_counts(coords2), "no node without neighbours"
    assert any(x == 0 for x, _ in coords1) and any(y == 0 for _, y in coords1) and any(x == 0 for x, _ in coords2) and any(y == 0 for _, y in coords2)
    return _slide(coords1, cover, coords2, feat, seed)


def random_tree(w, h, feat=6, seed=0, keep1=0.9, keep2=0.9, origin=(0, 0)):
    """A w x h level-1 grid with cells missing; cell (i, j) covers the level-2 columns 2i and 2i + 1 + e and rows 2j and 2j + 1 + f with e, f
    drawn from {0 (6 times in 8), +1, -1} (+1 reaches into the neighbour's cells: double cover; -1 gives a == b); the level-2 nodes are a random part of
    the covered cells.  Both levels shuffled."""
    g = torch.Generator().manual_seed(seed)
    draw = lambda n: torch.rand(n, generator=g).tolist()
    cells = [(i, j) for i in range(w) for j in range(h)]
    cells = [c for c, u in zip(cells, draw(len(cells))) if u < keep1] or [(0, 0)]
    jitter = torch.tensor([0, 0, 0, 0, 0, 0, 1, -1])[torch.randint(0, 8, (len(cells), 2), generator=g)].tolist()
    ox, oy = origin
    cover = {(i, j): (2 * i + ox, 2 * i + 1 + e + ox, 2 * j + oy, 2 * j + 1 + f + oy) for (i, j), (e, f) in zip(cells, jitter)}
    covered = sorted({(x, y) for a, b, c, d in cover.values() for x in (a, b) for y in (c, d)})
    coords2 = [p for p, u in zip(covered, draw(len(covered))) if u < keep2] or covered[:1]
    coords1 = _shuffled(cells, seed + 1)
    coords2 = _shuffled(coords2, seed + 2)
    return _slide(coords1, [cover[p] for p in coords1], coords2, feat, seed)


def rich_tree(w, h, feat=6, seed=0):
    """``random_tree`` at a seed whose case has all the properties: children counts 0 and 4, a double cover, a == b, a level-2 node with all 8
    neighbours (asserted)."""
    s = random_tree(w, h, feat, seed)
    cover, c2 = [tuple(r) for r in s["cover"].tolist()], [tuple(r) for r in s["coords2"].tolist()]
    kids = children_counts(cover, c2)
    assert 4 in kids and min(kids) < 4, "children counts"
    assert max(cover_counts(cover, c2)) >= 2 and any(a == b for a, b, _, _ in cover)
    assert 8 in neighbour_counts(c2), "no level-2 node with all 8 neighbours"
    return s


def zero_max_tree(feat=6):
    """Every level-1 coordinate 0 and every level-2 x 0: the maxima are 0 and the divisions give nan (0 / 0), as numpy's do."""
    return _slide([(0, 0)], [(0, 0, 0, 1)], [(0, 1), (0, 0)], feat, 7)


def restated(slide):
    """The slide with the reference's tensors made by the loops (what ``h2mil.from_slides`` takes)."""
    lists = [[tuple(r) for r in slide[k].tolist()] for k in ("coords1", "cover", "coords2")]
    return dict(tree_loops(*lists), x=slide["x"])


def same_doubles(a, b):
    """Bit-equal float64 tensors, a nan matching a nan (its sign and payload are the hardware's)."""
    a, b = a.detach().cpu(), b.detach().cpu()
    if a.dtype != torch.float64 or b.dtype != torch.float64 or a.shape != b.shape:
        return False
    nan = torch.isnan(a)
    return bool(torch.equal(nan, torch.isnan(b)) and torch.equal(a[~nan].view(torch.int64), b[~nan].view(torch.int64)))


def same_batches(got, want):
    """Field by field: what ``h2mil.from_grid`` built against ``h2mil.from_slides`` of the restated tensors."""
    assert got.sizes == want.sizes and got.n1 == want.n1 and got.n2 == want.n2
    assert torch.equal(got.x.cpu(), want.x.cpu())
    for name in ("node_type", "tree", "edge_index", "parent1", "roots", "idx1", "idx2"):
        a, b = getattr(got, name).cpu(), getattr(want, name).cpu()
        assert a.dtype == b.dtype and torch.equal(a, b), name
    assert same_doubles(got.x_y_index, want.x_y_index), "x_y_index"
