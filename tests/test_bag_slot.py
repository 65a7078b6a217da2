"""Patch dropout and bag slots without a GPU: the row counts against the fixture recorded from the reference's own ``dropout_patches``
(tests/golden/mil/reference_dropout_patches.json), the properties and the distribution of the project's draw in its tensor formulation,
the tie rule at 3 key bits against the pure-Python restatement of tests/bag_slot_cases.py, the tables of a ``BagSlot`` filled on the CPU, and
the argument errors of the new C entry points."""
import itertools
import json
import math
import os

import pytest
import torch

import bag_slot_cases as BC

HERE = os.path.dirname(os.path.abspath(__file__))


def _fixture():
    return json.load(open(os.path.join(HERE, "golden", "mil", "reference_dropout_patches.json")))["cases"]


def test_patch_counts_against_the_reference_fixture():
    from wsi_hgnn_amd import mil
    cases = _fixture()
    grid = {(c["n"], c["p"]) for c in cases}
    assert all((n, p) in grid for n in BC.SIZES for p in BC.RATES)
    assert {(100, 0.29), (7, 0.6), (1, 0.5)} <= grid
    for c in cases:
        if c["rows"] is None:
            with pytest.raises(ValueError):
                mil.patch_counts(c["n"], c["p"])
        else:
            k, m = mil.patch_counts(c["n"], c["p"])
            assert k + m == c["rows"] and 0 <= m <= k <= c["n"], c
    assert mil.patch_counts(100, 0.29) == (71, 28)            # not the 71 + 29 of exact arithmetic
    assert mil.patch_counts(1, 0.5) == (0, 0)                 # an empty bag is legal
    with pytest.raises(ValueError, match="larger sample"):
        mil.patch_counts(7, 0.6)                              # 2 kept, 4 to repeat


@pytest.mark.parametrize("key_bits", [32, 3])
@pytest.mark.parametrize("p", BC.RATES)
def test_tensor_formulation_properties(p, key_bits):
    from wsi_hgnn_amd import mil
    sizes = list(BC.SIZES)
    draws = BC.draws_for(sizes)
    x = torch.arange(sum(sizes), dtype=torch.float32).view(-1, 1).repeat(1, 3)       # a row's value is its global number
    rows, new_sizes, sel = mil.dropout_patches_tensor(x, sizes, p, draws, key_bits)
    assert sel.dtype == torch.int32 and rows.shape == (sum(new_sizes), 3)
    o_in, o_out = 0, 0
    for n, d, ns in zip(sizes, draws, new_sizes):
        k, m = mil.patch_counts(n, p)
        assert ns == k + m
        s = sel[o_out:o_out + ns].tolist()
        kept, pads = s[:k], s[k:]
        assert all(0 <= i < n for i in s)
        assert kept == sorted(set(kept)) and len(kept) == k                           # distinct rows of the bag, ascending
        assert pads == sorted(set(pads)) and len(pads) == m and set(pads) <= set(kept)
        assert rows[o_out:o_out + ns, 0].tolist() == [float(o_in + i) for i in s]     # the rows of the same bag
        assert s == BC.python_selection(n, k, m, d, key_bits)                         # (at 3 bits: the lower row wins nearly every comparison)
        # a bag's result does not depend on the bags around it
        alone = mil.dropout_patches_tensor(x[o_in:o_in + n], [n], p, [d], key_bits)[2].tolist()
        assert alone == s
        o_in, o_out = o_in + n, o_out + ns
    if p == 0:
        assert torch.equal(rows, x)


def test_ties_at_three_key_bits_go_to_the_lower_row():
    from wsi_hgnn_amd import mil
    from wsi_hgnn_amd.mil import slots
    n, p, d = 300, 0.25, 77
    keys = slots.patch_keys(torch.arange(n), d, False, 3)
    assert int(keys.max()) <= 7 and len(set(keys.tolist())) <= 8                       # 300 rows share 8 keys
    sel = mil.dropout_patches_tensor(torch.zeros(n, 1), [n], p, [d], 3)[2].tolist()
    k, m = mil.patch_counts(n, p)
    assert sel == BC.python_selection(n, k, m, d, 3)
    kept = sel[:k]
    edge = max(int(keys[i]) for i in kept)                                              # the threshold key: its rows are taken lowest first
    tied = [i for i in range(n) if int(keys[i]) == edge]
    taken = [i for i in tied if i in set(kept)]
    assert taken == tied[:len(taken)] and 0 < len(taken)


def test_keys_match_the_host_hash():
    from wsi_hgnn_amd import ops
    from wsi_hgnn_amd.mil import slots
    for d in (0, 1, 0xdeadbeef, 0xffffffff):
        for second in (False, True):
            got = slots.patch_keys(torch.arange(50), d, second).tolist()
            s = ops._fmix32(d ^ 0x85EBCA6B) if second else ops._fmix32(d)
            assert got == [ops._fmix32(i * 0x9E3779B1 + s) for i in range(50)]


def test_distribution_of_the_draw():
    """n = 12, p = 0.25 (9 kept, 3 repeated) over the draws 0 .. 3999: how often a row is kept, how often it is repeated and how often a pair
    of rows is kept together, each within 4 sigma of its binomial mean."""
    from wsi_hgnn_amd import mil
    n, p, T = 12, 0.25, 4000
    k, m = mil.patch_counts(n, p)
    assert (k, m) == (9, 3)
    keep = torch.zeros(n)
    pad = torch.zeros(n)
    pair = torch.zeros(n, n)
    x = torch.zeros(n, 1)
    for d in range(T):
        sel = mil.dropout_patches_tensor(x, [n], p, [d])[2].to(torch.int64)
        kept = torch.zeros(n)
        kept[sel[:k]] = 1
        keep += kept
        pad[sel[k:]] += 1
        pair += kept.view(-1, 1) * kept.view(1, -1)
    worst = {}
    for name, counts, q in (("keep", keep.tolist(), k / n), ("pad", pad.tolist(), m / n),
                            ("pair", [float(pair[a, b]) for a, b in itertools.combinations(range(n), 2)], k * (k - 1) / (n * (n - 1)))):
        sigma = math.sqrt(T * q * (1 - q))
        worst[name] = max(abs(c - T * q) for c in counts) / sigma
        print(f"{name}: largest deviation {worst[name]:.2f} sigma")
    assert all(w <= 4.0 for w in worst.values()), worst


@pytest.mark.parametrize("filler", list(BC.FILLERS))
@pytest.mark.parametrize("p", [0.0, 0.25, 0.29])
@pytest.mark.parametrize("feats", BC.FEATS)
def test_bag_slot_tables_on_the_cpu(feats, p, filler):
    from wsi_hgnn_amd import mil
    cap = max(BC.row_cap(sizes, filler) for sizes in BC.BATCHES)
    slot = mil.BagSlot(feats, cap, BC.BAG_CAP, num_classes=2, device="cpu", dropout_patch=p, seed=5)
    for r, sizes in enumerate(BC.BATCHES + BC.BATCHES[:1]):              # (the last load follows a larger one: the filler's rows are zero again)
        bags = BC.make_bags(sizes, feats, 40 + r)
        draws = BC.draws_for(sizes, r)
        labels = BC.LABELS[:len(sizes)]
        slot.load(bags, labels, draws)
        rows, new_sizes, _ = mil.dropout_patches_tensor(torch.cat(bags), sizes, p, draws)
        BC.check_slot_tables(slot, new_sizes, labels, rows)
    # the filler of exactly one row: the tightest batch fills the slot to its last row but one
    tight = max(BC.BATCHES, key=sum)
    if filler == "one_row":
        assert sum(tight) + 1 == slot.row_cap and slot.fits(tight)


def test_bag_slot_default_draws_follow_the_load_counter():
    from wsi_hgnn_amd import data, mil
    a = mil.BagSlot(8, 200, 2, device="cpu", dropout_patch=0.25, seed=9)
    b = mil.BagSlot(8, 200, 2, device="cpu", dropout_patch=0.25, seed=9)
    bags = BC.make_bags((100, 60), 8, 3)
    for counter in range(3):
        a.load(bags, [0, 1])
        b.load(bags, [0, 1], draws=[data.augment_draw(9, counter, 0), data.augment_draw(9, counter, 1)])
        assert torch.equal(a.rows, b.rows)
        if counter:
            assert not torch.equal(a.rows, first)
        first = a.rows.clone()


def test_bag_slot_fits_edges():
    from wsi_hgnn_amd import mil
    slot = mil.BagSlot(4, 257, bag_cap=2, device="cpu")
    assert slot.fits([256]) and not slot.fits([257])                     # one row is left for the filler
    assert slot.fits([128, 128]) and slot.fits([0, 0]) and slot.fits([0])
    assert not slot.fits([]) and not slot.fits([1, 1, 1])                # no bag; more bags than bag_cap
    assert slot.fits([1, 255]) and not slot.fits([2, 255])
    with pytest.raises(ValueError, match="does not fit"):
        slot.load([torch.zeros(257, 4)], [0])
    with pytest.raises(ValueError, match="labels"):
        slot.load([torch.zeros(3, 4)], [0, 1])
    with pytest.raises(ValueError):
        mil.BagSlot(4, 100, dropout_patch=0.6, device="cpu")
    # the undropped sizes decide: a batch that would fit only after dropping does not fit
    drop = mil.BagSlot(4, 257, bag_cap=1, device="cpu", dropout_patch=0.25)
    assert not drop.fits([257]) and drop.fits([256])


def test_bag_loss_with_device_side_weights():
    """``bag_loss(weights=, targets=)`` is the weighted sum of the per-bag losses; with a slot's tables it is the loss of the real bags."""
    from wsi_hgnn_amd import mil
    torch.manual_seed(3)
    pred = torch.randn(4, 2)
    labels = [1, 0, 2]
    slot = mil.BagSlot(4, 50, bag_cap=3, num_classes=2, device="cpu")
    slot.load([torch.zeros(5, 4), torch.zeros(0, 4), torch.zeros(7, 4)], labels)
    got = mil.bag_loss(pred, None, 2, "abmil", slot.plan, weights=slot.weights, targets=slot.targets)
    want = mil.bag_loss(pred[:3], labels, 2, "abmil", mil.bag_plan([5, 0, 7], "cpu"))
    assert abs(float(got) - float(want)) < 1e-6
    with pytest.raises(ValueError, match="come together"):
        mil.bag_loss(pred, labels, 2, "abmil", slot.plan, weights=slot.weights)


def test_new_entry_points_reject_bad_arguments_without_a_gpu():
    """Arguments are checked on the host before any launch: with values that must be rejected no kernel runs and no GPU is needed."""
    from wsi_hgnn_amd import _native as N
    lib = N.load()
    assert lib.wsi_abi_version() == 26
    err = lambda: lib.wsi_last_error().decode()
    EINVAL, P = -22, 4096                       # P: a non-null address that is never dereferenced
    sel = lambda desc=P, nb=2, bits=32, out=P, rows=10: lib.wsi_bag_dropout_select(desc, nb, bits, out, rows, None)
    for bits in (0, -1, 33):
        assert sel(bits=bits) == EINVAL and "bad argument" in err()
    assert sel(nb=-1) == EINVAL and sel(rows=-1) == EINVAL
    assert sel(desc=None) == EINVAL and "null pointer" in err()
    assert sel(out=None) == EINVAL and "null pointer" in err()
    assert sel(nb=0) == 0 and sel(rows=0) == 0                            # nothing to do
    fill = lambda desc=P, nb=2, s=P, rows=P, ld=8, feats=8, n=10, seg=P, src=P, dst=P, words=4: lib.wsi_bag_slot_fill(
        desc, nb, s, rows, ld, feats, n, seg, 2, src, dst, words, None)
    assert fill(feats=0) == EINVAL and "bad argument" in err()
    assert fill(ld=7) == EINVAL and fill(nb=-1) == EINVAL and fill(n=-1) == EINVAL and fill(words=-1) == EINVAL
    assert fill(n=1 << 31) == EINVAL
    for null in ("desc", "rows", "src", "dst"):
        assert fill(**{null: None}) == EINVAL and "null pointer" in err(), null
    assert fill(nb=0, desc=None, n=0, rows=None, words=0, src=None, dst=None) == 0


def test_ops_refuse_cpu_tensors_and_bad_counts():
    from wsi_hgnn_amd import mil, ops
    x = torch.zeros(10, 4)
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.bag_dropout_rows([x], [(7, 2)], [1])
    with pytest.raises(RuntimeError, match="GPU only"):
        mil.dropout_patches(x, [10], 0.25, kernels=True)
    with pytest.raises(ValueError, match="cannot keep"):
        ops.bag_descriptors([x], [(11, 0)], [1], 4)
    with pytest.raises(ValueError, match="cannot keep"):
        ops.bag_descriptors([x], [(4, 5)], [1], 4)
    rows, plan = mil.dropout_patches(x, [4, 6], 0.25, draws=[3, 4])                    # the CPU route: the tensor formulation
    assert rows.shape[0] == plan.num_rows == sum(sum(mil.patch_counts(n, 0.25)) for n in (4, 6))
    same, plan0 = mil.dropout_patches(x, [4, 6], 0.0)
    assert same is x and plan0.num_rows == 10
