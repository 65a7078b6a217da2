"""tests/segment_tail_cases.py checked without a GPU: its float64 references against independent formulations (autograd of the gated
residual, einsum, the header's index formulas written as loops, F.cross_entropy), the exactness condition of every ``integers`` case, and
that the width, group and layout tables reach both sides of every edge they are meant to reach."""
import pytest
import torch

import segment_tail_cases as C


def test_plans_hold_the_edges_they_are_for():
    p = C.PLAN
    assert p.total_rows == 695 and p.num_segs == 11 and p.first_row == 0
    assert p.sizes[0] == p.sizes[-1] == p.sizes[8] == 0                          # empty at the start, in the middle, at the end
    assert {1, 2, 3} <= set(p.sizes) and {C.CHUNK - 1, C.CHUNK, C.CHUNK + 1} <= set(p.sizes)
    assert max(p.seg_chunk[s + 1] - p.seg_chunk[s] for s in range(p.num_segs)) == 3
    for q in (C.PLAN, C.PLAN7, C.PLAN_LONG, C.PLAN_EMPTY, C.pool_plan(3, 3), C.many_segments(40)[0]):
        assert len(q.chunk_row) == q.num_chunks + 1 and len(q.seg_chunk) == q.num_segs + 1 and q.seg_chunk[-1] == q.num_chunks
        for s, (a, b) in enumerate(q.ranges):
            cs = range(q.seg_chunk[s], q.seg_chunk[s + 1])
            assert (b == a) == (len(cs) == 0)
            if len(cs):
                assert q.chunk_row[cs[0]] == a and q.chunk_row[cs[-1] + 1] == b
            assert all(0 < q.chunk_row[c + 1] - q.chunk_row[c] <= C.CHUNK and q.chunk_seg[c] == s for c in cs)
    assert C.PLAN7.first_row == 7 and C.PLAN7.total_rows > C.PLAN7.end_row and int(C.PLAN7.live().sum()) == 695
    assert C.PLAN_EMPTY.num_chunks == 0 and C.PLAN_EMPTY.num_segs == 3
    assert max(C.PLAN_LONG.seg_chunk[s + 1] - C.PLAN_LONG.seg_chunk[s] for s in range(3)) > 64
    for T, H, Bg in C.POOL_SHAPES:
        sizes = [C.pool_plan(T, Bg, v).sizes for v in C.pool_variants(T, Bg)]
        assert all(len(s) == T * Bg for s in sizes)
        assert any(0 in s for s in sizes) and any(1 in s for s in sizes)
        assert max(sum(s) for s in sizes) <= C.WSUM_ROWS


def test_width_and_group_lists_straddle_their_edges():
    for values, edges in ((C.DOT_D, (4, 256)), (C.WSUM_D, (4, 256)), (C.GATE_D, (4, 256)), (C.POOL_D, (4, 256)), (C.WSUM_J, (16, 32))):
        for e in edges:
            assert any(v < e for v in values) and any(v > e for v in values), (values, e)
    assert {4, 256} <= set(C.DOT_D) and {4, 256} <= set(C.WSUM_D) and {16, 32} <= set(C.WSUM_J)
    assert {1, 15, 17, 33} <= set(C.WSUM_J)
    assert [T * H for T, H, _ in C.POOL_SHAPES] == [1, 16, 16, 15, 32]
    # with x_mean the ones column is weight T * H: in an open group (15, 1), alone in a new one (16, 32)
    assert {(T * H) % 16 for T, H, _ in C.POOL_SHAPES} == {0, 1, 15}
    assert set(C.GATE_D) <= set(C.DOT_D) and set(C.DOT_D_ROW7) <= set(C.DOT_D)


def test_layout_table_reaches_both_paths():
    for D in sorted(set(C.DOT_D + C.WSUM_D)):
        (o0, l0), (o4, l4), (o1, l1), (oo, lo) = (C.LAYOUTS[n](D) for n in C.X_LAYOUTS)
        assert (o0, l0) == (0, D) and C.vec_ok(o0, l0) == (D % 4 == 0)
        assert l4 % 4 == 0 and l4 >= D + 4 and C.vec_ok(o4, l4)
        assert l1 == D + 1 and C.vec_ok(o1, l1) == (D % 4 == 3)
        assert oo == 1 and lo % 4 == 0 and lo >= D and not C.vec_ok(oo, lo)
    for D in C.DOT_D:
        assert C.dot_vec("pad4", D) and not C.dot_vec("offset", D) and not C.dot_vec("mixed", D)
        assert sorted(C.dot_layouts("mixed", D)) == ["offset", "plain", "plain"]
    assert {C.dot_layouts("mixed", D).index("offset") for D in C.DOT_D} == {0, 1, 2}        # each operand is the odd one somewhere
    assert any(C.dot_vec("plain", D) for D in C.DOT_D) and any(not C.dot_vec("plain", D) for D in C.DOT_D)
    assert any(not C.dot_vec("pad1", D) and D > 4 for D in C.DOT_D)
    # the 16-byte path with a scalar tail, and the 16-byte path without one
    assert any(D % 4 and D > 4 for D in C.DOT_D) and any(D % 4 == 0 for D in C.DOT_D)


def test_embed_poisons_what_must_not_be_read():
    t = torch.arange(15, dtype=torch.float32).view(5, 3)
    live = torch.tensor([False, True, True, True, False])
    for name in C.X_LAYOUTS:
        buf, off, ld = C.embed(t, name, live)
        view = buf[off:off + 5 * ld].view(5, ld)
        assert torch.equal(view[1:4, :3], t[1:4])
        mask = torch.ones_like(buf, dtype=torch.bool)
        mask[off:off + 5 * ld].view(5, ld)[1:4, :3] = False
        assert torch.isnan(buf[mask]).all() and int(mask.sum()) == buf.numel() - 9
    w = C.embed_ld(t, 6).view(5, 6)
    assert torch.equal(w[:, :3], t) and torch.isnan(w[:, 3:]).all()


def _dot_cases():
    for D in C.DOT_D:
        yield C.PLAN, D
    for D in C.DOT_D_ROW7:
        yield C.PLAN7, D
    for D in C.DOT_D_LONG:
        yield C.PLAN_LONG, D


def test_integer_cases_are_exact_in_fp32():
    for plan, D in _dot_cases():
        g, a, b = C.dot_inputs("integers", plan, D)
        ref, scale, _ = C.dot_reference("integers", plan, D)
        assert C.exact_condition(scale), (plan.name, D)
        live = plan.live()
        terms = (g * (a - b))[live]
        assert (terms != 0).all() and terms.abs().max() <= 8 and torch.equal(terms, terms.round())
        assert torch.equal(ref, ref.round())
    plan, _ = C.many_segments(8192)
    assert C.exact_condition(C.dot_reference("integers", plan, 4)[1])
    for D in C.WSUM_D:
        for J in C.WSUM_J:
            r = C.wsum_reference("integers", C.PLAN, D, J)
            assert C.exact_condition(r["scale"]) and C.exact_condition(r["wscale"]) and torch.equal(r["out"], r["out"].round())
    assert C.exact_condition(C.wsum_reference("integers", C.PLAN, 1, 1024)["scale"])
    for T, H, Bg in C.POOL_SHAPES:
        for v in C.pool_variants(T, Bg):
            plan = C.pool_plan(T, Bg, v)
            for D in C.POOL_D:
                x, w = C.wsum_inputs("integers", plan, D, T * H)
                r = C.pool_reference(x, w, plan, T, H, Bg)
                assert C.exact_condition(r["hp_scale"]) and C.exact_condition(r["csum_scale"])
                assert (x != 0).all() and (w != 0).all()
                # the ones column: the plain sums of |x| stay below 2^24 as well
                assert float(x.double().abs().sum(dim=0).max()) < 2.0 ** 24


def test_gaussian_families_are_what_they_claim():
    g, a, b = C.dot_inputs("cancelling", C.PLAN, 257)
    assert float((a - b).abs().max()) < 1e-2 and float(a.abs().max()) > 1.0
    ref, scale, bound = C.dot_reference("gaussian", C.PLAN, 257)
    assert (scale[torch.tensor(C.PLAN.sizes) > 0] > ref.abs()[torch.tensor(C.PLAN.sizes) > 0]).all()
    assert (bound[torch.tensor(C.PLAN.sizes) == 0] == 0).all() and (ref[torch.tensor(C.PLAN.sizes) == 0] == 0).all()


def test_rounding_chains():
    assert C.n_chain_dot(0, 5) == 0 and C.n_chain_wsum(0) == 0
    assert C.n_chain_dot(1, 1) == 1 + 1 + 6 + 2 + 1 + 6
    assert C.n_chain_dot(128, 4) == 1 + 4 * 32 + 6 + 2 + 1 + 6 and C.n_chain_dot(129, 1027) == C.n_chain_dot(128, 4)
    assert C.n_chain_dot(70 * 128 + 3, 5) == 1 + 4 * 32 + 6 + 2 + 2 + 6
    assert C.n_chain_wsum(1) == 1 + 2 + 1 and C.n_chain_wsum(300) == 32 + 2 + 3


@pytest.mark.parametrize("n_gates", sorted(C.GATE_MAPS))
def test_gate_reference_is_the_gradient_of_the_gated_residual(n_gates):
    """out = s y + (1 - s) h with s = sigmoid(skip[gate of the row's segment]), loss = sum g out:  skip.grad = (1 - s) sum g (out - h)."""
    plan, D, seg_gate = C.PLAN, 5, C.GATE_MAPS[n_gates]
    gen = torch.Generator().manual_seed(11)
    g, y, h = (torch.randn(plan.total_rows, D, generator=gen, dtype=torch.float64) for _ in range(3))
    skip = C.gate_skip("randn", n_gates).double().requires_grad_(True)
    out = y.clone()                                       # seg_gate < 0: passed through
    for s, (r0, r1) in enumerate(plan.ranges):
        if seg_gate[s] >= 0:
            sg = torch.sigmoid(skip[seg_gate[s]])
            out = torch.cat([out[:r0], sg * y[r0:r1] + (1 - sg) * h[r0:r1], out[r1:]])
    (g * out).sum().backward()
    terms = g * (out.detach() - h)
    dots = torch.stack([terms[r0:r1].sum() for r0, r1 in plan.ranges])
    ref, bound, sums = C.gate_reference(dots, torch.zeros_like(dots), seg_gate, skip.detach().float(), n_gates)
    fed = sorted({gt for gt in seg_gate if gt >= 0})
    assert (skip.grad - ref).abs().max() <= 1e-12 * max(1.0, float(ref.abs().max()))
    assert all(float(ref[gt]) == 0.0 and float(bound[gt]) == 0.0 for gt in range(n_gates) if gt not in fed)


def test_gate_maps_hold_their_cases():
    sizes = C.PLAN.sizes
    for n_gates, m in C.GATE_MAPS.items():
        assert len(m) == len(sizes) and -1 in m and max(m) < n_gates
    m3, m300 = C.GATE_MAPS[3], C.GATE_MAPS[300]
    assert sum(gt == 0 for gt in m3) > 1                                          # several segments on one gate
    fed_by = lambda m, gt: [sizes[s] for s in range(len(m)) if m[s] == gt]
    assert fed_by(m3, 1) and set(fed_by(m3, 1)) == {0}                            # only empty segments feed gate 1
    assert not fed_by(m300, 2) and max(m300) >= 256                               # a gate nobody feeds; gates of the loop's second turn
    assert torch.equal(C.gate_skip("saturated", 3), torch.tensor([30.0, -30.0, 30.0]))
    assert float(1 - torch.sigmoid(torch.tensor(-100.0))) == 1.0 and float(1 - torch.sigmoid(torch.tensor(30.0))) == 0.0
    plan, seg_gate = C.many_segments(8192)
    assert plan.num_segs == 8192 and plan.num_chunks == 8192 and set(seg_gate) == {-1, 0, 1, 2}


@pytest.mark.parametrize("family", C.WSUM_FAMILIES)
def test_weighted_sum_reference_equals_einsum(family):
    plan, D, J = C.PLAN, 5, 17
    x, w = C.wsum_inputs(family, plan, D, J)
    r = C.wsum_reference(family, plan, D, J)
    seg = torch.zeros(plan.total_rows, plan.num_segs, dtype=torch.float64)
    for s, (r0, r1) in enumerate(plan.ranges):
        seg[r0:r1, s] = 1.0
    ein = torch.einsum("rs,rj,rd->sjd", seg, w.double(), x.double())
    assert (r["out"] - ein).abs().max() <= 1e-12 * max(1.0, float(ein.abs().max()))
    assert (r["ws"] - torch.einsum("rs,rj->sj", seg, w.double())).abs().max() <= 1e-12
    assert (r["scale"] >= r["out"].abs() - 1e-12).all() and (r["bound"][torch.tensor(plan.sizes) == 0] == 0).all()


@pytest.mark.parametrize("T,H,Bg", [(2, 8, 1), (4, 4, 2), (3, 5, 3)])
def test_pool_permutation_equals_the_header_formulas(T, H, Bg):
    """include/wsi_hgnn.h: hp[b * Bg + g][hh][tau][:] = sum_u w[u, b * H + hh] x[u, :] and csum[tau][b * Bg + g][hh] = sum_u w[u, b * H + hh]
    over the rows u of source segment tau * Bg + g; x_mean[tau * Bg + g] = the mean of its rows."""
    plan, D = C.pool_plan(T, Bg), 3
    x, w = C.wsum_inputs("gaussian", plan, D, T * H)
    r = C.pool_reference(x, w, plan, T, H, Bg)
    S = T * Bg
    assert r["hp"].shape == (S, H, T, D) and r["csum"].shape == (T, S, H) and r["x_mean"].shape == (S, D)
    xd, wd = x.double(), w.double()
    for tau in range(T):
        for g in range(Bg):
            r0, r1 = plan.ranges[tau * Bg + g]
            for b in range(T):
                for hh in range(H):
                    col = wd[r0:r1, b * H + hh]
                    assert (r["hp"][b * Bg + g, hh, tau] - (col.view(-1, 1) * xd[r0:r1]).sum(dim=0)).abs().max() <= 1e-12
                    assert abs(float(r["csum"][tau, b * Bg + g, hh] - col.sum())) <= 1e-12
            want = xd[r0:r1].sum(dim=0) / max(r1 - r0, 1)
            assert (r["x_mean"][tau * Bg + g] - want).abs().max() <= 1e-12
    empty = torch.tensor(plan.sizes) == 0
    assert (r["x_mean"][empty] == 0).all() and (r["x_mean_bound"][empty] == 0).all()
    ib = C.integer_mean_bound(r["x_mean"], plan)
    pow2 = torch.tensor([n in (1, 2, 128) for n in plan.sizes])
    assert (ib[pow2] == 0).all() and (ib[~pow2 & ~empty] > 0).all()


def test_cross_entropy_references_agree_and_cases_hold_their_edges():
    cases = C.ce_cases()
    for name, (x, y) in cases.items():
        B, Cc = x.shape
        assert B * Cc <= C.CE_LIMIT and y.shape == (B,) and y.dtype == torch.int64
        loss, grad = C.ce_reference(x, y)
        loss2, grad2 = C.ce_closed_form(x, y)
        assert torch.isfinite(loss) and torch.isfinite(grad).all(), name
        assert abs(float(loss - loss2)) <= 1e-12 * max(1.0, abs(float(loss))), name
        assert (grad - grad2).abs().max() <= 1e-12, name
        assert (grad[y == C.CE_IGNORE] == 0).all()
    for mag in ("80", "10000"):
        x, _ = cases[f"large{mag}"]
        assert torch.isinf(torch.exp(x)).any(dim=1).all()                         # expf of the raw logit overflows in every row
    x, y = cases["neg_inf"]
    assert int(torch.isinf(x[2]).sum()) == x.shape[1] - 1 and torch.isfinite(x[2, y[2]])
    x, y = cases["equal_maxima"]
    assert int((x[1] == x[1].max()).sum()) == 2 and int((x[4] == x[4].max()).sum()) == 2
    assert {tuple(cases[k][0].shape) for k in cases if k.startswith("limit")} == {(256, 256), (65536, 1), (1, 65536), (257, 255)}
    for B in (255, 256, 257):
        y = cases[f"ignored{B}"][1]
        assert [int(i) for i in (y == C.CE_IGNORE).nonzero().view(-1)] == [r for r in (0, 255, 256) if r < B]
    loss, grad = C.ce_reference(*cases["limit65536x1"])
    assert float(loss) == 0.0 and (grad == 0).all()
    assert all(B * Cc == C.CE_LIMIT + 1 for B, Cc in C.CE_OVER_LIMIT)
