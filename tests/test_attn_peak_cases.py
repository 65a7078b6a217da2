"""What tests/attn_peak_cases.py claims, held without a GPU: the scores are exact in fp32 under any summation order; the graph and the pattern
placement have every property the GPU tests rely on; the float64 restatement equals autograd; the fp32 emulation in kernel order stays under a
quarter of every bound in every block (so a block over its bound on the GPU is a wrong kernel, not rounding); and the cases DISCRIMINATE - a hub
merge with part 0's maximum and a softmax without a maximum break the bounds on these inputs and pass them all on the inputs every other test of
these kernels uses (0.5 randn, 0.7, 0.3).  That last result is the gap these cases close."""
import math

import pytest
import torch

import attn_peak_cases as C

W = C.Worst()
CHECKED = ("t", "a", "lse", "g_q", "g_k", "g_v", "g_e")
CASES = [("heat", D, H) for D, H in C.CONFIGS] + [("hgt",) + C.HGT_DH]
EXACT = [(layout, D, H) for layout, D, H in CASES if C.exact(D, H)]


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    W.report("fp32 emulation on the CPU")


def _got(em):
    return {k: em[k] for k in CHECKED}


def test_the_configurations_are_the_ones_the_kernels_dispatch_on():
    assert len(C.CONFIGS) == 10 and [dh for dh in C.CONFIGS if not C.exact(*dh)] == [(512, 4)]
    assert all(D in (128, 256, 512) and 64 % H == 0 for D, H in C.SPECIALISED) and all(D not in (128, 256, 512) for D, H in C.GENERIC)
    assert {C.light_unroll(D) for D, _ in C.SPECIALISED} == {2, 4}


def test_the_graph_has_the_properties_the_gpu_tests_rely_on():
    c = C.graph_case()
    facts = c.facts()
    assert set(facts) == set(C.FACTS)
    assert all(facts.values()), {k: v for k, v in facts.items() if not v}
    for name in ("src", "rowptr", "node_seg", "colptr", "csc_eid", "csc_dst", "inv_rd"):
        assert torch.equal(getattr(c.plan, name), getattr(c.hub_plan, name)), name
    assert c.hub_plan.heavy_degree == C.HUB_DEGREE and c.plan.num_src_rows == c.n
    # HGT's layout: the same CSR, K|V rows per (relation, source node)
    for name in ("rowptr", "node_seg"):
        assert torch.equal(getattr(c.plan, name), getattr(c.rel_plan, name)), name
    assert c.rel_plan.num_src_rows > c.n


@pytest.mark.parametrize("layout,D,H", CASES)
def test_the_patterns_are_where_they_are_said_to_be(layout, D, H):
    facts = C.pattern_facts(D, H, layout)
    seen = facts.pop("patterns_seen")
    assert all(facts.values()), {k: v for k, v in facts.items() if not v}
    want = {"peak", "plateau_hi"} if layout == "hgt" else {"peak", "tie", "plateau_hi", "plateau_lo", "stairs_up", "stairs_down", "negative_ea"}
    assert seen - {"ordinary"} == want and (H == 1 or "ordinary" in seen)
    x = C.inputs(D, H, layout)
    assert float(x["ew"]) == (0.0 if layout == "hgt" else 0.5) and float(x["eb"]) == 0.25 and float(x["sim"].abs().max()) <= 1.0


@pytest.mark.parametrize("layout,D,H", EXACT)
def test_the_fp32_scores_are_exact_under_any_summation_order(layout, D, H):
    ref = C.evaluate(D, H, layout)["score"]
    for name, s in C.summation_orders(D, H, layout).items():
        assert torch.equal(s.double(), ref), name
    assert torch.equal(C.emulate(D, H, layout)["score"].double(), ref)


@pytest.mark.parametrize("layout,D,H", CASES)
def test_the_restatement_equals_autograd(layout, D, H):
    ev, ag = C.evaluate(D, H, layout), C.autograd(D, H, layout)
    for name in ("t", "g_q", "g_k", "g_v", "g_e"):
        rel = ((ev[name] - ag[name]).abs().max() / ag[name].abs().max().clamp(min=1e-300)).item()
        assert rel < 1e-10, (name, rel)
    c = C.graph_case()
    sums = C._segment_sum(ev["a"], c.seg, c.S)[c.seg_len > 0]
    assert float((sums - 1.0).abs().max()) < 1e-12


@pytest.mark.parametrize("hub", [False, True])
@pytest.mark.parametrize("layout,D,H", CASES)
def test_fp32_in_kernel_order_stays_under_a_quarter_of_every_bound(layout, D, H, hub):
    ref, em = C.evaluate(D, H, layout), C.emulate(D, H, layout, hub=hub)
    label = f"{layout} D={D} H={H} {'hub' if hub else 'plain'}"
    W.hold(C.ratios(_got(em), ref, D, H, hub, layout), label, limit=0.25)
    # the GPU module's own check of the probabilities, |sum a - 1| <= 4 * 2^-23 max(1, |lse|): fp32 takes 0.31 .. 0.42 of it, in the CONTROL
    # segments (|lse| of 1 .. 3, where the bound is four ulps of 1 for a sum of up to 40 rounded terms) - held at half
    W.hold({"sum a": C.sum_a_ratio(em["a"], ref)}, label, limit=0.5)


@pytest.mark.parametrize("D,H", C.CONFIGS)
def test_the_g_e_term_is_what_the_saved_lse_costs(D, H):
    """Under the plain 1e-4 max(1, |ref|) the emulation's g_e is over the bound at six of the ten configurations ((256, 1): 29 times) - with lse kept in
    float64 and everything else as before it is under it at all of them.  The derived term (attn_peak_cases.evaluate) covers the first and is
    not needed for the second."""
    ref = C.evaluate(D, H)
    fp32 = C.ratios({"g_e": C.emulate(D, H, hub=True)["g_e"]}, ref, D, H, True, g_e_term=False)["g_e"]
    fp64 = C.ratios({"g_e": C.emulate(D, H, hub=True, lse_dtype=torch.float64)["g_e"]}, ref, D, H, True, g_e_term=False)["g_e"]
    print(f"D={D} H={H}: g_e error / plain bound {fp32:.3f} with lse in fp32, {fp64:.3f} with lse in float64")
    assert fp64 <= 1.0
    if (D, H) in ((64, 1), (256, 1), (512, 2), (128, 2)):
        assert fp32 > 1.0 and fp32 > 4 * fp64


def _broken(blocks):
    return {b for b, v in blocks.items() if not v <= 1.0}


@pytest.mark.parametrize("layout,D,H", CASES)
def test_a_merge_with_part_0s_maximum_breaks_the_hub_blocks(layout, D, H):
    ref, em = C.evaluate(D, H, layout), C.emulate(D, H, layout, hub=True, max_rule="first_part")
    ar = C.all_ratios(_got(em), ref, D, H, True, layout)
    for name in ("t", "a"):
        bad = _broken(ar[name])
        want = {f"patterned hub head {h}" for h in range(H)}
        assert want <= bad, (name, sorted(want - bad))
        assert not any("light" in b for b in bad), (name, sorted(bad))          # one-wave destinations never merge


@pytest.mark.parametrize("layout,D,H", CASES)
def test_a_softmax_without_a_maximum_breaks_every_patterned_block(layout, D, H):
    ref, em = C.evaluate(D, H, layout), C.emulate(D, H, layout, hub=True, max_rule="none")
    ar = C.all_ratios(_got(em), ref, D, H, True, layout)
    for name in ("t", "a"):
        bad = _broken(ar[name])
        want = {f"patterned {part} head {h}" for h in range(H) for part in ("hub", "light")}
        assert want <= bad, (name, sorted(want - bad))
    assert not math.isfinite(max(ar["lse"].values())) or max(ar["lse"].values()) > 1.0


@pytest.mark.parametrize("rule", ["first_part", "none"])
@pytest.mark.parametrize("D,H", C.CONFIGS)
def test_at_the_old_score_scale_both_mutants_pass_every_bound(D, H, rule):
    """The gap: on K|Q = 0.5 randn, e_weight 0.7, e_bias 0.3 - the inputs of every other test of these kernels - on this very graph, neither
    mutant leaves a single block over its bound."""
    ref, em = C.evaluate(D, H, "old"), C.emulate(D, H, "old", hub=True, max_rule=rule)
    rs = C.ratios(_got(em), ref, D, H, True, "old")
    assert all(v <= 1.0 for v in rs.values()), rs
    assert float(ref["score"].abs().max()) < 20.0
