"""The attention readout on the CPU: ``ops.attention_readout``'s tensor formulation against the numpy restatement of
tests/attn_readout_cases.py and against the composite GlobalAttentionPooling of the oracle under autograd, both in float64; and the
switch - off by default, the composite path of ``pooling.GlobalAttentionPooling`` untouched while it is off."""
import numpy as np
import pytest
import torch

import attn_readout_cases as AC

F64 = 1e-12          # x the largest entry of the block: the formulations sum the same float64 numbers in different orders


class _Graph:
    """What the readouts ask of a batched graph with one node type: the node counts of its graphs."""
    ntypes = ["n"]
    batch_size = AC.S

    def batch_num_nodes(self, ntype=None):
        return torch.tensor(AC.LENS, dtype=torch.int64)


def _plan():
    from wsi_hgnn_amd import ops
    return ops.ReducePlan.from_ptr(AC.OFF, "cpu", AC.CHUNK)


def _close(got, ref, what):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, what
    assert np.abs(got - ref).max() <= F64 * max(np.abs(ref).max(), 1e-300), (what, float(np.abs(got - ref).max()), float(np.abs(ref).max()))


def _run(fn, case):
    """out and the gradients of x, w, b under g_out, in float64 on the case's float32 inputs; ``fn(x, w, b) -> out``."""
    x, w, b, g_out = AC.inputs(case)
    x, w, b = (t.double().clone().requires_grad_(True) for t in (x, w, b))
    out = fn(x, w, b)
    out.backward(g_out.double())
    return out.detach().numpy(), x.grad.numpy(), np.concatenate([w.grad.numpy().reshape(-1), b.grad.numpy().reshape(-1)])


@pytest.mark.parametrize("case", AC.CASES, ids=AC.case_id)
def test_tensor_formulation_equals_the_restatement(case):
    from wsi_hgnn_amd import ops
    rp = _plan()
    out, g_x, g_wb = _run(lambda x, w, b: ops.attention_readout(x, w.view(1, -1), b, rp), case)
    ref = AC.restate(*AC.inputs(case))
    _close(out, ref["out"], "out")
    _close(g_x, ref["g_x"], "g_x")
    _close(g_wb, ref["g_wb"], "g_wb")
    for s, n in enumerate(AC.LENS):
        if n == 0:
            assert not out[s].any(), f"empty segment {s}"
    a, e = AC.OFF[AC.ZERO_SEG], AC.OFF[AC.ZERO_SEG + 1]
    assert not g_x[a:e].any() and not ref["g_x"][a:e].any()               # the segment without gradient: exact zeros


@pytest.mark.parametrize("case", AC.CASES, ids=AC.case_id)
def test_tensor_formulation_equals_the_composite_readout_under_autograd(case):
    from oracle import models as OM
    from wsi_hgnn_amd import ops
    rp, graph = _plan(), _Graph()

    def composite(x, w, b):
        gate_nn = lambda h: h @ w.view(-1, 1) + b                # (a Linear on the leaves of _run: the gradients go to them)
        return OM.GlobalAttentionPooling(gate_nn)(graph, x, ntype="n")

    got = _run(lambda x, w, b: ops.attention_readout(x, w.view(1, -1), b, rp), case)
    want = _run(composite, case)
    for name, g, r in zip(("out", "g_x", "g_wb"), got, want):       # (g_b, 0 up to rounding in both, is held against the scale of g_w | g_b)
        _close(g, r, name)


def test_ties_give_the_mean_and_a_missing_bias_is_zero():
    from wsi_hgnn_amd import ops
    case = (67, "ties", 67)
    x, w, b, _ = AC.inputs(case)
    out = ops.attention_readout(x.double(), w.double(), None, _plan())
    for s, (a, e) in enumerate(zip(AC.OFF[:-1], AC.OFF[1:])):
        if e > a:
            _close(out[s].numpy(), x[a:e].double().mean(0).numpy(), f"segment {s}")
    with pytest.raises(ValueError, match="gate weight"):
        ops.attention_readout(x.double(), w.double()[:-1], None, _plan())


def test_switch_is_off_by_default_and_the_composite_path_is_untouched(monkeypatch):
    """Off: ``GlobalAttentionPooling.forward`` makes exactly the calls it made before - one ``ops.linear`` and three ``ops.segment_reduce``
    (max, sum, sum) - and never reaches ``ops.attention_readout``.  On: one ``ops.attention_readout`` and nothing else."""
    from wsi_hgnn_amd import ops
    from wsi_hgnn_amd.pooling import GlobalAttentionPooling
    assert ops.fused_attention_readout() is False
    case = (4, "ordinary", 4)
    x, w, b, _ = AC.inputs(case)
    x, w, b = x.double(), w.double(), b.double()
    pool = GlobalAttentionPooling(torch.nn.Linear(4, 1).double())
    with torch.no_grad():
        pool.gate_nn.weight.copy_(w.view(1, -1)); pool.gate_nn.bias.copy_(b)
    graph, calls = _Graph(), []
    assert not pool.fused(graph)

    def linear(x_, w_, b_):
        calls.append("linear")
        return x_ @ w_.t() + b_

    def segment_reduce(x_, rp, op):
        calls.append(op)
        out = torch.zeros((rp.num_segs, x_.shape[1]), dtype=x_.dtype)
        for s, (a, e) in enumerate(rp.ranges):
            if e > a:
                out[s] = x_[a:e].max(0).values if op == "max" else x_[a:e].sum(0)
        return out

    real = ops.attention_readout
    monkeypatch.setattr(ops, "linear", linear)
    monkeypatch.setattr(ops, "segment_reduce", segment_reduce)
    monkeypatch.setattr(ops, "attention_readout", lambda *a: calls.append("fused") or real(*a))
    ref = AC.restate(x, w, b, torch.zeros(AC.S, 4))["out"]
    _close(pool(graph, x, ntype="n").detach().numpy(), ref, "composite")
    assert calls == ["linear", "max", "sum", "sum"]
    del calls[:]
    ops.set_fused_attention_readout(True)
    try:
        assert pool.fused(graph)
        _close(pool(graph, x, ntype="n").detach().numpy(), ref, "fused")
        assert calls == ["fused"]
    finally:
        ops.set_fused_attention_readout(False)
    assert ops.fused_attention_readout() is False


def test_restatement_in_float32_stays_under_a_quarter_of_the_bound():
    """The bound the GPU test holds the kernels to (1e-4 x the block's largest entry) against the error float32 arithmetic itself makes on
    these inputs: the restatement run in float32 stays under a quarter of it, for every case and block."""
    worst = {}
    for case in AC.CASES:
        args = AC.inputs(case)
        ref, f32 = AC.restate(*args), AC.restate(*args, dtype=np.float32)
        for k in ref:
            r = AC.error_ratio(f32[k], ref[k])
            worst[k] = max(worst.get(k, 0.0), r)
            assert r <= 0.25, (AC.case_id(case), k, r)
    print("float32 restatement, worst error / bound:", {k: round(v, 4) for k, v in worst.items()})
