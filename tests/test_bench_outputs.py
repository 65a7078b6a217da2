"""bench.py --dump-outputs: what the last timed step computed, written as float32 .npy files so that two builds can be compared output for output.
CPU: the layout, the seeded sample and the size bound of ``bench.dump_outputs``.  GPU (-m gpu): the option end to end on a small workload."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _params(n0=40 * 30, n1=30, n2=5):
    """Three parameters whose values are their positions in the flat order and whose gradients are twice that; the last has no gradient."""
    flat = torch.arange(n0 + n1 + n2, dtype=torch.float32)
    ps = [torch.nn.Parameter(flat[:n0].reshape(40, 30).clone()), torch.nn.Parameter(flat[n0:n0 + n1].clone()),
          torch.nn.Parameter(flat[n0 + n1:].clone())]
    ps[0].grad = 2 * ps[0].detach().clone()
    ps[1].grad = 2 * ps[1].detach().clone()
    return ps


def _load(d):
    return {n: np.load(os.path.join(d, n + ".npy")) for n in ("logits", "loss", "grads", "params")}


def test_dump_outputs_layout_sample_and_budget(tmp_path, monkeypatch):
    import bench
    assert 2 * bench.DUMP_SAMPLE * 4 < 64e6 - 1e6      # grads + params at most, with room for logits and loss
    ps = _params()
    n = sum(p.numel() for p in ps)
    logits, loss = torch.randn(4, 2), torch.tensor(0.75)
    assert bench.dump_outputs(str(tmp_path / "full"), logits, loss, ps) == ["grads", "logits", "loss", "params"]
    full = _load(tmp_path / "full")
    assert all(a.dtype == np.float32 for a in full.values())
    assert np.array_equal(full["logits"], logits.numpy()) and full["loss"].shape == () and full["loss"] == np.float32(0.75)
    assert np.array_equal(full["params"], np.arange(n, dtype=np.float32))
    assert np.array_equal(full["grads"][:-5], 2 * full["params"][:-5]) and not full["grads"][-5:].any()   # no gradient: zeros

    monkeypatch.setattr(bench, "DUMP_SAMPLE", 100)
    bench.dump_outputs(str(tmp_path / "a"), logits, loss, ps)
    bench.dump_outputs(str(tmp_path / "b"), logits, loss, ps)
    a, b = _load(tmp_path / "a"), _load(tmp_path / "b")
    pos = a["params"]                                   # the values are the positions kept
    assert pos.shape == (100,) and np.all(np.diff(pos) > 0) and pos[-1] < n
    assert len(np.unique(pos.astype(np.int64) // 400)) > 1          # spread over the whole flat order, not a prefix
    assert np.array_equal(a["grads"], np.where(pos < n - 5, 2 * pos, 0))
    for k in a:
        assert np.array_equal(a[k], b[k]), k           # the same positions in every run


@pytest.mark.gpu
def test_bench_dumps_the_last_timed_step(tmp_path):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    out_dir = str(tmp_path / "outputs")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--batch", "2", "--nodes", "600",
                        "--in-dim", "64", "--hidden", "128", "--no-cpu-baseline", "--no-alt-gemm", "--no-knn", "--no-captured", "--no-training-config",
                        "--no-full-depth", "--no-kernel-timing", "--dump-outputs", out_dir],
                       capture_output=True, text=True, timeout=900, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    line = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert line["steps"] == 3 and line["ms_per_step"] > 0
    d = _load(out_dir)
    assert all(a.dtype == np.float32 and np.isfinite(a).all() for a in d.values())
    assert d["logits"].shape == (2, 2) and d["grads"].shape == d["params"].shape and np.abs(d["grads"]).max() > 0
    assert abs(float(d["loss"]) - line["loss"]) <= 1e-6 * max(1.0, abs(line["loss"]))      # the loss of the same (last timed) step
    assert sum(os.path.getsize(os.path.join(out_dir, f)) for f in os.listdir(out_dir)) <= 64e6
