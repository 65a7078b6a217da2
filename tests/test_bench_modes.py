"""bench.py's two kinds of run: a plain run times the headline steps and nothing else, --full adds the per-kernel pass, the side legs and the
CPU baseline.  CPU: the option check.  GPU (-m gpu): both kinds end to end on a small workload."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = ["--gpus", "1", "--steps", "3", "--warmup", "1", "--batch", "2", "--nodes", "600", "--in-dim", "64", "--hidden", "128"]
SIDE = ["roofline", "edge_phase_roofline", "cpu_baseline", "fwd_bwd_only", "full_depth_last_layer", "training_config", "other_gemm_modes"]


def _run(args, timeout=900):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, capture_output=True, text=True, timeout=timeout, env=env, cwd=ROOT)


def _line(r):
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


def test_pmc_needs_full():
    r = _run(["--pmc"], timeout=120)
    assert r.returncode == 2 and "--full" in r.stderr and not r.stdout.strip()


@pytest.mark.gpu
def test_plain_run_reports_the_headline_and_full_adds_the_rest():
    plain = _line(_run(SMALL))
    assert plain["value"] > 0 and plain["ms_per_step"] > 0 and plain["steps"] == 3 and plain["warmup"] == 1
    assert all(plain[k] is None for k in SIDE + ["single_graph_step", "knn_locality"]), {k: plain[k] for k in SIDE}
    assert plain["grad_allreduce"]["ms_per_step"] is None

    full = _line(_run(SMALL + ["--full", "--no-captured", "--no-knn"]))
    assert all(full[k] is not None for k in SIDE), [k for k in SIDE if full[k] is None]
    assert full["single_graph_step"] is None and full["knn_locality"] is None          # dropped by their --no-* options
    assert full["grad_allreduce"]["ms_per_step"] is not None
    assert {a["gemm"] for a in full["other_gemm_modes"]} == {"bf16x6", "fp16x3", "fp32"}
    # the side legs run after the timed steps: the headline's steps compute the same in both kinds of run
    assert abs(full["loss"] - plain["loss"]) <= 1e-6 * max(1.0, abs(plain["loss"]))
