"""csrc/row_group.h's ``row_cfg`` itself, compiled for the host, against the restatement the dispatch tests of GAT, RAConv and GIN rely on
(tests/row_group_cases.py), over every shape the three families accept; and every code it gives inside the family's compiled set."""
import os
import shutil
import subprocess

import pytest

import row_group_cases as R


def test_row_cfg_is_what_the_tests_restate(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not found")
    exe = str(tmp_path / "row_group_check")
    subprocess.check_call([hipcc, "-x", "hip", "--cuda-host-only", "-std=c++17", "-O1", "-I", R.CSRC,
                           os.path.join(os.path.dirname(os.path.abspath(__file__)), "row_group_check.cpp"), "-o", exe])
    lines = subprocess.run([exe], capture_output=True, text=True, check=True).stdout.splitlines()
    compiled = {"gat": set(R.family_codes("gat_attn.hip")), "ra": set(R.family_codes("ra_attn.hip")), "gin": set(R.family_codes("gin.hip"))}
    count = dict.fromkeys(compiled, 0)
    for line in lines:
        family, *nums = line.split()
        H, D, ok, vec, G, NK = map(int, nums)
        assert (vec, G, NK) == R.row_cfg(H * D, D, H if family == "gat" else 1, bool(ok)), line
        assert R.code(vec, G, NK) in compiled[family], line
        count[family] += 1
    assert count == {"gat": 2 * sum(4096 // H for H in range(1, 17)), "ra": 2 * 4096, "gin": 2 * 1024}
