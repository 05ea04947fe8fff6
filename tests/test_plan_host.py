"""The render launch plan (csrc/mcpt_plan.h: pass geometry, limits, sub-launch cutting, AUTO's
tuner) is plain host C++: tests/cpp/plan_test.cpp checks it against known answers on the CPU, as a
plain build and as a stand-alone AddressSanitizer + UBSan build."""
import os
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "montecarlo-pathtracing_amd", "csrc")
CASES = ("pass_segments", "max_seg", "may_steal", "grid_bound", "cutting", "pass_split", "items", "tuner_order",
         "tuner_decision", "candidate_knobs")


@pytest.mark.parametrize("flags", [["-O1"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]],
                         ids=["plain", "sanitized"])
def test_plan_known_answers(tmp_path, flags):
    out = str(tmp_path / "plan_test")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror"] + flags + ["-I", CSRC,
                    os.path.join(REPO, "tests", "cpp", "plan_test.cpp"), "-o", out], check=True)
    r = subprocess.run([out], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    for name in CASES:
        assert f"{name}: ok" in r.stdout, r.stdout
