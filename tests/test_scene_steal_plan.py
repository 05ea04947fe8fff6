"""plan::limits for the LDS-scene kernel's pass stealing (csrc/mcpt_plan.h):
tests/cpp/scene_steal_plan_test.cpp checks may_steal, the sub-launch bound and the byte budgets for
C2's and C5's shapes, a mesh shape and the inputs that do not steal, as a plain build and as a
stand-alone AddressSanitizer + UBSan build."""
import os
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "montecarlo-pathtracing_amd", "csrc")


@pytest.mark.parametrize("flags", [["-O1"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]],
                         ids=["plain", "sanitized"])
def test_scene_steal_limits(tmp_path, flags):
    out = str(tmp_path / "scene_steal_plan_test")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror"] + flags + ["-I", CSRC,
                    os.path.join(REPO, "tests", "cpp", "scene_steal_plan_test.cpp"), "-o", out], check=True)
    r = subprocess.run([out], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "scene_steal_limits: ok" in r.stdout, r.stdout
