"""The frame gathers' row plan (csrc/mcpt_gather_plan.h: full-frame targets, rows held once, runs of
rows, source rows in range) is plain host C++: tests/cpp/gather_plan_test.cpp checks it against
known answers on the CPU, as a plain build and as a stand-alone AddressSanitizer + UBSan build.  The
partition typed into that file is compared here with the package's own balanced partition."""
import os
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "montecarlo-pathtracing_amd", "csrc")
CASES = ("row_runs", "is_full_frame", "rows_held_once", "src_rows_in_range")


@pytest.mark.parametrize("flags", [["-O1"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]],
                         ids=["plain", "sanitized"])
def test_gather_plan_known_answers(tmp_path, flags):
    from mcpt.dist import local_rows
    out = str(tmp_path / "gather_plan_test")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror"] + flags + ["-I", CSRC,
                    os.path.join(REPO, "tests", "cpp", "gather_plan_test.cpp"), "-o", out], check=True)
    r = subprocess.run([out], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    for name in CASES:
        assert f"{name}: ok" in r.stdout, r.stdout
    typed = [[int(v) for v in line.split(":")[1].split()] for line in r.stdout.splitlines() if line.startswith("balanced 53 8 3:")]
    assert typed == [local_rows(53, 8, 3, k, "balanced").tolist() for k in range(3)]
