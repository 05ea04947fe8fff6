"""The order of a render call on the device (csrc/mcpt_launch_seq.h: the lane hand-off and the timing
ring) is plain host C++ over a handful of HIP calls: tests/cpp/launch_seq_test.cpp replays launch()'s
steps against a logging stand-in for the HIP runtime (tests/cpp/fake_hip) on the CPU and compares the
calls, one by one, with logs written out in the test, as a plain build and as a stand-alone
AddressSanitizer + UBSan build whose leak check at exit is the last assertion."""
import os
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "montecarlo-pathtracing_amd", "csrc")
CASES = ("in_order", "lanes_alternating", "lane_after_in_order", "across_calls", "empty_call", "failure_part_way",
         "ring", "queries", "order_copy", "all")


@pytest.mark.parametrize("flags", [["-O1"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]],
                         ids=["plain", "sanitized"])
def test_launch_seq_known_answers(tmp_path, flags):
    out = str(tmp_path / "launch_seq_test")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror"] + flags +
                   ["-I", os.path.join(REPO, "tests", "cpp", "fake_hip"), "-I", CSRC,
                    os.path.join(REPO, "tests", "cpp", "launch_seq_test.cpp"), "-o", out], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1")
    r = subprocess.run([out], capture_output=True, text=True, timeout=60, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    for name in CASES:
        assert f"{name}: ok" in r.stdout, r.stdout
