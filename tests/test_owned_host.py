"""The owners of the context's device buffers, events and streams (csrc/mcpt_owned.h) are plain host
C++ over a handful of HIP calls: tests/cpp/owned_test.cpp checks them against a counting stand-in for
the HIP runtime (tests/cpp/fake_hip) on the CPU, as a plain build and as a stand-alone
AddressSanitizer + UBSan build whose leak check at exit is the last assertion."""
import os
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "montecarlo-pathtracing_amd", "csrc")
CASES = ("devbuf", "hostbuf", "event_stream", "group", "all")


@pytest.mark.parametrize("flags", [["-O1"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]],
                         ids=["plain", "sanitized"])
def test_owned_known_answers(tmp_path, flags):
    out = str(tmp_path / "owned_test")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror"] + flags +
                   ["-I", os.path.join(REPO, "tests", "cpp", "fake_hip"), "-I", CSRC,
                    os.path.join(REPO, "tests", "cpp", "owned_test.cpp"), "-o", out], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1")
    r = subprocess.run([out], capture_output=True, text=True, timeout=60, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    for name in CASES:
        assert f"{name}: ok" in r.stdout, r.stdout
