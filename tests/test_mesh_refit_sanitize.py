"""The host refit under AddressSanitizer + UndefinedBehaviorSanitizer: tests/cpp/mesh_refit_sanitize.cpp
(its own main) links mcpt_scene.cpp alone, built with -fsanitize=address,undefined, and runs on the CPU:
updates of meshes of 1, 2, 3, 5 and 600 triangles, the idempotent update, the refusals."""
import os
import subprocess

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_host_refit_clean_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "mesh_refit_sanitize")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fno-fast-math",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                    os.path.join(REPO, "montecarlo-pathtracing_amd", "csrc", "mcpt_scene.cpp"),
                    os.path.join(REPO, "tests", "cpp", "mesh_refit_sanitize.cpp"), "-o", exe], check=True, timeout=300)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1:verify_asan_link_order=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stdout + r.stderr[-4000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
    assert r.stdout.count(": ok") == 5, r.stdout
