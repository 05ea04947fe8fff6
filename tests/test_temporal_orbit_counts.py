"""Which branches the orbit cases of tests/test_gpu_temporal.py take, computed on the CPU: the
restatement (tests/test_temporal_restate.py) over the oracle's primary hits, the way
tests/test_gpu_guides.py obtains expected guides.  TABLE holds the last of four frames' (n_history,
n_new - n_miss, n_offscreen) per (scene, width, degrees per frame) at max_history 8, plane_tol 0.01;
the test below recomputes it, and the GPU test asserts its records against it.  Also the stand-alone
ASan/UBSan run of the 4x4 inverse behind mcpt_mat4_inverse."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

import test_temporal_restate as tr
from test_meshes import mesh_scene

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = ((37, 21), (16, 16), (3, 2))
STEPS = (0.0, 1.0, 12.0, 180.0)
FRAMES, MAXH, TOL = 4, 8, 0.01
TABLE = {
    (6, 37, 0.0): (561, 0, 0), (6, 37, 1.0): (561, 0, 0), (6, 37, 12.0): (469, 90, 46), (6, 37, 180.0): (64, 497, 135),
    (6, 16, 0.0): (176, 0, 0), (6, 16, 1.0): (173, 3, 0), (6, 16, 12.0): (152, 28, 9), (6, 16, 180.0): (16, 160, 12),
    (6, 3, 0.0): (3, 0, 0), (6, 3, 1.0): (3, 0, 0), (6, 3, 12.0): (3, 0, 0), (6, 3, 180.0): (2, 1, 0),
    ("mesh", 37, 0.0): (467, 0, 0), ("mesh", 37, 1.0): (465, 3, 0), ("mesh", 37, 12.0): (411, 42, 21),
    ("mesh", 37, 180.0): (107, 371, 73),
    ("mesh", 16, 0.0): (164, 0, 0), ("mesh", 16, 1.0): (162, 1, 0), ("mesh", 16, 12.0): (150, 14, 8),
    ("mesh", 16, 180.0): (12, 158, 10),
    ("mesh", 3, 0.0): (3, 0, 0), ("mesh", 3, 1.0): (3, 0, 0), ("mesh", 3, 12.0): (3, 0, 0), ("mesh", 3, 180.0): (2, 2, 0),
}


def oracle_guides(orc, sc, W, H, invPV, invV, meshes=None):
    """A read_guides()-shaped dict from the oracle's trace of every pixel's camera ray."""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
    import gen_golden as g
    prims, nodes, leaves = sc.buffers()
    o = np.zeros((H, W, 3), np.float32)
    d = np.zeros((H, W, 3), np.float32)
    for y in range(H):
        for x in range(W):
            ori, dr, _, _ = g.camera_dir(invPV, invV, W, H, x, y)
            o[y, x], d[y, x] = ori, dr
    oi, of = orc.trace(prims, nodes, leaves, sc.depth(), o, d, meshes=meshes)
    hit = oi[:, 0] >= 0
    key = np.where(hit, (oi[:, 0] << 28) | oi[:, 1], -1).astype(np.int32).reshape(H, W)
    return {"key": key, "normal": of[:, 7:10].reshape(H, W, 3).copy(), "position": of[:, 10:13].reshape(H, W, 3).copy(),
            "dist": of[:, 0].reshape(H, W).copy()}


@pytest.mark.parametrize("scene", [6, "mesh"])
def test_table_from_the_oracles_primary_hits(mcpt_mod, oracle_mod, scene):
    sc = mesh_scene(mcpt_mod) if scene == "mesh" else mcpt_mod.Scene.reference(scene)
    mv = oracle_mod.MeshView(sc.mesh_buffers(), flat_face=False) if scene == "mesh" else None
    got = {}
    for W, H in SIZES:
        for step in STEPS:
            hist, prev = None, None
            for k in range(FRAMES):
                ipv, iv, pv = tr.orbit_camera(mcpt_mod, W, H, k * step)
                g = oracle_guides(oracle_mod, sc, W, H, ipv, iv, mv)
                hist, rec = tr.accumulate(np.ones((H, W, 4), np.float32), g, hist, prev, MAXH, TOL)
                prev = pv
            got[(scene, W, step)] = (rec["n_history"], rec["n_new"] - rec["n_miss"], rec["n_offscreen"])
    assert got == {k: v for k, v in TABLE.items() if k[0] == scene}


def test_table_exercises_both_branches():
    """Every moving sequence blends a history and starts pixels over somewhere, the 1 degree orbit too
    (at 16x16 on both scenes and at 37x21 on the mesh scene; scene 6 at 37x21 and every 3x2 frame turn
    too little in three degrees for a hit pixel to lose its history), and the 12 degree step is the
    one at which pixels leave the frame."""
    for step in (1.0, 12.0, 180.0):
        both = [k for k, v in TABLE.items() if k[2] == step and v[0] > 0 and v[1] > 0]
        assert {k[0] for k in both} == {6, "mesh"}, step
    assert all(TABLE[(s, w, 12.0)][2] > 0 for s in (6, "mesh") for w in (37, 16))
    assert all(v[0] > 0 for v in TABLE.values())


def test_mat4_inverse_clean_under_asan_ubsan(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path / "mat4_sanitize")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-fno-omit-frame-pointer", os.path.join(REPO, "tests", "cpp", "mat4_sanitize.cpp"), "-o", exe],
                   check=True, timeout=600)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stdout + r.stderr[-4000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
    assert "mat4_sanitize ok" in r.stdout
