"""mcpt_render --temporal: an orbit of three frames writes three images, the last
one the library's own loop's bits, and every combination that is not built is refused with its
message."""
import json
import os
import subprocess

import numpy as np
import pytest

import test_temporal_restate as tr
from test_cpp_host import read_pfm, read_png_rgb8

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
APP = os.path.join(REPO, "montecarlo-pathtracing_amd", "bin", "mcpt_render")
W, H = 32, 24


def test_three_orbit_frames(mcpt_mod, tmp_path):
    out, pfm = str(tmp_path / "orbit.png"), str(tmp_path / "orbit.pfm")
    r = subprocess.run([APP, "--scene", "6", "--width", str(W), "--height", str(H), "--frames", "3", "--orbit-deg", "1",
                        "--temporal", "--denoise-variance", "--out", out, "--pfm", pfm],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    rec = json.loads(r.stdout.strip().splitlines()[-1])
    assert rec["frames"] == 3 and rec["temporal"] == mcpt_mod.TEMPORAL_MAX_HISTORY and rec["denoise_variance"] == 5
    assert rec["passes"] == 48 and rec["max_len"] == 3 and rec["n_history"] > 0
    for k in range(3):
        png = read_png_rgb8(str(tmp_path / f"orbit_{k:03d}.png"))
        assert png.shape == (H, W, 3) and png.any()
    assert not os.path.exists(out)
    # the same loop through the binding: the app's defaults are 16 spp (two batches of 8) and 3 bounces
    rr = mcpt_mod.Renderer(0)
    try:
        rr.upload_scene(mcpt_mod.Scene.reference(6))
        rr.set_target(W, H)
        prev = None
        for k in range(3):
            ipv, iv, pv = tr.orbit_camera(mcpt_mod, W, H, float(k))
            img, last = rr.render_frame_temporal(ipv, iv, prev, 1 + 16 * k, 16, 2)
            prev = pv
            assert np.array_equal(tr.bits(read_pfm(str(tmp_path / f"orbit_{k:03d}.pfm"))), tr.bits(img)), k
        assert last["n_history"] == rec["n_history"] and last["max_len"] == 3
    finally:
        rr.close()


def test_default_output_name_and_history_argument(tmp_path):
    r = subprocess.run([APP, "--scene", "6", "--width", str(W), "--height", str(H), "--spp", "4", "--frames", "2",
                        "--temporal", "1", "--denoise-variance", "2"], capture_output=True, text=True, timeout=120,
                       cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr
    rec = json.loads(r.stdout.strip().splitlines()[-1])
    assert rec["temporal"] == 1 and rec["max_len"] == 1 and rec["orbit_deg"] == 0
    assert os.path.exists(tmp_path / "out_000.png") and os.path.exists(tmp_path / "out_001.png")


@pytest.mark.parametrize("extra,message", [
    (["--frames", "3"], "give --temporal"),
    (["--orbit-deg", "1"], "give --temporal"),
    (["--temporal", "--denoise-variance", "--devices", "0,0"], "not with --devices"),
    (["--temporal", "--denoise-variance", "--adaptive", "--target-error", "0.1"], "not with --adaptive"),
    (["--temporal", "--denoise-variance", "--checkpoint", "x.ckpt"], "not with --checkpoint or --resume"),
    (["--temporal", "--denoise-variance", "--resume", "x.ckpt"], "not with --checkpoint or --resume"),
    (["--temporal"], "give --denoise-variance"),
    (["--temporal", "--denoise", "3"], "not with --denoise or --denoise-guided"),
    (["--temporal", "--denoise-variance", "--denoise-guided", "3"], "not with --denoise or --denoise-guided"),
    (["--temporal", "--denoise-variance", "--aov", "x"], "not with --aov"),
    (["--temporal", "--denoise-variance", "--spp", "1"], "--spp 2 or more"),
])
def test_refused_combinations(extra, message, tmp_path):
    r = subprocess.run([APP, "--scene", "6", "--width", str(W), "--height", str(H)] + extra, capture_output=True,
                       text=True, timeout=60, cwd=str(tmp_path))
    assert r.returncode == 2 and message in r.stderr and "usage" in r.stderr, (extra, r.returncode, r.stderr[:200])
    assert not os.listdir(tmp_path)
