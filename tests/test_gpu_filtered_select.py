"""The select on the denoised frame's error on the GPU (mcpt_adaptive_select_filtered, DESIGN.md
§3.9.2).  Every round's active list, both records, the error map and the filter's image and variance
are compared bit for bit with the numpy restatement (tests/test_filtered_select_restate.py) fed the
GPU's own read_accum and read_guides; the thresholds are chosen on the CPU from the restatement of
the first round's state, so that the first select retires some blocks but not all, which is asserted
on the GPU's result."""
import copy
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import test_adaptive_restate as ar
import test_filtered_select_restate as fr
import test_stats_restate as st
from test_meshes import mesh_scene

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "montecarlo-pathtracing_amd")
APP = os.path.join(PKG, "bin", "mcpt_render")
bits = st.bits
FLOOR = 0.01
K, SP = 3.0, 0.75        # the filter's widths in the bit-equality cases (any positive values: the contract is the same)
BOUNCES, BATCH = 3, 4
NO_ADAPTIVE, NO_STATS, NO_GUIDES, INVALID = -9, -8, -7, -1
RAW_KEYS = ("n_px", "n_above", "sum_q", "mean_r", "passes", "batches", "n_active_blocks", "n_blocks", "samples")
F_KEYS = ("n_above_f", "sum_qf", "mean_rf")


@pytest.fixture(scope="module")
def renderer(mcpt_mod):
    r = mcpt_mod.Renderer(0)
    yield r
    r.close()


@pytest.fixture(scope="module")
def second(mcpt_mod):
    r = mcpt_mod.Renderer(0)
    yield r
    r.close()


def status(mcpt_mod, fn, *args):
    with pytest.raises(mcpt_mod.MCPTError) as e:
        fn(*args)
    return str(e.value)


def begin(mcpt_mod, r, scene, W, H, min_passes=0, rows=None):
    """Scene, target, guides, a statistics window and the adaptive mode; returns the camera."""
    r.upload_scene(mesh_scene(mcpt_mod) if scene == "mesh" else mcpt_mod.Scene.reference(scene))
    if rows is None:
        r.set_target(W, H)
    else:
        r.set_target_rows(W, H, rows)
    cam = mcpt_mod.camera_canonical(W, H)
    r.render_guides(*cam)
    r.stats_begin()
    r.adaptive_begin(min_passes)
    return cam


class Run:
    """A device run with the restatement's state beside it: batches of BATCH passes into the active
    blocks, the statistics restated from the accumulator the device returns."""

    def __init__(self, mcpt_mod, r, scene, W, H, min_passes=0):
        self.r, self.W, self.H = r, W, H
        self.cam = begin(mcpt_mod, r, scene, W, H, min_passes)
        acc, n0 = r.read_accum()
        assert n0 == 0
        self.state, self.ad = st.begin(acc), ar.begin(W, H, 0, min_passes)
        self.first = 1
        self.g = r.read_guides()

    def resume(self, r, ad, state, first):
        """The same run continued on another context (after a checkpoint load)."""
        self.r, self.ad, self.state, self.first = r, copy.deepcopy(ad), copy.deepcopy(state), first

    def batch(self):
        self.r.render_adaptive(self.cam[0], self.cam[1], self.first, BATCH, 0.0, BOUNCES, 1.0, 0)
        idle = not self.ad["active"].any()                    # an empty list: no launch, no batch
        ar.rendered(self.ad, BATCH)
        self.first += BATCH
        self.acc, _ = self.r.read_accum()
        if not idle:
            st.batch(self.state, self.acc, BATCH)

    def probe(self, it):
        """Per block the largest rf and the largest r of the current state (the restatement's)."""
        p = copy.deepcopy(self.ad)
        _, c4 = fr.select_filtered(p, self.state, self.acc, self.g["key"], self.g["normal"], self.g["position"], 1e-9,
                                   64.0, FLOOR, it, K, SP)
        return fr.block_max(p, fr.filtered_error(c4, FLOOR)), fr.block_max(p, p["map"][..., 1])

    def select(self, thr, cap, it):
        """The device's select against the restatement's: everything bit for bit."""
        rec = self.r.adaptive_select_filtered(thr, cap, FLOOR, it, K, SP)
        ref, c4 = fr.select_filtered(self.ad, self.state, self.acc, self.g["key"], self.g["normal"], self.g["position"],
                                     thr, cap, FLOOR, it, K, SP)
        print(f"N={self.state['N']} B={self.state['B']} gpu {rec}")
        for k in RAW_KEYS + F_KEYS:
            assert rec[k] == ref[k], (k, rec, ref)
        assert bits(np.float32(rec["max_r"])) == bits(ref["max_r"]), (rec, ref)
        assert bits(np.float32(rec["max_rf"])) == bits(ref["max_rf"]), (rec, ref)
        assert self.r.read_active_blocks().tolist() == ar.active_list(self.ad).tolist()
        for got, want, what in ((self.r.read_error_map(), self.ad["map"], "map"),
                                (self.r.read_denoised(), c4[..., :3], "denoised"),
                                (self.r.read_denoised_variance(), c4[..., 3], "variance")):
            same = bits(got) == bits(want)
            assert same.all(), (what, int((~same).sum()), np.argwhere(~same)[:4].tolist())
        return rec


@pytest.mark.parametrize("iterations", [0, 1, 3])
@pytest.mark.parametrize("scene,W,H", [(6, 37, 21), ("mesh", 29, 19)])
def test_bit_parity_with_the_restatement(mcpt_mod, renderer, scene, W, H, iterations):
    """Frames smaller than a step-8 halo with partial blocks on both edges, three select rounds."""
    run = Run(mcpt_mod, renderer, scene, W, H)
    run.batch()
    run.batch()
    fm, rm = run.probe(iterations)
    thr, cap = float(np.median(fm)), float(np.quantile(rm, 0.75))
    assert thr > 0 and cap > 0
    rec = run.select(thr, cap, iterations)
    assert 0 < rec["n_active_blocks"] < rec["n_blocks"] == ((W + 7) // 8) * ((H + 7) // 8), rec     # not vacuous
    assert rec["n_px"] == W * H
    for _ in range(2):
        run.batch()
        run.select(thr, cap, iterations)
    assert np.array_equal(renderer.read_sample_counts(), ar.counts(run.ad))
    sel_ms, _ = renderer.last_adaptive_ms()
    assert sel_ms > 0.0 and renderer.last_denoise_ms()[1] > 0.0


def two_contexts(mcpt_mod, a, b, W, H, min_b=0):
    """The same two batches into both; every block active in both."""
    cams = [begin(mcpt_mod, r, 6, W, H, m) for r, m in ((a, 0), (b, min_b))]
    for r, cam in zip((a, b), cams):
        for k in range(2):
            r.render_adaptive(cam[0], cam[1], 1 + k * BATCH, BATCH, 0.0, BOUNCES, 1.0, 0)
    assert np.array_equal(bits(a.read_accum()[0]), bits(b.read_accum()[0]))
    return cams


def test_same_bits_as_the_separate_calls_and_plain_select_unchanged(mcpt_mod, renderer, second):
    """Step B leaves what adaptive_select (retiring nothing) + denoise_resolved_variance leave, and
    step A the error map adaptive_select writes."""
    W, H = 37, 21
    two_contexts(mcpt_mod, renderer, second, W, H, min_b=10 ** 6)
    rec = renderer.adaptive_select_filtered(0.05, 0.2, FLOOR, 3, K, SP)
    img, var = renderer.read_denoised(), renderer.read_denoised_variance()
    raw = second.adaptive_select(63.9, FLOOR)
    assert raw["n_active_blocks"] == raw["n_blocks"]
    assert np.array_equal(bits(second.read_error_map()), bits(renderer.read_error_map()))
    want = second.denoise_resolved_variance(3, K, SP)
    assert np.array_equal(bits(img), bits(want))
    assert np.array_equal(bits(var), bits(second.read_denoised_variance()))
    assert renderer.last_denoise_path() == second.last_denoise_path()
    for k in ("n_px", "sum_q", "mean_r", "passes", "batches", "n_blocks", "samples"):
        assert rec[k] == raw[k], k
    assert bits(np.float32(rec["max_r"])) == bits(np.float32(raw["max_r"]))
    # the two calls alternate: a plain select after the filtered one only retires
    before = set(renderer.read_active_blocks().tolist())
    renderer.adaptive_select(0.05, FLOOR)
    assert set(renderer.read_active_blocks().tolist()) <= before


def test_superset_of_the_raw_rule_on_the_device(mcpt_mod, renderer, second):
    """96x54, raw_cap == threshold: the filtered rule keeps every block the raw rule keeps."""
    W, H = 96, 54
    two_contexts(mcpt_mod, renderer, second, W, H)
    rmap = second.adaptive_select(63.9, FLOOR) and second.read_error_map()[..., 1]
    second.adaptive_begin(0)
    bmax = np.array([rmap[y:y + 8, x:x + 8].max() for y in range(0, H, 8) for x in range(0, W, 8)])
    mixed = 0
    for q in (0.3, 0.6, 0.9):
        thr = float(np.quantile(bmax[bmax > 0], q))
        renderer.adaptive_begin(0)
        second.adaptive_begin(0)
        kept = second.adaptive_select(thr, FLOOR)["n_active_blocks"]
        raw = set(second.read_active_blocks().tolist())
        rec = renderer.adaptive_select_filtered(thr, thr, FLOOR, 5)
        got = set(renderer.read_active_blocks().tolist())
        assert raw <= got and len(got) == rec["n_active_blocks"] and len(raw) == kept, (q, len(raw), len(got))
        assert np.array_equal(bits(second.read_error_map()), bits(renderer.read_error_map()))
        mixed += 0 < kept < rec["n_blocks"]
    assert mixed == 3


CHILD = """
import json, sys
import torch
sys.path.insert(0, sys.argv[1])
import mcpt
W, H = 45, 37
r = mcpt.Renderer(0)
r.upload_scene(mcpt.Scene.reference(6)); r.set_target(W, H)
cam = mcpt.camera_canonical(W, H)
r.render_guides(*cam); r.stats_begin(); r.adaptive_begin(0)
out = []
for k in range(3):
    r.render_adaptive(cam[0], cam[1], 1 + 4 * k, 4, 0.0, 3, 1.0, 0)
    if k:
        rec = r.adaptive_select_filtered(float(sys.argv[2]), float(sys.argv[3]), 0.01, 3, 3.0, 0.75)
        rec["max_r"] = float(rec["max_r"]).hex(); rec["max_rf"] = float(rec["max_rf"]).hex()
        out.append({"rec": rec, "list": r.read_active_blocks().tolist(), "path": r.last_denoise_path()})
print("RESULT " + json.dumps(out))
r.close()
"""


def test_lds_and_global_tap_paths_give_the_same_selects(mcpt_mod, renderer, monkeypatch):
    """MCPT_DENOISE_NAIVE=1 in a fresh child process against the LDS-tile kernels here: 45x37, 3
    iterations (steps 1 and 2 in LDS), two rounds."""
    W, H, thr, cap = 45, 37, 0.02, 0.3
    monkeypatch.setenv("MCPT_DENOISE_NAIVE", "0")
    cam = begin(mcpt_mod, renderer, 6, W, H)
    here = []
    for k in range(3):
        renderer.render_adaptive(cam[0], cam[1], 1 + BATCH * k, BATCH, 0.0, BOUNCES, 1.0, 0)
        if k:
            rec = renderer.adaptive_select_filtered(thr, cap, FLOOR, 3, K, SP)
            rec["max_r"], rec["max_rf"] = float(rec["max_r"]).hex(), float(rec["max_rf"]).hex()
            here.append({"rec": rec, "list": renderer.read_active_blocks().tolist(), "path": renderer.last_denoise_path()})
    p = subprocess.run([sys.executable, "-c", CHILD, PKG, repr(thr), repr(cap)], capture_output=True, text=True,
                       timeout=120, env=dict(os.environ, MCPT_DENOISE_NAIVE="1"))
    assert p.returncode == 0, p.stdout[-1000:] + p.stderr[-2000:]
    there = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][0][7:])
    assert [h["path"] for h in here] == [0b011, 0b011] and [t["path"] for t in there] == [0, 0]
    for h, t in zip(here, there):
        assert h["list"] == t["list"] and h["rec"] == t["rec"], (h, t)
    assert here[0]["rec"]["n_above_f"] > 0 and 0 < len(here[0]["list"]) < 30      # not vacuous


def snapshot(r):
    return r.read_active_blocks().tolist(), r.read_error_map(), r.read_denoised(), r.read_denoised_variance()


def same_snapshot(a, b):
    return a[0] == b[0] and all(np.array_equal(bits(x), bits(y)) for x, y in zip(a[1:], b[1:]))


def test_error_codes_leave_the_state_alone(mcpt_mod, renderer):
    r, W, H = renderer, 37, 21
    cam = begin(mcpt_mod, r, 6, W, H)
    r.render_adaptive(cam[0], cam[1], 1, BATCH, 0.0, BOUNCES, 1.0, 0)
    assert f"({NO_STATS})" in status(mcpt_mod, r.adaptive_select_filtered, 0.05)          # one batch only
    r.render_adaptive(cam[0], cam[1], 5, BATCH, 0.0, BOUNCES, 1.0, 0)
    rmap = r.convergence(0.05) and r.read_error_map()[..., 1]
    bmax = [rmap[y:y + 8, x:x + 8].max() for y in range(0, H, 8) for x in range(0, W, 8)]
    rec = r.adaptive_select(float(np.median(bmax)))
    assert 0 < rec["n_active_blocks"] < rec["n_blocks"]
    r.denoise_resolved_variance(2, K, SP)
    snap = snapshot(r)
    for bad in ((0.05, 64.0, FLOOR, 9), (0.05, 64.0, FLOOR, -1), (0.05, 0.0), (0.05, float("inf")), (0.0,),
                (float("nan"),), (0.05, 64.0, 0.0), (0.05, 64.0, FLOOR, 3, 0.0), (0.05, 64.0, FLOOR, 3, 1.0, -1.0)):
        assert f"({INVALID})" in status(mcpt_mod, r.adaptive_select_filtered, *bad), bad
    assert same_snapshot(snapshot(r), snap)
    r.set_flat_face(True)                                     # the guides are not current
    assert f"({NO_GUIDES})" in status(mcpt_mod, r.adaptive_select_filtered, 1e-6)
    r.set_flat_face(False)
    assert f"({NO_GUIDES})" in status(mcpt_mod, r.adaptive_select_filtered, 1e-6)
    r.render_guides(*cam)
    assert same_snapshot(snapshot(r), snap)
    assert r.adaptive_select_filtered(1e-6, 64.0, FLOOR, 2, K, SP)["n_active_blocks"] == rec["n_active_blocks"]
    r.adaptive_end()                                          # the mode off: before every other check
    assert f"({NO_ADAPTIVE})" in status(mcpt_mod, r.adaptive_select_filtered, 0.0)
    # a shard: not a full frame
    rows = [y for y in range(H) if y % 3 != 1]
    cam = begin(mcpt_mod, r, 6, W, H, rows=rows)
    for k in range(2):
        r.render_adaptive(cam[0], cam[1], 1 + BATCH * k, BATCH, 0.0, BOUNCES, 1.0, 0)
    rmap = r.convergence(0.05) and r.read_error_map()[..., 1]
    bmax = [rmap[y:y + 8, x:x + 8].max() for y in range(0, len(rows), 8) for x in range(0, W, 8)]
    rec = r.adaptive_select(float(np.median(bmax)))
    assert 0 < rec["n_active_blocks"] < rec["n_blocks"]
    before = r.read_active_blocks().tolist(), r.read_error_map()
    assert f"({INVALID})" in status(mcpt_mod, r.adaptive_select_filtered, 1e-6)
    assert "full-frame" in status(mcpt_mod, r.adaptive_select_filtered, 1e-6)
    assert r.read_active_blocks().tolist() == before[0] and np.array_equal(bits(r.read_error_map()), bits(before[1]))
    r.stats_end()


def test_checkpoint_resumes_the_filtered_rule(mcpt_mod, renderer, second, tmp_path):
    """Three rounds, a checkpoint, two more; a fresh context loads it, renders its guides and runs
    the same two rounds: lists, records, counts and sums bit for bit (both against the restatement)."""
    W, H, it = 37, 21, 2
    run = Run(mcpt_mod, renderer, 6, W, H)
    run.batch()
    run.batch()
    fm, _ = run.probe(it)
    thr = float(0.6 * np.median(fm[fm > 0]))
    run.select(thr, 64.0, it)
    for _ in range(2):
        run.batch()
        rec = run.select(thr, 64.0, it)
    assert 0 < rec["n_active_blocks"] < rec["n_blocks"], rec
    path = str(tmp_path / "filtered.ckpt")
    renderer.save_adaptive_checkpoint(path, run.first, "t")
    saved = copy.deepcopy(run.ad), copy.deepcopy(run.state), run.first
    a = []
    for _ in range(2):
        run.batch()
        a.append((run.select(thr, 64.0, it), renderer.read_active_blocks().tolist()))
    end_a = renderer.read_accum(), renderer.read_sample_counts()
    second.upload_scene(mcpt_mod.Scene.reference(6))
    second.set_target(W, H)
    assert second.load_adaptive_checkpoint(path, "t") == saved[2]
    assert f"({NO_GUIDES})" in status(mcpt_mod, second.adaptive_select_filtered, thr)     # a checkpoint holds no guides
    second.render_guides(*run.cam)
    run.resume(second, *saved)
    for k in range(2):
        run.batch()
        rec = run.select(thr, 64.0, it)
        assert rec == a[k][0] or all(rec[key] == a[k][0][key] for key in RAW_KEYS + F_KEYS), (rec, a[k][0])
        assert bits(np.float32(rec["max_rf"])) == bits(np.float32(a[k][0]["max_rf"]))
        assert second.read_active_blocks().tolist() == a[k][1]
    acc, n = second.read_accum()
    assert n == end_a[0][1] and np.array_equal(bits(acc), bits(end_a[0][0]))
    assert np.array_equal(second.read_sample_counts(), end_a[1])
    second.stats_end()


def test_render_adaptive_until_filtered(mcpt_mod, renderer):
    """filtered=True renders the guides itself and selects with the filtered rule; the defaults are
    the raw loop."""
    W, H = 45, 37
    renderer.upload_scene(mcpt_mod.Scene.reference(6))
    renderer.set_target(W, H)
    cam = mcpt_mod.camera_canonical(W, H)
    rec = renderer.render_adaptive_until(cam[0], cam[1], 0.05, batch=8, max_passes=48, filtered=True, iterations=3)
    assert "n_above_f" in rec and rec["rendered"] <= 48 and (rec["n_active_blocks"] == 0 or rec["rendered"] == 48)
    cnt = renderer.read_sample_counts()
    assert rec["samples"] == int(cnt.sum()) and rec["rendered"] == cnt.max()
    assert np.isfinite(renderer.read_denoised()).all() and renderer.read_guides()["key"].shape == (H, W)
    renderer.set_target(W, H)
    raw = renderer.render_adaptive_until(cam[0], cam[1], 0.05, batch=8, max_passes=48)
    assert "n_above_f" not in raw and raw["samples"] == int(renderer.read_sample_counts().sum())


def test_program_target_denoised(tmp_path):
    from test_cpp_host import read_pfm
    aov, png = str(tmp_path / "X"), str(tmp_path / "X.png")
    base = [APP, "--scene", "6", "--width", "48", "--height", "27", "--spp", "64", "--chunk", "8"]
    rule = ["--adaptive", "--target-error", "0.2", "--target-denoised", "2", "--aov", aov, "--out", png]
    p = subprocess.run(base + rule, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr
    j = json.loads([ln for ln in p.stdout.splitlines() if ln.strip()][0])
    assert j["adaptive"] is True and j["target_denoised"] == 2 and j["denoise_variance"] == 2 and j["raw_cap"] == 64
    assert j["n_above_f"] >= 0 and j["mean_rf"] >= 0 and j["passes"] <= 64
    assert os.path.getsize(png) > 0
    var, smp = read_pfm(aov + "_variance.pfm"), read_pfm(aov + "_samples.pfm")
    assert var.shape[:2] == (27, 48) and (var >= 0).all() and smp.max() == j["passes"]
    assert abs(float(smp[..., 0].mean()) - j["mean_spp"]) < 1e-3
    for extra, word in ((["--devices", "0"], "--devices"), (None, "--adaptive")):
        cmd = base + (rule + extra if extra else ["--target-denoised", "2", "--out", png])
        q = subprocess.run(cmd, capture_output=True, text=True, timeout=60)
        assert q.returncode == 2 and "--target-denoised" in q.stderr and word in q.stderr, (cmd, q.returncode, q.stderr[:300])
