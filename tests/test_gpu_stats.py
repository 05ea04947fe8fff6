"""Noise statistics, the convergence metric, the adaptive stop and the noise-guided filter on the
GPU, bit for bit against the numpy float32 restatement
(tests/test_stats_restate.py) fed the accumulator snapshots the GPU itself returned (read_accum
after each call) or the arrays given to write_accum."""
import ctypes
import json
import os
import subprocess

import numpy as np
import pytest

import test_denoise_restate as rs
import test_stats_restate as st
from test_cpp_host import read_pfm
from test_meshes import mesh_scene

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
bits = rs.bits
THR, FLOOR = 0.1, 0.01
SIZES = (4, 4, 8, 3, 32, 40)      # unequal; 32 (passes 20..51) and 40 (52..91) span a chunk boundary
NO_STATS, INVALID = -8, -1


@pytest.fixture(scope="module")
def renderer(mcpt_mod):
    r = mcpt_mod.Renderer(0)
    yield r
    r.close()


def target(mcpt_mod, r, scene, W, H, rows=None):
    sc = mesh_scene(mcpt_mod) if scene == "mesh" else mcpt_mod.Scene.reference(scene)
    r.upload_scene(sc)
    if rows is None:
        r.set_target(W, H)
    else:
        r.set_target_rows(W, H, rows)
    return mcpt_mod.camera_canonical(W, H)


def check_query(r, state, thr=THR, floor=FLOOR):
    """convergence() and read_error_map() against the restatement's state; returns (record, map)."""
    rec = r.convergence(thr, floor)
    m = r.read_error_map()
    se, rr, q = st.error(state, floor)
    ref = st.record(rr, q, thr)
    got = {k: rec[k] for k in ("n_px", "n_above", "sum_q")}
    print(f"N={state['N']} B={state['B']} gpu {rec} ref {ref}")
    assert got == {k: ref[k] for k in got}, (rec, ref)
    assert bits(np.float32(rec["max_r"])) == bits(ref["max_r"]), (rec, ref)
    assert rec["mean_r"] == ref["mean_r"] and rec["passes"] == state["N"] and rec["batches"] == state["B"]
    assert np.array_equal(bits(m[..., 0]), bits(se)), np.argwhere(bits(m[..., 0]) != bits(se))[:4].tolist()
    assert np.array_equal(bits(m[..., 1]), bits(rr)), np.argwhere(bits(m[..., 1]) != bits(rr))[:4].tolist()
    return rec, m


def run_batches(r, cam, sizes, bounces=4, check=True):
    """stats_begin on the accumulator as it is, then one render call per batch; with check, the
    accumulator is read after each call and every query from the second batch on is compared."""
    acc, n0 = r.read_accum()
    state = st.begin(acc)
    r.stats_begin()
    first, rec, m = n0 + 1, None, None
    for n in sizes:
        r.render(cam[0], cam[1], first, n, 0.0, bounces, 1.0, 0)
        first += n
        if check:
            acc, _ = r.read_accum()
            st.batch(state, acc, n)
            if state["B"] >= 2:
                rec, m = check_query(r, state)
    return state, rec, m


@pytest.fixture(scope="module")
def full_frame(mcpt_mod, renderer):
    """Scene 6 at 45x37 (1,665 pixels: 26 full waves and one lane; partial tiles), SIZES, read after
    every call: the final record and map, shared by the tests that compare with it."""
    cam = target(mcpt_mod, renderer, 6, 45, 37)
    state, rec, m = run_batches(renderer, cam, SIZES)
    return {"state": state, "rec": rec, "map": m}


def test_scene6_every_batch_against_restatement(full_frame, renderer):
    rec, m = full_frame["rec"], full_frame["map"]
    assert rec["n_px"] == 45 * 37 == 1665 and rec["passes"] == sum(SIZES) and rec["batches"] == len(SIZES)
    assert 0 < rec["n_above"] < rec["n_px"] and 0 < rec["mean_r"] < 64 and (m[..., 0] > 0).any()
    assert renderer.stats_info() == {"on": True, "passes": sum(SIZES), "batches": len(SIZES)}
    up, er = renderer.last_stats_ms()
    assert up > 0.0 and er > 0.0


@pytest.mark.parametrize("lanes", [True, False])
def test_queued_calls_give_the_same_record(mcpt_mod, renderer, full_frame, lanes):
    """The same calls queued with nothing read in between: the batch updates are ordered behind
    each call's combines on the context's stream, with render lanes on (the several-segment calls
    run on the lanes' streams once the traversal is fixed) and off."""
    cam = target(mcpt_mod, renderer, 6, 45, 37)
    renderer.set_traversal(mcpt_mod.TRAVERSAL_LANE)
    renderer.set_render_lanes(lanes)
    try:
        run_batches(renderer, cam, SIZES, check=False)
        rec = renderer.convergence(THR, FLOOR)
        m = renderer.read_error_map()
    finally:
        renderer.set_traversal(mcpt_mod.TRAVERSAL_AUTO)
        renderer.set_render_lanes(True)
    assert rec == full_frame["rec"]
    assert np.array_equal(bits(m), bits(full_frame["map"]))


@pytest.mark.parametrize("W,H", [(1, 1), (7, 3)])
def test_tiny_frames(mcpt_mod, renderer, W, H):
    cam = target(mcpt_mod, renderer, 6, W, H)
    _, rec, _ = run_batches(renderer, cam, (4, 4, 8))
    assert rec["n_px"] == W * H


def test_row_shards(mcpt_mod, renderer, full_frame):
    """5 scattered rows of the 45x37 frame: the map is those rows of the full frame's, and the
    records of two complementary shards add up to the full frame's (max for max_r)."""
    rows = [3, 36, 20, 4, 11]
    rest = [y for y in range(37) if y not in rows]
    recs = []
    for rr in (rows, rest):
        cam = target(mcpt_mod, renderer, 6, 45, 37, rr)
        _, rec, m = run_batches(renderer, cam, SIZES)
        assert np.array_equal(bits(m), bits(full_frame["map"][rr]))
        recs.append(rec)
    whole = full_frame["rec"]
    for k in ("n_px", "n_above", "sum_q"):
        assert recs[0][k] + recs[1][k] == whole[k], k
    assert max(recs[0]["max_r"], recs[1]["max_r"]) == whole["max_r"]
    assert recs[0]["n_px"] == 5 * 45


def test_synthetic_batches(mcpt_mod, renderer):
    """write_accum + stats_add_batch at 7x3: a zero-variance pixel, a 1e30 pixel, a pixel whose sum
    decreases, random ones; batches of one pass."""
    W, H = 7, 3
    target(mcpt_mod, renderer, 6, W, H)
    rng = np.random.default_rng(31)
    acc = rng.uniform(0, 2, (H, W, 3)).astype(np.float32)
    acc[0, 0] = (0.5, 0.25, 2.0)
    acc[2, 5] = 50.0
    renderer.write_accum(acc, 5)
    state = st.begin(acc)
    renderer.stats_begin()
    tot = 5
    for k, n in enumerate((1, 1, 3, 1, 6, 1)):
        acc = (acc + rng.uniform(0, 1.5, (H, W, 3)).astype(np.float32) * np.float32(n)).astype(np.float32)
        acc[0, 0] = (0.5, 0.25, 2.0)                    # never changes
        acc[1, 2] = 1e30 if k >= 2 else 0.0             # jumps to 1e30 in the third batch
        acc[2, 5] = np.float32(40.0 - 3.0 * k)          # decreases from 50: a negative mean
        tot += n
        renderer.write_accum(acc, tot)
        renderer.stats_add_batch(n)
        st.batch(state, acc, n)
        if state["B"] >= 2:
            rec, m = check_query(renderer, state)
    assert m[0, 0, 0] == 0 and m[0, 0, 1] == 0
    assert m[1, 2, 1] == 64 and rec["max_r"] == 64.0 and rec["sum_q"] >= 4194304
    assert m[2, 5, 1] > 0                                # mean clamped at 0: r = se / mu_floor
    assert renderer.stats_info() == {"on": True, "passes": 13, "batches": 6}


def test_error_paths(mcpt_mod, renderer):
    L, h = mcpt_mod.lib(), renderer._h
    rec = mcpt_mod.Convergence()
    buf = np.zeros((37, 45, 2), np.float32)

    def query():
        return L.mcpt_convergence(h, 0.1, 0.01, ctypes.byref(rec))

    cam = target(mcpt_mod, renderer, 6, 45, 37)
    renderer.render(cam[0], cam[1], 1, 2, 0.0, 3, 1.0, 0)
    assert renderer.stats_info() == {"on": False, "passes": 0, "batches": 0}
    assert query() == NO_STATS and b"statistics" in L.mcpt_error_string(NO_STATS)       # before stats_begin
    assert L.mcpt_read_error_map(h, mcpt_mod._fp(buf)) == NO_STATS
    assert L.mcpt_stats_add_batch(h, 2) == NO_STATS
    renderer.stats_begin()
    assert L.mcpt_stats_add_batch(h, 0) == INVALID and L.mcpt_stats_add_batch(h, -3) == INVALID
    assert query() == NO_STATS                                                           # B = 0
    renderer.render(cam[0], cam[1], 3, 2, 0.0, 3, 1.0, 0)
    assert query() == NO_STATS                                                           # B = 1
    renderer.render(cam[0], cam[1], 5, 2, 0.0, 3, 1.0, 0)
    assert L.mcpt_read_error_map(h, mcpt_mod._fp(buf)) == NO_STATS                       # no query yet
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        assert L.mcpt_convergence(h, 0.1, bad, ctypes.byref(rec)) == INVALID
        assert L.mcpt_convergence(h, bad, 0.01, ctypes.byref(rec)) == INVALID
    assert query() == 0 and rec.batches == 2 and rec.passes == 4
    assert L.mcpt_read_error_map(h, mcpt_mod._fp(buf)) == 0
    renderer.clear_accum()                                      # does not touch the statistics
    assert renderer.stats_info() == {"on": True, "passes": 4, "batches": 2}
    renderer.stats_begin()                                      # a new window
    assert renderer.stats_info() == {"on": True, "passes": 0, "batches": 0} and query() == NO_STATS
    renderer.render(cam[0], cam[1], 1, 2, 0.0, 3, 1.0, 0)
    renderer.render(cam[0], cam[1], 3, 2, 0.0, 3, 1.0, 0)
    assert query() == 0
    renderer.set_target(45, 37)                                 # frees the buffers, statistics off
    assert renderer.stats_info()["on"] is False and query() == NO_STATS
    renderer.stats_begin()
    renderer.stats_end()
    assert renderer.stats_info()["on"] is False and query() == NO_STATS
    with pytest.raises(mcpt_mod.MCPTError):
        renderer.convergence(0.1)


def test_statistics_leave_the_accumulator_alone(mcpt_mod, renderer, full_frame):
    cam = target(mcpt_mod, renderer, 6, 45, 37)
    first = 1
    for n in SIZES:
        renderer.render(cam[0], cam[1], first, n, 0.0, 4, 1.0, 0)
        first += n
    off, n_off = renderer.read_accum()
    renderer.set_target(45, 37)
    run_batches(renderer, cam, SIZES, check=False)
    on, n_on = renderer.read_accum()
    assert n_on == n_off == sum(SIZES) and np.array_equal(bits(on), bits(off))


def test_mesh_scene(mcpt_mod, renderer):
    cam = target(mcpt_mod, renderer, "mesh", 45, 37)
    _, rec, _ = run_batches(renderer, cam, (4, 4, 4))
    assert rec["passes"] == 12 and rec["batches"] == 3 and rec["mean_r"] > 0


# ---- the noise-guided filter
KC, SP = 3.0, 0.75      # (any positive values: the contract is the same)


def guided_setup(mcpt_mod, r, W, H):
    cam = target(mcpt_mod, r, 6, W, H)
    run_batches(r, cam, (4, 4), check=False)
    r.render_guides(*cam)
    acc, n = r.read_accum()
    return cam, acc, n, r.read_guides()


def test_denoise_guided_small_frame_every_iteration_count(mcpt_mod, renderer):
    L, h = mcpt_mod.lib(), renderer._h
    cam, acc, n, g = guided_setup(mcpt_mod, renderer, 45, 37)
    assert L.mcpt_denoise_guided(h, 3, KC, SP) == NO_STATS             # statistics on, no error map yet
    renderer.convergence(THR, FLOOR)
    se = renderer.read_error_map()[..., 0]
    assert n == 8 and (se > 0).any()
    for it in (1, 2, 3, 4, 5):
        gpu = renderer.denoise_guided(it, KC, SP)
        ref = st.denoise_guided(acc, n, g, se, it, KC, SP)
        same = bits(gpu) == bits(ref)
        assert same.all(), (it, int((~same).sum()), np.argwhere(~same)[:4].tolist())
    assert np.array_equal(bits(renderer.denoise_guided(0, KC, SP)), bits(mcpt_mod.average(acc, n)))
    assert renderer.denoise_iteration_ms(-1) >= 0.0
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        assert L.mcpt_denoise_guided(h, 3, bad, SP) == INVALID
    # the fixed-sigma filter still serves, on the same buffers
    assert np.array_equal(bits(renderer.denoise(2, 1.5, SP)), bits(rs.denoise_guides(acc, n, g, 2, 1.5, SP)))
    renderer.stats_end()
    assert L.mcpt_denoise_guided(h, 3, KC, SP) == NO_STATS             # statistics off
    assert L.mcpt_denoise(h, 3, 1.5, SP) == 0


def test_denoise_guided_interior_tiles_both_paths(mcpt_mod, renderer, monkeypatch):
    """131x67, 5 iterations: interior LDS tiles with halos, the global-tap kernel from step 4 on;
    MCPT_DENOISE_NAIVE=1 runs every step from global memory: the same bits, and
    last_denoise_path() names the path."""
    cam, acc, n, g = guided_setup(mcpt_mod, renderer, 131, 67)
    renderer.convergence(THR, FLOOR)
    se = renderer.read_error_map()[..., 0]
    ref = st.denoise_guided(acc, n, g, se, 5, KC, SP)
    monkeypatch.setenv("MCPT_DENOISE_NAIVE", "0")
    a = renderer.denoise_guided(5, KC, SP)
    assert renderer.last_denoise_path() == 0b00011
    monkeypatch.setenv("MCPT_DENOISE_NAIVE", "1")
    b = renderer.denoise_guided(5, KC, SP)
    assert renderer.last_denoise_path() == 0
    assert np.array_equal(bits(a), bits(ref)) and np.array_equal(bits(b), bits(ref))


# ---- the adaptive stop
def test_render_until(mcpt_mod, renderer):
    W, H = 96, 54
    cam = target(mcpt_mod, renderer, 1, W, H)
    renderer.stats_begin()
    for k in range(2):
        renderer.render(cam[0], cam[1], 1 + 8 * k, 8)
    prior = renderer.convergence(THR)
    assert 0 < prior["mean_r"] < 64
    # a target the first check meets: the same 16 passes give the same record
    renderer.set_target(W, H)
    rec = renderer.render_until(cam[0], cam[1], 2 * prior["mean_r"], batch=8, max_passes=96, check_every=2)
    assert rec["rendered"] == 16 and rec["converged"] and rec["sum_q"] == prior["sum_q"]
    assert renderer.stats_info() == {"on": True, "passes": 16, "batches": 2}
    assert renderer.read_accum()[1] == 16
    # one it cannot meet before the cap of 96 passes
    renderer.set_target(W, H)
    rec = renderer.render_until(cam[0], cam[1], 1e-6, batch=32, max_passes=96)
    assert rec["rendered"] == 96 and not rec["converged"] and rec["passes"] == 96 and rec["batches"] == 3
    assert renderer.stats_info()["passes"] == 96 and renderer.read_accum()[1] == 96
    # more passes, less error
    means = []
    for total in (64, 256):
        renderer.set_target(W, H)
        rec = renderer.render_until(cam[0], cam[1], 1e-6, batch=16, max_passes=total, check_every=64)
        assert rec["rendered"] == total == rec["passes"]
        means.append(rec["mean_r"])
    print("mean_r at 64 and 256 passes:", means)
    assert means[1] <= means[0]


def test_cli_target_error(mcpt_mod, renderer, tmp_path):
    """mcpt_render --target-error with a target the first check (4 chunks of 16) meets: it stops at
    64 of the 128 passes; the error AOV and the guided filter are the library's, bit for bit."""
    app = os.path.join(REPO, "montecarlo-pathtracing_amd", "bin", "mcpt_render")
    W, H = 96, 54
    cam = target(mcpt_mod, renderer, 1, W, H)
    renderer.stats_begin()
    for k in range(4):
        renderer.render(cam[0], cam[1], 1 + 16 * k, 16)            # the app's defaults: 3 bounces, ior 1
    early = 2 * renderer.convergence(THR)["mean_r"]
    aov, pfm = str(tmp_path / "aov"), str(tmp_path / "img.pfm")
    out = subprocess.run([app, "--scene", "1", "--width", str(W), "--height", str(H), "--spp", "128", "--chunk", "16",
                          "--target-error", repr(early), "--denoise-guided", "3", "--aov", aov, "--pfm", pfm],
                         capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    lines = [ln for ln in out.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1
    j = json.loads(lines[0])
    assert j["passes"] == 64 < 128 and j["converged"] is True and j["mean_r"] <= early and j["batches"] == 4
    rec = renderer.convergence(np.float32(early))
    assert j["sum_q"] == rec["sum_q"] and j["n_above"] == rec["n_above"]
    err = read_pfm(aov + "_error.pfm")
    assert np.array_equal(bits(err[..., :2]), bits(renderer.read_error_map()))
    renderer.render_guides(*cam)
    assert np.array_equal(bits(read_pfm(pfm)), bits(renderer.denoise_guided(3)))
