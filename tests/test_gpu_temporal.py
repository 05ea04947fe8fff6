"""Temporal reprojection on the GPU: the history's colour, variance and lengths, the
record, and mcpt_denoise_temporal's image and variance, bit for bit against the numpy float32
restatement (tests/test_temporal_restate.py) fed the GPU's own read_accum, read_guides and
read_error_map, frame after frame; every precondition's status; the existing filters' bits beside the
new mode; the quality of the last frame of a static and an orbiting sequence.

Which branches each camera sequence takes on its last frame is computed on the CPU from the oracle's
primary hits and kept, with the test that recomputes it, in tests/test_temporal_orbit_counts.py
(TABLE: n_history, n_new - n_miss, n_offscreen); the records here are asserted against it.  12 degrees
per frame is the step at which an edge column leaves the frame."""
import numpy as np
import pytest

import torch

import test_temporal_restate as tr
from test_meshes import mesh_scene
from test_temporal_orbit_counts import TABLE

pytestmark = pytest.mark.gpu

bits = tr.bits
K, SP, ITS = 3.0, 0.75, 3      # the filter's widths and iterations of the bit-equality cases
MAXH, TOL = 8, 0.01
NO_TEMPORAL, NO_STATS, NO_GUIDES, NO_TARGET, INVALID = -10, -8, -7, -3, -1


@pytest.fixture(scope="module")
def renderer(mcpt_mod):
    r = mcpt_mod.Renderer(0)
    yield r
    r.close()


def same_bits(got, want, what):
    """Bit equality; a NaN equals a NaN (its payload is no part of the contract)."""
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    same = (bits(got) == bits(want)) | (np.isnan(got) & np.isnan(want))
    assert same.all(), (what, int((~same).sum()), np.argwhere(~same)[:4].tolist())


def upload(mcpt_mod, r, scene, W, H):
    r.upload_scene(mesh_scene(mcpt_mod) if scene == "mesh" else mcpt_mod.Scene.reference(scene))
    r.set_target(W, H)


def render_frame(r, cam, first_pass, bounces=4, spp=4):
    """Steps 1-5 of the frame loop: 4 spp as 2 batches of 2."""
    r.clear_accum()
    r.stats_begin()
    for b in range(2):
        r.render(cam[0], cam[1], first_pass + b * (spp // 2), spp // 2, 0.0, bounces, 1.0, 0)
    r.convergence(0.05)
    r.render_guides(cam[0], cam[1])


def accumulate_and_check(r, hist, prev_pv, max_history=MAXH, tol=TOL, filt=True):
    """Steps 6-8 against the restatement of the GPU's own inputs; returns (history, record, guides)."""
    acc, n = r.read_accum()
    g = r.read_guides()
    se = r.read_error_map()[..., 0]
    rec = r.temporal_accumulate(prev_pv, max_history, tol)
    new, want = tr.accumulate(tr.current(acc, n, se), g, hist, prev_pv, max_history, tol)
    c, length = r.read_temporal()
    same_bits(c[..., :3], new["c"][..., :3], "colour")
    same_bits(c[..., 3], new["c"][..., 3], "variance")
    assert np.array_equal(length, new["len"])
    assert {k: rec[k] for k in tr.KEYS} == want, (rec, want)
    if filt:
        img, var = r.denoise_temporal(ITS, K, SP), r.read_denoised_variance()
        ref = tr.denoise_temporal(new["c"], g, ITS, K, SP)
        same_bits(img, ref[..., :3], "filtered colour")
        same_bits(var, ref[..., 3], "filtered variance")
    return new, rec, g


@pytest.mark.parametrize("step", [0.0, 1.0, 12.0, 180.0])
@pytest.mark.parametrize("W,H", [(37, 21), (16, 16), (3, 2)])
@pytest.mark.parametrize("scene", [6, "mesh"])
def test_four_frames_bit_equal(mcpt_mod, renderer, scene, W, H, step):
    """Four frames, the world turned `step` degrees per frame (0: the same camera)."""
    r = renderer
    upload(mcpt_mod, r, scene, W, H)
    r.temporal_begin()
    assert r.temporal_info() == {"on": True, "history_valid": False, "frames": 0}
    hist, prev = None, None
    for k in range(4):
        ipv, iv, pv = tr.orbit_camera(mcpt_mod, W, H, k * step)
        render_frame(r, (ipv, iv), 1 + 4 * k)
        hist, rec, g = accumulate_and_check(r, hist, prev)
        assert rec["frames"] == k + 1 and rec["n_new"] == rec["n_px"] - rec["n_history"]
        prev = pv
    assert r.temporal_info() == {"on": True, "history_valid": True, "frames": 4}
    assert r.last_temporal_ms()[0] > 0.0 and r.last_temporal_ms()[1] == 0.0       # (ping-pong: no copy)
    # the branches this sequence takes, as computed on the CPU from the oracle's primary hits
    assert (rec["n_history"], rec["n_new"] - rec["n_miss"], rec["n_offscreen"]) == TABLE[(scene, W, step)], rec
    assert rec["n_history"] > 0
    if step == 0.0:
        assert rec["n_new"] == rec["n_miss"] and rec["max_len"] == 4
    if step > 0.0 and W > 3 and (scene, W, step) != (6, 37, 1.0):
        assert rec["n_new"] - rec["n_miss"] > 0, rec            # both branches (see test_table_exercises_both_branches)
    if step == 12.0 and W > 3:
        assert rec["n_offscreen"] > 0, rec
    r.temporal_end()
    assert r.temporal_info() == {"on": False, "history_valid": False, "frames": 0}


@pytest.mark.parametrize("max_history", [1, 2])
def test_history_cap(mcpt_mod, renderer, max_history):
    """max_history 1: the history is never blended in and out = c; 2: the cap is reached and held."""
    r, W, H = renderer, 37, 21
    upload(mcpt_mod, r, 6, W, H)
    r.temporal_begin()
    ipv, iv, pv = tr.orbit_camera(mcpt_mod, W, H, 0.0)
    hist = None
    for k in range(4):
        render_frame(r, (ipv, iv), 1 + 4 * k)
        hist, rec, _ = accumulate_and_check(r, hist, pv if k else None, max_history)
        assert rec["max_len"] == min(k + 1, max_history)
        if max_history == 1:
            acc, n = r.read_accum()
            same_bits(hist["c"][..., :3], acc / np.float32(n), "out = c")
    r.temporal_end()


def test_overflowed_pixels_through_a_synthetic_accumulator(mcpt_mod, renderer):
    """Seeded sums with one 1e30 pixel and one inf pixel through write_accum and stats_add_batch, two
    frames under one camera: c propagates as written, and the variance stays finite whatever the error
    kernel stores for such a pixel (the restatement reads the same map)."""
    r, W, H = renderer, 16, 16
    upload(mcpt_mod, r, 6, W, H)
    ipv, iv, pv = tr.orbit_camera(mcpt_mod, W, H, 0.0)
    r.render_guides(ipv, iv)
    g = r.read_guides()
    hit = np.argwhere(g["key"] >= 0)
    (ya, xa), (yb, xb) = hit[len(hit) // 2], hit[len(hit) // 3]
    r.temporal_begin()
    rng = np.random.default_rng(31)
    hist = None
    for k in range(2):
        base = rng.uniform(0, 2, (H, W, 3)).astype(np.float32)
        base[ya, xa], base[yb, xb] = 1e30, np.inf
        r.write_accum(base, 2)
        r.stats_begin()
        for n in (4, 6):
            r.write_accum((base * np.float32(n / 2) + rng.uniform(0, 0.5, (H, W, 3)).astype(np.float32)), n)
            r.stats_add_batch(2)
        r.convergence(0.05)
        hist, rec, _ = accumulate_and_check(r, hist, pv if k else None)
    assert rec["n_history"] == len(hit)
    assert hist["c"][ya, xa, 0] > 1e29 and not np.isfinite(hist["c"][yb, xb, :3]).all()
    assert np.isfinite(hist["c"][..., 3]).all() and (hist["c"][..., 3] <= tr.VMAX).all()
    r.temporal_end()


def test_scene_upload_empties_the_history(mcpt_mod, renderer):
    r, W, H = renderer, 16, 16
    upload(mcpt_mod, r, 6, W, H)
    r.temporal_begin()
    ipv, iv, pv = tr.orbit_camera(mcpt_mod, W, H, 0.0)
    hist = None
    for k in range(2):
        render_frame(r, (ipv, iv), 1 + 4 * k)
        hist, rec, _ = accumulate_and_check(r, hist, pv if k else None, filt=False)
    assert rec["n_history"] > 0 and rec["frames"] == 2
    for change in ("scene", "meshes", "flat_face"):
        if change == "scene":
            r.upload_scene(mcpt_mod.Scene.reference(6))
        elif change == "meshes":
            r.upload_meshes(None)
        else:
            r.set_flat_face(False)
        assert r.temporal_info() == {"on": True, "history_valid": False, "frames": 0}
        assert mcpt_mod.lib().mcpt_denoise_temporal(r._h, 3, 1.0, 1.0) == NO_STATS
        render_frame(r, (ipv, iv), 9)
        hist, rec, _ = accumulate_and_check(r, None, pv, filt=False)       # prevPV given, the history empty: unused
        assert rec["n_history"] == 0 and rec["frames"] == 1 and rec["max_len"] == 1
        render_frame(r, (ipv, iv), 13)
        hist, rec, _ = accumulate_and_check(r, hist, pv, filt=False)
        assert rec["n_history"] > 0 and rec["frames"] == 2
    r.temporal_end()


def test_first_frame_is_the_variance_filter(mcpt_mod, renderer):
    r, W, H = renderer, 37, 21
    upload(mcpt_mod, r, 6, W, H)
    cam = mcpt_mod.camera_canonical(W, H)
    render_frame(r, cam, 1)
    want, vwant = r.denoise_variance(5, K, SP), r.read_denoised_variance()
    r.temporal_begin()
    rec = r.temporal_accumulate(None)
    assert rec["n_history"] == 0 and rec["n_new"] == W * H
    for it in (0, 5):
        a, va = r.denoise_variance(it, K, SP), r.read_denoised_variance()
        same_bits(r.denoise_temporal(it, K, SP), a, ("colour", it))
        same_bits(r.read_denoised_variance(), va, ("variance", it))
    same_bits(a, want, "unchanged")
    same_bits(va, vwant, "unchanged")
    assert r.denoise_iteration_ms(-1) > 0.0 and r.last_denoise_ms()[1] > 0.0 and r.last_denoise_path() == 0b00011
    r.temporal_end()


def test_preconditions_in_order_and_untouched_state(mcpt_mod, renderer):
    L, r, W, H = mcpt_mod.lib(), renderer, 16, 16
    rec = mcpt_mod.TemporalRecord()
    buf, lens = np.zeros((H, W, 4), np.float32), np.zeros((H, W), np.int32)
    fresh = mcpt_mod.Renderer(0)
    try:
        assert L.mcpt_temporal_begin(fresh._h) == NO_TARGET
        assert L.mcpt_temporal_accumulate(fresh._h, None, 8, 0.01, rec) == NO_TEMPORAL
    finally:
        fresh.close()
    upload(mcpt_mod, r, 6, W, H)
    h = r._h
    ipv, iv, pv = tr.orbit_camera(mcpt_mod, W, H, 0.0)
    pvp = mcpt_mod._fp(pv)
    # 1. the mode off: every other temporal call, whatever else is wrong
    assert L.mcpt_temporal_accumulate(h, None, 0, -1.0, rec) == NO_TEMPORAL
    assert L.mcpt_temporal_accumulate(h, None, 8, 0.01, None) == NO_TEMPORAL           # even without a record
    assert L.mcpt_denoise_temporal(h, 99, -1.0, 1.0) == NO_TEMPORAL
    assert L.mcpt_read_temporal(h, mcpt_mod._fp(buf), mcpt_mod._ip(lens)) == NO_TEMPORAL
    assert L.mcpt_last_temporal_ms(h, None, None) == NO_TEMPORAL
    assert L.mcpt_temporal_end(h) == 0
    r.temporal_begin()
    # 2. arguments and the accumulator's state before 3. the error map before 4. the guides
    assert L.mcpt_temporal_accumulate(h, None, 8, 0.01, None) == INVALID
    for mh, tol in ((0, 0.01), (65536, 0.01), (8, 0.0), (8, -1.0), (8, float("inf")), (8, float("nan"))):
        assert L.mcpt_temporal_accumulate(h, pvp, mh, tol, rec) == INVALID, (mh, tol)
    assert L.mcpt_temporal_accumulate(h, pvp, 8, 0.01, rec) == INVALID                  # no passes
    r.render(ipv, iv, 1, 2, 0.0, 3, 1.0, 0)
    assert L.mcpt_temporal_accumulate(h, pvp, 8, 0.01, rec) == NO_STATS                 # statistics off
    r.stats_begin()
    r.render(ipv, iv, 3, 2, 0.0, 3, 1.0, 0)
    r.render(ipv, iv, 5, 2, 0.0, 3, 1.0, 0)
    assert L.mcpt_temporal_accumulate(h, pvp, 8, 0.01, rec) == NO_STATS                 # no convergence yet
    r.convergence(0.05)
    assert L.mcpt_temporal_accumulate(h, pvp, 8, 0.01, rec) == NO_GUIDES
    assert L.mcpt_temporal_accumulate(h, pvp, 0, 0.01, rec) == INVALID                  # arguments come first
    r.render_guides(ipv, iv)
    assert L.mcpt_denoise_temporal(h, 3, 1.0, 1.0) == NO_STATS                          # no accumulate yet
    assert L.mcpt_read_temporal(h, mcpt_mod._fp(buf), mcpt_mod._ip(lens)) == NO_STATS
    assert r.temporal_info()["frames"] == 0
    assert L.mcpt_temporal_accumulate(h, None, 8, 0.01, rec) == 0 and rec.frames == 1   # an empty history takes no matrix
    c0, l0 = r.read_temporal()
    img0 = r.denoise_temporal(ITS, K, SP)
    # the history valid: a missing matrix and every bad argument are refused and change nothing
    assert L.mcpt_temporal_accumulate(h, None, 8, 0.01, rec) == INVALID
    for mh, tol in ((0, 0.01), (8, 0.0)):
        assert L.mcpt_temporal_accumulate(h, pvp, mh, tol, rec) == INVALID
    for bad in ((9, 1.0, 1.0), (-1, 1.0, 1.0), (3, 0.0, 1.0), (3, float("nan"), 1.0), (3, 1.0, 0.0), (3, 1.0, float("inf"))):
        assert L.mcpt_denoise_temporal(h, *bad) == INVALID, bad
    r.set_flat_face(False)                                                              # invalidates the guides, empties the history
    assert L.mcpt_denoise_temporal(h, 3, 1.0, 1.0) == NO_STATS
    assert L.mcpt_temporal_accumulate(h, pvp, 8, 0.01, rec) == NO_GUIDES
    r.render_guides(ipv, iv)
    assert L.mcpt_temporal_accumulate(h, pvp, 8, 0.01, rec) == 0 and rec.frames == 1
    c1, l1 = r.read_temporal()
    same_bits(c1, c0, "the same frame again")
    assert np.array_equal(l1, l0)
    same_bits(r.denoise_temporal(ITS, K, SP), img0, "the same image again")
    r.clear_accum()
    assert L.mcpt_temporal_accumulate(h, pvp, 8, 0.01, rec) == INVALID                  # no passes
    assert r.temporal_info() == {"on": True, "history_valid": True, "frames": 1}
    c2, _ = r.read_temporal()
    same_bits(c2, c0, "refusals change nothing")
    # a sharded target ends the mode; on it the mode begins but accumulates nothing
    r.set_target(W, H, 8, 2, 0)
    assert r.temporal_info()["on"] is False
    r.temporal_begin()
    r.stats_begin()
    for first in (1, 3):
        r.render(ipv, iv, first, 2, 0.0, 3, 1.0, 0)
    r.convergence(0.05)
    r.render_guides(ipv, iv)
    assert L.mcpt_temporal_accumulate(h, pvp, 8, 0.01, rec) == INVALID
    r.temporal_end()
    r.stats_end()


def history_of_one_frame(mcpt_mod, r, W, H):
    """A context in temporal mode whose history holds one frame; returns (camera, its P*V)."""
    upload(mcpt_mod, r, 6, W, H)
    r.temporal_begin()
    ipv, iv, pv = tr.orbit_camera(mcpt_mod, W, H, 0.0)
    render_frame(r, (ipv, iv), 1)
    r.temporal_accumulate(None)
    return (ipv, iv), pv


def refused_and_unchanged(mcpt_mod, r, pv, before):
    """mcpt_temporal_accumulate returns INVALID_ARG and leaves the mode's state and the history alone."""
    L, rec = mcpt_mod.lib(), mcpt_mod.TemporalRecord()
    assert L.mcpt_temporal_accumulate(r._h, mcpt_mod._fp(pv), 8, 0.01, rec) == INVALID
    assert r.temporal_info() == {"on": True, "history_valid": True, "frames": 1}
    c, length = r.read_temporal()
    same_bits(c, before[0], "refusals change nothing")
    assert np.array_equal(length, before[1])


def test_gathered_count_plane_is_refused(mcpt_mod, renderer):
    """A counted load of the context's own packed pixels fills the count plane: INVALID_ARG, before the
    error map's NO_STATS and the guides' NO_GUIDES, and nothing changes."""
    r, W, H = renderer, 16, 16
    cam, pv = history_of_one_frame(mcpt_mod, r, W, H)
    before = r.read_temporal()
    render_frame(r, cam, 5)
    buf = torch.zeros((H, W, 4), dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    r.pack_counted_device(buf.data_ptr(), H * W * 16)
    r.synchronize()
    r.load_rows_counted(buf.data_ptr(), H, np.arange(H, dtype=np.int32), r.pass_count())
    assert (r.read_sample_counts() == 4).all()                                      # the plane is valid
    refused_and_unchanged(mcpt_mod, r, pv, before)
    r.stats_end()                                                                   # no error map either: still the plane's refusal
    refused_and_unchanged(mcpt_mod, r, pv, before)
    r.clear_accum()                                                                 # the plane goes with the accumulator it described
    render_frame(r, cam, 5)
    rec = r.temporal_accumulate(pv)
    assert rec["frames"] == 2 and rec["n_history"] > 0
    # ... and before NO_GUIDES (invalidating the guides also empties the history: checked last)
    r.pack_counted_device(buf.data_ptr(), H * W * 16)
    r.synchronize()
    r.load_rows_counted(buf.data_ptr(), H, np.arange(H, dtype=np.int32), r.pass_count())
    r.set_flat_face(False)
    out = mcpt_mod.TemporalRecord()
    assert mcpt_mod.lib().mcpt_temporal_accumulate(r._h, mcpt_mod._fp(pv), 8, 0.01, out) == INVALID
    r.clear_accum()
    r.stats_begin()
    assert mcpt_mod.lib().mcpt_temporal_accumulate(r._h, mcpt_mod._fp(pv), 8, 0.01, out) == INVALID   # (no passes)
    r.temporal_end()
    r.stats_end()


def test_retired_adaptive_block_is_refused(mcpt_mod, renderer):
    """Adaptive mode on with every block active is a uniform frame and accumulates; once a select has
    retired a block the frame has per-pixel counts: INVALID_ARG (mcpt_denoise's refusal), before
    NO_STATS and NO_GUIDES, and nothing changes."""
    r, W, H = renderer, 37, 21
    cam, pv = history_of_one_frame(mcpt_mod, r, W, H)
    r.clear_accum()
    r.stats_begin()
    r.adaptive_begin(0)
    for first in (5, 7):
        r.render_adaptive(cam[0], cam[1], first, 2, 0.0, 4, 1.0, 0)
    r.convergence(0.05)
    r.render_guides(*cam)
    info = r.adaptive_info()
    assert info["n_active"] == info["n_blocks"] == 15
    rec = r.temporal_accumulate(pv)                                                 # nothing retired: accepted
    assert rec["frames"] == 2 and rec["n_history"] > 0
    r.temporal_begin()                                                              # start over: one frame of history
    r.temporal_accumulate(None)
    before = r.read_temporal()
    rmap = r.read_error_map()[..., 1]
    block_max = [rmap[y:y + 8, x:x + 8].max() for y in range(0, H, 8) for x in range(0, W, 8)]
    sel = r.adaptive_select(float(np.median(block_max)))
    assert 0 < sel["n_active_blocks"] < sel["n_blocks"], sel
    refused_and_unchanged(mcpt_mod, r, pv, before)
    assert mcpt_mod.lib().mcpt_denoise(r._h, 3, 1.0, 1.0) == INVALID                # the same refusal
    r.set_flat_face(False)                                                          # no guides (and an empty history): still INVALID
    out = mcpt_mod.TemporalRecord()
    assert mcpt_mod.lib().mcpt_temporal_accumulate(r._h, mcpt_mod._fp(pv), 8, 0.01, out) == INVALID
    r.adaptive_end()                                                                # uniform again
    assert mcpt_mod.lib().mcpt_temporal_accumulate(r._h, mcpt_mod._fp(pv), 8, 0.01, out) == NO_GUIDES
    r.temporal_end()
    r.stats_end()


def test_copy_form_same_bits(mcpt_mod, monkeypatch):
    """MCPT_TEMPORAL_COPY=1 (the history's guides copied behind the kernel, one guide buffer): the
    restatement's bits over an orbit that takes every branch, and a copy time is reported."""
    monkeypatch.setenv("MCPT_TEMPORAL_COPY", "1")
    W, H, step = 37, 21, 12.0
    r = mcpt_mod.Renderer(0)
    try:
        upload(mcpt_mod, r, "mesh", W, H)
        r.temporal_begin()
        hist, prev = None, None
        for k in range(4):
            ipv, iv, pv = tr.orbit_camera(mcpt_mod, W, H, k * step)
            render_frame(r, (ipv, iv), 1 + 4 * k)
            hist, rec, _ = accumulate_and_check(r, hist, prev)
            prev = pv
        assert (rec["n_history"], rec["n_new"] - rec["n_miss"], rec["n_offscreen"]) == TABLE[("mesh", W, step)]
        assert r.last_temporal_ms()[0] > 0.0 and r.last_temporal_ms()[1] > 0.0
    finally:
        r.close()


def test_existing_filters_keep_their_bits(mcpt_mod, renderer):
    """mcpt_denoise and mcpt_denoise_variance on a context that never began the mode, with the mode
    on, and after mcpt_temporal_end: the same bits."""
    W, H = 37, 21
    never = mcpt_mod.Renderer(0)
    try:
        upload(mcpt_mod, never, 6, W, H)
        cam = mcpt_mod.camera_canonical(W, H)
        render_frame(never, cam, 1)
        fixed, var = never.denoise(3), never.denoise_variance(3)
        vvar = never.read_denoised_variance()
    finally:
        never.close()
    r = renderer
    upload(mcpt_mod, r, 6, W, H)
    r.temporal_begin()
    for k in range(2):
        render_frame(r, cam, 1)
        r.temporal_accumulate(mcpt_mod.mat4_inverse(cam[0]) if k else None)
        r.denoise_temporal(3)
    for phase in ("on", "ended"):
        same_bits(r.denoise(3), fixed, ("denoise", phase))
        same_bits(r.denoise_variance(3), var, ("denoise_variance", phase))
        same_bits(r.read_denoised_variance(), vvar, ("variance", phase))
        r.temporal_end()
    assert mcpt_mod.lib().mcpt_denoise_temporal(r._h, 3, 1.0, 1.0) == NO_TEMPORAL


def rmse(a, b):
    return float(np.sqrt(np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2)))


@pytest.mark.parametrize("step", [0.0, 1.0])
def test_quality_last_frame(mcpt_mod, renderer, step):
    """Scene 6 at 96x54, 8 frames of 4 spp, 8 bounces, the defaults: the last frame's
    mcpt_denoise_temporal is closer (RMSE) to a 2,048-spp render of the last camera than
    mcpt_denoise_variance of that frame alone.  The ratio is printed."""
    r, W, H, B, frames = renderer, 96, 54, 8, 8
    upload(mcpt_mod, r, 6, W, H)
    r.temporal_begin()
    prev = None
    for k in range(frames):
        ipv, iv, pv = tr.orbit_camera(mcpt_mod, W, H, k * step)
        render_frame(r, (ipv, iv), 1 + 4 * k, bounces=B)
        rec = r.temporal_accumulate(prev)
        prev = pv
    alone = r.denoise_variance()
    temporal = r.denoise_temporal()
    r.stats_end()
    r.clear_accum()
    r.render(ipv, iv, 1001, 2048, 0.0, B, 1.0, 0)
    ref = r.read_image()
    e_alone, e_temporal = rmse(alone, ref), rmse(temporal, ref)
    print(f"scene 6 step {step}: rmse alone {e_alone:.5f} temporal {e_temporal:.5f} ratio {e_temporal / e_alone:.3f} "
          f"mean_len {rec['sum_len'] / rec['n_px']:.2f}")
    r.temporal_end()
    assert rec["max_len"] == min(frames, mcpt_mod.TEMPORAL_MAX_HISTORY)
    assert e_temporal < e_alone, (step, e_alone, e_temporal)
