"""Adaptive sampling of 8x8 blocks on the GPU.

Every select's active list, error map and record are compared bit for bit with the numpy
restatement (tests/test_adaptive_restate.py) fed the accumulator snapshots the GPU itself returned;
at the end every pixel's accumulator bits must equal a uniform render's snapshot at that pixel's
sample count.  The thresholds are chosen on the CPU from the oracle's snapshots of the same calls
and the restatement, so that the first select retires some blocks but not all and the final counts
take three values or more; both are asserted on the GPU's results."""
import os
import subprocess
import sys

import numpy as np
import pytest

import test_adaptive_restate as ar
import test_stats_restate as st
from test_meshes import mesh_scene

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHECKED = os.path.join(REPO, "montecarlo-pathtracing_amd", "mcpt", "variants", "libmcpt_checked.so")
bits = st.bits
FLOOR = 0.01
SIZES = (4, 4, 8, 3, 32, 40)      # 32 (passes 20..51) and 40 (52..91) span a chunk boundary
ENDS = np.cumsum(SIZES)           # a pixel's possible sample counts
BOUNCES = 4
W0, H0 = 45, 37                   # 6 x 5 blocks, partial in both directions
SHARD = [3, 36, 20, 4, 11]
NO_ADAPTIVE, NO_STATS, INVALID = -9, -8, -1


@pytest.fixture(scope="module")
def renderer(mcpt_mod):
    r = mcpt_mod.Renderer(0)
    yield r
    r.close()


def scene_of(mcpt_mod, scene):
    return mesh_scene(mcpt_mod) if scene == "mesh" else mcpt_mod.Scene.reference(scene)


def target(mcpt_mod, r, scene, W, H, rows=None):
    r.upload_scene(scene_of(mcpt_mod, scene))
    if rows is None:
        r.set_target(W, H)
    else:
        r.set_target_rows(W, H, rows)
    return mcpt_mod.camera_canonical(W, H)


_oracle_cache = {}


def oracle_snapshots(mcpt_mod, orc, scene, W, H):
    """The oracle's full-frame accumulator after each call of SIZES (computed once per scene)."""
    key = (scene, W, H)
    if key not in _oracle_cache:
        sc = scene_of(mcpt_mod, scene)
        prims, nodes, leaves = sc.buffers()
        mv = orc.MeshView(sc.mesh_buffers()) if scene == "mesh" else None
        ipv, iv = orc.camera(W, H)
        acc, first, snaps = np.zeros((H, W, 3), np.float32), 1, []
        for n in SIZES:
            acc, _ = orc.render(prims, nodes, leaves, sc.depth(), ipv, iv, W, H, first, n, 0.0, BOUNCES, 1.0, 0,
                                accum=acc.copy(), meshes=mv)
            first += n
            snaps.append(acc)
        for s in snaps:
            s.setflags(write=False)
        _oracle_cache[key] = snaps
    return _oracle_cache[key]


def simulate(snaps, W, rows, thr, min_passes=0):
    """The restatement's adaptive run over uniform snapshots (valid for active blocks: they received
    every pass).  Returns (active blocks after the first select, n_blocks, final counts)."""
    ad = ar.begin(W, rows, 0, min_passes)
    state = st.begin(np.zeros((rows, W, 3), np.float32))
    first = None
    for k, n in enumerate(SIZES):
        ar.rendered(ad, n)
        st.batch(state, snaps[k], n)
        if state["B"] >= 2:
            rec = ar.select(ad, state, thr, FLOOR)
            first = rec["n_active_blocks"] if first is None else first
    return first, ad["active"].size, ar.counts(ad)


def choose_threshold(snaps, W, rows):
    """A value between two blocks' largest r at the first select whose simulated run retires some
    blocks but not all at the first select and ends with three or more distinct counts."""
    state = st.begin(np.zeros((rows, W, 3), np.float32))
    st.batch(state, snaps[0], SIZES[0])
    st.batch(state, snaps[1], SIZES[1])
    _, r, _ = st.error(state, FLOOR)
    bmax = np.zeros(ar.block_ids(W, rows).max() + 1, np.float32)
    np.maximum.at(bmax, ar.block_ids(W, rows).ravel(), r.ravel())
    v = np.unique(bmax)
    mids = [float(np.float32(0.5) * (a + b)) for a, b in zip(v[:-1], v[1:])]    # each splits the blocks
    mids = [m for m in mids if m > 0.0]
    for thr in sorted(mids, key=lambda m: abs(int((bmax <= np.float32(m)).sum()) - bmax.size // 2)):
        first, n_blocks, cnt = simulate(snaps, W, rows, thr)
        if 0 < first < n_blocks and np.unique(cnt).size >= 3:
            return thr
    raise AssertionError("no threshold gives a partial first retirement and three distinct counts")


def uniform_run(r, cam):
    """The calls of SIZES as plain renders; the accumulator after each."""
    snaps, first = [], 1
    for n in SIZES:
        r.render(cam[0], cam[1], first, n, 0.0, BOUNCES, 1.0, 0)
        first += n
        snaps.append(r.read_accum()[0])
    return snaps


def check_select(r, ad, state, thr):
    rec = r.adaptive_select(thr, FLOOR)
    ref = ar.select(ad, state, thr, FLOOR)
    print(f"N={state['N']} B={state['B']} gpu {rec}")
    for k in ("n_px", "n_above", "sum_q", "mean_r", "passes", "batches", "n_active_blocks", "n_blocks", "samples"):
        assert rec[k] == ref[k], (k, rec, ref)
    assert bits(np.float32(rec["max_r"])) == bits(ref["max_r"]), (rec, ref)
    assert r.read_active_blocks().tolist() == ar.active_list(ad).tolist()
    m = r.read_error_map()
    assert np.array_equal(bits(m), bits(ad["map"])), np.argwhere(bits(m) != bits(ad["map"]))[:4].tolist()
    info = r.adaptive_info()
    assert info == {"on": True, "n_active": ref["n_active_blocks"], "n_blocks": ref["n_blocks"]}
    return rec


def adaptive_run(r, cam, thr, W, rows, min_passes=0, plain_at=()):
    """stats_begin + adaptive_begin on a cleared target, one render_adaptive per batch (a plain
    render for the calls in plain_at), a select after every call from the second on, each compared
    with the restatement.  Returns (restatement state, accumulator, first select's record)."""
    acc, n0 = r.read_accum()
    assert n0 == 0
    state, ad = st.begin(acc), ar.begin(W, rows, 0, min_passes)
    r.stats_begin()
    r.adaptive_begin(min_passes)
    first, rec0 = 1, None
    for k, n in enumerate(SIZES):
        if k in plain_at:
            r.render(cam[0], cam[1], first, n, 0.0, BOUNCES, 1.0, 0)
        else:
            r.render_adaptive(cam[0], cam[1], first, n, 0.0, BOUNCES, 1.0, 0)
        idle = k not in plain_at and not ad["active"].any()     # an empty list: no launch, no batch
        ar.rendered(ad, n, every_block=k in plain_at)
        first += n
        acc, _ = r.read_accum()
        if not idle:
            st.batch(state, acc, n)
        if state["B"] >= 2:
            rec = check_select(r, ad, state, thr)
            rec0 = rec if rec0 is None else rec0
    return ad, acc, rec0


def check_final(r, ad, acc, uniform, W, rows):
    """Counts, accumulator bits against the uniform snapshots at each pixel's count, resolve."""
    cnt = r.read_sample_counts()
    assert np.array_equal(cnt, ar.counts(ad))
    ids = ar.block_ids(W, rows)
    for b in range(ids.max() + 1):
        assert np.unique(cnt[ids == b]).size == 1, b
    assert set(np.unique(cnt).tolist()) <= set(ENDS.tolist())
    for k, e in enumerate(ENDS):
        px = cnt == e
        assert np.array_equal(bits(acc[px]), bits(uniform[k][px])), (int(e), int(px.sum()))
    res = r.read_resolved()
    assert np.array_equal(bits(res), bits(ar.resolve(acc, cnt)))
    return cnt


@pytest.mark.parametrize("scene", [6, 8, "mesh", 1])
def test_base_case_against_restatement_and_uniform_run(mcpt_mod, oracle_mod, renderer, scene):
    """Scene 6: LDS-scene kernel, 16-wide tiles (30 blocks: an odd list leaves a workgroup with an
    empty wave); scene 8: deep BVH, SUSPEND kernel over L2; the mesh scene: 8-wide tiles; scene 1:
    staged size above kLdsScene16, 32-wide tiles, four blocks per workgroup."""
    snaps = oracle_snapshots(mcpt_mod, oracle_mod, scene, W0, H0)
    thr = choose_threshold(snaps, W0, H0)
    r = renderer
    cam = target(mcpt_mod, r, scene, W0, H0)
    uniform = uniform_run(r, cam)
    for k in range(len(SIZES)):       # the contract: the oracle's snapshots are the uniform run's
        assert np.array_equal(bits(uniform[k]), bits(snaps[k])), k
    cam = target(mcpt_mod, r, scene, W0, H0)
    ad, acc, rec0 = adaptive_run(r, cam, thr, W0, H0)
    assert 0 < rec0["n_active_blocks"] < rec0["n_blocks"] == 30, rec0      # not vacuous
    cnt = check_final(r, ad, acc, uniform, W0, H0)
    assert np.unique(cnt).size >= 3, np.unique(cnt)
    sel_ms, ren_ms = r.last_adaptive_ms()
    assert sel_ms > 0.0 and ren_ms > 0.0
    if scene != "mesh":
        # a pixel of each count against the oracle's sums of its own pass ranges, each call cut at
        # the chunk boundaries and added in order
        sc = scene_of(mcpt_mod, scene)
        prims, nodes, leaves = sc.buffers()
        oipv, oiv = oracle_mod.camera(W0, H0)
        for e in np.unique(cnt):
            y, x = np.argwhere(cnt == e)[0]
            ref, first = np.zeros((1, 3), np.float32), 1
            for n in SIZES:
                if first > e:
                    break
                lo = first
                while lo < first + n:
                    hi = min(first + n, ((lo - 1) // 32 + 1) * 32 + 1)
                    ref = ref + oracle_mod.render_pixels(prims, nodes, leaves, sc.depth(), oipv, oiv, W0, H0,
                                                         [[x, y]], lo, hi - lo, 0.0, BOUNCES, 1.0, 0)
                    lo = hi
                first += n
            assert np.array_equal(bits(acc[y, x]), bits(ref[0])), (int(e), int(x), int(y))


@pytest.mark.parametrize("W,H", [(1, 1), (7, 3)])
def test_tiny_frames(mcpt_mod, oracle_mod, renderer, W, H):
    snaps = oracle_snapshots(mcpt_mod, oracle_mod, 6, W, H)
    cam = target(mcpt_mod, renderer, 6, W, H)
    uniform = uniform_run(renderer, cam)
    # one block: a threshold between its largest r at the third and fourth select retires it there
    state = st.begin(np.zeros((H, W, 3), np.float32))
    rs = []
    for k, n in enumerate(SIZES):
        st.batch(state, snaps[k], n)
        if state["B"] >= 2:
            rs.append(float(st.error(state, FLOOR)[1].max()))
    thr = max(rs[3] * 1.0001, 1e-6)
    cam = target(mcpt_mod, renderer, 6, W, H)
    ad, acc, rec0 = adaptive_run(renderer, cam, thr, W, H)
    assert rec0["n_blocks"] == 1 and rec0["n_px"] == W * H
    check_final(renderer, ad, acc, uniform, W, H)


def test_row_shard_blocks_are_local_rows(mcpt_mod, oracle_mod, renderer):
    """Rows [3, 36, 20, 4, 11] of 45x37: one row of six blocks of 8 local rows x 8 columns."""
    full = oracle_snapshots(mcpt_mod, oracle_mod, 6, W0, H0)
    snaps = [s[SHARD] for s in full]
    thr = choose_threshold(snaps, W0, len(SHARD))
    cam = target(mcpt_mod, renderer, 6, W0, H0, SHARD)
    uniform = uniform_run(renderer, cam)
    cam = target(mcpt_mod, renderer, 6, W0, H0, SHARD)
    ad, acc, rec0 = adaptive_run(renderer, cam, thr, W0, len(SHARD))
    assert rec0["n_blocks"] == 6 and 0 < rec0["n_active_blocks"] < 6
    cnt = check_final(renderer, ad, acc, uniform, W0, len(SHARD))
    assert np.unique(cnt).size >= 3


def test_everything_retires_then_nothing_is_launched(mcpt_mod, renderer):
    cam = target(mcpt_mod, renderer, 6, W0, H0)
    r = renderer
    r.stats_begin()
    r.adaptive_begin(0)
    r.render_adaptive(cam[0], cam[1], 1, 4, 0.0, BOUNCES, 1.0, 0)
    r.render_adaptive(cam[0], cam[1], 5, 4, 0.0, BOUNCES, 1.0, 0)
    rec = r.adaptive_select(60.0, 10.0)        # r = se / (mu + 10) stays far below 60
    assert rec["n_active_blocks"] == 0 and rec["samples"] == 8 * W0 * H0
    before, n = r.read_accum()
    r.render_adaptive(cam[0], cam[1], 9, 8, 0.0, BOUNCES, 1.0, 0)      # MCPT_OK (no exception)
    after, n2 = r.read_accum()
    assert np.array_equal(bits(before), bits(after)) and n2 == n == 8
    assert (r.read_sample_counts() == 8).all() and r.read_active_blocks().size == 0
    assert r.stats_info()["batches"] == 2


def test_nothing_retires_equals_plain_render(mcpt_mod, renderer):
    """Threshold 1e-6 on scene 8, whose every block holds a noisy pixel at every select.  (Scene 6
    at this size has sky-only blocks whose passes are all equal: se = r = 0 exactly, and a block of
    r = 0 retires at any positive threshold.)"""
    cam = target(mcpt_mod, renderer, 8, W0, H0)
    uniform = uniform_run(renderer, cam)
    cam = target(mcpt_mod, renderer, 8, W0, H0)
    ad, acc, rec0 = adaptive_run(renderer, cam, 1e-6, W0, H0)
    assert rec0["n_active_blocks"] == 30 and ad["active"].all()
    assert np.array_equal(bits(acc), bits(uniform[-1]))
    assert (renderer.read_sample_counts() == ENDS[-1]).all() and renderer.read_accum()[1] == ENDS[-1]


def test_min_passes_keeps_blocks_active(mcpt_mod, oracle_mod, renderer):
    """A threshold that retires every block at the first select, held by min_passes = 17: the blocks
    stay through the selects at 8 and 16 passes and retire at 19."""
    cam = target(mcpt_mod, renderer, 6, W0, H0)
    uniform = uniform_run(renderer, cam)
    cam = target(mcpt_mod, renderer, 6, W0, H0)
    ad, acc, rec0 = adaptive_run(renderer, cam, 63.5, W0, H0, min_passes=17)
    assert rec0["n_active_blocks"] == 30 and rec0["n_above"] < rec0["n_px"]
    cnt = check_final(renderer, ad, acc, uniform, W0, H0)
    assert set(np.unique(cnt).tolist()) <= {19, 51, 91} and (cnt == 19).any()


def test_plain_render_in_between_adds_to_every_block(mcpt_mod, oracle_mod, renderer):
    """Call 3 (8 passes) is a plain mcpt_render: retired blocks receive it too, so their counts are
    no uniform run's; the counts, list, map and record still follow the restatement."""
    snaps = oracle_snapshots(mcpt_mod, oracle_mod, 6, W0, H0)
    thr = choose_threshold(snaps, W0, H0)
    cam = target(mcpt_mod, renderer, 6, W0, H0)
    ad, acc, rec0 = adaptive_run(renderer, cam, thr, W0, H0, plain_at=(2,))
    cnt = renderer.read_sample_counts()
    assert np.array_equal(cnt, ar.counts(ad))
    retired_first = cnt == 4 + 4 + 8          # retired at the first select, then the plain render
    assert retired_first.any() and 0 < rec0["n_active_blocks"] < 30
    assert np.array_equal(bits(renderer.read_resolved()), bits(ar.resolve(acc, cnt)))


def _status(mcpt_mod, fn, *args):
    with pytest.raises(mcpt_mod.MCPTError) as e:
        fn(*args)
    return str(e.value)


def test_error_paths(mcpt_mod, renderer):
    r = renderer
    cam = target(mcpt_mod, r, 6, 16, 8)
    for fn, args in ((r.adaptive_select, (0.1,)), (r.read_sample_counts, ()), (r.read_resolved, ()),
                     (r.read_active_blocks, ()), (r.render_adaptive, (cam[0], cam[1], 1, 4))):
        assert f"({NO_ADAPTIVE})" in _status(mcpt_mod, fn, *args), fn
    assert "adaptive mode is off" in _status(mcpt_mod, r.adaptive_select, 0.1)
    assert r.adaptive_info() == {"on": False, "n_active": 0, "n_blocks": 0}
    assert f"({NO_STATS})" in _status(mcpt_mod, r.adaptive_begin, 0)          # statistics off
    r.stats_begin()
    assert f"({INVALID})" in _status(mcpt_mod, r.adaptive_begin, -1)
    r.adaptive_begin(0)
    assert r.adaptive_info() == {"on": True, "n_active": 2, "n_blocks": 2}
    assert f"({NO_STATS})" in _status(mcpt_mod, r.adaptive_select, 0.1)       # B < 2
    r.render_adaptive(cam[0], cam[1], 1, 4, 0.0, BOUNCES, 1.0, 0)
    assert f"({NO_STATS})" in _status(mcpt_mod, r.adaptive_select, 0.1)
    r.render_adaptive(cam[0], cam[1], 5, 4, 0.0, BOUNCES, 1.0, 0)
    for thr, floor in ((0.0, 0.01), (-1.0, 0.01), (float("nan"), 0.01), (float("inf"), 0.01), (0.1, 0.0),
                       (0.1, float("inf"))):
        assert f"({INVALID})" in _status(mcpt_mod, r.adaptive_select, thr, floor), (thr, floor)
    # denoise: allowed before a retirement, refused after
    r.render_guides(cam[0], cam[1])
    assert r.adaptive_select(1e-6)["n_active_blocks"] == 2
    assert np.isfinite(r.denoise(2)).all()
    assert r.adaptive_select(60.0, 10.0)["n_active_blocks"] == 0
    assert f"({INVALID})" in _status(mcpt_mod, r.denoise, 2)
    assert f"({INVALID})" in _status(mcpt_mod, r.denoise_guided, 2)
    # adaptive_end, stats_end and set_target turn the mode off
    r.adaptive_end()
    assert f"({NO_ADAPTIVE})" in _status(mcpt_mod, r.read_resolved)
    assert np.isfinite(r.denoise(2)).all()
    r.adaptive_begin(0)
    r.set_target(16, 8)
    assert r.adaptive_info()["on"] is False
    assert f"({NO_ADAPTIVE})" in _status(mcpt_mod, r.adaptive_select, 0.1)
    r.stats_begin()
    r.adaptive_begin(0)
    r.stats_end()
    assert f"({NO_ADAPTIVE})" in _status(mcpt_mod, r.adaptive_select, 0.1)


def test_existing_schedule_is_untouched(mcpt_mod, oracle_mod):
    """get_schedule reports after an adaptive session what it reported before, and a plain render
    of the base case gives the bits it gives on a fresh context."""
    snaps = oracle_snapshots(mcpt_mod, oracle_mod, 6, W0, H0)
    thr = choose_threshold(snaps, W0, H0)
    fresh = mcpt_mod.Renderer(0)
    used = mcpt_mod.Renderer(0)
    try:
        cam = target(mcpt_mod, fresh, 6, W0, H0)
        ref = uniform_run(fresh, cam)
        cam = target(mcpt_mod, used, 6, W0, H0)
        uniform_run(used, cam)
        sched = used.schedule()
        cam = target(mcpt_mod, used, 6, W0, H0)
        adaptive_run(used, cam, thr, W0, H0)
        used.adaptive_end()
        assert used.schedule() == sched
        cam = target(mcpt_mod, used, 6, W0, H0)
        again = uniform_run(used, cam)
        for a, b in zip(again, ref):
            assert np.array_equal(bits(a), bits(b))
        assert used.schedule() == sched
    finally:
        fresh.close()
        used.close()


def test_render_adaptive_until(mcpt_mod, oracle_mod, renderer):
    snaps = oracle_snapshots(mcpt_mod, oracle_mod, 6, W0, H0)
    thr = choose_threshold(snaps, W0, H0)
    cam = target(mcpt_mod, renderer, 6, W0, H0)
    rec = renderer.render_adaptive_until(cam[0], cam[1], thr, batch=8, max_passes=64, bounces=BOUNCES)
    cnt = renderer.read_sample_counts()
    assert rec["rendered"] <= 64 and rec["rendered"] == cnt.max() and rec["samples"] == int(cnt.sum())
    assert rec["n_active_blocks"] == 0 or rec["rendered"] == 64
    assert np.unique(cnt).size >= 2 and cnt.min() >= 16 and (cnt % 8 == 0).all()
    acc, n = renderer.read_accum()
    assert n == rec["rendered"]
    assert np.array_equal(bits(renderer.read_resolved()), bits(ar.resolve(acc, cnt)))
    with pytest.raises(mcpt_mod.MCPTError):
        renderer.render_adaptive_until(cam[0], cam[1], 0.0)


def test_checked_build_counts_no_bounds_violation(mcpt_mod, oracle_mod, renderer, tmp_path):
    """The base case in the bounds-checked build (its own process: a process loads one libmcpt):
    no out-of-range list index or block id, and the shipped build's bits."""
    assert os.path.exists(CHECKED), f"build the checked variant first (make -C montecarlo-pathtracing_amd/csrc checked): {CHECKED}"
    snaps = oracle_snapshots(mcpt_mod, oracle_mod, 6, W0, H0)
    thr = choose_threshold(snaps, W0, H0)
    out = str(tmp_path / "checked.npz")
    env = dict(os.environ, MCPT_LIB=CHECKED)
    p = subprocess.run([sys.executable, "-u", os.path.join(REPO, "tools", "adaptive_render.py"), "--scene", "6",
                        "--size", f"{W0}x{H0}", "--threshold", repr(thr), "--bounces", str(BOUNCES), "--batches",
                        ",".join(map(str, SIZES)), "--out", out], env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-3000:]
    assert "build_flags 1" in p.stdout and "bounds_violations 0" in p.stdout, p.stdout
    cam = target(mcpt_mod, renderer, 6, W0, H0)
    ad, acc, _ = adaptive_run(renderer, cam, thr, W0, H0)
    got = np.load(out)
    assert np.array_equal(bits(got["accum"]), bits(acc))
    assert np.array_equal(got["counts"], renderer.read_sample_counts())


def test_cli_adaptive(mcpt_mod, renderer, tmp_path):
    """mcpt_render --adaptive --target-error E: the JSON fields, PREFIX_samples.pfm equal to
    read_sample_counts and the image equal to read_resolved of the library's own loop."""
    import json
    from test_cpp_host import read_pfm
    app = os.path.join(REPO, "montecarlo-pathtracing_amd", "bin", "mcpt_render")
    W, H, thr = 96, 54, 0.6
    cam = target(mcpt_mod, renderer, 1, W, H)
    rec = renderer.render_adaptive_until(cam[0], cam[1], thr, batch=16, max_passes=96)     # the app's defaults: 3 bounces
    cnt = renderer.read_sample_counts()
    assert np.unique(cnt).size >= 2, "the threshold retires nothing or everything at once"
    aov, pfm = str(tmp_path / "aov"), str(tmp_path / "img.pfm")
    out = subprocess.run([app, "--scene", "1", "--width", str(W), "--height", str(H), "--spp", "96", "--chunk", "16",
                          "--adaptive", "--target-error", repr(thr), "--aov", aov, "--pfm", pfm],
                         capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    lines = [ln for ln in out.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1
    j = json.loads(lines[0])
    assert j["adaptive"] is True and j["passes"] == rec["rendered"]
    assert j["samples"] == rec["samples"] == int(cnt.sum()) and j["n_active_blocks"] == rec["n_active_blocks"]
    assert abs(j["mean_spp"] - cnt.mean()) < 1e-3 and j["sum_q"] == rec["sum_q"]
    smp = read_pfm(aov + "_samples.pfm")
    assert np.array_equal(smp[..., 0], cnt.astype(np.float32))
    assert np.array_equal(bits(read_pfm(pfm)), bits(renderer.read_resolved()))
    assert np.array_equal(bits(read_pfm(aov + "_error.pfm")[..., :2]), bits(renderer.read_error_map()))
