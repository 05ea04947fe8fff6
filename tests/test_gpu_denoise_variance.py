"""The variance-propagating à-trous filter on the GPU ("Variance filter"), colour and
variance bit for bit against the numpy float32 restatement (tests/test_variance_restate.py) fed the
GPU's own read_accum, read_guides and read_error_map; both kernel paths, the resolved form, a
gathered frame, every error path, the CLI and the quality at the default k."""
import os
import subprocess

import numpy as np
import pytest
import torch

import test_adaptive_restate as ar
import test_variance_restate as vr
from test_cpp_host import read_pfm
from test_meshes import mesh_scene

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
APP = os.path.join(REPO, "montecarlo-pathtracing_amd", "bin", "mcpt_render")
bits = vr.bits
K, SP = 3.0, 0.75        # widths of the bit-equality cases (any positive values: the contract is the same)
NO_ADAPTIVE, NO_STATS, NO_GUIDES, NO_TARGET, INVALID = -9, -8, -7, -3, -1
BATCHES = ((1, 4), (5, 4), (9, 4), (13, 4))      # 16 spp as 4 batches of 4


@pytest.fixture(scope="module")
def renderer(mcpt_mod):
    r = mcpt_mod.Renderer(0)
    yield r
    r.close()


def status(mcpt_mod, fn, *args):
    with pytest.raises(mcpt_mod.MCPTError) as e:
        fn(*args)
    return str(e.value)


def setup(mcpt_mod, r, scene, W, H, bounces=4, rows=None, batches=BATCHES):
    """Scene, target, a statistics window over the batches, the error map, the guides."""
    sc = mesh_scene(mcpt_mod) if scene == "mesh" else mcpt_mod.Scene.reference(scene)
    r.upload_scene(sc)
    if rows is None:
        r.set_target(W, H)
    else:
        r.set_target_rows(W, H, rows)
    cam = mcpt_mod.camera_canonical(W, H)
    r.stats_begin()
    for first, n in batches:
        r.render(cam[0], cam[1], first, n, 0.0, bounces, 1.0, 0)
    r.convergence(0.05)
    r.render_guides(*cam)
    return cam


def same_bits(got, want, what):
    same = bits(got) == bits(want)
    assert same.all(), (what, int((~same).sum()), np.argwhere(~same)[:4].tolist())


def check_against_restatement(r, iterations, first_input=None, form=None):
    """Colour and variance of every iteration count against the restatement of the GPU's inputs."""
    acc, n = r.read_accum()
    g = r.read_guides()
    se = r.read_error_map()[..., 0]
    first = vr.rs.average(acc, n) if first_input is None else first_input
    form = form or r.denoise_variance
    for it in iterations:
        img = form(it, K, SP)
        var = r.read_denoised_variance()
        ref = vr.denoise_variance4(first, g["key"], g["normal"], g["position"], se, it, K, SP)
        same_bits(img, ref[..., :3], ("colour", it))
        same_bits(var, ref[..., 3], ("variance", it))
    return acc, n, g, se


def test_scene6_every_iteration_count(mcpt_mod, renderer):
    """96x54, 16 spp in 4 batches, iterations 0..5: the init step alone, then every step."""
    setup(mcpt_mod, renderer, 6, 96, 54)
    acc, n, g, se = check_against_restatement(renderer, [0, 1, 2, 3, 4, 5])
    assert n == 16 and len(np.unique(g["key"])) >= 3 and (se > 0).any()
    assert renderer.denoise_iteration_ms(-1) > 0.0 and renderer.denoise_iteration_ms(4) > 0.0
    assert renderer.last_denoise_ms()[1] > 0.0
    # the filter does what it is for: the carried variance shrinks, and it is another image than the guided one
    renderer.denoise_variance(0, K, SP)
    v0 = renderer.read_denoised_variance()
    renderer.denoise_variance(5, K, SP)
    v5 = renderer.read_denoised_variance()
    assert np.median(v5[se > 0]) < 0.1 * np.median(v0[se > 0])
    assert not np.array_equal(bits(renderer.denoise_variance(3, K, SP)), bits(renderer.denoise_guided(3, K, SP)))


def test_lds_and_global_tap_kernels_same_bits(mcpt_mod, renderer, monkeypatch):
    """83x53: 6 x 4 tiles of 16x16 with interior tiles and partial edge tiles on both axes."""
    setup(mcpt_mod, renderer, 6, 83, 53)
    monkeypatch.setenv("MCPT_DENOISE_NAIVE", "0")
    check_against_restatement(renderer, [5])
    a, va = renderer.denoise_variance(5, K, SP), renderer.read_denoised_variance()
    assert renderer.last_denoise_path() == 0b00011
    monkeypatch.setenv("MCPT_DENOISE_NAIVE", "1")
    b, vb = renderer.denoise_variance(5, K, SP), renderer.read_denoised_variance()
    assert renderer.last_denoise_path() == 0
    assert np.array_equal(bits(a), bits(b)) and np.array_equal(bits(va), bits(vb))


@pytest.mark.parametrize("W,H", [(1, 1), (3, 2), (7, 5)])
def test_frames_smaller_than_a_halo(mcpt_mod, renderer, W, H):
    setup(mcpt_mod, renderer, 6, W, H)
    check_against_restatement(renderer, [0, 1, 3, 5])


def test_mesh_scene(mcpt_mod, renderer):
    setup(mcpt_mod, renderer, "mesh", 45, 37)
    _, _, g, _ = check_against_restatement(renderer, [0, 5])
    assert ((g["key"] >> 28) == 0).sum() > 50


def test_synthetic_accumulator_and_error_map(mcpt_mod, renderer):
    """Seeded random sums through write_accum and a synthetic {se, r} map through
    load_rows_error_map at 83x53, with se = 0, +inf and NaN pixels (corners, a tile seam, next to a
    key edge) and a region of se = 0: every output finite, the variance at most VMAX."""
    W, H = 83, 53
    renderer.upload_scene(mcpt_mod.Scene.reference(6))
    renderer.set_target(W, H)
    renderer.render_guides(*mcpt_mod.camera_canonical(W, H))
    rng = np.random.default_rng(21)
    acc = (rng.uniform(0, 40, (H, W, 3)) * rng.uniform(0, 1, (H, W, 1)) ** 4).astype(np.float32)
    acc[10:25, 60:80] = 0.0
    renderer.write_accum(acc, 7)
    emap = np.zeros((H, W, 2), np.float32)
    emap[..., 0] = rng.uniform(0, 0.5, (H, W)) ** 2
    emap[..., 1] = rng.uniform(0, 1, (H, W))
    emap[30:40, 5:30, 0] = 0.0
    for (y, x), val in {(0, 0): np.nan, (52, 82): np.inf, (15, 16): np.inf, (16, 15): np.nan, (31, 47): 0.0,
                        (32, 48): np.inf, (26, 40): np.nan, (26, 41): np.nan, (3, 70): 1e25}.items():
        emap[y, x, 0] = val
    buf = torch.from_numpy(emap.view(np.int32).copy()).to("cuda:0")
    torch.cuda.synchronize()
    renderer.load_rows_error_map(buf.data_ptr(), H, np.arange(H, dtype=np.int32))
    assert renderer.error_map_source() == 2
    got = renderer.read_error_map()
    assert np.array_equal(bits(got), bits(emap))
    _, n, _, se = check_against_restatement(renderer, [0, 1, 5])
    assert n == 7 and np.isnan(se).sum() == 4 and np.isinf(se).sum() == 3
    for it in (0, 5):
        img, var = renderer.denoise_variance(it, K, SP), renderer.read_denoised_variance()
        assert np.isfinite(img).all() and np.isfinite(var).all() and (var >= 0).all() and (var <= vr.VMAX).all()
    renderer.denoise_variance(0, K, SP)
    assert renderer.read_denoised_variance()[0, 0] >= vr.VMAX * np.float32(0.25)       # a NaN centre: VMAX in its place


def test_resolved_form(mcpt_mod, monkeypatch):
    """An adaptive render with retired blocks: the resolved form over accum / (float)count, both
    paths; before any block retires it equals the unresolved form's bits."""
    W, H = 45, 37
    r = mcpt_mod.Renderer(0)
    try:
        r.upload_scene(mcpt_mod.Scene.reference(6))
        r.set_target(W, H)
        cam = mcpt_mod.camera_canonical(W, H)
        r.render_guides(*cam)
        assert f"({NO_ADAPTIVE})" in status(mcpt_mod, r.denoise_resolved_variance, 2)   # no per-pixel counts
        r.stats_begin()
        r.adaptive_begin(0)
        r.render_adaptive(cam[0], cam[1], 1, 4, 0.0, 4, 1.0, 0)
        assert f"({NO_STATS})" in status(mcpt_mod, r.denoise_resolved_variance, 2)      # one batch: no map
        r.render_adaptive(cam[0], cam[1], 5, 4, 0.0, 4, 1.0, 0)
        r.convergence(0.05)
        rmap = r.read_error_map()[..., 1]
        info = r.adaptive_info()
        assert info["n_active"] == info["n_blocks"] == 30
        plain, vplain = r.denoise_variance(3, K, SP), r.read_denoised_variance()
        same_bits(r.denoise_resolved_variance(3, K, SP), plain, "nothing retired: colour")
        same_bits(r.read_denoised_variance(), vplain, "nothing retired: variance")
        # retire about half of the blocks: the threshold is the median of the blocks' largest r
        block_max = [rmap[y:y + 8, x:x + 8].max() for y in range(0, H, 8) for x in range(0, W, 8)]
        rec = r.adaptive_select(float(np.median(block_max)))
        assert 0 < rec["n_active_blocks"] < rec["n_blocks"], rec
        r.render_adaptive(cam[0], cam[1], 9, 8, 0.0, 4, 1.0, 0)
        r.adaptive_select(1e-6)                                                         # the map of the 16-pass window
        cnt = r.read_sample_counts()
        assert sorted(np.unique(cnt).tolist()) == [8, 16]
        assert f"({INVALID})" in status(mcpt_mod, r.denoise_variance, 3)                # blocks retired
        res = ar.resolve(r.read_accum()[0], cnt)
        assert np.array_equal(bits(r.read_resolved()), bits(res))
        monkeypatch.setenv("MCPT_DENOISE_NAIVE", "0")
        check_against_restatement(r, [0, 3], first_input=res, form=r.denoise_resolved_variance)
        a, va = r.denoise_resolved_variance(3, K, SP), r.read_denoised_variance()
        assert r.last_denoise_path() == 0b011 and r.denoise_iteration_ms(-1) > 0.0
        monkeypatch.setenv("MCPT_DENOISE_NAIVE", "1")
        b, vb = r.denoise_resolved_variance(3, K, SP), r.read_denoised_variance()
        assert r.last_denoise_path() == 0
        assert np.array_equal(bits(a), bits(b)) and np.array_equal(bits(va), bits(vb))
        assert np.array_equal(r.read_sample_counts(), cnt)
    finally:
        r.close()


def test_two_row_shards_gathered(mcpt_mod, renderer):
    """Two row shards on device 0 through mcpt_gather_rows + mcpt_gather_error_map: the full-frame
    context's bits, colour and variance."""
    W, H = 45, 37
    rows_a = [y for y in range(H) if (y // 5) % 2 == 0]
    rows_b = [y for y in range(H) if (y // 5) % 2 == 1]
    cam = setup(mcpt_mod, renderer, 6, W, H)
    want, vwant = renderer.denoise_variance(4, K, SP), renderer.read_denoised_variance()
    made = [mcpt_mod.Renderer(0) for _ in range(3)]
    try:
        a, b, frame = made
        setup(mcpt_mod, a, 6, W, H, rows=rows_a)
        setup(mcpt_mod, b, 6, W, H, rows=rows_b)
        assert f"({INVALID})" in status(mcpt_mod, a.denoise_variance, 2)                # a shard target
        frame.upload_scene(mcpt_mod.Scene.reference(6))
        frame.set_target(W, H)
        frame.render_guides(*cam)
        frame.gather_rows([a, b])
        assert f"({NO_STATS})" in status(mcpt_mod, frame.denoise_variance, 2)           # the rows alone: no map
        frame.gather_error_map([a, b])
        assert frame.error_map_source() == 2
        same_bits(frame.denoise_variance(4, K, SP), want, "colour")
        same_bits(frame.read_denoised_variance(), vwant, "variance")
        assert f"({NO_ADAPTIVE})" in status(mcpt_mod, frame.denoise_resolved_variance, 2)   # a plain gather: no counts
    finally:
        for r in made:
            r.close()


def test_error_paths_and_untouched_state(mcpt_mod, renderer):
    L = mcpt_mod.lib()
    W, H = 45, 37
    fresh = mcpt_mod.Renderer(0)
    try:
        assert L.mcpt_denoise_variance(fresh._h, 3, 1.0, 1.0) == NO_TARGET
        assert L.mcpt_denoise_resolved_variance(fresh._h, 3, 1.0, 1.0) == NO_TARGET
        assert L.mcpt_read_denoised_variance(fresh._h, mcpt_mod._fp(np.zeros(4, np.float32))) == NO_TARGET
    finally:
        fresh.close()
    r = renderer
    sc = mcpt_mod.Scene.reference(6)
    cam = mcpt_mod.camera_canonical(W, H)
    r.upload_scene(sc)
    r.set_target(W, H)
    h = r._h
    vbuf = np.zeros((H, W), np.float32)
    r.render(cam[0], cam[1], 1, 2, 0.0, 3, 1.0, 0)
    assert L.mcpt_denoise_variance(h, 3, 1.0, 1.0) == NO_GUIDES                         # no guides yet
    r.render_guides(*cam)
    assert L.mcpt_denoise_variance(h, 3, 1.0, 1.0) == NO_STATS                          # statistics off
    assert L.mcpt_read_denoised_variance(h, mcpt_mod._fp(vbuf)) == NO_STATS             # no filter run at all
    r.stats_begin()
    r.render(cam[0], cam[1], 3, 2, 0.0, 3, 1.0, 0)
    assert L.mcpt_denoise_variance(h, 3, 1.0, 1.0) == NO_STATS                          # one batch, no convergence
    r.render(cam[0], cam[1], 5, 2, 0.0, 3, 1.0, 0)
    assert L.mcpt_denoise_variance(h, 3, 1.0, 1.0) == NO_STATS                          # two batches, no convergence
    r.convergence(0.05)
    assert L.mcpt_denoise_resolved_variance(h, 3, 1.0, 1.0) == NO_ADAPTIVE              # no per-pixel counts
    # the existing filters' outputs, the accumulator and the pass count around the new calls
    acc, n = r.read_accum()
    fixed, guided = r.denoise(3), r.denoise_guided(3)
    assert L.mcpt_read_denoised_variance(h, mcpt_mod._fp(vbuf)) == NO_STATS             # the last run was no variance filter
    out = np.zeros((H, W, 3), np.float32)
    for bad in ((9, 1.0, 1.0), (-1, 1.0, 1.0), (3, 0.0, 1.0), (3, -1.0, 1.0), (3, float("inf"), 1.0), (3, float("nan"), 1.0),
                (3, 1.0, 0.0), (3, 1.0, -1.0), (3, 1.0, float("inf")), (3, 1.0, float("nan"))):
        assert L.mcpt_denoise_variance(h, *bad) == INVALID, bad
        assert L.mcpt_denoise_resolved_variance(h, *bad) == INVALID, bad
    assert L.mcpt_read_denoised(h, mcpt_mod._fp(out)) == 0 and np.array_equal(bits(out), bits(guided))   # refusals write nothing
    assert L.mcpt_denoise_variance(h, 8, 1.0, 1.0) == 0 and L.mcpt_denoise_variance(h, 0, 1.0, 1.0) == 0
    img = r.denoise_variance(3)
    assert L.mcpt_read_denoised_variance(h, mcpt_mod._fp(vbuf)) == 0 and (vbuf >= 0).all()
    assert L.mcpt_read_denoised_variance(h, None) == INVALID
    assert not np.array_equal(bits(img), bits(guided)) and not np.array_equal(bits(img), bits(fixed))
    acc2, n2 = r.read_accum()
    assert n2 == n == 6 and np.array_equal(bits(acc2), bits(acc))
    assert np.array_equal(bits(r.denoise(3)), bits(fixed)) and np.array_equal(bits(r.denoise_guided(3)), bits(guided))
    assert L.mcpt_read_denoised_variance(h, mcpt_mod._fp(vbuf)) == NO_STATS
    # invalidated with the guides and with the statistics
    r.set_flat_face(True)
    assert L.mcpt_denoise_variance(h, 3, 1.0, 1.0) == NO_GUIDES
    r.set_flat_face(False)
    r.render_guides(*cam)
    assert L.mcpt_denoise_variance(h, 3, 1.0, 1.0) == 0
    r.stats_end()
    assert L.mcpt_denoise_variance(h, 3, 1.0, 1.0) == NO_STATS
    r.clear_accum()                                                                     # pass_count == 0
    assert L.mcpt_denoise_variance(h, 3, 1.0, 1.0) == INVALID
    r.set_target(W, H, 8, 2, 0)                                                         # a sharded target
    r.stats_begin()
    for first in (1, 3):
        r.render(cam[0], cam[1], first, 2, 0.0, 3, 1.0, 0)
    r.convergence(0.05)
    r.render_guides(*cam)
    assert L.mcpt_denoise_variance(h, 3, 1.0, 1.0) == INVALID
    with pytest.raises(mcpt_mod.MCPTError):
        r.denoise_variance(3)
    r.stats_end()


def rmse(a, b):
    return float(np.sqrt(np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2)))


@pytest.mark.parametrize("scene_id", [1, 6, 8])
def test_quality_default_k(mcpt_mod, renderer, scene_id):
    """96x54, 16 spp as 4 batches of 4, 8 bounces, 5 iterations at the default k: closer (RMSE) to the
    scene's own 2,048-spp render than the raw frame.  The ratios are printed (the restatement gives
    0.240 / 0.351 / 0.385 on the CPU oracle's frames at k = 16)."""
    W, H, B = 96, 54, 8
    cam = setup(mcpt_mod, renderer, scene_id, W, H, B)
    raw = renderer.read_image()
    den = renderer.denoise_variance()
    renderer.stats_end()
    renderer.render(cam[0], cam[1], 17, 2032, 0.0, B, 1.0, 0)
    ref = renderer.read_image()
    e_raw, e_den = rmse(raw, ref), rmse(den, ref)
    print(f"scene {scene_id}: rmse raw {e_raw:.5f} variance filter {e_den:.5f} ratio {e_den / e_raw:.3f}")
    assert e_den < e_raw, (scene_id, e_raw, e_den)


def test_cli_denoise_variance(mcpt_mod, renderer, tmp_path):
    """mcpt_render --denoise-variance 3 --aov writes Renderer.denoise_variance(3) and its variance, on
    one device and over two shards; the refusals are --denoise-guided's."""
    W, H, S = 45, 37, 8
    base = [APP, "--scene", "6", "--width", str(W), "--height", str(H), "--spp", str(S)]
    den, aov, den2 = str(tmp_path / "den.pfm"), str(tmp_path / "aov"), str(tmp_path / "den2.pfm")
    r1 = subprocess.run(base + ["--chunk", "4", "--denoise-variance", "3", "--pfm", den, "--aov", aov],
                        capture_output=True, text=True, timeout=120)
    assert r1.returncode == 0, r1.stderr
    assert '"denoise_variance": 3' in r1.stdout
    r2 = subprocess.run(base + ["--chunk", "4", "--denoise-variance", "3", "--pfm", den2, "--devices", "0,0"],
                        capture_output=True, text=True, timeout=120)
    assert r2.returncode == 0, r2.stderr
    cam = setup(mcpt_mod, renderer, 6, W, H, bounces=3, batches=((1, 4), (5, 4)))       # the app's defaults: 3 bounces
    want = renderer.denoise_variance(3)
    vwant = renderer.read_denoised_variance()
    renderer.stats_end()
    assert np.array_equal(bits(read_pfm(den)), bits(want))
    assert np.array_equal(bits(read_pfm(den2)), bits(want))
    var = read_pfm(aov + "_variance.pfm")
    for k in range(3):
        assert np.array_equal(bits(var[..., k]), bits(vwant))
    assert os.path.exists(aov + "_error.pfm") and os.path.exists(aov + "_normal.pfm")
    # one chunk: no error map, as --denoise-guided (a run-time error, not a usage error)
    r3 = subprocess.run(base + ["--denoise-variance", "3"], capture_output=True, text=True, timeout=120)
    assert r3.returncode == 1 and "mcpt_denoise_variance" in r3.stderr, (r3.returncode, r3.stderr)
    # refused at the command line: two filters; --devices with --adaptive; more than 8 iterations
    for extra in (["--denoise", "3", "--denoise-variance", "3"], ["--denoise-guided", "3", "--denoise-variance", "3"],
                  ["--devices", "0,0", "--adaptive", "--target-error", "0.1", "--denoise-variance", "3"],
                  ["--denoise-variance", "9"]):
        rr = subprocess.run(base + ["--chunk", "4"] + extra, capture_output=True, text=True, timeout=60)
        assert rr.returncode == 2 and "usage" in rr.stderr, (extra, rr.returncode)
