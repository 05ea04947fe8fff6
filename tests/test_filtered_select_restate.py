"""The select on the denoised frame's error, restated in numpy float32 on top of
the existing restatements: step A is test_adaptive_restate's map and record without its retirement,
step B test_variance_restate's filter over the resolved colour, and only step C's arithmetic and
rule are stated here, so that tests/test_gpu_filtered_select.py can pin the HIP kernels bit for bit.
CPU checks of the restatement on synthetic states and of the binding's new entry point."""
import copy

import numpy as np

import test_adaptive_restate as ar
import test_stats_restate as st
import test_variance_restate as vr

F = np.float32
bits = st.bits
R_MAX = st.R_MAX
FLOOR = 0.01


def step_a(ad, state, threshold, mu_floor):
    """The map entries of the active blocks' pixels and the raw record (ar.select's, over fresh and
    stored values); no block retires and n_active_blocks is left to step C."""
    se, r, _ = st.error(state, mu_floor)
    fresh = ad["active"][ad["ids"]]
    ad["map"][fresh, 0] = se[fresh]
    ad["map"][fresh, 1] = r[fresh]
    rr = ad["map"][..., 1]
    with np.errstate(all="ignore"):
        q = (rr * st.Q_SCALE).astype(np.uint32)
    rec = st.record(rr, q, threshold)
    rec["passes"], rec["batches"] = state["N"], state["B"]
    rec["n_blocks"] = int(ad["active"].size)
    rec["samples"] = int(ar.counts(ad).astype(np.int64).sum())
    return rec


def filtered_error(c4, mu_floor):
    """rf per pixel from the filter's {r, g, b, v}: sqrt(v) / (max(0, Y) + mu_floor), 64 where Y is
    not finite or rf is not <= 64."""
    c4 = np.asarray(c4, np.float32)
    with np.errstate(all="ignore"):
        yf = (F(0.2126) * c4[..., 0] + F(0.7152) * c4[..., 1]) + F(0.0722) * c4[..., 2]
        sef = np.sqrt(c4[..., 3])
        rf = sef / (np.where(F(0) < yf, yf, F(0)).astype(np.float32) + F(mu_floor))
        bad = ~np.isfinite(yf) | ~(rf <= R_MAX)
        rf = np.where(bad, R_MAX, rf).astype(np.float32)
    assert yf.dtype == np.float32 and sef.dtype == np.float32
    return rf


def block_max(ad, values):
    """Per block the largest of `values` (>= 0) over its in-frame pixels."""
    out = np.zeros(ad["active"].size, np.float32)
    np.maximum.at(out, ad["ids"].ravel(), np.asarray(values, np.float32).ravel())
    return out


def step_c(ad, c4, threshold, raw_cap, mu_floor):
    """The filtered record over all pixels and the new active set."""
    rf = filtered_error(c4, mu_floor)
    stay = ad["active"] & ((block_max(ad, rf) > F(threshold)) | (block_max(ad, ad["map"][..., 1]) > F(raw_cap)) |
                           (ad["passes"] < ad["min_passes"]))
    ad["active"] = stay
    with np.errstate(all="ignore"):
        q = (rf * st.Q_SCALE).astype(np.uint32)
    f = st.record(rf, q, threshold)
    return {"n_above_f": f["n_above"], "sum_qf": f["sum_q"], "max_rf": f["max_r"], "mean_rf": f["mean_r"]}, rf


def select_filtered(ad, state, accum, key, N, P, threshold, raw_cap=64.0, mu_floor=FLOOR, iterations=5,
                    k_color=16.0, sigma_plane=1.0):
    """Steps A, B, C on a test_stats_restate state, a test_adaptive_restate block state, the
    accumulator and the guides.  Returns (record with flat keys, the filter's H x W x 4 image)."""
    rec = step_a(ad, state, threshold, mu_floor)
    first = ar.resolve(accum, ar.counts(ad))
    c4 = vr.denoise_variance4(first, key, N, P, ad["map"][..., 0], iterations, k_color, sigma_plane)
    frec, _ = step_c(ad, c4, threshold, raw_cap, mu_floor)
    rec.update(frec)
    rec["n_active_blocks"] = int(ad["active"].sum())
    return rec, c4


# ---- CPU checks of the restatement -------------------------------------------------------------
def _flat_run(W, rows, sigma, n_batches=16, n=4, seed=0, min_passes=0):
    """A flat one-key frame with ar._state's statistics: (ad, state, accum, key, N, P)."""
    s, acc = ar._state(rows, W, sigma, n_batches=n_batches, n=n, seed=seed)
    ad = ar.begin(W, rows, 0, min_passes)
    ar.rendered(ad, n_batches * n)
    key, N, P = vr._flat(rows, W)
    return ad, s, acc, key, N, P


def test_partial_blocks_13x11():
    """2 x 2 blocks, the right ones 5 wide and the lower ones 3 high: the maxima and the records
    against per-block loops over the in-frame pixels only."""
    W, rows = 13, 11
    rng = np.random.default_rng(3)
    ad, s, acc, key, N, P = _flat_run(W, rows, rng.uniform(0.1, 2.0, (rows, W)), seed=3)
    _, r, _ = st.error(s, FLOOR)
    probe = copy.deepcopy(ad)
    _, c4 = select_filtered(probe, s, acc, key, N, P, 1e-9, iterations=1)
    rf = filtered_error(c4, FLOOR)
    fm = [float(rf[y:y + 8, x:x + 8].max()) for y in (0, 8) for x in (0, 8)]
    rm = [float(r[y:y + 8, x:x + 8].max()) for y in (0, 8) for x in (0, 8)]
    assert np.array_equal(block_max(ad, rf), np.array(fm, np.float32))
    thr = float(np.sort(fm)[1] + np.sort(fm)[2]) / 2          # two blocks above, two below
    rec, _ = select_filtered(ad, s, acc, key, N, P, thr, iterations=1)
    assert ar.active_list(ad).tolist() == [b for b in range(4) if fm[b] > F(thr)] and rec["n_active_blocks"] == 2
    assert rec["n_px"] == W * rows and rec["samples"] == 64 * W * rows and rec["n_blocks"] == 4
    assert rec["n_above_f"] == int((rf > F(thr)).sum()) and rec["n_above"] == int((r > F(thr)).sum())
    assert rec["sum_qf"] == int((rf * st.Q_SCALE).astype(np.uint32).astype(np.uint64).sum())
    assert bits(rec["max_rf"]) == bits(F(max(fm))) and bits(rec["max_r"]) == bits(F(max(rm)))
    assert rec["mean_rf"] == rec["sum_qf"] / 65536.0 / (W * rows)
    # the guard alone: a cap between the blocks' raw maxima keeps exactly the blocks above it
    ad2 = copy.deepcopy(probe)
    ad2["active"][:] = True
    cap = float(np.sort(rm)[0] + np.sort(rm)[1]) / 2
    select_filtered(ad2, s, acc, key, N, P, 60.0, raw_cap=cap, iterations=1)
    assert ar.active_list(ad2).tolist() == [b for b in range(4) if rm[b] > F(cap)]


def test_superset_of_the_raw_rule_when_cap_equals_threshold():
    rng = np.random.default_rng(11)
    W, rows = 29, 19
    sigma = rng.uniform(0.0, 1.0, (rows, W)) ** 3
    _, r0, _ = st.error(ar._state(rows, W, sigma, seed=11)[0], FLOOR)
    for thr in np.quantile(r0, [0.2, 0.5, 0.8, 0.95]):
        for it in (0, 2):
            ad, s, acc, key, N, P = _flat_run(W, rows, sigma, n_batches=4, n=8, seed=11)
            raw = copy.deepcopy(ad)
            ar.select(raw, s, float(thr), FLOOR)
            select_filtered(ad, s, acc, key, N, P, float(thr), raw_cap=float(thr), iterations=it)
            assert set(ar.active_list(raw).tolist()) <= set(ar.active_list(ad).tolist())
            assert np.array_equal(bits(ad["map"]), bits(raw["map"]))          # step A writes select's map


def _grey(W, rows, island=None, seed=5):
    ad, s, acc, key, N, P = _flat_run(W, rows, np.full((rows, W), 0.5), seed=seed)
    if island is not None:
        key[island] = (1 << 28) | 9
    _, r, _ = st.error(s, FLOOR)
    thr = float(F(0.9) * block_max(ad, r).min())              # every block's largest raw r is just above
    return ad, s, acc, key, N, P, r, thr


def test_flat_field_retires_with_the_guard_disabled():
    ad, s, acc, key, N, P, r, thr = _grey(24, 16)
    raw = copy.deepcopy(ad)
    assert ar.select(raw, s, thr, FLOOR)["n_active_blocks"] == 6          # the raw rule keeps every block
    capped = copy.deepcopy(ad)
    rec, c4 = select_filtered(ad, s, acc, key, N, P, thr, raw_cap=64.0, iterations=2)
    rf = filtered_error(c4, FLOOR)
    assert rf.max() < F(thr) < r.max() and rec["n_above_f"] == 0 and rec["n_above"] > 0
    assert rec["n_active_blocks"] == 0 and ar.active_list(ad).size == 0
    assert select_filtered(capped, s, acc, key, N, P, thr, raw_cap=thr, iterations=2)[0]["n_active_blocks"] == 6


def test_one_pixel_key_island_gets_no_benefit():
    y, x = 11, 18                                             # block 5 of 3 x 2
    ad, s, acc, key, N, P, r, thr = _grey(24, 16, island=(y, x))
    s["S2"][y, x] = s["S2"].max() * F(4)                      # make it the block's noisiest pixel
    _, r, _ = st.error(s, FLOOR)
    assert r[y, x] > F(thr)
    rec, c4 = select_filtered(ad, s, acc, key, N, P, thr, raw_cap=64.0, iterations=2)
    se = ad["map"][y, x, 0]
    avg = ar.resolve(acc, ar.counts(ad))[y, x]
    assert np.array_equal(bits(c4[y, x, :3]), bits(avg)) and bits(c4[y, x, 3]) == bits(se * se)   # no taps
    want = filtered_error(np.array([avg[0], avg[1], avg[2], se * se], np.float32), FLOOR)
    rf = filtered_error(c4, FLOOR)
    assert bits(rf[y, x]) == bits(want) and abs(float(rf[y, x]) / float(r[y, x]) - 1) < 1e-5
    assert ar.active_list(ad).tolist() == [5] and rec["n_above_f"] == 1


def test_overflowed_pixel_keeps_its_block_and_counts_64():
    ad, s, acc, key, N, P, r, thr = _grey(24, 16)
    s["S2"][3, 20] = np.inf                                   # block 2
    rec, c4 = select_filtered(ad, s, acc, key, N, P, 60.0, raw_cap=64.0, iterations=2)
    assert np.isinf(ad["map"][3, 20, 0]) and bits(ad["map"][3, 20, 1]) == bits(R_MAX)
    rf = filtered_error(c4, FLOOR)
    assert bits(rf[3, 20]) == bits(R_MAX) and bits(rec["max_rf"]) == bits(R_MAX) and rec["n_above_f"] >= 1
    assert c4[3, 20, 3] <= vr.VMAX and np.isfinite(c4).all()
    # r = 64 is not above the cap: rf keeps block 2, and the blocks its VMAX reaches through the taps
    # of steps 1 and 2 (6 pixels: columns 14.., rows ..9); blocks 0 and 3 are out of reach and retire
    assert ar.active_list(ad).tolist() == [1, 2, 4, 5]
    assert rf[:, :8].max() < F(60.0)


def test_retired_blocks_stay_retired_and_enter_the_filtered_record():
    ad, s, acc, key, N, P, r, thr = _grey(24, 16)
    ad["active"][[0, 4]] = False
    ad["map"][:8, :8] = (0.25, 0.5)                           # stale entries of blocks 0 and 4
    ad["map"][8:, 8:16] = (0.125, 0.75)
    stale = ad["map"].copy()
    rec, c4 = select_filtered(ad, s, acc, key, N, P, 1e-9, iterations=1)
    assert ar.active_list(ad).tolist() == [1, 2, 3, 5] and rec["n_active_blocks"] == 4
    assert np.array_equal(bits(ad["map"][:8, :8]), bits(stale[:8, :8]))
    rf = filtered_error(c4, FLOOR)
    assert (rf > 0).all() and rec["n_above_f"] == rec["n_px"] == 24 * 16          # retired blocks' rf too
    assert rec["sum_qf"] == int((rf * st.Q_SCALE).astype(np.uint32).astype(np.uint64).sum())
    assert rec["n_above"] == int((ad["map"][..., 1] > F(1e-9)).sum())


def test_min_passes_holds_a_block():
    ad, s, acc, key, N, P = _flat_run(16, 8, np.zeros((8, 16)), n_batches=4, n=8, min_passes=40)
    rec, _ = select_filtered(ad, s, acc, key, N, P, 0.5, iterations=1)
    assert rec["n_above_f"] == 0 and rec["n_above"] == 0 and rec["n_active_blocks"] == 2      # 32 < 40
    ar.rendered(ad, 8)
    acc2 = (acc * F(1.25)).astype(np.float32)                 # (40 passes of the same mean)
    assert select_filtered(ad, s, acc2, key, N, P, 0.5, iterations=1)[0]["n_active_blocks"] == 0


def test_records_of_two_halves_split_along_a_key_edge_add_up():
    W, rows = 21, 13
    rng = np.random.default_rng(8)
    sigma = rng.uniform(0.05, 1.5, (rows, W))
    ad, s, acc, key, N, P = _flat_run(W, rows, sigma, n_batches=4, n=8, seed=8)
    key[:, 8:] = (1 << 28) | 7                                # the edge at a block boundary: x = 8
    thr, cap = 0.0102, 0.5        # the blocks' largest rf: .0115 .0078 .0103 | .0099 .0136 .0104, of r: .60 .44 .63 | .61 .46 .37
    halves = []
    for cols in (slice(0, 8), slice(8, W)):
        w = cols.stop - cols.start
        h_ad = ar.begin(w, rows, 0)
        ar.rendered(h_ad, 32)
        h_s = {k: (v[:, cols].copy() if isinstance(v, np.ndarray) else v) for k, v in s.items()}
        halves.append(select_filtered(h_ad, h_s, acc[:, cols], key[:, cols], N[:, cols], P[:, cols], thr,
                                      raw_cap=cap, iterations=3) + (h_ad,))
    rec, c4 = select_filtered(ad, s, acc, key, N, P, thr, raw_cap=cap, iterations=3)
    (ra, ca, ada), (rb, cb, adb) = halves
    assert np.array_equal(bits(c4[:, :8]), bits(ca)) and np.array_equal(bits(c4[:, 8:]), bits(cb))
    for k in ("n_px", "n_above", "sum_q", "samples", "n_blocks", "n_active_blocks", "n_above_f", "sum_qf"):
        assert rec[k] == ra[k] + rb[k], k
    assert bits(rec["max_rf"]) == bits(max(ra["max_rf"], rb["max_rf"]))
    assert bits(rec["max_r"]) == bits(max(ra["max_r"], rb["max_r"]))
    assert ar.active_list(ad).tolist() == [0, 2, 3, 4, 5]     # block 1 retires; block 3 is held by the cap alone
    whole = ad["active"].reshape(2, 3)
    assert np.array_equal(whole[:, 0], ada["active"]) and np.array_equal(whole[:, 1:].ravel(), adb["active"])


def test_binding_declares_the_filtered_select(mcpt_mod):
    L = mcpt_mod.lib()
    assert L.mcpt_adaptive_select_filtered.argtypes is not None
    assert callable(mcpt_mod.Renderer.adaptive_select_filtered)
    rec = mcpt_mod.AdaptiveFiltered()
    assert L.mcpt_adaptive_select_filtered(None, 0.1, 64.0, 0.01, 5, 16.0, 1.0, rec) == -1
    names = [n for n, _ in mcpt_mod.AdaptiveFiltered._fields_]
    assert names == ["raw", "n_above_f", "sum_qf", "max_rf", "mean_rf"]
    assert [n for n, _ in mcpt_mod.Adaptive._fields_] == [n for n, _ in type(rec.raw)._fields_]
    import inspect
    p = inspect.signature(mcpt_mod.Renderer.render_adaptive_until).parameters
    assert p["filtered"].default is False and p["raw_cap"].default == 64.0 and p["iterations"].default == 5
    import os
    hdr = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "mcpt.h")).read()
    assert "mcpt_adaptive_select_filtered(" in hdr and "mcpt_adaptive_filtered_t;" in hdr
