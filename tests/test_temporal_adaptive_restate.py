"""Temporal adaptive sampling's arithmetic contract, restated in numpy float32 on top
of the existing restatements: the resolved accumulate is test_temporal_restate's accumulate fed accum /
(float)count, the select's step A the adaptive restatement's map and raw record without its retirement,
and only the dry run's rt, the block rule and the record are stated here, so that
tests/test_gpu_temporal_adaptive.py can pin the HIP kernels bit for bit.  CPU checks of the restatement
on the synthetic plane-guides fixture and of the binding's new entry points."""
import copy

import numpy as np
import pytest

import test_adaptive_restate as ar
import test_filtered_select_restate as fs
import test_stats_restate as st
import test_temporal_restate as tr

F = np.float32
bits = st.bits
R_MAX = st.R_MAX
VMAX = tr.VMAX
FLOOR = 0.01
T_KEYS = ("n_px_t", "n_above_t", "sum_qt", "max_rt", "mean_rt", "n_history")


def current_resolved(accum, counts, se):
    """{c, v} H x W x 4: accum / (float)count with the pixel's own count (ar.resolve) and min(se^2, 2^60)."""
    c = ar.resolve(accum, counts)
    with np.errstate(all="ignore"):
        t = (np.asarray(se, np.float32) * np.asarray(se, np.float32)).astype(np.float32)
        v = np.where(t < VMAX, t, VMAX).astype(np.float32)
    return np.concatenate([c, v[..., None]], axis=-1).astype(np.float32)


def accumulate_resolved(accum, counts, se, guides, hist, prevPV, max_history, plane_tol):
    """mcpt_temporal_accumulate_resolved: tr.accumulate fed accum / count."""
    return tr.accumulate(current_resolved(accum, counts, se), guides, hist, prevPV, max_history, plane_tol)


def dry_run(ad, accum, guides, hist, prevPV, max_history, plane_tol, mu_floor, fresh):
    """What the resolved accumulate would write now and its rt per pixel; n_history over `fresh` pixels
    (a pixel's result depends on its own words and the history alone, so the others are masked out as
    misses for the count)."""
    new, _ = accumulate_resolved(accum, ar.counts(ad), ad["map"][..., 0], guides, hist, prevPV, max_history, plane_tol)
    rt = fs.filtered_error(new["c"], mu_floor)
    masked = dict(guides)
    masked["key"] = np.where(fresh, guides["key"], -1).astype(guides["key"].dtype)
    _, rec = accumulate_resolved(accum, ar.counts(ad), ad["map"][..., 0], masked, hist, prevPV, max_history, plane_tol)
    return new, rt, rec["n_history"]


def select_temporal(ad, state, accum, guides, hist, prevPV, max_history, plane_tol, threshold, mu_floor=FLOOR):
    """Steps A and T on a test_stats_restate state, a test_adaptive_restate block state, the accumulator,
    the current guides and the history (None: empty; never changed).  Returns (record with flat keys,
    rt H x W with 0 outside the blocks active on entry, the per-block maxima of it)."""
    entry = ad["active"].copy()
    rec = fs.step_a(ad, state, threshold, mu_floor)
    fresh = entry[ad["ids"]]
    _, rt, n_hist = dry_run(ad, accum, guides, hist, prevPV, max_history, plane_tol, mu_floor, fresh)
    rt = np.where(fresh, rt, F(0)).astype(np.float32)
    bmax = fs.block_max(ad, rt)
    ad["active"] = entry & ((bmax > F(threshold)) | (ad["passes"] < ad["min_passes"]))
    sel = rt[fresh]
    with np.errstate(all="ignore"):
        q = (sel * st.Q_SCALE).astype(np.uint32)
    t = st.record(sel, q, threshold)
    rec.update({"n_px_t": t["n_px"], "n_above_t": t["n_above"], "sum_qt": t["sum_q"], "max_rt": t["max_r"],
                "mean_rt": t["mean_r"], "n_history": int(n_hist)})
    rec["n_active_blocks"] = int(ad["active"].sum())
    return rec, rt, bmax


def split_threshold(bmax, entry):
    """The midpoint between two distinct adjacent values of the sorted maxima of the blocks active on
    entry (the middle pair), or None when they hold fewer than two distinct values."""
    u = np.unique(np.asarray(bmax, np.float32)[entry])
    if u.size < 2:
        return None
    k = u.size // 2
    return float((np.float64(u[k - 1]) + np.float64(u[k])) / 2)


# ---- CPU checks of the restatement -------------------------------------------------------------
def _scene(mcpt, W, H, seed, sigma=None, n_batches=4, n=2, min_passes=0):
    """Plane guides under the canonical camera with ar._state's statistics: (guides, pv, ad, state, accum)."""
    ipv, iv = mcpt.camera_canonical(W, H)
    g = tr.plane_guides(mcpt, W, H, ipv, iv)
    rng = np.random.default_rng(seed)
    if sigma is None:
        sigma = rng.uniform(0.02, 0.3, (H, W))
    s, acc = ar._state(H, W, sigma, n_batches=n_batches, n=n, seed=seed)
    ad = ar.begin(W, H, 0, min_passes)
    ar.rendered(ad, n_batches * n)
    return g, mcpt.mat4_inverse(ipv), ad, s, acc


def _history(g, pv, frames, seed, v=1e-4, max_history=32):
    """A history of `frames` same-camera accumulates of quiet frames (variance v)."""
    rng = np.random.default_rng(seed)
    H, W = g["key"].shape
    hist = None
    for _ in range(frames):
        cv = np.empty((H, W, 4), np.float32)
        cv[..., :3] = rng.uniform(0.9, 1.1, (H, W, 3))
        cv[..., 3] = v
        hist, _ = tr.accumulate(cv, g, hist, pv, max_history, 0.01)
    return hist


def test_empty_history_is_the_raw_rule_on_c_v(mcpt_mod):
    g, pv, ad, s, acc = _scene(mcpt_mod, 16, 12, 1)
    probe = copy.deepcopy(ad)
    _, rt, bmax = select_temporal(probe, s, acc, g, None, None, 8, 0.01, 1e-9)
    cv = current_resolved(acc, ar.counts(ad), probe["map"][..., 0])
    assert np.array_equal(bits(rt), bits(fs.filtered_error(cv, FLOOR)))          # every pixel NEW: out = {c, v}
    thr = split_threshold(bmax, ad["active"])
    rec, rt2, _ = select_temporal(ad, s, acc, g, None, None, 8, 0.01, thr)
    assert rec["n_history"] == 0 and rec["n_px_t"] == 16 * 12 and np.array_equal(bits(rt2), bits(rt))
    assert ar.active_list(ad).tolist() == [b for b in range(4) if bmax[b] > F(thr)]
    assert 0 < rec["n_active_blocks"] < 4
    assert rec["n_above_t"] == int((rt > F(thr)).sum()) and bits(rec["max_rt"]) == bits(rt.max())
    assert rec["sum_qt"] == int((rt * st.Q_SCALE).astype(np.uint32).astype(np.uint64).sum())
    assert rec["mean_rt"] == rec["sum_qt"] / 65536.0 / (16 * 12)
    # the raw half is step A's: select's record of the same state but for the active blocks
    raw = ar.select(copy.deepcopy(probe), s, thr, FLOOR)
    assert all(rec[k] == raw[k] for k in ("n_px", "n_above", "sum_q", "mean_r", "samples", "passes", "batches"))


def test_no_block_retired_accumulate_resolved_equals_accumulate(mcpt_mod):
    g, pv, ad, s, acc = _scene(mcpt_mod, 16, 12, 2)
    se, _, _ = st.error(s, FLOOR)
    hist = _history(g, pv, 3, 2)
    cnt = ar.counts(ad)
    assert (cnt == 8).all()
    a, ra = accumulate_resolved(acc, cnt, se, g, hist, pv, 8, 0.01)
    b, rb = tr.accumulate(tr.current(acc, 8, se), g, hist, pv, 8, 0.01)
    assert ra == rb and ra["n_history"] > 0
    assert np.array_equal(bits(a["c"]), bits(b["c"])) and np.array_equal(a["len"], b["len"])
    # a retired block divides by its own count
    ad["active"][0] = False
    ar.rendered(ad, 2)
    c, _ = accumulate_resolved(acc, ar.counts(ad), se, g, None, None, 8, 0.01)
    assert np.array_equal(bits(c["c"][:8, :8, :3]), bits(acc[:8, :8] / F(8)))
    assert np.array_equal(bits(c["c"][:8, 8:, :3]), bits(acc[:8, 8:] / F(10)))


def test_max_history_one_never_blends(mcpt_mod):
    g, pv, ad, s, acc = _scene(mcpt_mod, 16, 12, 3)
    hist = _history(g, pv, 4, 3)
    a = copy.deepcopy(ad)
    rec1, rt1, _ = select_temporal(a, s, acc, g, hist, pv, 1, 0.01, 0.1)
    rec0, rt0, _ = select_temporal(copy.deepcopy(ad), s, acc, g, None, None, 1, 0.01, 0.1)
    assert np.array_equal(bits(rt1), bits(rt0))                      # k = 0, a = 1: the blend is {c, v}
    assert rec1["n_history"] == int((g["key"] >= 0).sum()) and rec0["n_history"] == 0
    assert all(bits(F(rec1[k])) == bits(F(rec0[k])) for k in ("n_above_t", "sum_qt", "max_rt", "n_active_blocks"))
    new, rec = accumulate_resolved(acc, ar.counts(a), a["map"][..., 0], g, hist, pv, 1, 0.01)
    assert np.array_equal(bits(new["c"]), bits(current_resolved(acc, ar.counts(a), a["map"][..., 0])))
    assert rec["max_len"] == 1


def test_long_history_retires_a_block_an_empty_history_keeps(mcpt_mod):
    W, H = 16, 12
    g, pv, ad, s, acc = _scene(mcpt_mod, W, H, 4, sigma=np.full((H, W), 0.5))
    hit = g["key"] >= 0
    assert hit[:8, :].all()                                          # blocks 0 and 1 (rows 0..7) hold hits only
    hist = _history(g, pv, 8, 4)
    assert (hist["len"][hit] == 8).all()
    empty, held = copy.deepcopy(ad), copy.deepcopy(ad)
    _, _, b_empty = select_temporal(copy.deepcopy(ad), s, acc, g, None, None, 8, 0.01, 1e-9)
    _, _, b_held = select_temporal(copy.deepcopy(ad), s, acc, g, hist, pv, 8, 0.01, 1e-9)
    assert (b_held[:2] < b_empty[:2]).all()                          # a = 1/8: the blend's sd is about 1/8 of v's
    thr = float(b_held[:2].max() + b_empty[:2].min()) / 2
    re_, _, _ = select_temporal(empty, s, acc, g, None, None, 8, 0.01, thr)
    rh, _, _ = select_temporal(held, s, acc, g, hist, pv, 8, 0.01, thr)
    assert {0, 1} <= set(ar.active_list(empty).tolist()) and not held["active"][:2].any()
    assert rh["n_active_blocks"] < re_["n_active_blocks"] and rh["n_history"] == int(hit.sum())
    assert np.array_equal(bits(empty["map"]), bits(held["map"]))     # step A does not see the history


def test_nan_or_inf_colour_counts_64(mcpt_mod):
    g, pv, ad, s, acc = _scene(mcpt_mod, 16, 12, 5)
    hist = _history(g, pv, 2, 5)
    hit = np.argwhere(g["key"] >= 0)
    (ya, xa), (yb, xb) = hit[len(hit) // 3], hit[2 * len(hit) // 3]
    acc = acc.copy()
    acc[ya, xa, 1], acc[yb, xb, 0] = np.nan, np.inf
    rec, rt, bmax = select_temporal(ad, s, acc, g, hist, pv, 8, 0.01, 63.0)
    assert bits(rt[ya, xa]) == bits(R_MAX) and bits(rt[yb, xb]) == bits(R_MAX) and bits(rec["max_rt"]) == bits(R_MAX)
    ids = ad["ids"]
    assert sorted(set(ar.active_list(ad).tolist())) == sorted({int(ids[ya, xa]), int(ids[yb, xb])})
    assert rec["n_above_t"] == 2 and np.isfinite(rt).all()


@pytest.mark.parametrize("W,H", [(37, 21), (3, 2)])
def test_partial_blocks(mcpt_mod, W, H):
    g, pv, ad, s, acc = _scene(mcpt_mod, W, H, 6 + W)
    hist = _history(g, pv, 3, 6 + W)
    ad["active"][0] = W > 8                                          # 37x21: fifteen blocks, one retired below
    if W > 8:
        ad["active"][7] = False
        ad["map"][ad["ids"] == 7] = (0.25, 0.5)
    stale = ad["map"].copy()
    entry = ad["active"].copy()
    probe = copy.deepcopy(ad)
    _, rt, bmax = select_temporal(probe, s, acc, g, hist, pv, 8, 0.01, 1e-9)
    bx, by = ar.grid(W, H)
    for b in range(bx * by):                                         # maxima over the in-frame pixels only
        y0, x0 = (b // bx) * 8, (b % bx) * 8
        want = rt[y0:y0 + 8, x0:x0 + 8].max() if entry[b] else F(0)
        assert bits(bmax[b]) == bits(F(want)), b
    thr = split_threshold(bmax, entry)
    if thr is None:                                                  # 3x2 with its one block off: nothing to do
        rec, _, _ = select_temporal(ad, s, acc, g, hist, pv, 8, 0.01, 0.1)
        assert rec["n_px_t"] == 0 and rec["mean_rt"] == 0.0 and rec["n_active_blocks"] == 0 and rec["n_history"] == 0
        return
    rec, rt, _ = select_temporal(ad, s, acc, g, hist, pv, 8, 0.01, thr)
    fresh = entry[ad["ids"]]
    assert rec["n_px_t"] == int(fresh.sum()) == W * H - 64 and rec["n_px"] == W * H
    assert 0 < rec["n_active_blocks"] < int(entry.sum()) and not ad["active"][7]
    assert ar.active_list(ad).tolist() == [b for b in range(bx * by) if entry[b] and bmax[b] > F(thr)]
    assert np.array_equal(bits(ad["map"][ad["ids"] == 7]), bits(stale[ad["ids"] == 7]))
    assert (rt[~fresh] == 0).all() and rec["n_history"] == int(((g["key"] >= 0) & fresh).sum())


def test_one_block_3x2(mcpt_mod):
    g, pv, ad, s, acc = _scene(mcpt_mod, 3, 2, 9)
    rec, rt, bmax = select_temporal(ad, s, acc, g, None, None, 8, 0.01, 1e-9)
    assert rec["n_px_t"] == 6 and rec["n_blocks"] == 1 and rec["n_active_blocks"] == 1
    assert bits(bmax[0]) == bits(rt.max())
    rec, _, _ = select_temporal(ad, s, acc, g, None, None, 8, 0.01, 60.0)
    assert rec["n_active_blocks"] == 0 and rec["n_px_t"] == 6


def test_min_passes_holds_a_block(mcpt_mod):
    g, pv, ad, s, acc = _scene(mcpt_mod, 16, 12, 10, min_passes=10)
    rec, _, _ = select_temporal(ad, s, acc, g, None, None, 8, 0.01, 60.0)
    assert rec["n_above_t"] == 0 and rec["n_active_blocks"] == 4      # 8 < 10
    ar.rendered(ad, 2)
    assert select_temporal(ad, s, acc, g, None, None, 8, 0.01, 60.0)[0]["n_active_blocks"] == 0


def test_dry_run_leaves_the_history_untouched(mcpt_mod):
    g, pv, ad, s, acc = _scene(mcpt_mod, 16, 12, 11)
    hist = _history(g, pv, 3, 11)
    before = copy.deepcopy(hist)
    select_temporal(ad, s, acc, g, hist, pv, 8, 0.01, 0.05)
    assert set(hist) == set(before)
    for k in hist:
        assert hist[k].dtype == before[k].dtype and np.array_equal(bits(hist[k]) if hist[k].dtype == np.float32
                                                                   else hist[k], bits(before[k])
                                                                   if hist[k].dtype == np.float32 else before[k]), k


def test_binding_argument_checks_need_no_device(mcpt_mod):
    L = mcpt_mod.lib()
    trec, arec, run = mcpt_mod.TemporalRecord(), mcpt_mod.AdaptiveTemporal(), mcpt_mod.AdaptiveRun()
    assert L.mcpt_temporal_accumulate_resolved(None, None, 8, 0.01, trec) == -1
    assert L.mcpt_adaptive_select_temporal(None, None, 8, 0.01, 0.05, 0.01, arec) == -1
    recs = (mcpt_mod.AdaptiveTemporal * 2)()
    cam = mcpt_mod.camera_canonical(8, 8)
    assert L.mcpt_adaptive_run_temporal(None, mcpt_mod._fp(cam[0]), mcpt_mod._fp(cam[1]), 1, 2, 2, 1, 0.05, 0.01, None,
                                        8, 0.01, 0.0, 3, 1.0, 0, recs, 2, run) == -1
    names = [n for n, _ in mcpt_mod.AdaptiveTemporal._fields_]
    assert names == ["raw"] + list(T_KEYS)
    assert [n for n, _ in mcpt_mod.Adaptive._fields_] == [n for n, _ in type(arec.raw)._fields_]
    assert 0 < mcpt_mod.TEMPORAL_TARGET < 64
    for meth in ("temporal_accumulate_resolved", "adaptive_select_temporal", "adaptive_run_temporal",
                 "render_frame_temporal_adaptive"):
        assert callable(getattr(mcpt_mod.Renderer, meth))
    r = object.__new__(mcpt_mod.Renderer)           # no context: the checks below come before any call
    r._h = None
    for cap, n, thr in ((3, 2, 0.05), (4, 0, 0.05), (16, 2, 0.0), (16, 2, float("nan"))):
        with pytest.raises(mcpt_mod.MCPTError):
            r.render_frame_temporal_adaptive(cam[0], cam[1], None, 1, cap, n, thr)
    import os
    hdr = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "mcpt.h")).read()
    for name in ("mcpt_temporal_accumulate_resolved(", "mcpt_adaptive_select_temporal(", "mcpt_adaptive_run_temporal(",
                 "mcpt_adaptive_temporal_t;"):
        assert name in hdr, name
