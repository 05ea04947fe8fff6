#!/usr/bin/env python3
"""Measurements of the adaptive select on the denoised frame's error
-> profiles/adaptive_filtered_bench.json.

    python tools/adaptive_filtered_bench.py [--out profiles/adaptive_filtered_bench.json] [--reps 9]

(a) quality and sample cost: scenes 1, 6, 8 at 480x270, 8 bounces, batches of 32, min_passes 64, cap
    1,024, each against the scene's own 2,048-spp render on other pass numbers.  For every threshold:
    the raw rule (mcpt_adaptive_select) followed by denoise_resolved_variance(5); the filtered rule
    with raw_cap 64; the filtered rule with raw_cap = 4 x threshold; and a uniform render of the raw
    rule's mean spp (rounded) denoised with denoise_variance(5) over batches of 32.  Per run: mean
    spp, select rounds, wall ms (render loop, selects and the final filter; the guides included where
    the rule needs them), and the RMSE of the DENOISED image.  One run each: no spread (the bits do
    not vary; the wall time does, and is a single sample).
(b) cost of a check: scene 6 at 1080p and 4K, two batches of 8 passes, every block active; HIP-event
    times of mcpt_adaptive_select, of mcpt_adaptive_select_filtered's select part (steps A + C with
    the scan, mcpt_last_adaptive_ms) and of its filter (step B, mcpt_last_denoise_ms), interleaved,
    medians of `reps` after 3 warm-ups; the spread is (max - min) / median."""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "montecarlo-pathtracing_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402,F401  (HIP runtime first)
import mcpt  # noqa: E402

W0, H0, BOUNCES, BATCH, MIN_PASSES, CAP, ITER = 480, 270, 8, 32, 64, 1024, 5


def med(v):
    v = sorted(v)
    m = v[len(v) // 2]
    return {"median": m, "min": v[0], "max": v[-1], "spread": (v[-1] - v[0]) / m if m else 0.0, "n": len(v)}


def rmse(a, b):
    return float(np.sqrt(np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2)))


def adaptive_run(r, cam, thr, raw_cap):
    """raw_cap None: the raw rule, then the filter once; else the filtered rule (its last check's
    image is not reused: the final filter runs on the final state, as mcpt_render does)."""
    r.set_target(W0, H0)
    r.synchronize()
    t0 = time.perf_counter()
    r.render_guides(*cam)
    r.stats_begin()
    r.adaptive_begin(MIN_PASSES)
    done, rounds, rec = 0, 0, None
    while done < CAP:
        r.render_adaptive(cam[0], cam[1], 1 + done, BATCH, 0.0, BOUNCES)
        done += BATCH
        if done >= 2 * BATCH:
            rec = r.adaptive_select(thr) if raw_cap is None else r.adaptive_select_filtered(thr, raw_cap, iterations=ITER)
            rounds += 1
            if rec["n_active_blocks"] == 0:
                break
    img = r.denoise_resolved_variance(ITER)
    wall = (time.perf_counter() - t0) * 1e3
    raw = r.read_resolved()
    r.adaptive_end()
    r.stats_end()
    return {"mean_spp": rec["samples"] / rec["n_px"], "rendered": done, "select_rounds": rounds, "wall_ms": wall,
            "n_active_blocks_at_end": rec["n_active_blocks"], "mean_r": rec["mean_r"], "mean_rf": rec.get("mean_rf")}, img, raw


def uniform_run(r, cam, spp):
    r.set_target(W0, H0)
    r.synchronize()
    t0 = time.perf_counter()
    r.render_guides(*cam)
    r.stats_begin()
    done = 0
    while done < spp:
        n = min(BATCH, spp - done)
        r.render(cam[0], cam[1], 1 + done, n, 0.0, BOUNCES)
        done += n
    r.convergence(0.05)
    img = r.denoise_variance(ITER)
    wall = (time.perf_counter() - t0) * 1e3
    raw = r.read_image()
    r.stats_end()
    return {"spp": spp, "wall_ms": wall}, img, raw


def bench_quality(r, thresholds):
    out = []
    for scene in (1, 6, 8):
        r.upload_scene(mcpt.Scene.reference(scene))
        r.set_target(W0, H0)
        cam = mcpt.camera_canonical(W0, H0)
        r.render(cam[0], cam[1], 100001, 2048, 0.0, BOUNCES)       # the reference: other passes
        acc, n = r.read_accum()
        ref = acc / np.float32(n)
        uniform_run(r, cam, 64)                                     # warm-up (schedule trials, allocations)
        adaptive_run(r, cam, 0.5, 64.0)
        for thr in thresholds:
            row = {"scene": scene, "W": W0, "H": H0, "bounces": BOUNCES, "threshold": thr}
            for name, cap in (("raw_rule", None), ("filtered_cap64", 64.0), ("filtered_cap4x", 4.0 * thr)):
                info, img, raw = adaptive_run(r, cam, thr, cap)
                info["denoised_rmse"], info["resolved_rmse"] = rmse(img, ref), rmse(raw, ref)
                row[name] = info
            spp = max(2 * BATCH, int(round(row["raw_rule"]["mean_spp"])))
            info, img, raw = uniform_run(r, cam, spp)
            info["denoised_rmse"], info["raw_rmse"] = rmse(img, ref), rmse(raw, ref)
            row["uniform_same_samples_as_raw_rule"] = info
            out.append(row)
            print(json.dumps(row), flush=True)
    return out


def bench_check(r, reps, warm=3):
    out = []
    r.upload_scene(mcpt.Scene.reference(6))
    for W, H in ((1920, 1080), (3840, 2160)):
        r.set_target(W, H)
        cam = mcpt.camera_canonical(W, H)
        r.render_guides(*cam)
        r.stats_begin()
        r.adaptive_begin(10 ** 6)                 # (min_passes holds every block: each repetition sees the same state)
        for k in range(2):
            r.render_adaptive(cam[0], cam[1], 1 + 8 * k, 8, 0.0, BOUNCES)
        raw, sel, flt = [], [], []
        for k in range(reps + warm):
            r.adaptive_select(0.05)
            a = r.last_adaptive_ms()[0]
            r.adaptive_select_filtered(0.05, 64.0, iterations=ITER)
            b, c = r.last_adaptive_ms()[0], r.last_denoise_ms()[1]
            if k >= warm:
                raw.append(a)
                sel.append(b)
                flt.append(c)
        info = r.adaptive_info()
        assert info["n_active"] == info["n_blocks"]
        row = {"W": W, "H": H, "n_blocks": info["n_blocks"], "iterations": ITER, "raw_select_ms": med(raw),
               "filtered_select_ms": med(sel), "filter_ms": med(flt)}
        row["filtered_check_ms"] = row["filtered_select_ms"]["median"] + row["filter_ms"]["median"]
        row["filter_share"] = row["filter_ms"]["median"] / row["filtered_check_ms"]
        out.append(row)
        print(json.dumps(row), flush=True)
        r.adaptive_end()
        r.stats_end()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "adaptive_filtered_bench.json"))
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--thresholds", default="0.2,0.1,0.05")
    a = ap.parse_args()
    r = mcpt.Renderer(0)
    try:
        res = {"device": torch.cuda.get_device_name(0), "reps": a.reps,
               "quality": bench_quality(r, [float(x) for x in a.thresholds.split(",")]),
               "check": bench_check(r, a.reps)}
    finally:
        r.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
