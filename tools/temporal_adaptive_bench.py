"""Measure temporal adaptive sampling -> profiles/temporal_adaptive_bench.json.

Select time: mcpt_adaptive_select_temporal (step A, step T temporal_select_kernel and the list scan,
mcpt_last_adaptive_ms) on scene 6 at 1080p and 4K with the history looked up across a 1 degree orbit
step, beside mcpt_adaptive_select on a twin context in the same state (the retiring step A and the
scan): their difference is step T's time.  The contexts are interleaved A/B/A/B, medians of 20 repeats
after 3 warm-ups with their spread.  The timed selects ask with a threshold below every positive value,
so the list they see stays (blocks of black misses leave it during the warm-ups): "full" is the list of
a frame two rounds in, "frame4" the list at the fraction the fourth frame of the orbit reaches at the
default target.  Beside them step
T's byte floor at the 8 TB/s HBM peak over the pixels of the active blocks, reads only: 12 B of
accumulator, 8 B of error map, 32 B of guides, 52 B of history.

Quality at equal budget: scenes 1, 6 and 8 at 96x54 and 480x270, a static camera and a 1 degree per
frame orbit, 8 frames, 8 bounces, a 2,048-spp reference of the last camera; per threshold in {0.02, 0.05,
0.1, 0.2} the temporal-adaptive run's (cap 16, 2 passes per round) mean samples per pixel per frame and
filtered RMSE, beside the uniform temporal render at the next integer spp at or above that mean.

Wall time per frame at 480x270: the host loop against the queued form against the uniform 4-spp frame.

  python tools/temporal_adaptive_bench.py [--out ...] [--repeats 20] [--skip-select] [--skip-quality] [--skip-wall]
"""
import argparse
import json
import math
import os
import statistics
import sys
import time

import numpy as np
import torch  # noqa: F401  (HIP runtime first)

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "montecarlo-pathtracing_amd")]
import mcpt  # noqa: E402

HBM_PEAK = 8.0e12
STEP_T_BYTES = 12 + 8 + 32 + 52
THRESHOLDS = (0.02, 0.05, 0.1, 0.2)


def spread(v):
    q = statistics.quantiles(v, n=4)
    return {"median_ms": statistics.median(v), "q1_ms": q[0], "q3_ms": q[2], "min_ms": min(v), "max_ms": max(v)}


def orbit_camera(W, H, deg):
    ipv, iv = mcpt.camera_canonical(W, H)
    rinv = mcpt.Transfo.rotateZ(-deg)
    ipv2, iv2 = mcpt.Transfo.mul(rinv, ipv), mcpt.Transfo.mul(rinv, iv)
    return ipv2, iv2, mcpt.mat4_inverse(ipv2)


def select_state(W, H, temporal, frames, target):
    """A context on frame `frames` of a 1 degree orbit (4 frames: the list as a real frame 4 leaves it
    before its last select; 2 frames: the list of a frame two rounds in)."""
    r = mcpt.Renderer(0)
    r.upload_scene(mcpt.Scene.reference(6))
    r.set_target(W, H)
    r.temporal_begin()
    prev = None
    for k in range(frames - 1):
        ipv, iv, pv = orbit_camera(W, H, float(k))
        r.render_frame_temporal_adaptive(ipv, iv, prev, 1 + 16 * k, 16, 2, target, bounces=8)
        prev = pv
    ipv, iv, _ = orbit_camera(W, H, float(frames - 1))
    r.clear_accum()
    r.stats_begin()
    r.adaptive_begin(0)
    r.render_guides(ipv, iv)
    first = 1 + 16 * (frames - 1)
    rounds = 2
    for i in range(2):
        r.render_adaptive(ipv, iv, first + 2 * i, 2, 0.0, 8, 1.0, 0)
    if frames == 4:       # the frame's own selects up to the last round but one
        while rounds < 7 and r.adaptive_select_temporal(prev, target)["n_active_blocks"] > 0:
            r.render_adaptive(ipv, iv, first + 2 * rounds, 2, 0.0, 8, 1.0, 0)
            rounds += 1
    if not temporal:
        r.temporal_end()
    return r, prev


def select_times(a):
    out = []
    for W, H in ((1920, 1080), (3840, 2160)):
        for name, frames in (("full", 2), ("frame4", 4)):
            rt, prev = select_state(W, H, True, frames, a.target)
            rr, _ = select_state(W, H, False, frames, a.target)
            times = {"temporal": [], "raw": []}
            rec = {}
            for k in range(a.warmup + a.repeats):
                # (a threshold below every positive value: the list stays as the warm-ups left it)
                rec = rt.adaptive_select_temporal(prev, 1e-30)
                t_ms = rt.last_adaptive_ms()[0]
                rr.adaptive_select(1e-30)
                r_ms = rr.last_adaptive_ms()[0]
                if k >= a.warmup:
                    times["temporal"].append(t_ms)
                    times["raw"].append(r_ms)
            n_px = rec["n_px_t"]
            step_t = [x - y for x, y in zip(times["temporal"], times["raw"])]
            floor_ms = 1e3 * n_px * STEP_T_BYTES / HBM_PEAK
            entry = {"width": W, "height": H, "list": name, "n_blocks": rec["n_blocks"],
                     "n_active_blocks": rec["n_active_blocks"], "n_px_t": n_px, "n_history": rec["n_history"],
                     "select_temporal": spread(times["temporal"]), "select_raw": spread(times["raw"]),
                     "step_t": spread(step_t), "floor_bytes_per_px": STEP_T_BYTES, "floor_ms": floor_ms,
                     "step_t_over_floor": statistics.median(step_t) / floor_ms if floor_ms > 0 else None}
            out.append(entry)
            print(json.dumps(entry), flush=True)
            rt.close()
            rr.close()
    return out


def rmse(x, y):
    return float(np.sqrt(np.mean((x.astype(np.float64) - y.astype(np.float64)) ** 2)))


def quality(a):
    rows = []
    r = mcpt.Renderer(0)
    frames, B = 8, 8
    for scene in (1, 6, 8):
        r.upload_scene(mcpt.Scene.reference(scene))
        for W, H in ((96, 54), (480, 270)):
            r.set_target(W, H)
            for step in (0.0, 1.0):
                ipv, iv, _ = orbit_camera(W, H, (frames - 1) * step)
                r.render(ipv, iv, 100001, 2048, 0.0, B, 1.0, 0)
                ref = r.read_image()
                uniform = {}
                for thr in THRESHOLDS:
                    r.temporal_begin()
                    prev, spp = None, 0.0
                    for k in range(frames):
                        ipv, iv, pv = orbit_camera(W, H, k * step)
                        img, rec, sel = r.render_frame_temporal_adaptive(ipv, iv, prev, 1 + 16 * k, 16, 2, thr, bounces=B)
                        spp += sel["samples"] / sel["n_px"]
                        prev = pv
                    r.adaptive_end()
                    r.stats_end()
                    mean_spp = spp / frames
                    u = max(2, math.ceil(mean_spp))
                    if u not in uniform:
                        r.temporal_begin()
                        prev = None
                        for k in range(frames):
                            ipv, iv, pv = orbit_camera(W, H, k * step)
                            uimg, _ = r.render_frame_temporal(ipv, iv, prev, 1 + 16 * k, u, 2, bounces=B)
                            prev = pv
                        r.stats_end()
                        uniform[u] = rmse(uimg, ref)
                    row = {"scene": scene, "width": W, "height": H, "orbit_deg": step, "threshold": thr,
                           "mean_spp": mean_spp, "rmse_adaptive": rmse(img, ref), "uniform_spp": u,
                           "rmse_uniform": uniform[u], "last_frame_active_blocks": sel["n_active_blocks"],
                           "last_frame_rendered": sel["rendered"]}
                    row["ratio"] = row["rmse_adaptive"] / row["rmse_uniform"]
                    rows.append(row)
                    print(json.dumps(row), flush=True)
                r.temporal_end()
                r.clear_accum()
    r.close()
    return rows


def wall(a):
    rows = []
    r = mcpt.Renderer(0)
    frames, B, W, H = 8, 8, 480, 270
    for scene in (1, 6, 8):
        r.upload_scene(mcpt.Scene.reference(scene))
        r.set_target(W, H)
        for step in (0.0, 1.0):
            row = {"scene": scene, "width": W, "height": H, "orbit_deg": step, "threshold": a.target}
            for form in ("loop", "queued", "uniform4"):
                per_frame = []
                for rep in range(a.wall_repeats + 1):
                    r.temporal_begin()
                    prev = None
                    r.synchronize()
                    t0 = time.perf_counter()
                    for k in range(frames):
                        ipv, iv, pv = orbit_camera(W, H, k * step)
                        if form == "uniform4":
                            r.render_frame_temporal(ipv, iv, prev, 1 + 16 * k, 4, 2, bounces=B)
                        else:
                            r.render_frame_temporal_adaptive(ipv, iv, prev, 1 + 16 * k, 16, 2, a.target, bounces=B,
                                                             queued=form == "queued")
                        prev = pv
                    r.synchronize()
                    if rep:                                   # (the first repeat warms up)
                        per_frame.append(1e3 * (time.perf_counter() - t0) / frames)
                    if form != "uniform4":
                        r.adaptive_end()
                    r.stats_end()
                row[form + "_ms_per_frame"] = spread(per_frame) if len(per_frame) > 1 else {"median_ms": per_frame[0]}
            rows.append(row)
            print(json.dumps(row), flush=True)
        r.temporal_end()
    r.close()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "temporal_adaptive_bench.json"))
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--wall-repeats", type=int, default=5)
    ap.add_argument("--target", type=float, default=mcpt.TEMPORAL_TARGET)
    ap.add_argument("--skip-select", action="store_true")
    ap.add_argument("--skip-quality", action="store_true")
    ap.add_argument("--skip-wall", action="store_true")
    a = ap.parse_args()
    res = {"device": torch.cuda.get_device_name(0), "repeats": a.repeats, "warmup": a.warmup, "target": a.target,
           "hbm_peak_bytes_per_s": HBM_PEAK}
    if not a.skip_select:
        res["select"] = select_times(a)
    if not a.skip_quality:
        res["quality"] = quality(a)
    if not a.skip_wall:
        res["wall"] = wall(a)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
