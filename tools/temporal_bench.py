"""Measure temporal reprojection -> profiles/temporal_bench.json.

Kernel time: the accumulate kernel (and the guides' copy behind it, where there is one) on scene 6 at
1080p and 4K, the history reprojected across a 1 degree orbit step; the ping-pong form
(MCPT_TEMPORAL_COPY=0: the kernel writes the history's guides) against the copy form (=1: a device copy
behind the kernel), one context each, interleaved A/B/A/B so drift hits both alike, medians of 20
repeats after 3 warm-ups with their spread; HIP-event times (mcpt_last_temporal_ms).  Beside them the
byte floor at the 8 TB/s HBM peak from the contract's traffic per pixel: 12 B of accumulator, 8 B of
error map and 32 B of guides read, the history's 52 B (guides 32, colour and variance 16, length 4)
read once (neighbouring pixels share their 2x2 taps) and 20 B written, plus the history's guides: 32 B
written by the kernel (ping-pong: 156 B) or 64 B moved by the copy (copy: 124 + 64 B).

Quality: scenes 1, 6 and 8 at 96x54 and 480x270, 8 frames of 4 spp (two batches of 2), 8 bounces, a
static camera and a 1 degree per frame orbit, max_history 4 / 8 / 32: the RMSE of the last frame's
mcpt_denoise_temporal and of mcpt_denoise_variance on that frame alone against a 2,048-spp render of
the last camera, and their ratio.

  python tools/temporal_bench.py [--out profiles/temporal_bench.json] [--repeats 20] [--skip-quality]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch  # noqa: F401  (HIP runtime first)

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "montecarlo-pathtracing_amd")]
import mcpt  # noqa: E402

HBM_PEAK = 8.0e12
FLOOR_BYTES = {"pingpong": {"kernel": 156, "copy": 0}, "copy": {"kernel": 124, "copy": 64}}


def spread(v):
    q = statistics.quantiles(v, n=4)
    return {"median_ms": statistics.median(v), "q1_ms": q[0], "q3_ms": q[2], "min_ms": min(v), "max_ms": max(v)}


def orbit_camera(W, H, deg):
    ipv, iv = mcpt.camera_canonical(W, H)
    rinv = mcpt.Transfo.rotateZ(-deg)
    ipv2, iv2 = mcpt.Transfo.mul(rinv, ipv), mcpt.Transfo.mul(rinv, iv)
    return ipv2, iv2, mcpt.mat4_inverse(ipv2)


def kernel_times(a):
    out = []
    for W, H in ((1920, 1080), (3840, 2160)):
        ctx = {}
        for form, env in (("pingpong", "0"), ("copy", "1")):
            os.environ["MCPT_TEMPORAL_COPY"] = env       # read by temporal_begin
            r = mcpt.Renderer(0)
            r.upload_scene(mcpt.Scene.reference(6))
            r.set_target(W, H)
            r.temporal_begin()
            ipv, iv, _ = orbit_camera(W, H, 1.0)
            r.stats_begin()
            for k in range(2):
                r.render(ipv, iv, 1 + 2 * k, 2, 0.0, 8, 1.0, 0)
            r.convergence(0.05)
            r.render_guides(ipv, iv)
            ctx[form] = r
        del os.environ["MCPT_TEMPORAL_COPY"]
        prev = orbit_camera(W, H, 0.0)[2]                # the history is looked up one degree away
        times = {f: {"kernel": [], "copy": []} for f in ctx}
        rec = {}
        for k in range(a.warmup + a.repeats):
            for form, r in ctx.items():
                rec[form] = r.temporal_accumulate(prev)
                km, cm = r.last_temporal_ms()
                if k >= a.warmup:
                    times[form]["kernel"].append(km)
                    times[form]["copy"].append(cm)
        n = W * H
        entry = {"width": W, "height": H, "forms": {}}
        for form in ctx:
            total = [x + y for x, y in zip(times[form]["kernel"], times[form]["copy"])]
            fb = FLOOR_BYTES[form]
            entry["forms"][form] = {
                "kernel": spread(times[form]["kernel"]), "copy": spread(times[form]["copy"]), "total": spread(total),
                "floor_bytes_per_px": fb, "floor_ms": {k: 1e3 * n * b / HBM_PEAK for k, b in fb.items()},
                "n_history": rec[form]["n_history"], "n_new": rec[form]["n_new"]}
        pt, ct = entry["forms"]["pingpong"]["total"], entry["forms"]["copy"]["total"]
        entry["verdict"] = ("pingpong_faster" if pt["q3_ms"] < ct["q1_ms"] else
                            "copy_faster" if ct["q3_ms"] < pt["q1_ms"] else "tie")
        out.append(entry)
        for r in ctx.values():
            r.close()
        print(json.dumps(entry), flush=True)
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
                for mh in (4, 8, 32):
                    r.temporal_begin()
                    prev = None
                    for k in range(frames):
                        ipv, iv, pv = orbit_camera(W, H, k * step)
                        img, rec = r.render_frame_temporal(ipv, iv, prev, 1 + 4 * k, 4, 2, bounces=B, max_history=mh)
                        prev = pv
                    alone = r.denoise_variance()
                    raw = r.read_image()
                    r.stats_end()
                    row = {"scene": scene, "width": W, "height": H, "orbit_deg": step, "max_history": mh,
                           "plane_tol": mcpt.TEMPORAL_PLANE_TOL, "rmse_raw": rmse(raw, ref), "rmse_alone": rmse(alone, ref),
                           "rmse_temporal": rmse(img, ref), "mean_len": rec["sum_len"] / rec["n_px"],
                           "n_history": rec["n_history"], "n_rejected": rec["n_rejected"], "n_offscreen": rec["n_offscreen"]}
                    row["ratio"] = row["rmse_temporal"] / row["rmse_alone"]
                    rows.append(row)
                    print(json.dumps(row), flush=True)
                r.clear_accum()
    r.close()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "temporal_bench.json"))
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--skip-quality", action="store_true")
    a = ap.parse_args()
    res = {"device": torch.cuda.get_device_name(0), "scene": 6, "repeats": a.repeats, "warmup": a.warmup,
           "hbm_peak_bytes_per_s": HBM_PEAK, "kernel": kernel_times(a)}
    if not a.skip_quality:
        res["quality"] = quality(a)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
