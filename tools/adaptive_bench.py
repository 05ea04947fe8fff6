#!/usr/bin/env python3
"""Measurements of the adaptive sampling of 8x8 blocks -> profiles/adaptive_bench.json.

    python tools/adaptive_bench.py [--out profiles/adaptive_bench.json] [--reps 9]

(a) select: device time of mcpt_adaptive_select (select kernel + list scan) at 1080p and 4K against
    its byte floor (16 B of state read, 8 B of map written per active pixel, 12 B per block).
(b) list path: mcpt_render_adaptive with every block active against mcpt_render of the same passes in
    dispatch order (MCPT_ITEM_ORDER=0), render lanes off, per-lane traversal, one segment per item —
    the plain twin of the same kernel — interleaved, device times, medians and spread.
(d) scenes 1, 6, 8 at 480x270: RMSE of the resolved adaptive image against the scene's own 2,048-spp
    render (other passes), beside a uniform render of the same sample count and of the same wall time.
(e) the resolve step of mcpt_denoise_resolved (accum / each pixel's own count -> the filter's first
    float4 buffer) against the averaging step of mcpt_denoise, mcpt_denoise_iteration_ms(-1) of each,
    interleaved in one process, scene 6 at 1080p and 4K, medians of 20 after 3 warm-ups: with nothing
    retired (both read the same frame), and with about half the blocks retired, the counts from the
    block arrays and from the count plane of a counted gather separately.  Byte floor: 12 B read and
    16 B written per pixel, plus 8 B per block or 4 B per pixel for the counts.
    `--only e` measures (e) alone and keeps the other sections of an existing --out file.
(f) the gathered error map, scene 6 at 1080p, eight balanced uniform shards and the
    frame on one GPU and one stream, HIP events around the calls, medians of 20 after 3 warm-ups,
    interleaved: the counted gather alone (mcpt_gather_rows_counted: 16 B/px moved), the map gather
    after it (mcpt_gather_error_map: 8 B/px), the multi-process form's ends for the rows
    (mcpt_pack_counted_device x 8 + mcpt_load_rows_counted) and for the map
    (mcpt_pack_error_map_device x 8 + mcpt_load_rows_error_map), and mcpt_error_map_record on the
    gathered map beside mcpt_convergence's error kernel (mcpt_last_stats_ms) on a full-frame context.
    `--only f` likewise.
Medians of `reps` runs after warm-ups; the spread is (max - min) / median."""
import argparse
import json
import os
import sys
import time

os.environ["MCPT_ITEM_ORDER"] = "0"      # (b)'s twin: dispatch order, one segment per item
os.environ["MCPT_SEG_PER_ITEM"] = "1"
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "montecarlo-pathtracing_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402,F401  (HIP runtime first)
import mcpt  # noqa: E402


def med(v):
    v = sorted(v)
    m = v[len(v) // 2]
    return {"median": m, "min": v[0], "max": v[-1], "spread": (v[-1] - v[0]) / m if m else 0.0, "n": len(v)}


def setup(r, scene, W, H):
    r.upload_scene(mcpt.Scene.reference(scene))
    r.set_target(W, H)
    return mcpt.camera_canonical(W, H)


def bench_select(r, reps):
    out = []
    for W, H in ((1920, 1080), (3840, 2160)):
        cam = setup(r, 6, W, H)
        r.stats_begin()
        r.adaptive_begin(0)
        r.render_adaptive(cam[0], cam[1], 1, 8, 0.0, 8)
        r.render_adaptive(cam[0], cam[1], 9, 8, 0.0, 8)
        ms = []
        for k in range(reps + 3):
            r.adaptive_select(1e-6)            # (nothing above r = 0 retires: the active set stays)
            if k >= 3:
                ms.append(r.last_adaptive_ms()[0])
        info = r.adaptive_info()
        px_active = info["n_active"] * 64      # (an upper bound at partial blocks)
        floor_bytes = px_active * (16 + 8) + (W * H - min(W * H, px_active)) * 8 + info["n_blocks"] * 12
        m = med(ms)
        out.append({"W": W, "H": H, "n_blocks": info["n_blocks"], "n_active": info["n_active"], "select_ms": m,
                    "floor_bytes": floor_bytes, "floor_ms_at_8TBs": floor_bytes / 8e12 * 1e3,
                    "achieved_GBs": floor_bytes / (m["median"] * 1e-3) / 1e9})
        r.adaptive_end()
    return out


def bench_list_path(r, reps):
    out = []
    r.set_traversal(mcpt.TRAVERSAL_LANE)
    r.set_render_lanes(False)
    for scene, W, H, n in ((6, 1920, 1080, 64), (8, 1920, 1080, 32), (1, 1920, 1080, 64)):
        cam = setup(r, scene, W, H)
        r.stats_begin()
        r.adaptive_begin(0)
        plain, listed, first = [], [], 1
        for k in range(reps + 2):
            r.render(cam[0], cam[1], first, n, 0.0, 8)
            a = sum(r.last_kernel_ms())
            first += n
            r.render_adaptive(cam[0], cam[1], first, n, 0.0, 8)
            b = r.last_adaptive_ms()[1]
            first += n
            if k >= 2:
                plain.append(a)
                listed.append(b)
        assert r.adaptive_info()["n_active"] == r.adaptive_info()["n_blocks"]
        p, q = med(plain), med(listed)
        out.append({"scene": scene, "W": W, "H": H, "passes": n, "bounces": 8, "plain_ms": p, "list_ms": q,
                    "ratio": q["median"] / p["median"]})
        r.adaptive_end()
    r.set_traversal(mcpt.TRAVERSAL_AUTO)
    r.set_render_lanes(True)
    return out


def rmse(a, b):
    return float(np.sqrt(np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2)))


def timed_uniform(r, cam, spp, bounces):
    r.clear_accum()
    r.synchronize()
    t0 = time.perf_counter()
    done = 0
    while done < spp:
        n = min(32, spp - done)
        r.render(cam[0], cam[1], 1 + done, n, 0.0, bounces)
        done += n
    acc, n = r.read_accum()
    return acc / np.float32(n), (time.perf_counter() - t0) * 1e3


def bench_point(r, thresholds):
    out = []
    W, H, B = 480, 270, 8
    for scene in (1, 6, 8):
        cam = setup(r, scene, W, H)
        r.render(cam[0], cam[1], 100001, 2048, 0.0, B)       # the reference: other passes
        acc, n = r.read_accum()
        ref = acc / np.float32(n)
        timed_uniform(r, cam, 64, B)                          # warm-up (schedule trials)
        timed_uniform(r, cam, 64, B)
        for thr in thresholds:
            r.set_target(W, H)
            r.synchronize()
            t0 = time.perf_counter()
            rec = r.render_adaptive_until(cam[0], cam[1], thr, batch=32, max_passes=1024, min_passes=64, bounces=B)
            img = r.read_resolved()
            t_ad = (time.perf_counter() - t0) * 1e3
            r.adaptive_end()
            r.stats_end()
            mean_spp = rec["samples"] / rec["n_px"]
            spp_eq = max(1, int(round(mean_spp)))
            u_eq, t_eq = timed_uniform(r, cam, spp_eq, B)
            spp_t = max(1, int(round(spp_eq * t_ad / t_eq)))
            u_t, t_t = timed_uniform(r, cam, spp_t, B)
            out.append({"scene": scene, "W": W, "H": H, "bounces": B, "threshold": thr, "rendered": rec["rendered"],
                        "mean_spp": mean_spp, "n_active_blocks_at_end": rec["n_active_blocks"],
                        "adaptive_rmse": rmse(img, ref), "adaptive_wall_ms": t_ad,
                        "uniform_same_samples": {"spp": spp_eq, "rmse": rmse(u_eq, ref), "wall_ms": t_eq},
                        "uniform_same_time": {"spp": spp_t, "rmse": rmse(u_t, ref), "wall_ms": t_t}})
            print(json.dumps(out[-1]), flush=True)
    return out


def compare(base, other):
    """other / base of two interleaved series, and whether the medians differ by more than either
    series' own run-to-run spread."""
    ratio = other["median"] / base["median"]
    return {"ratio": ratio, "outside_spread": abs(ratio - 1.0) > max(base["spread"], other["spread"])}


def bench_resolve(r, reps=20, warm=3):
    out = []
    frame = mcpt.Renderer(0)
    try:
        for W, H in ((1920, 1080), (3840, 2160)):
            cam = setup(r, 6, W, H)
            r.stats_begin()
            r.adaptive_begin(0)
            r.render_adaptive(cam[0], cam[1], 1, 8, 0.0, 8)
            r.render_adaptive(cam[0], cam[1], 9, 8, 0.0, 8)
            r.render_guides(*cam)
            lib = mcpt.lib()

            def step_ms(ctx, fn):       # the step alone: 0 iterations, no image read back
                st = fn(ctx._h, 0, 1.0, 1.0)
                assert st == 0, st
                return ctx.denoise_iteration_ms(-1)

            avg, blk = [], []
            for k in range(reps + warm):
                a = step_ms(r, lib.mcpt_denoise)
                b = step_ms(r, lib.mcpt_denoise_resolved)
                if k >= warm:
                    avg.append(a)
                    blk.append(b)
            info = r.adaptive_info()
            assert info["n_active"] == info["n_blocks"]
            n_px, n_blocks = W * H, info["n_blocks"]
            a, b = med(avg), med(blk)
            row = {"W": W, "H": H, "n_blocks": n_blocks,
                   "floor_bytes": {"average": n_px * 28, "resolve_blocks": n_px * 28 + n_blocks * 8,
                                   "resolve_plane": n_px * 32},
                   "nothing_retired": {"average_ms": a, "resolve_blocks_ms": b, **compare(a, b),
                                       "average_GBs": n_px * 28 / (a["median"] * 1e-3) / 1e9,
                                       "resolve_blocks_GBs": (n_px * 28 + n_blocks * 8) / (b["median"] * 1e-3) / 1e9}}
            # about half the blocks retired: a threshold at the median of the blocks' largest r
            r.adaptive_select(1e-6)
            rr = r.read_error_map()[..., 1]
            by, bx = (H + 7) // 8, (W + 7) // 8
            pad = np.zeros((by * 8, bx * 8), np.float32)
            pad[:H, :W] = rr
            bmax = pad.reshape(by, 8, bx, 8).max(axis=(1, 3))
            rec = r.adaptive_select(float(np.median(bmax[bmax > 0])))
            retired = 1.0 - rec["n_active_blocks"] / rec["n_blocks"]
            r.render_adaptive(cam[0], cam[1], 17, 8, 0.0, 8)      # the counts now take two values
            setup(frame, 6, W, H)
            frame.render_guides(*cam)
            frame.gather_rows_counted([r])                          # the same frame with its counts in a plane
            avg, blk, pln = [], [], []
            for k in range(reps + warm):
                a = step_ms(frame, lib.mcpt_denoise)
                b = step_ms(r, lib.mcpt_denoise_resolved)
                c = step_ms(frame, lib.mcpt_denoise_resolved)
                if k >= warm:
                    avg.append(a)
                    blk.append(b)
                    pln.append(c)
            a, b, c = med(avg), med(blk), med(pln)
            row["half_retired"] = {"retired_fraction": retired, "average_ms": a, "resolve_blocks_ms": b,
                                   "resolve_plane_ms": c, "blocks": compare(a, b), "plane": compare(a, c)}
            out.append(row)
            print(json.dumps(row), flush=True)
            r.adaptive_end()
            r.stats_end()
    finally:
        frame.close()
    return out


def bench_emap_gather(reps=20, warm=3, W=1920, H=1080, n_shards=8):
    import ctypes
    ts = torch.cuda.Stream()
    made = []

    def uniform(rows):
        r = mcpt.Renderer(0)
        made.append(r)
        r.set_stream(ts.cuda_stream)
        r.upload_scene(mcpt.Scene.reference(6))
        if rows is None:
            r.set_target(W, H)
        else:
            r.set_target_rows(W, H, rows)
        cam = mcpt.camera_canonical(W, H)
        r.stats_begin()
        for first in (1, 5):
            r.render(cam[0], cam[1], first, 4, 0.0, 4)
        r.convergence(0.05)
        return r

    def balanced(k):
        rows, n = np.zeros(H, np.int32), ctypes.c_int()
        assert mcpt.lib().mcpt_balanced_rows(H, n_shards, k, 8, mcpt._ip(rows), ctypes.byref(n)) == 0
        return rows[:n.value].tolist()

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(ts)
        fn()
        b.record(ts)
        b.synchronize()
        return a.elapsed_time(b)

    try:
        row_sets = [balanced(k) for k in range(n_shards)]
        shards = [uniform(rows) for rows in row_sets]
        full = uniform(None)
        frame = mcpt.Renderer(0)
        made.append(frame)
        frame.set_stream(ts.cuda_stream)
        frame.set_target(W, H)
        m = max(len(rows) for rows in row_sets)
        src = np.zeros(H, np.int32)
        for k, rows in enumerate(row_sets):
            src[np.asarray(rows)] = k * m + np.arange(len(rows))
        with torch.cuda.stream(ts):
            rows_buf = torch.zeros((n_shards * m, W, 4), dtype=torch.int32, device="cuda:0")
            map_buf = torch.zeros((n_shards * m, W, 2), dtype=torch.int32, device="cuda:0")
        ts.synchronize()

        def pack_load_rows():
            for k, s in enumerate(shards):
                s.pack_counted_device(rows_buf[k * m].data_ptr(), s.n_local_rows * W * 16)
            frame.load_rows_counted(rows_buf.data_ptr(), rows_buf.shape[0], src, 8)

        def pack_load_map():
            for k, s in enumerate(shards):
                s.pack_error_map_device(map_buf[k * m].data_ptr(), s.n_local_rows * W * 8)
            frame.load_rows_error_map(map_buf.data_ptr(), map_buf.shape[0], src)

        series = {k: [] for k in ("gather_rows_counted_ms", "gather_error_map_ms", "pack_load_rows_ms", "pack_load_map_ms",
                                  "error_map_record_ms", "convergence_call_ms", "convergence_error_kernel_ms")}
        for k in range(reps + warm):
            row = {"gather_rows_counted_ms": timed(lambda: frame.gather_rows_counted(shards)),
                   "gather_error_map_ms": timed(lambda: frame.gather_error_map(shards)),
                   "error_map_record_ms": timed(lambda: frame.error_map_record(0.05)),
                   "pack_load_rows_ms": timed(pack_load_rows),
                   "pack_load_map_ms": timed(pack_load_map),
                   "convergence_call_ms": timed(lambda: full.convergence(0.05))}
            row["convergence_error_kernel_ms"] = full.last_stats_ms()[1]
            if k >= warm:
                for name, v in row.items():
                    series[name].append(v)
        same = bool(np.array_equal(frame.read_error_map().view(np.uint32), full.read_error_map().view(np.uint32)))
        out = {"W": W, "H": H, "n_shards": n_shards, "reps": reps, "map_equals_full_frame": same,
               "bytes_moved": {"rows_counted": W * H * 16, "map": W * H * 8}}
        out.update({name: med(v) for name, v in series.items()})
        out["map_over_counted_gather"] = out["gather_error_map_ms"]["median"] / out["gather_rows_counted_ms"]["median"]
        out["map_over_rows_pack_load"] = out["pack_load_map_ms"]["median"] / out["pack_load_rows_ms"]["median"]
        out["record_over_convergence_call"] = out["error_map_record_ms"]["median"] / out["convergence_call_ms"]["median"]
        print(json.dumps(out), flush=True)
        return out
    finally:
        for r in made:
            r.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "adaptive_bench.json"))
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--thresholds", default="0.2,0.1,0.05")
    ap.add_argument("--only", default="", help="e / f: measure section (e) / (f) alone, keep the rest of --out")
    a = ap.parse_args()
    r = mcpt.Renderer(0)
    try:
        if a.only == "f":
            res = json.load(open(a.out)) if os.path.exists(a.out) else {"device": torch.cuda.get_device_name(0)}
            res["emap_gather"] = bench_emap_gather()
        elif a.only == "e":
            res = json.load(open(a.out)) if os.path.exists(a.out) else {"device": torch.cuda.get_device_name(0)}
            res["resolve"] = bench_resolve(r)
        else:
            res = {"device": torch.cuda.get_device_name(0), "reps": a.reps,
                   "select": bench_select(r, a.reps), "list_path": bench_list_path(r, a.reps),
                   "point": bench_point(r, [float(x) for x in a.thresholds.split(",")]),
                   "resolve": bench_resolve(r), "emap_gather": bench_emap_gather()}
    finally:
        r.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps({k: res[k] for k in ("select", "list_path", "resolve", "emap_gather") if k in res}, indent=1))


if __name__ == "__main__":
    main()
