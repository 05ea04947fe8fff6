#!/usr/bin/env python3
"""Device times of the counted gather's two kernels -> profiles/dist_adaptive_bench.json.

    python tools/dist_adaptive_bench.py [--out profiles/dist_adaptive_bench.json] [--reps 15] [--burst 20]

At 1920x1080, for a world-8 balanced shard (135 rows; the frame side: 8 x 135 packed rows into 1,080)
and for the full frame as one shard (world 1), interleaved in one process on one stream:
  send side   mcpt_copy_accum_device (the plain gather: a 12 B/px device copy)   against
              mcpt_pack_counted_device (16 B/px records, counts from the block arrays; also with
              the adaptive mode off: the pass count for every pixel)
  frame side  torch.index_select of the float [world * m, W, 3] receive buffer into the frame   against
              mcpt_load_rows_counted (the same row scatter of 16 B/px records, split into sums and counts)
A sample is `burst` launches between two events, queued behind a spinning gate kernel so that they
run back to back, divided by `burst` (a launch is a few microseconds: a single one is below what an
event pair resolves, and the host queues slower than the device runs); medians of `reps` samples after
warm-ups, spread = (max - min) / median.  The yardstick for the new kernels is the plain path's time
scaled by the bytes per pixel, 16 / 12."""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "montecarlo-pathtracing_amd"))
import numpy as np  # noqa: E402,F401
import torch  # noqa: E402  (HIP runtime first)
import mcpt  # noqa: E402
from mcpt.dist import frame_row_index, local_rows, max_local_rows  # noqa: E402

W, H, BAND = 1920, 1080, 8
GATE_CYCLES = 2_000_000      # the gate kernel's spin: longer than the host needs to queue a burst


def med(v):
    v = sorted(v)
    m = v[len(v) // 2]
    return {"median": m, "min": v[0], "max": v[-1], "spread": (v[-1] - v[0]) / m if m else 0.0, "n": len(v)}


def sample(stream, fn, burst):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.cuda.stream(stream):
        # a spinning kernel first: the burst is queued behind it and then runs back to back, so the
        # interval holds device time and not the host's launch rate
        torch.cuda._sleep(GATE_CYCLES)
        a.record()
        for _ in range(burst):
            fn()
        b.record()
    b.synchronize()
    return a.elapsed_time(b) / burst * 1e3          # microseconds per launch


def series(stream, fns, reps, burst, warm=3):
    out = {k: [] for k in fns}
    for i in range(reps + warm):
        for k, fn in fns.items():                    # interleaved
            us = sample(stream, fn, burst)
            if i >= warm:
                out[k].append(us)
    return {k: med(v) for k, v in out.items()}


def against(plain, new):
    yard = plain["median"] * 16.0 / 12.0
    ratio = new["median"] / yard
    return {"yardstick_us": yard, "new_over_yardstick": ratio,
            "slower_beyond_spread": ratio - 1.0 > max(plain["spread"], new["spread"])}


def bench(world, reps, burst):
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev)
    rows = local_rows(H, BAND, world, 0, "balanced")
    m, n = max_local_rows(H, BAND, world, "balanced"), len(rows)
    shard, frame = mcpt.Renderer(0), mcpt.Renderer(0)
    try:
        for r in (shard, frame):
            r.set_stream(stream.cuda_stream)
            r.upload_scene(mcpt.Scene.reference(6))
        shard.set_target_rows(W, H, rows)
        frame.set_target(W, H)
        cam = mcpt.camera_canonical(W, H)
        send3 = torch.zeros((m, W, 3), dtype=torch.float32, device=dev)
        recv3 = torch.zeros((world * m, W, 3), dtype=torch.float32, device=dev)
        frame3 = torch.empty((H, W, 3), dtype=torch.float32, device=dev)
        send4 = torch.zeros((m, W, 4), dtype=torch.int32, device=dev)
        recv4 = torch.ones((world * m, W, 4), dtype=torch.int32, device=dev)
        src = frame_row_index(H, BAND, world, "balanced").astype(np.int32)
        index = torch.as_tensor(src, device=dev)
        torch.cuda.synchronize()
        shard.render(cam[0], cam[1], 1, 8, 0.0, 4)
        fns = {"copy_accum_device": lambda: shard.copy_accum_device(send3.data_ptr(), n * W * 12),
               "pack_mode_off": lambda: shard.pack_counted_device(send4.data_ptr(), n * W * 16)}
        off = series(stream, fns, reps, burst)
        shard.stats_begin()
        shard.adaptive_begin(0)
        shard.render_adaptive(cam[0], cam[1], 9, 8, 0.0, 4)
        shard.render_adaptive(cam[0], cam[1], 17, 8, 0.0, 4)
        fns = {"copy_accum_device": lambda: shard.copy_accum_device(send3.data_ptr(), n * W * 12),
               "pack_blocks": lambda: shard.pack_counted_device(send4.data_ptr(), n * W * 16),
               "index_select": lambda: torch.index_select(recv3, 0, index, out=frame3),
               "load_rows_counted": lambda: frame.load_rows_counted(recv4.data_ptr(), world * m, src, 24)}
        on = series(stream, fns, reps, burst)
        px_s, px_f = n * W, H * W
        return {"world": world, "W": W, "H": H, "shard_rows": n, "packed_rows": world * m,
                "send_side_us": {"copy_accum_device": on["copy_accum_device"], "pack_blocks": on["pack_blocks"],
                                 "pack_mode_off": off["pack_mode_off"], "copy_accum_device_mode_off": off["copy_accum_device"],
                                 "bytes": {"copy": px_s * 24, "pack": px_s * 28},
                                 "blocks": against(on["copy_accum_device"], on["pack_blocks"]),
                                 "mode_off": against(off["copy_accum_device"], off["pack_mode_off"])},
                "frame_side_us": {"index_select": on["index_select"], "load_rows_counted": on["load_rows_counted"],
                                  "bytes": {"index_select": px_f * 24, "load": px_f * 32},
                                  **against(on["index_select"], on["load_rows_counted"])}}
    finally:
        shard.close()
        frame.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "dist_adaptive_bench.json"))
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--burst", type=int, default=20)
    a = ap.parse_args()
    res = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "burst": a.burst,
           "unit": "microseconds per launch (device time between events / burst)",
           "cases": [bench(8, a.reps, a.burst), bench(1, a.reps, a.burst)]}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
