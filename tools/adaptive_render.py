#!/usr/bin/env python3
"""One adaptive session with one library build (MCPT_LIB), saved as an .npz
(tests/test_gpu_adaptive.py runs it with the checked build, libmcpt_checked.so).

    MCPT_LIB=.../variants/libmcpt_checked.so python tools/adaptive_render.py --scene 6 \
        --size 45x37 --threshold 0.3 --batches 4,4,8,3,32,40 --out run.npz

stats_begin + adaptive_begin on a cleared target, one render_adaptive per batch, a select after
every batch from the second on.  Prints the build flags, each select's record and the checked
build's bounds count; a checked build also fails the render call on an out-of-range index."""
import argparse
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "montecarlo-pathtracing_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402,F401  (HIP runtime first)
import mcpt  # noqa: E402

CHECKED_COUNT_SLOT = 60   # mcpt_internal.h kCheckedCountSlot


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", type=int, default=6)
    ap.add_argument("--size", default="45x37")
    ap.add_argument("--threshold", type=float, required=True)
    ap.add_argument("--mu-floor", type=float, default=mcpt.ERROR_MU_FLOOR)
    ap.add_argument("--min-passes", type=int, default=0)
    ap.add_argument("--bounces", type=int, default=4)
    ap.add_argument("--batches", default="4,4,8,3,32,40")
    ap.add_argument("--out", required=True)
    a = ap.parse_args()
    W, H = map(int, a.size.split("x"))
    print("lib", mcpt.lib_path(), "build_flags", mcpt.build_flags(), flush=True)
    r = mcpt.Renderer(0)
    try:
        r.upload_scene(mcpt.Scene.reference(a.scene))
        r.set_target(W, H)
        ipv, iv = mcpt.camera_canonical(W, H)
        r.stats_begin()
        r.adaptive_begin(a.min_passes)
        first = 1
        for k, n in enumerate(int(x) for x in a.batches.split(",")):
            r.render_adaptive(ipv, iv, first, n, 0.0, a.bounces, 1.0, mcpt.MONTECARLO)
            first += n
            if k >= 1:
                print("select", r.adaptive_select(a.threshold, a.mu_floor), flush=True)
        acc, _ = r.read_accum()
        np.savez(a.out, accum=acc, counts=r.read_sample_counts(), resolved=r.read_resolved(),
                 active=r.read_active_blocks())
        print("bounds_violations", int(r.debug_counters(reset=False)[CHECKED_COUNT_SLOT]), flush=True)
    finally:
        r.close()
    print("ok", flush=True)


if __name__ == "__main__":
    main()
