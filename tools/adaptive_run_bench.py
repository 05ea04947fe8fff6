#!/usr/bin/env python3
"""Wall time of an adaptive render as a host loop and as queued runs
-> profiles/adaptive_run_bench.json.

    python tools/adaptive_run_bench.py [--out profiles/adaptive_run_bench.json] [--reps 9] [--warm 2]
                                       [--sizes 480x270,1920x1080] [--scenes 1,6,8] [--rules raw,filtered]
                                       [--threshold 0.1] [--budget-s S]

§3.9 (d)'s protocol: 8 bounces, batches of 32 passes, min_passes 64, cap 1,024, a select after every
batch from the second on.  Per scene, size and rule (mcpt_adaptive_select, or
mcpt_adaptive_select_filtered with 5 iterations and raw_cap 64), in one process and interleaved
repetition by repetition:
  host     the loop over render_adaptive and the select, one host wait per select;
  queued K the same rounds as mcpt_adaptive_run* calls of up to K rounds, K in 4, 16, 31 (the same bits:
           the records' sample totals are compared);
  uniform  render() of the host loop's mean sample count (rounded to whole passes) in calls of 32 passes.
Per run: wall ms on the host clock from the target's set-up to the last wait (the guides included for
the filtered rule), for the queued runs the sum of device_ms, and dead_entry_share: of the list entries
the run's render launches held (the list's length when each run was queued), the share that lay past
the length the device read (their workgroups return before the scene is staged; per round this is the
share of dead workgroups up to one workgroup group).  Medians of `reps` after `warm` warm-ups; spread =
(max - min) / median.  The ratios are host / queued and host / uniform of the medians."""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "montecarlo-pathtracing_amd"))
import torch  # noqa: E402,F401  (HIP runtime first)
import mcpt  # noqa: E402

BOUNCES, BATCH, MIN_PASSES, CAP, ITER, RAW_CAP = 8, 32, 64, 1024, 5, 64.0
KS = (4, 16, 31)


def med(v):
    v = sorted(v)
    m = v[len(v) // 2]
    return {"median": m, "min": v[0], "max": v[-1], "spread": (v[-1] - v[0]) / m if m else 0.0, "n": len(v)}


def begin(r, cam, W, H, filtered):
    r.set_target(W, H)
    r.synchronize()
    t0 = time.perf_counter()
    if filtered:
        r.render_guides(*cam)
    r.stats_begin()
    r.adaptive_begin(MIN_PASSES)
    return t0


def end(r, t0, rec, done, extra):
    r.synchronize()
    wall = (time.perf_counter() - t0) * 1e3
    r.adaptive_end()
    r.stats_end()
    return dict({"wall_ms": wall, "rendered": done, "samples": rec["samples"], "mean_spp": rec["samples"] / rec["n_px"],
                 "n_active_blocks_at_end": rec["n_active_blocks"]}, **extra)


def host_loop(r, cam, W, H, thr, filtered):
    t0 = begin(r, cam, W, H, filtered)
    done, rec, selects = 0, None, 0
    while done < CAP:
        r.render_adaptive(cam[0], cam[1], 1 + done, BATCH, 0.0, BOUNCES)
        done += BATCH
        if done >= 2 * BATCH:
            rec = r.adaptive_select_filtered(thr, RAW_CAP, iterations=ITER) if filtered else r.adaptive_select(thr)
            selects += 1
            if rec["n_active_blocks"] == 0:
                break
    return end(r, t0, rec, done, {"host_waits": selects})


def queued(r, cam, W, H, thr, filtered, K):
    t0 = begin(r, cam, W, H, filtered)
    done, rec, runs, dev, held, live = 0, None, 0, 0.0, 0, 0
    n_list = r.adaptive_info()["n_blocks"]
    while done < CAP and n_list > 0:
        k = min(K, (CAP - done) // BATCH)
        if filtered:
            got = r.adaptive_run_filtered(cam[0], cam[1], 1 + done, BATCH, k, thr, 1, RAW_CAP, iterations=ITER, bounces=BOUNCES)
        else:
            got = r.adaptive_run(cam[0], cam[1], 1 + done, BATCH, k, thr, 1, bounces=BOUNCES)
        runs += 1
        dev += got["device_ms"]
        b0, cur, j = done // BATCH, n_list, 0
        for i in range(k):                       # round i's launch held n_list entries, `cur` of them live
            held += n_list
            live += cur
            if b0 + i + 1 >= 2 and j < len(got["records"]):
                cur = got["records"][j]["n_active_blocks"]
                j += 1
            elif b0 + i + 1 >= 2:
                cur = 0                          # (queued behind the select that emptied the list)
        done += got["rounds_run"] * BATCH
        if got["records"]:
            rec = got["records"][-1]
            n_list = rec["n_active_blocks"]
    return end(r, t0, rec, done, {"host_waits": runs, "device_ms": dev, "dead_entry_share": 1.0 - live / held if held else 0.0})


def uniform(r, cam, W, H, spp):
    r.set_target(W, H)
    r.synchronize()
    t0 = time.perf_counter()
    done = 0
    while done < spp:
        n = min(BATCH, spp - done)
        r.render(cam[0], cam[1], 1 + done, n, 0.0, BOUNCES)
        done += n
    r.synchronize()
    return {"wall_ms": (time.perf_counter() - t0) * 1e3, "spp": spp}


def bench(r, scene, W, H, filtered, thr, reps, warm):
    cam = mcpt.camera_canonical(W, H)
    modes = ["host"] + [f"queued_{k}" for k in KS] + ["uniform"]
    wall = {m: [] for m in modes}
    dev = {f"queued_{k}": [] for k in KS}
    last = {}
    for rep in range(reps + warm):
        runs = {"host": host_loop(r, cam, W, H, thr, filtered)}
        for k in KS:
            runs[f"queued_{k}"] = queued(r, cam, W, H, thr, filtered, k)
            assert runs[f"queued_{k}"]["samples"] == runs["host"]["samples"], (k, runs)      # the same render
            assert runs[f"queued_{k}"]["rendered"] == runs["host"]["rendered"], (k, runs)
        runs["uniform"] = uniform(r, cam, W, H, max(1, int(round(runs["host"]["mean_spp"]))))
        if rep >= warm:
            for m in modes:
                wall[m].append(runs[m]["wall_ms"])
            for k in KS:
                dev[f"queued_{k}"].append(runs[f"queued_{k}"]["device_ms"])
        last = runs
    row = {"scene": scene, "W": W, "H": H, "rule": "filtered" if filtered else "raw", "threshold": thr,
           "bounces": BOUNCES, "batch": BATCH, "min_passes": MIN_PASSES, "cap": CAP,
           "mean_spp": last["host"]["mean_spp"], "rendered": last["host"]["rendered"],
           "n_active_blocks_at_end": last["host"]["n_active_blocks_at_end"], "uniform_spp": last["uniform"]["spp"]}
    for m in modes:
        row[m] = {"wall_ms": med(wall[m])}
        if m in dev:
            row[m]["device_ms"] = med(dev[m])
            row[m]["dead_entry_share"] = last[m]["dead_entry_share"]
        if m != "uniform":
            row[m]["host_waits"] = last[m]["host_waits"]
    h = row["host"]["wall_ms"]["median"]
    row["host_over_queued"] = {f"queued_{k}": h / row[f"queued_{k}"]["wall_ms"]["median"] for k in KS}
    row["host_over_uniform"] = h / row["uniform"]["wall_ms"]["median"]
    row["best_queued_over_uniform"] = min(row[f"queued_{k}"]["wall_ms"]["median"] for k in KS) / row["uniform"]["wall_ms"]["median"]
    return row


def save(path, res):
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(res, f, indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "adaptive_run_bench.json"))
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warm", type=int, default=2)
    ap.add_argument("--sizes", default="480x270,1920x1080")
    ap.add_argument("--scenes", default="1,6,8")
    ap.add_argument("--rules", default="raw,filtered")
    ap.add_argument("--threshold", type=float, default=0.1)
    ap.add_argument("--budget-s", type=float, default=0.0, help="start no further row after this many seconds (0: no limit)")
    a = ap.parse_args()
    t_start = time.perf_counter()
    r = mcpt.Renderer(0)
    rows = []
    res = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "warm": a.warm, "rows": rows}
    try:
        for size in a.sizes.split(","):
            W, H = (int(x) for x in size.split("x"))
            for scene in (int(s) for s in a.scenes.split(",")):
                r.upload_scene(mcpt.Scene.reference(scene))
                for rule in a.rules.split(","):
                    if a.budget_s and time.perf_counter() - t_start > a.budget_s:
                        res.setdefault("not_measured", []).append({"scene": scene, "W": W, "H": H, "rule": rule,
                                                                   "why": "--budget-s reached"})
                        continue
                    rows.append(bench(r, scene, W, H, rule == "filtered", a.threshold, a.reps, a.warm))
                    print(json.dumps(rows[-1]), flush=True)
                    save(a.out, res)                     # (after every row: a run cut short keeps what it measured)
    finally:
        r.close()
    save(a.out, res)


if __name__ == "__main__":
    main()
