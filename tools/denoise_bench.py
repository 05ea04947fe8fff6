"""Time the guide kernel and every à-trous iteration: scene 6 at 1080p and 4K, 64 spp, the LDS
variant (LDS tiles for steps 1-2, global taps from step 4; MCPT_DENOISE_NAIVE=0) against the
naive variant (every tap from global memory, MCPT_DENOISE_NAIVE=1), and which of them the
library runs when the variable is unset ("shipped").  Per size and step a verdict: "lds_faster" /
"naive_faster" when the quartile ranges of the 20 repeats do not overlap, else "tie"; the LDS
kernels may ship only where no step is "naive_faster".  Each figure is the median of 20 repeats after 3
warm-up runs, interleaved A/B/A/B so drift hits both alike; HIP-event times
(mcpt_last_denoise_ms, mcpt_denoise_iteration_ms).  Beside them the traffic floor: 64 B per pixel
and iteration (read colour 16 + guides 32, write 16) at the 8 TB/s HBM peak.

  python tools/denoise_bench.py [--out profiles/denoise_bench.json] [--repeats 20]

--variance: the variance-propagating filter against the noise-guided one instead,
same sizes and protocol (64 spp as 4 batches of 16 for the error map; the shipped kernel paths;
guided / variance interleaved): the first step (slot -1: the averaging, for the variance filter
with the 3x3 prefilter of se^2 fused in) and every iteration, with a verdict per slot as above.

  python tools/denoise_bench.py --variance [--out profiles/variance_filter_bench.json]
"""
import argparse
import json
import os
import statistics
import sys

import torch  # noqa: F401  (HIP runtime first)

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "montecarlo-pathtracing_amd")]
import mcpt  # noqa: E402

HBM_PEAK = 8.0e12
ITERS = 5


def spread(v):
    q = statistics.quantiles(v, n=4)
    return {"median_ms": statistics.median(v), "q1_ms": q[0], "q3_ms": q[2], "min_ms": min(v), "max_ms": max(v)}


def variance_ab(a):
    r = mcpt.Renderer(0)
    r.upload_scene(mcpt.Scene.reference(6))
    res = {"scene": 6, "spp": a.spp, "batches": 4, "iterations": ITERS, "repeats": a.repeats, "warmup": a.warmup,
           "k_color": mcpt.DENOISE_K_COLOR, "k_variance": mcpt.DENOISE_K_VARIANCE,
           "sigma_plane": mcpt.DENOISE_SIGMA_PLANE, "device": torch.cuda.get_device_name(0), "sizes": []}
    slots = ["first_step"] + [f"step_{1 << s}" for s in range(ITERS)] + ["filter_total"]
    for W, H in ((1920, 1080), (3840, 2160)):
        r.set_target(W, H)
        cam = mcpt.camera_canonical(W, H)
        r.stats_begin()
        for k in range(4):
            r.render(cam[0], cam[1], 1 + k * (a.spp // 4), a.spp // 4, 0.0, 8, 1.0, 0)
        r.convergence(0.05)
        r.render_guides(*cam)
        forms = {"guided": r.denoise_guided, "variance": r.denoise_variance}
        times = {name: {sl: [] for sl in slots} for name in forms}
        for k in range(a.warmup + a.repeats):
            for name, form in forms.items():
                form(ITERS)
                if k >= a.warmup:
                    t = times[name]
                    t["first_step"].append(r.denoise_iteration_ms(-1))
                    for s in range(ITERS):
                        t[f"step_{1 << s}"].append(r.denoise_iteration_ms(s))
                    t["filter_total"].append(r.last_denoise_ms()[1])
        r.stats_end()
        entry = {"W": W, "H": H, "lds_mask": r.last_denoise_path(),
                 "guided": {sl: spread(v) for sl, v in times["guided"].items()},
                 "variance": {sl: spread(v) for sl, v in times["variance"].items()}, "verdicts": {}}
        for sl in slots:
            g, v = entry["guided"][sl], entry["variance"][sl]
            entry["verdicts"][sl] = {
                "verdict": "variance_faster" if v["q3_ms"] < g["q1_ms"] else ("guided_faster" if g["q3_ms"] < v["q1_ms"] else "tie"),
                "variance_over_guided": v["median_ms"] / g["median_ms"]}
        res["sizes"].append(entry)
        print(json.dumps(entry), flush=True)
    r.close()
    with open(a.out or os.path.join(REPO, "profiles", "variance_filter_bench.json"), "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--variance", action="store_true")
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--spp", type=int, default=64)
    a = ap.parse_args()
    if a.variance:
        return variance_ab(a)
    a.out = a.out or os.path.join(REPO, "profiles", "denoise_bench.json")
    r = mcpt.Renderer(0)
    r.upload_scene(mcpt.Scene.reference(6))
    res = {"scene": 6, "spp": a.spp, "iterations": ITERS, "repeats": a.repeats, "warmup": a.warmup,
           "sigma_color": mcpt.DENOISE_SIGMA_COLOR, "sigma_plane": mcpt.DENOISE_SIGMA_PLANE,
           "device": torch.cuda.get_device_name(0), "sizes": []}
    for W, H in ((1920, 1080), (3840, 2160)):
        r.set_target(W, H)
        cam = mcpt.camera_canonical(W, H)
        r.render(cam[0], cam[1], 1, a.spp, 0.0, 8, 1.0, 0)
        r.synchronize()
        guides = []
        times = {"lds": [[] for _ in range(ITERS + 2)], "naive": [[] for _ in range(ITERS + 2)]}
        images = {}
        for k in range(a.warmup + a.repeats):
            r.render_guides(*cam)
            g_ms = r.last_denoise_ms()[0]
            for name in ("lds", "naive"):
                os.environ["MCPT_DENOISE_NAIVE"] = "1" if name == "naive" else "0"
                images[name] = r.denoise(ITERS)
                assert r.last_denoise_path() == (0 if name == "naive" else 3)
                if k >= a.warmup:
                    t = times[name]
                    for s in range(ITERS):
                        t[s].append(r.denoise_iteration_ms(s))
                    t[ITERS].append(r.denoise_iteration_ms(-1))
                    t[ITERS + 1].append(r.last_denoise_ms()[1])
            os.environ.pop("MCPT_DENOISE_NAIVE", None)
            if k >= a.warmup:
                guides.append(g_ms)
        same = bool((images["lds"].view("uint32") == images["naive"].view("uint32")).all())
        r.denoise(ITERS)   # the variable unset: what the library ships
        shipped = "lds" if r.last_denoise_path() else "naive"
        floor_ms = 64.0 * W * H / HBM_PEAK * 1e3
        entry = {"W": W, "H": H, "guides": spread(guides), "same_bits": same,
                 "traffic_floor_ms_per_iteration": floor_ms, "bytes_per_pixel_per_iteration": 64,
                 "hbm_peak_bytes_per_s": HBM_PEAK}
        for name, t in times.items():
            entry[name] = {"iterations": [dict(step=1 << s, **spread(t[s])) for s in range(ITERS)],
                           "average": spread(t[ITERS]), "filter_total": spread(t[ITERS + 1])}
        verdicts = []
        for s in range(ITERS):
            l, n = entry["lds"]["iterations"][s], entry["naive"]["iterations"][s]
            v = "lds_faster" if l["q3_ms"] < n["q1_ms"] else ("naive_faster" if n["q3_ms"] < l["q1_ms"] else "tie")
            verdicts.append({"step": 1 << s, "same_kernel": s >= 2, "verdict": v,
                             "lds_over_naive": l["median_ms"] / n["median_ms"]})
        entry["verdicts"] = verdicts
        entry["shipped"] = shipped
        entry["lds_may_ship"] = all(v["verdict"] != "naive_faster" for v in verdicts if not v["same_kernel"])
        entry["shipped_meets_condition"] = shipped == "naive" or entry["lds_may_ship"]
        res["sizes"].append(entry)
        print(json.dumps(entry), flush=True)
    r.close()
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
