"""Quality of the variance-propagating filter beside the fixed-sigma and the
noise-guided filters at their defaults, and the sweep that chooses its default k:

scenes 1, 6 and 8 at 96x54 and 480x270, 16 spp rendered as 4 batches of 4, 8 bounces, 5 iterations,
RMSE(denoised) / RMSE(raw) against each scene's own 2,048-spp render; denoise_variance over k_color
in powers of two from 0.5 to 256.  chosen_k = the k with the smallest worst-case ratio over the six
(size, scene) cases: mcpt.DENOISE_K_VARIANCE.  All three filters run in the same session on the
same frames.

  python tools/variance_filter_sweep.py [out.json]      (default profiles/variance_filter_sweep.json)
"""
import json
import os
import sys

import numpy as np
import torch  # noqa: F401  (HIP runtime first)

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "montecarlo-pathtracing_amd")]
import mcpt  # noqa: E402

K_SWEEP = (0.5, 1.0, 2.0, 4.0, 8.0, 16.0, 32.0, 64.0, 128.0, 256.0)


def rmse(a, b):
    return float(np.sqrt(np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2)))


def main():
    cases = []
    r = mcpt.Renderer(0)
    for (W, H) in ((96, 54), (480, 270)):
        for sid in (1, 6, 8):
            r.upload_scene(mcpt.Scene.reference(sid))
            r.set_target(W, H)
            cam = mcpt.camera_canonical(W, H)
            r.stats_begin()
            for k in range(4):
                r.render(cam[0], cam[1], 1 + 4 * k, 4, 0.0, 8, 1.0, 0)
            rec = r.convergence(0.05)
            r.render_guides(*cam)
            raw = r.read_image()
            fixed = r.denoise()
            guided = r.denoise_guided()
            var = {k: r.denoise_variance(5, k) for k in K_SWEEP}
            r.stats_end()
            r.render(cam[0], cam[1], 17, 2032, 0.0, 8, 1.0, 0)
            ref = r.read_image()
            e0 = rmse(raw, ref)
            case = {"W": W, "H": H, "scene": sid, "mean_r": rec["mean_r"], "rmse_raw": e0,
                    "ratio_denoise": rmse(fixed, ref) / e0, "ratio_denoise_guided": rmse(guided, ref) / e0,
                    "ratio_variance": {str(k): rmse(v, ref) / e0 for k, v in var.items()}}
            cases.append(case)
            print(json.dumps(case), flush=True)
    r.close()
    worst = {k: max(c["ratio_variance"][str(k)] for c in cases) for k in K_SWEEP}
    chosen = min(K_SWEEP, key=lambda k: worst[k])
    for c in cases:
        c["ratio_variance_chosen"] = c["ratio_variance"][str(chosen)]
        c["variance_over_denoise"] = c["ratio_variance_chosen"] / c["ratio_denoise"]
        c["variance_over_guided"] = c["ratio_variance_chosen"] / c["ratio_denoise_guided"]
    res = {"device": torch.cuda.get_device_name(0), "spp": 16, "batches": [4, 4, 4, 4], "bounces": 8,
           "reference_spp": 2048, "iterations": 5, "sigma_color": mcpt.DENOISE_SIGMA_COLOR,
           "sigma_plane": mcpt.DENOISE_SIGMA_PLANE, "k_color_guided": mcpt.DENOISE_K_COLOR, "k_sweep": list(K_SWEEP),
           "worst_ratio_by_k": {str(k): v for k, v in worst.items()}, "chosen_k": chosen,
           "library_default_k": mcpt.DENOISE_K_VARIANCE, "cases": cases}
    print(json.dumps({"worst_ratio_by_k": res["worst_ratio_by_k"], "chosen_k": chosen}), flush=True)
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(REPO, "profiles", "variance_filter_sweep.json")
    with open(path, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
