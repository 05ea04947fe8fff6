#!/usr/bin/env python3
"""An adaptive render over N processes, one per GPU, gathered WITH its per-pixel sample counts
(DESIGN.md §3.9.1): ShardedRenderer.render_adaptive_until on every rank, gather_counted() to rank 0,
which writes PREFIX.png (the resolved image, or the filtered one with --denoise N or, with
--denoise-guided N / --denoise-variance N, the noise-guided / the variance-propagating filter over
the shards' gathered error maps) and
PREFIX_samples.pfm (every pixel's sample count in all three channels, as mcpt_render --aov does).

    python tools/adaptive_dist_render.py --gpus 8 --scene 6 --width 1920 --height 1080 \\
        --spp 1024 --chunk 32 --target-error 0.05 [--denoise 3 | --denoise-guided 3 | --denoise-variance 3] --out frame
    python -m torch.distributed.run --nproc-per-node 8 tools/adaptive_dist_render.py --gpus 8 ...

Without a launcher (WORLD_SIZE unset) the tool starts its own --gpus N ranks, as
bench.py --gpus does; each child runs under --timeout seconds of its own, and the first child that
fails (or runs out of time) stops the others.  Ranks that outnumber the GPUs share them (LOCAL_RANK
modulo the device count) over gloo, the rehearsal of the N-GPU path on one GPU; with a GPU per rank
the backend is nccl (RCCL).  Rank 0 prints one JSON line with the merged select record."""
import argparse
import json
import os
import signal
import socket
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "montecarlo-pathtracing_amd"))


def parse():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--gpus", type=int, default=1, help="ranks (one process each)")
    ap.add_argument("--scene", type=int, default=6)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--height", type=int, default=360)
    ap.add_argument("--spp", type=int, default=256, help="the cap on passes per pixel")
    ap.add_argument("--chunk", type=int, default=32, help="passes per render call (one statistics batch)")
    ap.add_argument("--target-error", type=float, default=0.1, help="a block retires once its largest r <= this")
    ap.add_argument("--min-passes", type=int, default=0)
    ap.add_argument("--bounces", type=int, default=3)
    ap.add_argument("--denoise", type=int, default=0, help="a-trous iterations over the resolved image (0: none)")
    ap.add_argument("--denoise-guided", type=int, default=0,
                    help="noise-guided a-trous iterations over the resolved image, the colour width from the "
                         "shards' error maps, which travel with the gather (0: none)")
    ap.add_argument("--denoise-variance", type=int, default=0,
                    help="variance-propagating a-trous iterations over the resolved image, the variance from the "
                         "shards' error maps, which travel with the gather (0: none)")
    ap.add_argument("--out", default="adaptive_dist", help="output prefix")
    ap.add_argument("--backend", choices=("auto", "nccl", "gloo"), default="auto")
    ap.add_argument("--timeout", type=float, default=300.0, help="seconds each child rank may run")
    a = ap.parse_args()
    if a.gpus < 1 or a.spp < 1 or a.chunk < 1 or not a.target_error > 0 or not 0 <= a.denoise <= 8:
        ap.error("--gpus, --spp, --chunk must be >= 1, --target-error > 0, --denoise in 0..8")
    if not 0 <= a.denoise_guided <= 8 or not 0 <= a.denoise_variance <= 8:
        ap.error("--denoise-guided and --denoise-variance in 0..8")
    if (a.denoise > 0) + (a.denoise_guided > 0) + (a.denoise_variance > 0) > 1:
        ap.error("one filter only")
    return a


def launch(a) -> int:
    """Start --gpus child ranks of this script; no HIP call happens in the parent."""
    with socket.socket(socket.AF_INET, socket.SOCK_STREAM) as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    procs = []
    for r in range(a.gpus):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(a.gpus), LOCAL_WORLD_SIZE=str(a.gpus),
                   MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__)] + sys.argv[1:], env=env))
    t_end, status = time.time() + a.timeout, 0
    while status == 0 and any(p.poll() is None for p in procs):
        bad = [(r, p.returncode) for r, p in enumerate(procs) if p.poll() not in (None, 0)]
        if bad:
            status = bad[0][1]
            print(f"adaptive_dist_render: rank {bad[0][0]} exited with status {status}", file=sys.stderr)
        elif time.time() > t_end:
            status = 124
            print(f"adaptive_dist_render: a rank ran longer than {a.timeout:g} s", file=sys.stderr)
        else:
            time.sleep(0.1)
    status = status or next((p.returncode for p in procs if p.returncode), 0)
    for p in procs:                 # the others would block in a collective
        if p.poll() is None:
            p.send_signal(signal.SIGTERM)
    for p in procs:
        try:
            p.wait(timeout=10)
        except subprocess.TimeoutExpired:
            p.kill()
            p.wait()
    return status


def rank_main(a) -> int:
    import numpy as np
    import torch
    import torch.distributed as dist
    import mcpt
    from mcpt.dist import ShardedRenderer

    world, rank = int(os.environ.get("WORLD_SIZE", "1")), int(os.environ.get("RANK", "0"))
    if world != a.gpus:
        print(f"adaptive_dist_render: --gpus {a.gpus} but WORLD_SIZE is {world}", file=sys.stderr)
        return 2
    n_dev = torch.cuda.device_count()
    if n_dev < 1:
        print("adaptive_dist_render: no GPU", file=sys.stderr)
        return 2
    local = int(os.environ.get("LOCAL_RANK", "0")) % n_dev
    torch.cuda.set_device(local)
    backend = a.backend if a.backend != "auto" else ("nccl" if n_dev >= int(os.environ.get("LOCAL_WORLD_SIZE", world)) else "gloo")
    if world > 1:
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=torch.device("cuda", local))
        else:
            dist.init_process_group("gloo")
    sr = None
    try:
        W, H = a.width, a.height
        ipv, iv = mcpt.camera_canonical(W, H)
        sr = ShardedRenderer(W, H, 8, world, rank, local)
        sr.upload_scene(mcpt.Scene.reference(a.scene))
        t0 = time.perf_counter()
        rec = sr.render_adaptive_until(ipv, iv, a.target_error, batch=a.chunk, max_passes=a.spp,
                                       min_passes=a.min_passes, bounces=a.bounces)
        frame = sr.gather_counted(error_map=a.denoise_guided > 0 or a.denoise_variance > 0)
        if frame is not None:
            counts = frame.read_sample_counts()
            if a.denoise_guided > 0:
                frame.render_guides(ipv, iv)
                img = frame.denoise_resolved_guided(a.denoise_guided)
            elif a.denoise_variance > 0:      # (after both gathers: the rows with their counts, the error map)
                frame.render_guides(ipv, iv)
                img = frame.denoise_resolved_variance(a.denoise_variance)
            elif a.denoise > 0:
                frame.render_guides(ipv, iv)
                img = frame.denoise_resolved(a.denoise)
            else:
                img = frame.read_resolved()
            wall = time.perf_counter() - t0
            mcpt.write_png(a.out + ".png", img)
            mcpt.write_pfm(a.out + "_samples.pfm", np.repeat(counts.astype(np.float32)[..., None], 3, axis=2))
            rec.pop("local")
            print(json.dumps(dict(rec, scene=a.scene, W=W, H=H, n_gpus=world, backend=backend if world > 1 else None,
                                  denoise=a.denoise, denoise_guided=a.denoise_guided, denoise_variance=a.denoise_variance,
                                  mean_spp=rec["samples"] / rec["n_px"], wall_s=wall,
                                  png=a.out + ".png", samples=int(counts.sum()))), flush=True)
    finally:
        if sr is not None:
            sr.close()
        if world > 1:
            dist.destroy_process_group()
    return 0


def main() -> int:
    a = parse()
    if "WORLD_SIZE" not in os.environ:   # (one rank too: every process that uses a GPU is a timed child)
        return launch(a)
    return rank_main(a)


if __name__ == "__main__":
    sys.exit(main())
