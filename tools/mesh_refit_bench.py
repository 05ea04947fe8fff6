#!/usr/bin/env python3
"""The device refit of mesh BVH records on the HBM-sized mesh workloads:
big_mesh_scene (one 1 M-triangle sphere, bench.py --config mesh) and big_mesh4_scene (four meshes of
1 M triangles, --config mesh_big).  Three figures per scene:

1. the refit's device time (HIP events around its kernels, mcpt_refit_t) against its byte floor —
   per leaf 16 B of triangle ids and 3 x 16 B of vertices read and a 64 B leaf record written, per
   internal node a 64 B pair record written — at the device-to-device copy bandwidth this box
   sustains, measured here (a 512 MB torch copy: read + written bytes over its event time);
2. against the only other route to a moved vertex: the wall time of add_mesh + mesh_buffers +
   upload_meshes for the same meshes;
3. the mesh workload's Msamples/s (kernel time of full-frame renders) before and after a refit with
   unchanged vertices: the records are the same bits, so the two must agree within their spread.

    python tools/mesh_refit_bench.py [--tris 1000000] [--out profiles/mesh_refit_bench.json]
"""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "montecarlo-pathtracing_amd")]

import numpy as np  # noqa: E402
import torch  # noqa: E402  (HIP runtime first)

import mcpt  # noqa: E402
from mcpt import meshes  # noqa: E402


def spread(v):
    q1, med, q3 = np.percentile(np.asarray(v, np.float64), [25, 50, 75])
    return {"median": round(float(med), 4), "q1": round(float(q1), 4), "q3": round(float(q3), 4), "n": len(v)}


def copy_bandwidth(reps=20, nbytes=512 << 20):
    """GB/s of a device-to-device copy, read + written bytes over the copy's event time."""
    a = torch.empty(nbytes, dtype=torch.uint8, device="cuda:0")
    b = torch.empty_like(a)
    for _ in range(3):
        b.copy_(a)
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        b.copy_(a)
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    del a, b
    return spread([2 * nbytes / (t * 1e-3) / 1e9 for t in ms]), spread(ms)


def floor_bytes(mb):
    n_leaves = sum(1 << int(d) for d in mb["info"][:, 2])
    n_tris = int((mb["leaves"] >= 0).sum())
    n_internal = n_leaves - len(mb["info"])
    return {"read": n_tris * (16 + 3 * 16) + n_leaves * 4, "written": n_tris * 64 + n_internal * 64,
            "triangles": n_tris, "leaves": n_leaves, "internal_nodes": n_internal}


def render_rate(r, ipv, iv, W, H, spp, bounces, first, reps):
    rates = []
    for k in range(reps):
        r.render(ipv, iv, first + k * spp, spp, 0.0, bounces, 1.0, 0)
        rates.append(W * H * spp / (r.last_kernel_ms()[0] * 1e-3) / 1e6)
    return rates


def bench_scene(name, build, a, bw):
    t0 = time.perf_counter()
    sc, n_tris = build(a.tris)
    t_scene = time.perf_counter() - t0
    mb = sc.mesh_buffers()
    r = mcpt.Renderer(0)
    r.set_traversal(1)
    r.upload_scene(sc)
    # (2) the host route, timed on the same meshes: rebuild every mesh, fetch the buffers, upload them
    t0 = time.perf_counter()
    s2 = mcpt.Scene()
    for k in range(len(mb["info"])):
        first, n = sc.mesh_vertex_range(k)
        to = int(mb["info"][k, 3])
        te = int(mb["info"][k + 1, 3]) if k + 1 < len(mb["info"]) else len(mb["tris"])
        s2.add_mesh(mb["verts"][first:first + n], mb["normals"][first:first + n], mb["tris"][to:te] - first)
    t_add = time.perf_counter() - t0
    mb2 = s2.mesh_buffers()
    t_buf = time.perf_counter() - t0 - t_add
    r.upload_meshes(mb2)
    r.synchronize()
    t_host = time.perf_counter() - t0
    # (1) the refit: warm-up, then repeats, each with its own events
    fb = floor_bytes(mb)
    r.refit_mesh(-1)
    ms = [r.refit_mesh(-1)["device_ms"] for _ in range(a.reps)]
    t0 = time.perf_counter()
    for k in range(len(mb["info"])):
        first, n = sc.mesh_vertex_range(k)
        r.update_mesh_vertices(first, mb["verts"][first:first + n], mb["normals"][first:first + n])
    r.synchronize()
    t_push = time.perf_counter() - t0
    floor_ms = (fb["read"] + fb["written"]) / (bw["median"] * 1e9) * 1e3
    med = spread(ms)["median"]
    # (3) the render path before and after a refit of the unchanged meshes, alternating
    W, H = 1920, 1080
    r.set_target(W, H)
    ipv, iv = mcpt.camera_canonical(W, H)
    render_rate(r, ipv, iv, W, H, a.spp, a.bounces, 1, 1)   # warm-up
    before, after = [], []
    for k in range(a.render_reps):
        before += render_rate(r, ipv, iv, W, H, a.spp, a.bounces, 1 + a.spp * (2 * k + 1), 1)
        r.refit_mesh(-1)
        after += render_rate(r, ipv, iv, W, H, a.spp, a.bounces, 1 + a.spp * (2 * k + 2), 1)
    r.close()
    return {"scene": name, "triangles": n_tris, "scene_build_s": round(t_scene, 2), "floor_bytes": fb,
            "bytes_per_triangle": round((fb["read"] + fb["written"]) / fb["triangles"], 1),
            "refit_device_ms": spread(ms), "floor_ms_at_copy_bandwidth": round(floor_ms, 4),
            "refit_over_floor": round(med / floor_ms, 2),
            "refit_gb_s": round((fb["read"] + fb["written"]) / (med * 1e-3) / 1e9, 1),
            "vertex_update_host_arrays_wall_ms": round(t_push * 1e3, 2),
            "host_route_wall_s": {"add_mesh": round(t_add, 3), "mesh_buffers": round(t_buf, 3),
                                  "upload_meshes": round(t_host - t_add - t_buf, 3), "total": round(t_host, 3)},
            "host_route_over_refit": round(t_host * 1e3 / med, 1),
            "render_msamples_s": {"before_refit": spread(before), "after_refit": spread(after), "spp": a.spp,
                                  "bounces": a.bounces, "target": [W, H], "traversal": "lane"}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tris", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--render-reps", type=int, default=4)
    ap.add_argument("--spp", type=int, default=32)
    ap.add_argument("--bounces", type=int, default=8)
    ap.add_argument("--scenes", nargs="+", default=["mesh", "mesh_big"])
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "mesh_refit_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mesh_refit_bench needs a GPU")
    bw, bw_ms = copy_bandwidth()
    builders = {"mesh": meshes.big_mesh_scene, "mesh_big": meshes.big_mesh4_scene}
    res = {"device": torch.cuda.get_device_name(0), "copy_bandwidth_gb_s": bw, "copy_512MB_ms": bw_ms, "scenes": []}
    for name in a.scenes:
        entry = bench_scene(name, builders[name], a, bw)
        res["scenes"].append(entry)
        print(json.dumps(entry), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
