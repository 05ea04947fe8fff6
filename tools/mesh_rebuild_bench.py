#!/usr/bin/env python3
"""The device rebuild of mesh BVHs on the HBM-sized mesh workloads: big_mesh_scene
(one 1 M-triangle sphere, bench.py --config mesh) and big_mesh4_scene (four meshes of 1 M triangles,
--config mesh_big).  Per scene:

1. the rebuild's device time (HIP events, mcpt_rebuild_t), its sort and its refit apart, against the
   sort's byte floor — per radix pass and triangle 28 B: the id read twice (count, scatter), its
   64-bit sort word looked up twice, the id written once — at the device-to-device copy bandwidth
   measured here;
2. against the host route, timed in the same run: add_mesh + mesh_buffers + upload_meshes;
3. a strongly deformed mesh (a twist of several turns about z, drawn in so that every vertex stays in
   the mesh's box) rendered through (a) the refitted tree of the uploaded order and (b) the rebuilt
   tree, two contexts alternating: kernel Msamples/s and the `mesh` / `tri` event counters per
   traversal (counts: they do not depend on timing).

    python tools/mesh_rebuild_bench.py [--tris 1000000] [--out profiles/mesh_rebuild_bench.json]
"""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "montecarlo-pathtracing_amd"), os.path.join(REPO, "tools")]

import numpy as np  # noqa: E402
import torch  # noqa: E402  (HIP runtime first)

import mcpt  # noqa: E402
from mcpt import meshes  # noqa: E402
from mesh_refit_bench import copy_bandwidth, spread  # noqa: E402

PASS_BYTES_PER_TRIANGLE = 4 + 8 + 4 + 8 + 4   # count: id, word; scatter: id, word, id written


def sort_passes(depth):
    return sum((32 + r - 1 + 7) // 8 for r in range(1, depth))


def twisted(v, n, turns):
    """v turned about z by `turns` turns over the mesh's height and drawn in by 0.7 in x and y."""
    v64, n64 = v.astype(np.float64), n.astype(np.float64)
    z = v64[:, 2]
    a = 2.0 * np.pi * turns * (z - z.min()) / max(1e-9, z.max() - z.min())
    c, s = np.cos(a), np.sin(a)
    rot = lambda p: np.stack([0.7 * (c * p[:, 0] - s * p[:, 1]), 0.7 * (s * p[:, 0] + c * p[:, 1]), p[:, 2]], 1)
    return rot(v64).astype(np.float32), rot(n64).astype(np.float32)


def render_rate(r, ipv, iv, W, H, spp, bounces, first):
    r.render(ipv, iv, first, spp, 0.0, bounces, 1.0, 0)
    return W * H * spp / (r.last_kernel_ms()[0] * 1e-3) / 1e6


def bench_scene(name, build, a, bw):
    sc, n_tris = build(a.tris)
    mb = sc.mesh_buffers()
    n_meshes = len(mb["info"])
    ranges = [sc.mesh_vertex_range(k) for k in range(n_meshes)]
    r = mcpt.Renderer(0)
    r.set_traversal(1)
    r.upload_scene(sc)
    # (2) the host route on the same meshes: build every mesh, fetch the buffers, upload them
    t0 = time.perf_counter()
    s2 = mcpt.Scene()
    for k, (first, n) in enumerate(ranges):
        to = int(mb["info"][k, 3])
        te = int(mb["info"][k + 1, 3]) if k + 1 < n_meshes else len(mb["tris"])
        s2.add_mesh(mb["verts"][first:first + n], mb["normals"][first:first + n], mb["tris"][to:te] - first)
    t_add = time.perf_counter() - t0
    mb2 = s2.mesh_buffers()
    t_buf = time.perf_counter() - t0 - t_add
    r.upload_meshes(mb2)
    r.synchronize()
    t_host = time.perf_counter() - t0
    del s2, mb2
    # (1) the rebuild: warm-up (it sizes the scratch), then repeats, each with its own events
    r.rebuild_mesh(-1)
    recs = [r.rebuild_mesh(-1) for _ in range(a.reps)]
    sort_ms, refit_ms = [x["sort_ms"] for x in recs], [x["refit_ms"] for x in recs]
    total_ms = [x["device_ms"] for x in recs]
    tris_per_mesh = [int(mb["info"][k + 1, 3] if k + 1 < n_meshes else len(mb["tris"])) - int(mb["info"][k, 3])
                     for k in range(n_meshes)]
    passes = [sort_passes(int(d)) for d in mb["info"][:, 2]]
    floor_b = sum(p * t * PASS_BYTES_PER_TRIANGLE for p, t in zip(passes, tris_per_mesh))
    floor_ms = floor_b / (bw["median"] * 1e9) * 1e3
    med = spread(total_ms)["median"]
    # (3) the deformed meshes through the refitted and through the rebuilt tree
    A = mcpt.Renderer(0)
    A.set_traversal(1)
    for ctx in (r, A):
        ctx.upload_scene(sc)      # (r: the uploaded order again)
        for first, n in ranges:
            ctx.update_mesh_vertices(first, *twisted(mb["verts"][first:first + n], mb["normals"][first:first + n], a.turns))
    r.refit_mesh(-1)
    A.rebuild_mesh(-1)
    W, H = 1920, 1080
    ipv, iv = mcpt.camera_canonical(W, H)
    counters = {}
    for key, ctx in (("refit", r), ("rebuild", A)):
        ctx.set_target(480, 270)
        ev = ctx.render_counted(mcpt.camera_canonical(480, 270)[0], mcpt.camera_canonical(480, 270)[1], 1, 4, 0.0,
                                a.bounces, 1.0, 0)
        e = dict(zip(mcpt.EVENT_NAMES, (int(x) for x in ev)))
        counters[key] = {"events": e, "mesh_per_trav": round(e["mesh"] / max(1, e["trav"]), 3),
                         "tri_per_trav": round(e["tri"] / max(1, e["trav"]), 3)}
        ctx.set_target(W, H)
        render_rate(ctx, ipv, iv, W, H, a.spp, a.bounces, 1)   # warm-up
    rate = {"refit": [], "rebuild": []}
    for k in range(a.render_reps):
        for key, ctx in (("refit", r), ("rebuild", A)):
            rate[key].append(render_rate(ctx, ipv, iv, W, H, a.spp, a.bounces, 1 + a.spp * (k + 1)))
    r.close()
    A.close()
    return {"scene": name, "triangles": n_tris, "rebuild_device_ms": spread(total_ms), "sort_ms": spread(sort_ms),
            "refit_ms": spread(refit_ms), "rounds": recs[0]["rounds"], "sort_passes": recs[0]["sort_passes"],
            "sort_floor": {"bytes_per_pass_and_triangle": PASS_BYTES_PER_TRIANGLE, "passes_per_mesh": passes,
                           "bytes": floor_b, "ms_at_copy_bandwidth": round(floor_ms, 4),
                           "sort_over_floor": round(spread(sort_ms)["median"] / floor_ms, 2)},
            "host_route_wall_s": {"add_mesh": round(t_add, 3), "mesh_buffers": round(t_buf, 3),
                                  "upload_meshes": round(t_host - t_add - t_buf, 3), "total": round(t_host, 3)},
            "host_route_over_rebuild": round(t_host * 1e3 / med, 1),
            "deformed": {"turns": a.turns, "counters_480x270_4spp": counters,
                         "render_msamples_s": {k: spread(v) for k, v in rate.items()},
                         "spp": a.spp, "bounces": a.bounces, "target": [W, H], "traversal": "lane"}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tris", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--render-reps", type=int, default=4)
    ap.add_argument("--spp", type=int, default=32)
    ap.add_argument("--bounces", type=int, default=8)
    ap.add_argument("--turns", type=float, default=3.0)
    ap.add_argument("--scenes", nargs="+", default=["mesh", "mesh_big"])
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "mesh_rebuild_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mesh_rebuild_bench needs a GPU")
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
