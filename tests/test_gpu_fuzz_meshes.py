"""Mesh fuzz on the GPU: the random mesh scenes of fuzz_meshes.py (one-triangle to 400-triangle
meshes, open, planar, degenerate and far-from-origin ones, mirrored and strongly non-uniform
instances) rendered, queried and event-counted against the oracle.  Every comparison is on bits;
a non-finite value must simply be the oracle's too."""
import numpy as np
import pytest

import fuzz_meshes as fm

pytestmark = pytest.mark.gpu

IN_VIEW_SEEDS = (4, 7, 12, 18, 24, 25, 30, 45)   # (18, 24, 30: far meshes; 7, 25: the tiny soups)


def bits(a):
    return np.asarray(a, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def renderer(mcpt_mod):
    r = mcpt_mod.Renderer(0)
    yield r
    r.close()


def reset(renderer):
    renderer.set_traversal(0)
    renderer.set_walk_exit(-1)
    renderer.set_leaf_batch(-1)
    renderer.set_flat_face(False)


def compare_queries(mcpt_mod, oracle_mod, renderer, sc, o, d):
    """Closest and any-hit queries field by field (test_gpu_meshes.test_mesh_queries); returns
    the closest hits."""
    prims, nodes, leaves = sc.buffers()
    mv = oracle_mod.MeshView(sc.mesh_buffers())
    closest = None
    for any_hit in (False, True):
        hits = renderer.trace(o, d, any_hit=any_hit)
        oi, of = oracle_mod.trace(prims, nodes, leaves, sc.depth(), o, d, any_hit=any_hit, meshes=mv)
        assert np.array_equal(hits["shape"], oi[:, 0]), any_hit
        hit = oi[:, 0] >= 0
        assert np.array_equal(hits["prim"][hit], oi[hit, 1]) and np.array_equal(hits["dir"][hit], oi[hit, 2]), any_hit
        flat = np.concatenate([hits["dist"][:, None], hits["pl"], hits["pg"], hits["N"], hits["P"], hits["color"],
                               hits["material"]], axis=1)
        assert np.array_equal(bits(flat), bits(of)), any_hit
        closest = hits if closest is None else closest
    return closest


@pytest.mark.parametrize("seed", range(48))
def test_random_mesh_scene_render(mcpt_mod, oracle_mod, renderer, seed):
    rng = np.random.default_rng(3000 + seed)
    sc, spec = fm.random_mesh_scene(mcpt_mod, seed)
    prims, nodes, leaves = sc.buffers()
    W, H = int(rng.integers(8, 49)), int(rng.integers(8, 41))
    first, S, B = int(rng.integers(1, 81)), int(rng.integers(1, 4)), int(rng.integers(0, 9))
    ior = 1.0 if rng.random() < 0.4 else float(rng.uniform(1.05, 2.0))
    variant = 0 if rng.random() < 0.8 else int(rng.integers(1, 3))
    traversal = int(rng.integers(1, 4))
    walk_exit = int(rng.choice([-1, 0, 4, 16, 40, 63]))
    leaf_batch = int(rng.choice([-1, 0, 2, 8, 64]))
    flat = bool(rng.random() < 0.3)
    ipv, iv = mcpt_mod.camera_canonical(W, H)
    bare = None
    try:
        renderer.set_traversal(traversal)
        renderer.set_walk_exit(walk_exit)
        renderer.set_leaf_batch(leaf_batch)
        renderer.set_flat_face(flat)
        renderer.upload_scene(sc)
        renderer.set_target(W, H)
        renderer.render(ipv, iv, first, S, 0.0, B, ior, variant)
        gpu, n = renderer.read_accum()
        if seed in IN_VIEW_SEEDS:               # the same scene without its meshes
            renderer.upload_scene(fm.build_scene(mcpt_mod, spec, with_meshes=False))
            renderer.set_target(W, H)
            renderer.render(ipv, iv, first, S, 0.0, B, ior, variant)
            bare, _ = renderer.read_accum()
    finally:
        reset(renderer)
    mv = oracle_mod.MeshView(sc.mesh_buffers(), flat_face=flat)
    ref, _ = oracle_mod.render(prims, nodes, leaves, sc.depth(), ipv, iv, W, H, first, S, 0.0, B, ior, variant,
                               meshes=mv)
    assert n == S
    bad = int((bits(gpu) != bits(ref.reshape(gpu.shape))).sum())
    assert bad == 0, (f"seed {seed}: {bad} channels differ (families {spec['families']} placements "
                      f"{[p[0] for p in spec['placements']]} W {W} H {H} first {first} S {S} B {B} ior {ior} "
                      f"variant {variant} traversal {traversal} walk_exit {walk_exit} leaf_batch {leaf_batch} "
                      f"flat_face {flat})")
    if bare is not None:
        moved = int((bits(gpu) != bits(bare)).any(axis=-1).sum())
        print(f"seed {seed}: {moved} of {W * H} pixels differ from the scene without its meshes")
        assert moved > 0, f"seed {seed}: no mesh in view (families {spec['families']})"


@pytest.mark.parametrize("seed", range(100, 116))
def test_random_mesh_scene_queries(mcpt_mod, oracle_mod, renderer, seed):
    rng = np.random.default_rng(4000 + seed)
    sc, spec = fm.random_mesh_scene(mcpt_mod, seed)
    renderer.upload_scene(sc)
    o = rng.uniform(-200, 200, (1000, 3)).astype(np.float32)
    d = (rng.uniform(-60, 60, (1000, 3)) - o).astype(np.float32)
    ao, ad, _ = fm.aimed_rays(rng, spec, 1000)
    hits = compare_queries(mcpt_mod, oracle_mod, renderer, sc, np.concatenate([o, ao]), np.concatenate([d, ad]))
    n_mesh = int((hits["shape"] == 0).sum())
    assert n_mesh > 200, f"seed {seed}: {n_mesh} mesh hits (families {spec['families']})"


@pytest.mark.parametrize("seed", range(200, 212))
def test_random_mesh_event_counters(mcpt_mod, oracle_mod, renderer, seed):
    """Every event slot equal: a cull decision that differs without changing the image shows
    here (seeds 204 and 210 hold far meshes: flat boxes, flag-0 pair records)."""
    sc, spec = fm.random_mesh_scene(mcpt_mod, seed)
    prims, nodes, leaves = sc.buffers()
    W, H, S, B = 24, 16, 2, 6
    renderer.upload_scene(sc)
    renderer.set_target(W, H)
    ipv, iv = mcpt_mod.camera_canonical(W, H)
    ev = renderer.render_counted(ipv, iv, 1, S, 0.0, B, 1.0, 0)
    mv = oracle_mod.MeshView(sc.mesh_buffers())
    _, ref_ev = oracle_mod.render(prims, nodes, leaves, sc.depth(), ipv, iv, W, H, 1, S, 0.0, B, 1.0, 0, meshes=mv)
    assert np.array_equal(ev, ref_ev), (seed, spec["families"], ev, ref_ev)
    assert ev[9] > 0 and ev[10] > 0, (seed, spec["families"], ev)      # triangle tests, mesh hit infos


def tiny_spec(mcpt_mod, reverse):
    """One fixed scene whose only meshes are a one-triangle and a two-triangle soup, two
    placements each, over a ground slab under a light."""
    T, M = mcpt_mod.Transfo, mcpt_mod.material
    ms = [fm.random_mesh(1, "soup", 1), fm.random_mesh(2, "soup", 2)]
    one, two = (1, 0) if reverse else (0, 1)
    if reverse:
        ms.reverse()
    placements = [(one, T.mul(T.translate(-40, 10, 0), T.rotateZ(20), T.scale(40)), M([0.9, 0.2, 0.2, 1], 0.3, 0.8)),
                  (two, T.mul(T.translate(30, -20, 5), T.rotateX(35), T.scale(45, 30, 50)), M([0.2, 0.9, 0.2, 1], 0.6, 0.5)),
                  (one, T.mul(T.translate(10, 50, -10), T.rotateY(60), T.scale(25, -35, 30)), M([0.2, 0.2, 0.9, 0.5], 0.5, 0.9)),
                  (two, T.mul(T.translate(-20, -50, 20), T.rotateZ(110), T.rotateX(70), T.scale(-50, 40, 35)),
                   M([0.9, 0.9, 0.2, 0.6], 0.8, 0.95))]
    ops = [(2, T.mul(T.translate(0, 0, -60), T.scale(400, 400, 2)), M([0.8, 0.8, 0.8, 1], 0.2, 0.9))]
    light = (5, T.mul(T.translate(0, 0, 160), T.rotateX(180), T.scale(70, 70, 1)), mcpt_mod.light([0.9, 0.9, 0.9, 1], 24))
    return {"families": ["soup", "soup"], "meshes": ms, "placements": placements, "ops": ops, "light": light}, two


@pytest.mark.parametrize("reverse", [False, True])
def test_tiny_meshes_only(mcpt_mod, oracle_mod, renderer, reverse):
    """Mesh BVH depth 0 (the root is the only leaf and keeps id -1: the mesh can never be hit,
    as in the reference) and depth 1 (the walk's child prefetch goes straight to leaf records),
    in both upload orders, under all three traversals."""
    spec, two = tiny_spec(mcpt_mod, reverse)
    sc = fm.build_scene(mcpt_mod, spec)
    prims, nodes, leaves = sc.buffers()
    mb = sc.mesh_buffers()
    assert sorted(mb["info"][:, 2].tolist()) == [0, 1] and mb["info"][two, 2] == 1
    W, H, S, B = 32, 24, 2, 6
    ipv, iv = mcpt_mod.camera_canonical(W, H)
    ref, _ = oracle_mod.render(prims, nodes, leaves, sc.depth(), ipv, iv, W, H, 1, S, 0.0, B, 1.3, 0,
                               meshes=oracle_mod.MeshView(mb))
    o, d, _ = fm.aimed_rays(np.random.default_rng(5), spec, 500)
    try:
        for traversal in (1, 2, 3):
            renderer.set_traversal(traversal)
            renderer.upload_scene(sc)
            renderer.set_target(W, H)
            renderer.render(ipv, iv, 1, S, 0.0, B, 1.3, 0)
            gpu, n = renderer.read_accum()
            assert n == S and np.array_equal(bits(gpu), bits(ref)), traversal
            hits = compare_queries(mcpt_mod, oracle_mod, renderer, sc, o, d)
            mesh_of = prims[hits["prim"][hits["shape"] == 0], 49]
            assert len(mesh_of) > 50 and (mesh_of == float(two)).all(), (traversal, mesh_of)
    finally:
        reset(renderer)
