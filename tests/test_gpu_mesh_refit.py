"""Deforming meshes on the GPU: new vertices into an uploaded scene's meshes and
the device refit of their BVH records.  The reference of every check is a second context loaded
through the existing path (Scene.update_mesh, then upload_scene) — its records bit for bit — and the
oracle over the same buffers: renders, ray queries and event counters."""
import numpy as np
import pytest

from mcpt import meshes
from test_meshes import MESHES, mesh_scene

pytestmark = pytest.mark.gpu

F = np.float32
NAMES = ("cube", "sphere", "torus")   # the mesh ids of mesh_scene, in add order


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def deform(name, phase=0.0):
    """Mesh `name` pulled towards its centre by a smooth factor in [0.8, 1] (the boxes of MESHES are
    convex around the origin, so every vertex stays inside) and its normals turned."""
    v, n = MESHES[name][0].astype(np.float64), MESHES[name][1].astype(np.float64)
    f = 0.9 + 0.1 * np.sin(3 * v[:, 0] + phase) * np.cos(2 * v[:, 1] - v[:, 2])
    n2 = n + 0.15 * np.stack([np.sin(2 * v[:, 1]), np.cos(3 * v[:, 2] + phase), np.sin(v[:, 0])], 1)
    return (v * f[:, None]).astype(F), n2.astype(F)


DEFORMED = {name: deform(name, 0.4 * k) for k, name in enumerate(NAMES)}


def deformed_scene(mcpt_mod):
    sc = mesh_scene(mcpt_mod)
    for k, name in enumerate(NAMES):
        sc.update_mesh(k, *DEFORMED[name])
    return sc


def push_vertices(r, sc, which=NAMES):
    for k, name in enumerate(NAMES):
        if name in which:
            r.update_mesh_vertices(sc.mesh_vertex_range(k)[0], *DEFORMED[name])


def same_records(a, b):
    return np.array_equal(bits(a["pairs"]), bits(b["pairs"])) and np.array_equal(bits(a["leaves"]), bits(b["leaves"]))


@pytest.fixture(scope="module")
def pair(mcpt_mod):
    """(A, B, the deformed scene): A uploaded undeformed, then updated and refitted on the device;
    B uploaded from the host's update."""
    A, B = mcpt_mod.Renderer(0), mcpt_mod.Renderer(0)
    sc0, sc1 = mesh_scene(mcpt_mod), deformed_scene(mcpt_mod)
    A.upload_scene(sc0)
    push_vertices(A, sc0)
    rec = A.refit_mesh(-1)
    B.upload_scene(sc1)
    yield A, B, sc1, rec
    A.close()
    B.close()


def test_records_all_meshes(mcpt_mod, pair):
    A, B, sc1, rec = pair
    mb = sc1.mesh_buffers()
    ra, rb = A.mesh_records(), B.mesh_records()
    assert same_records(ra, rb)
    fresh = mcpt_mod.Renderer(0)
    fresh.upload_scene(mesh_scene(mcpt_mod))
    assert not same_records(fresh.mesh_records(), rb)   # (the deformation moves the records)
    fresh.close()
    n_leaves = sum(1 << int(d) for d in mb["info"][:, 2])
    assert rec["leaves"] == n_leaves and rec["internal_nodes"] == n_leaves - len(NAMES)
    assert rec["triangles"] == sum(len(MESHES[k][2]) for k in NAMES)
    assert rec["root_box"] is None and rec["device_ms"] >= 0.0


def test_records_mesh_by_mesh(mcpt_mod, pair):
    _, B, sc1, _ = pair
    mb = sc1.mesh_buffers()
    want = B.mesh_records()
    r = mcpt_mod.Renderer(0)
    sc0 = mesh_scene(mcpt_mod)
    r.upload_scene(sc0)
    before = r.mesh_records()
    push_vertices(r, sc0)
    assert same_records(r.mesh_records(), before)       # (new vertices alone leave the records)
    for k, name in enumerate(NAMES):
        rec = r.refit_mesh(k)
        root = mb["nodes"][int(mb["info"][k, 0])]
        assert np.array_equal(bits(rec["root_box"]), bits(root)), name
        assert rec["triangles"] == len(MESHES[name][2]) and rec["leaves"] == 1 << int(mb["info"][k, 2])
        got = r.mesh_records()
        lo, nl = int(mb["info"][k, 1]), 1 << int(mb["info"][k, 2])
        assert np.array_equal(bits(got["leaves"][lo:lo + nl]), bits(want["leaves"][lo:lo + nl])), name
        assert same_records(got, want) == (k == len(NAMES) - 1)
    r.close()


def strip(n_tris, seed):
    rng = np.random.default_rng(seed)
    v = rng.uniform(-1, 1, (n_tris + 2, 3)).astype(F)
    n = rng.normal(size=(n_tris + 2, 3)).astype(F)
    t = np.stack([np.arange(n_tris), np.arange(n_tris) + 1, np.arange(n_tris) + 2], 1).astype(np.uint32)
    return v, n, t, np.array([-1, -1, -1, 1, 1, 1], F)


# k = 8: one leaf pair's worth and less (depth 0, 1, 2), one triangle past a stage-one workgroup
# (depth 9: a short second stage), and depth 17 (8 + 8 + 1 levels: a third stage runs)
@pytest.mark.parametrize("n_tris", [1, 2, 3, 257, 67080])
def test_stages(mcpt_mod, n_tris):
    v, n, t, bb = meshes.uv_sphere(260, 130) if n_tris == 67080 else strip(n_tris, n_tris)
    assert len(t) == n_tris
    f = 0.9 + 0.1 * np.sin(5 * v[:, 0].astype(np.float64)) * np.cos(4 * v[:, 1].astype(np.float64))
    v2, n2 = (v * f[:, None]).astype(F), n[::-1].copy()
    T, M = mcpt_mod.Transfo, mcpt_mod.material

    def scene(vv, nn):
        s = mcpt_mod.Scene()
        mid = s.add_mesh(v, n, t, bb)
        s.place_mesh(mid, T.scale(40), M([0.8, 0.8, 0.8, 1]))
        s.add_sphere(T.mul(T.translate(0, 0, 90), T.scale(10)), mcpt_mod.light([1, 1, 1, 1], 10))
        s.finalize()
        if vv is not None:
            s.update_mesh(mid, vv, nn)
        return s

    A, B = mcpt_mod.Renderer(0), mcpt_mod.Renderer(0)
    A.upload_scene(scene(None, None))
    sc1 = scene(v2, n2)
    B.upload_scene(sc1)
    mb = sc1.mesh_buffers()
    d = int(mb["info"][0, 2])
    assert d == {1: 0, 2: 1, 3: 2, 257: 9, 67080: 17}[n_tris]
    A.update_mesh_vertices(0, v2, n2)
    rec = A.refit_mesh(0)
    assert same_records(A.mesh_records(), B.mesh_records())
    if d == 0:
        assert rec["root_box"] is None and rec["leaves"] == 0 and rec["triangles"] == 0
    else:
        assert np.array_equal(bits(rec["root_box"]), bits(mb["nodes"][0]))
        assert rec["triangles"] == n_tris and rec["leaves"] == 1 << d and rec["internal_nodes"] == (1 << d) - 1
    # the vertices and normals arrived too: a smooth-normal query through both contexts
    rng = np.random.default_rng(3)
    o = rng.uniform(-90, 90, (500, 3)).astype(F)
    dirs = (rng.uniform(-30, 30, (500, 3)) - o).astype(F)
    ha, hb = A.trace(o, dirs), B.trace(o, dirs)
    assert ha.tobytes() == hb.tobytes()
    A.close()
    B.close()


W, H, S, BOUNCES = 64, 48, 3, 8
_oracle_cache = {}


def oracle_render(oracle_mod, mcpt_mod, sc, flat, variant):
    key = (flat, variant)
    if key not in _oracle_cache:
        prims, nodes, leaves = sc.buffers()
        ipv, iv = mcpt_mod.camera_canonical(W, H)
        mv = oracle_mod.MeshView(sc.mesh_buffers(), flat_face=flat)
        _oracle_cache[key] = oracle_mod.render(prims, nodes, leaves, sc.depth(), ipv, iv, W, H, 1, S, 0.0, BOUNCES, 1.2,
                                               variant, meshes=mv)[0]
    return _oracle_cache[key]


@pytest.mark.parametrize("flat", [False, True])
@pytest.mark.parametrize("variant", [0, 1, 2])
@pytest.mark.parametrize("traversal", [1, 2, 3])
def test_render_after_refit(mcpt_mod, oracle_mod, pair, traversal, variant, flat):
    A, B, sc1, _ = pair
    ipv, iv = mcpt_mod.camera_canonical(W, H)
    got = []
    for r in (A, B):
        r.set_traversal(traversal)
        r.set_flat_face(flat)
        r.set_target(W, H)
        r.render(ipv, iv, 1, S, 0.0, BOUNCES, 1.2, variant)
        acc, n = r.read_accum()
        r.set_traversal(0)
        r.set_flat_face(False)
        assert n == S and np.isfinite(acc).all()
        got.append(acc)
    ref = oracle_render(oracle_mod, mcpt_mod, sc1, flat, variant)
    assert np.array_equal(bits(got[0]), bits(ref))
    assert np.array_equal(bits(got[0]), bits(got[1]))


def test_queries_after_refit(mcpt_mod, oracle_mod, pair):
    A, _, sc1, _ = pair
    prims, nodes, leaves = sc1.buffers()
    mv = oracle_mod.MeshView(sc1.mesh_buffers())
    rng = np.random.default_rng(9)
    o = rng.uniform(-200, 200, (4000, 3)).astype(F)
    d = (rng.uniform(-80, 80, (4000, 3)) - o).astype(F)
    for any_hit in (False, True):
        hits = A.trace(o, d, any_hit=any_hit)
        oi, of = oracle_mod.trace(prims, nodes, leaves, sc1.depth(), o, d, any_hit=any_hit, meshes=mv)
        assert np.array_equal(hits["shape"], oi[:, 0])
        hit = oi[:, 0] >= 0
        assert np.array_equal(hits["prim"][hit], oi[hit, 1]) and np.array_equal(hits["dir"][hit], oi[hit, 2])
        flat = np.concatenate([hits["dist"][:, None], hits["pl"], hits["pg"], hits["N"], hits["P"], hits["color"],
                               hits["material"]], axis=1)
        assert np.array_equal(bits(flat), bits(of))
    assert (hits["shape"] == 0).sum() > 200          # mesh hits


def test_event_counters_after_refit(mcpt_mod, oracle_mod, pair):
    A, _, sc1, _ = pair
    prims, nodes, leaves = sc1.buffers()
    w, h, s = 40, 30, 2
    A.set_target(w, h)
    ipv, iv = mcpt_mod.camera_canonical(w, h)
    ev = A.render_counted(ipv, iv, 1, s, 0.0, 8, 1.0, 0)
    mv = oracle_mod.MeshView(sc1.mesh_buffers())
    _, ref_ev = oracle_mod.render(prims, nodes, leaves, sc1.depth(), ipv, iv, w, h, 1, s, 0.0, 8, 1.0, 0, meshes=mv)
    assert np.array_equal(ev, ref_ev), (ev, ref_ev)
    assert ev[9] > 0 and ev[10] > 0                   # triangle tests, mesh hit infos


@pytest.mark.parametrize("traversal", [1, 0])
def test_ordering_between_queued_renders(mcpt_mod, oracle_mod, traversal):
    """Passes 1-32 on the old meshes, update + refit, passes 33-64 on the new ones, queued without a
    host wait in between (render lanes on; a fixed traversal, or AUTO settled by earlier calls): the
    accumulator is the sum of a fresh context's 1-32 on the old meshes and another's 33-64 on the new."""
    w, h, b = 32, 24, 8
    ipv, iv = mcpt_mod.camera_canonical(w, h)
    sc0, sc1 = mesh_scene(mcpt_mod), deformed_scene(mcpt_mod)

    def fresh(sc, first):
        r = mcpt_mod.Renderer(0)
        r.set_traversal(1)
        r.upload_scene(sc)
        r.set_target(w, h)
        r.render(ipv, iv, first, 32, 0.0, b, 1.2, 0)
        acc, _ = r.read_accum()
        r.close()
        return acc

    want = fresh(sc0, 1) + fresh(sc1, 33)
    A = mcpt_mod.Renderer(0)
    A.set_render_lanes(True)
    A.set_traversal(traversal)
    A.upload_scene(sc0)
    A.set_target(w, h)
    if traversal == 0:      # let AUTO settle on throw-away passes of the same shape, then start over
        for k in range(12):
            A.render(ipv, iv, 1 + 32 * k, 32, 0.0, b, 1.2, 0)
        A.clear_accum()
    A.render(ipv, iv, 1, 32, 0.0, b, 1.2, 0)
    push_vertices(A, sc0)
    A.refit_mesh(-1, record=False)
    A.render(ipv, iv, 33, 32, 0.0, b, 1.2, 0)
    acc, n = A.read_accum()
    A.close()
    assert n == 64
    assert np.array_equal(bits(acc), bits(want))
    orc = []
    for sc, first in ((sc0, 1), (sc1, 33)):
        prims, nodes, leaves = sc.buffers()
        mv = oracle_mod.MeshView(sc.mesh_buffers())
        orc.append(oracle_mod.render(prims, nodes, leaves, sc.depth(), ipv, iv, w, h, first, 32, 0.0, b, 1.2, 0, meshes=mv)[0])
    assert np.array_equal(bits(acc), bits(orc[0] + orc[1]))


def test_state_after_refit(mcpt_mod):
    L = mcpt_mod.lib()
    w, h = 32, 24
    ipv, iv = mcpt_mod.camera_canonical(w, h)
    sc0 = mesh_scene(mcpt_mod)
    r = mcpt_mod.Renderer(0)
    r.upload_scene(sc0)
    r.set_target(w, h)
    r.stats_begin()
    r.temporal_begin()
    for k in range(2):
        r.render(ipv, iv, 1 + 4 * k, 4, 0.0, 4, 1.2, 0)
    r.render_guides(ipv, iv)
    r.convergence(0.05)
    r.temporal_accumulate(None)
    assert r.temporal_info()["frames"] == 1
    assert L.mcpt_denoise(r._h, 1, 1.0, 1.0) == 0
    sched, passes = r.schedule(), r.pass_count()
    push_vertices(r, sc0, ("torus",))
    r.refit_mesh(2)
    assert L.mcpt_denoise(r._h, 1, 1.0, 1.0) == mcpt_mod.NO_GUIDES
    info = r.temporal_info()
    assert info["on"] and info["frames"] == 0 and not info["history_valid"]
    assert r.schedule() == sched and r.pass_count() == passes and r.stats_info()["passes"] == 8
    r.close()


def test_refusals_leave_the_records(mcpt_mod):
    L = mcpt_mod.lib()
    fp = lambda a: a.ctypes.data_as(mcpt_mod._c_float_p)
    BAD_SCENE, INVALID = -6, -1
    sc0 = mesh_scene(mcpt_mod)
    mb = sc0.mesh_buffers()
    v, n = DEFORMED["cube"]
    nv = len(mb["verts"])
    r = mcpt_mod.Renderer(0)
    r.upload_scene(mcpt_mod.Scene.reference(6))                       # no meshes uploaded
    assert L.mcpt_refit_mesh(r._h, -1, None) == BAD_SCENE
    assert L.mcpt_update_mesh_vertices(r._h, 0, len(v), fp(v), fp(n)) == BAD_SCENE
    assert L.mcpt_update_mesh_vertices_device(r._h, 0, len(v), fp(v), fp(n)) == BAD_SCENE
    r.upload_scene(sc0)
    before = r.mesh_records()
    assert L.mcpt_refit_mesh(r._h, 3, None) == INVALID and L.mcpt_refit_mesh(r._h, -2, None) == INVALID
    assert L.mcpt_update_mesh_vertices(r._h, nv - len(v) + 1, len(v), fp(v), fp(n)) == INVALID
    assert L.mcpt_update_mesh_vertices(r._h, -1, len(v), fp(v), fp(n)) == INVALID
    assert L.mcpt_update_mesh_vertices(r._h, 0, len(v), None, fp(n)) == INVALID
    assert same_records(r.mesh_records(), before)
    # hand-made buffers: the torus' last leaf pair emptied (its triangles dropped from the leaves)
    bad = {k: a.copy() for k, a in mb.items()}
    lo, d = int(mb["info"][2, 1]), int(mb["info"][2, 2])
    bad["leaves"][lo + (1 << d) - 2:lo + (1 << d)] = -1
    r.upload_meshes(bad)
    before = r.mesh_records()
    assert L.mcpt_refit_mesh(r._h, 2, None) == BAD_SCENE and L.mcpt_refit_mesh(r._h, -1, None) == BAD_SCENE
    assert L.mcpt_refit_mesh(r._h, 0, None) == 0                       # (the other meshes refit)
    assert same_records(r.mesh_records(), before)                      # (unchanged vertices: the same bits)
    r.close()


def test_device_pointer_form(mcpt_mod, pair):
    import torch
    _, B, _, _ = pair
    sc0 = mesh_scene(mcpt_mod)
    r = mcpt_mod.Renderer(0)
    r.upload_scene(sc0)
    for k, name in enumerate(NAMES):
        v, n = (torch.from_numpy(a).to("cuda:0") for a in DEFORMED[name])
        r.update_mesh_vertices(sc0.mesh_vertex_range(k)[0], v, n)
    r.refit_mesh(-1, record=False)
    assert same_records(r.mesh_records(), B.mesh_records())
    rng = np.random.default_rng(5)
    o = rng.uniform(-200, 200, (1000, 3)).astype(F)
    d = (rng.uniform(-80, 80, (1000, 3)) - o).astype(F)
    assert r.trace(o, d).tobytes() == B.trace(o, d).tobytes()
    r.close()
