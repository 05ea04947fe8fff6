"""Rebuilding a mesh's BVH on the GPU: new vertices into an uploaded scene's meshes,
then the device rebuild — a new leaf order by segmented stable radix sorts, and the refit.  The
reference of every check is a second context loaded through the host path (Scene.update_mesh +
Scene.rebuild_mesh, then upload_scene) — its records bit for bit — and the oracle over the same
buffers: renders, ray queries and event counters."""
import numpy as np
import pytest

from mcpt import meshes
from test_gpu_mesh_refit import NAMES, bits, same_records
from test_mesh_rebuild_host import copies_mesh, grid_mesh
from test_meshes import MESHES, mesh_scene

pytestmark = pytest.mark.gpu

F = np.float32


def twist(name, phase=0.0):
    """Mesh `name` twisted about z by more than a turn over its height and drawn in by 0.7 in x and y
    (a square box about the axis holds every turned vertex: 0.7 * sqrt(2) < 1): uploaded neighbours
    separate, so the rebuilt order differs from the uploaded one."""
    v, n = MESHES[name][0].astype(np.float64), MESHES[name][1].astype(np.float64)
    a = 4.0 * v[:, 2] / max(1e-9, np.abs(v[:, 2]).max()) + phase + 2.0 * np.sin(3 * v[:, 0])
    c, s = np.cos(a), np.sin(a)
    rot = lambda p: np.stack([0.7 * (c * p[:, 0] - s * p[:, 1]), 0.7 * (s * p[:, 0] + c * p[:, 1]), p[:, 2]], 1)
    return rot(v).astype(F), rot(n).astype(F)


TWISTED = {name: twist(name, 0.4 * k) for k, name in enumerate(NAMES)}


def rebuilt_scene(mcpt_mod, rebuild=True):
    sc = mesh_scene(mcpt_mod)
    for k, name in enumerate(NAMES):
        sc.update_mesh(k, *TWISTED[name])
        if rebuild:
            sc.rebuild_mesh(k)
    return sc


def push_vertices(r, sc, which=NAMES):
    for k, name in enumerate(NAMES):
        if name in which:
            r.update_mesh_vertices(sc.mesh_vertex_range(k)[0], *TWISTED[name])


@pytest.fixture(scope="module")
def pair(mcpt_mod):
    """(A, B, the rebuilt scene): A uploaded undeformed, then updated and rebuilt on the device;
    B uploaded from the host's update + rebuild."""
    A, B = mcpt_mod.Renderer(0), mcpt_mod.Renderer(0)
    sc0, sc1 = mesh_scene(mcpt_mod), rebuilt_scene(mcpt_mod)
    A.upload_scene(sc0)
    push_vertices(A, sc0)
    rec = A.rebuild_mesh(-1)
    B.upload_scene(sc1)
    yield A, B, sc1, rec
    A.close()
    B.close()


def test_records_all_meshes(mcpt_mod, pair):
    A, B, sc1, rec = pair
    mb = sc1.mesh_buffers()
    rb = B.mesh_records()
    assert same_records(A.mesh_records(), rb)
    refit = mcpt_mod.Renderer(0)                          # (the rebuild moves the leaves: a refit alone differs)
    refit.upload_scene(rebuilt_scene(mcpt_mod, rebuild=False))
    assert not same_records(refit.mesh_records(), rb)
    refit.close()
    depths = [int(d) for d in mb["info"][:, 2]]
    assert rec["triangles"] == sum(len(MESHES[k][2]) for k in NAMES) and rec["rounds"] == sum(d - 1 for d in depths)
    assert rec["sort_passes"] == sum((32 + r - 1 + 7) // 8 for d in depths for r in range(1, d))
    assert rec["root_box"] is None and rec["sort_ms"] >= 0.0 and rec["refit_ms"] >= 0.0


def test_records_mesh_by_mesh(mcpt_mod, pair):
    _, B, sc1, _ = pair
    mb = sc1.mesh_buffers()
    want = B.mesh_records()
    r = mcpt_mod.Renderer(0)
    sc0 = mesh_scene(mcpt_mod)
    r.upload_scene(sc0)
    push_vertices(r, sc0)
    for k, name in enumerate(NAMES):
        rec = r.rebuild_mesh(k)
        root = mb["nodes"][int(mb["info"][k, 0])]
        assert np.array_equal(bits(rec["root_box"]), bits(root)), name
        assert rec["triangles"] == len(MESHES[name][2]) and rec["rounds"] == int(mb["info"][k, 2]) - 1
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


def one_mesh_scene(mcpt_mod, v, n, t, bb, v2=None, n2=None, tris=None, rebuild=False):
    T, M = mcpt_mod.Transfo, mcpt_mod.material
    s = mcpt_mod.Scene()
    mid = s.add_mesh(v, n, t, bb)
    s.place_mesh(mid, T.scale(40), M([0.8, 0.8, 0.8, 1]))
    s.add_sphere(T.mul(T.translate(0, 0, 90), T.scale(10)), mcpt_mod.light([1, 1, 1, 1], 10))
    s.finalize()
    if v2 is not None:
        s.update_mesh(mid, v2, n2)
    if rebuild:
        s.rebuild_mesh(mid, tris)
    return s


def sized_mesh(case):
    if case == "grid":
        return grid_mesh(40, 33)          # 2640 triangles: ties in every round, ranges across workgroups' steps
    if case == "copies37":
        return copies_mesh(37)
    if case >= 60000:
        n_lat = {67080: 130, 140624: 188, 269360: 260}[case]
        return meshes.uv_sphere(2 * n_lat, n_lat)
    return strip(case, case)


# 1, 2, 3: no round, none, one; 257 and 300: ranges straddle a scatter step of 256 positions; 5000: two
# workgroups' tiles; 67080 (depth 17), 140624 (depth 18: 16 range bits, two range passes), 269360 (depth
# 19: a third range pass); the grid's and the copies' ties test stability
@pytest.mark.parametrize("case", [1, 2, 3, 5, 257, 300, 5000, 67080, 140624, 269360, "grid", "copies37"])
def test_sizes(mcpt_mod, case):
    v, n, t, bb = sized_mesh(case)
    n_tris = len(t)
    if case == "copies37":
        v2, n2 = v, n
    else:                                 # a swirl about z, drawn in: neighbours in the uploaded order part
        a = 5.0 * v[:, 2].astype(np.float64) + 3.0 * np.sin(4.0 * v[:, 0].astype(np.float64))
        c, s = np.cos(a), np.sin(a)
        v2 = np.stack([0.7 * (c * v[:, 0] - s * v[:, 1]), 0.7 * (s * v[:, 0] + c * v[:, 1]), v[:, 2]], 1).astype(F)
        n2 = n[::-1].copy()
    A, B = mcpt_mod.Renderer(0), mcpt_mod.Renderer(0)
    A.upload_scene(one_mesh_scene(mcpt_mod, v, n, t, bb))
    sc1 = one_mesh_scene(mcpt_mod, v, n, t, bb, v2, n2, rebuild=True)
    B.upload_scene(sc1)
    mb = sc1.mesh_buffers()
    d = int(mb["info"][0, 2])
    A.update_mesh_vertices(0, v2, n2)
    rec = A.rebuild_mesh(0)
    ra, rb = A.mesh_records(), B.mesh_records()
    ids = lambda r: r["leaves"][:, 0, 3].view(np.int32)
    assert np.array_equal(ids(ra), ids(rb)), int((ids(ra) != ids(rb)).sum())
    assert same_records(ra, rb)
    if case == "copies37":
        assert np.array_equal(ids(ra)[ids(ra) >= 0], np.arange(37))
    if d == 0:
        assert rec["root_box"] is None and rec["triangles"] == 0 and rec["rounds"] == 0
    else:
        assert np.array_equal(bits(rec["root_box"]), bits(mb["nodes"][0]))
        assert rec["rounds"] == d - 1 and rec["triangles"] == (n_tris if d >= 2 else 0)
    rng = np.random.default_rng(3)
    o = rng.uniform(-90, 90, (500, 3)).astype(F)
    dirs = (rng.uniform(-30, 30, (500, 3)) - o).astype(F)
    assert A.trace(o, dirs).tobytes() == B.trace(o, dirs).tobytes()
    A.close()
    B.close()


def test_new_triangles(mcpt_mod):
    """tris= replacing a mesh's triangles by a permutation of them, then by another triangulation of
    the same vertices (the grid's cells cut along the other diagonal), the second of two meshes."""
    T, M = mcpt_mod.Transfo, mcpt_mod.material
    v0, n0, t0, bb0 = meshes.uv_sphere(20, 10)            # (its vertex 0 is in no triangle)
    v, n, t, bb = grid_mesh(12, 9)
    rng = np.random.default_rng(6)
    perm = t[rng.permutation(len(t))][:, [2, 0, 1]]
    q = t.reshape(-1, 2, 3)                               # cell (a, b, c) (a, c, d) -> (a, b, d) (b, c, d)
    a, b, c, d = q[:, 0, 0], q[:, 0, 1], q[:, 0, 2], q[:, 1, 2]
    other = np.stack([np.stack([a, b, d], 1), np.stack([b, c, d], 1)], 1).reshape(-1, 3).astype(np.uint32)

    def scene(tris):
        s = mcpt_mod.Scene()
        m0, m1 = s.add_mesh(v0, n0, t0, bb0), s.add_mesh(v, n, t, bb)
        s.place_mesh(m0, T.mul(T.translate(50, 0, 0), T.scale(30)), M([0.8, 0.8, 0.8, 1]))
        s.place_mesh(m1, T.scale(40), M([0.8, 0.2, 0.2, 1]))
        s.add_sphere(T.mul(T.translate(0, 0, 90), T.scale(10)), mcpt_mod.light([1, 1, 1, 1], 10))
        s.finalize()
        if tris is not None:
            s.rebuild_mesh(m1, tris)
        return s

    A = mcpt_mod.Renderer(0)
    A.upload_scene(scene(None))
    rng = np.random.default_rng(7)
    o = rng.uniform(-90, 90, (1000, 3)).astype(F)
    dirs = (rng.uniform(-20, 20, (1000, 3)) - o).astype(F)
    for tris in (perm, other):
        B = mcpt_mod.Renderer(0)
        B.upload_scene(scene(tris))
        A.rebuild_mesh(1, tris, record=False)
        assert same_records(A.mesh_records(), B.mesh_records())
        ha, hb = A.trace(o, dirs), B.trace(o, dirs)       # (the triangle rows arrived too)
        assert ha.tobytes() == hb.tobytes() and (ha["shape"] == 0).sum() > 100
        B.close()
    A.close()


W, H, S, BOUNCES = 64, 64, 4, 8
_oracle_cache = {}


def oracle_render(oracle_mod, mcpt_mod, sc, flat):
    if flat not in _oracle_cache:
        prims, nodes, leaves = sc.buffers()
        ipv, iv = mcpt_mod.camera_canonical(W, H)
        mv = oracle_mod.MeshView(sc.mesh_buffers(), flat_face=flat)
        _oracle_cache[flat] = oracle_mod.render(prims, nodes, leaves, sc.depth(), ipv, iv, W, H, 1, S, 0.0, BOUNCES, 1.2,
                                                0, meshes=mv)[0]
    return _oracle_cache[flat]


@pytest.mark.parametrize("flat", [False, True])
@pytest.mark.parametrize("traversal", [1, 2, 3])
def test_render_after_rebuild(mcpt_mod, oracle_mod, pair, traversal, flat):
    A, B, sc1, _ = pair
    ipv, iv = mcpt_mod.camera_canonical(W, H)
    got = []
    for r in (A, B):
        r.set_traversal(traversal)
        r.set_flat_face(flat)
        r.set_target(W, H)
        r.render(ipv, iv, 1, S, 0.0, BOUNCES, 1.2, 0)
        acc, n = r.read_accum()
        r.set_traversal(0)
        r.set_flat_face(False)
        assert n == S and np.isfinite(acc).all()
        got.append(acc)
    ref = oracle_render(oracle_mod, mcpt_mod, sc1, flat)
    assert np.array_equal(bits(got[0]), bits(ref))
    assert np.array_equal(bits(got[0]), bits(got[1]))


def test_queries_after_rebuild(mcpt_mod, oracle_mod, pair):
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
    assert (hits["shape"] == 0).sum() > 100          # mesh hits


def test_event_counters_after_rebuild(mcpt_mod, oracle_mod, pair):
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


def test_ordering_between_queued_renders(mcpt_mod):
    """Passes 1-16 on the old meshes, update + rebuild, passes 17-32 on the new ones, queued without a
    host wait in between (render lanes on): the accumulator is the sum of a fresh context's 1-16 on
    the old meshes and another's 17-32 on the host-rebuilt ones."""
    w, h, b = 32, 24, 8
    ipv, iv = mcpt_mod.camera_canonical(w, h)
    sc0, sc1 = mesh_scene(mcpt_mod), rebuilt_scene(mcpt_mod)

    def fresh(sc, first):
        r = mcpt_mod.Renderer(0)
        r.set_traversal(1)
        r.upload_scene(sc)
        r.set_target(w, h)
        r.render(ipv, iv, first, 16, 0.0, b, 1.2, 0)
        acc, _ = r.read_accum()
        r.close()
        return acc

    want = fresh(sc0, 1) + fresh(sc1, 17)
    A = mcpt_mod.Renderer(0)
    A.set_render_lanes(True)
    A.set_traversal(1)
    A.upload_scene(sc0)
    A.set_target(w, h)
    A.render(ipv, iv, 1, 16, 0.0, b, 1.2, 0)
    push_vertices(A, sc0)
    A.rebuild_mesh(-1, record=False)
    A.render(ipv, iv, 17, 16, 0.0, b, 1.2, 0)
    acc, n = A.read_accum()
    A.close()
    assert n == 32
    assert np.array_equal(bits(acc), bits(want))


def test_state_after_rebuild(mcpt_mod):
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
    acc0, _ = r.read_accum()
    push_vertices(r, sc0, ("torus",))
    r.rebuild_mesh(2)
    assert L.mcpt_denoise(r._h, 1, 1.0, 1.0) == mcpt_mod.NO_GUIDES
    info = r.temporal_info()
    assert info["on"] and info["frames"] == 0 and not info["history_valid"]
    assert r.schedule() == sched and r.pass_count() == passes and r.stats_info()["passes"] == 8
    acc1, n1 = r.read_accum()
    assert n1 == passes and np.array_equal(bits(acc0), bits(acc1))
    r.close()


def test_refusals_leave_the_records(mcpt_mod):
    L = mcpt_mod.lib()
    ip = lambda a: a.ctypes.data_as(mcpt_mod._c_int_p)
    BAD_SCENE, INVALID = -6, -1
    w, h = 32, 24
    ipv, iv = mcpt_mod.camera_canonical(w, h)
    sc0 = mesh_scene(mcpt_mod)
    mb = sc0.mesh_buffers()
    t_torus = np.ascontiguousarray(MESHES["torus"][2].astype(np.int32))
    nv_torus = len(MESHES["torus"][0])
    r = mcpt_mod.Renderer(0)
    r.upload_scene(mcpt_mod.Scene.reference(6))                       # no meshes uploaded
    assert L.mcpt_rebuild_mesh(r._h, -1, None, 0, None) == BAD_SCENE
    r.upload_scene(sc0)
    r.set_traversal(1)
    r.set_target(w, h)
    r.render(ipv, iv, 1, 2, 0.0, 4, 1.2, 0)
    want, _ = r.read_accum()
    r.clear_accum()
    before = r.mesh_records()
    rng = np.random.default_rng(5)
    o = rng.uniform(-200, 200, (500, 3)).astype(F)
    d = (rng.uniform(-80, 80, (500, 3)) - o).astype(F)
    tr0 = r.trace(o, d).tobytes()
    assert L.mcpt_rebuild_mesh(r._h, 3, None, 0, None) == INVALID and L.mcpt_rebuild_mesh(r._h, -2, None, 0, None) == INVALID
    assert L.mcpt_rebuild_mesh(r._h, -1, ip(t_torus), len(t_torus), None) == INVALID      # new triangles: one mesh
    assert L.mcpt_rebuild_mesh(r._h, 2, ip(t_torus), len(t_torus) - 1, None) == INVALID   # a wrong count
    bad = t_torus.copy()
    bad[7, 2] = nv_torus                                                                   # outside the mesh's vertices
    assert L.mcpt_rebuild_mesh(r._h, 2, ip(bad), len(bad), None) == INVALID
    bad[7, 2] = -1
    assert L.mcpt_rebuild_mesh(r._h, 2, ip(bad), len(bad), None) == INVALID
    with pytest.raises(mcpt_mod.MCPTError):
        r.rebuild_mesh(2, bad)
    assert same_records(r.mesh_records(), before) and r.trace(o, d).tobytes() == tr0
    r.render(ipv, iv, 1, 2, 0.0, 4, 1.2, 0)
    got, _ = r.read_accum()
    assert np.array_equal(bits(got), bits(want))
    # hand-made buffers: the torus' last leaf pair emptied; and no vertex counts given after a bare upload
    hand = {k: a.copy() for k, a in mb.items()}
    lo, dd = int(mb["info"][2, 1]), int(mb["info"][2, 2])
    hand["leaves"][lo + (1 << dd) - 2:lo + (1 << dd)] = -1
    r.upload_meshes(hand)
    before = r.mesh_records()
    assert L.mcpt_rebuild_mesh(r._h, 2, None, 0, None) == BAD_SCENE and L.mcpt_rebuild_mesh(r._h, -1, None, 0, None) == BAD_SCENE
    t_cube = np.ascontiguousarray(MESHES["cube"][2].astype(np.int32))
    assert L.mcpt_rebuild_mesh(r._h, 0, ip(t_cube), len(t_cube), None) == BAD_SCENE
    assert same_records(r.mesh_records(), before)
    r.close()
