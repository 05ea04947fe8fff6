"""Deforming meshes on the CPU: Scene.update_mesh, the specification of the device
refit, against a numpy restatement written here (leaf boxes -+ 0.001 in float32, the lone leaf's
sibling box, the bottom-up merge with std::min / std::max's comparisons), its refusals, and the
oracle's traversal of the refitted boxes against a brute-force loop over all triangles."""
import numpy as np
import pytest

from mcpt import meshes
from test_meshes import _np_closest_triangle

F = np.float32
ROOMY = np.array([-2, -2, -2, 2, 2, 2], F)


def bits(a):
    return np.asarray(a, F).view(np.uint32)


def strip(n_tris, seed):
    """n_tris triangles (i, i+1, i+2) over random vertices in [-1, 1]^3."""
    rng = np.random.default_rng(seed)
    v = rng.uniform(-1, 1, (n_tris + 2, 3)).astype(F)
    n = rng.normal(size=(n_tris + 2, 3)).astype(F)
    t = np.stack([np.arange(n_tris), np.arange(n_tris) + 1, np.arange(n_tris) + 2], 1).astype(np.uint32)
    return v, n, t, ROOMY


def cases():
    out = {f"strip{k}": strip(k, k) for k in (1, 2, 3, 5)}
    out["cube"] = meshes.cube()[:3] + (ROOMY,)
    out["sphere"] = meshes.uv_sphere(24, 12)[:3] + (ROOMY,)
    out["torus"] = meshes.torus()[:3] + (ROOMY,)
    return out


CASES = cases()


def deform(v, n, phase=0.0):
    """A smooth displacement of at most 0.45 per axis (inside ROOMY for |v| <= 1.35) and turned normals."""
    v = v.astype(np.float64)
    d = 0.45 * np.stack([np.sin(3 * v[:, 1] + phase), np.cos(2 * v[:, 2] - phase), np.sin(2 * v[:, 0] + 1 + phase)], 1)
    n2 = n.astype(np.float64) + 0.2 * np.stack([np.cos(v[:, 0]), np.sin(v[:, 1]), np.cos(v[:, 2] + phase)], 1)
    return (v + d).astype(F), n2.astype(F)


def np_tri_box(v, tri):
    """tri_box: std::min / std::max over {A, B, C} (the first of equals stays), then -+ 0.001f."""
    A, B, C = v[tri[0]], v[tri[1]], v[tri[2]]
    mn = np.where(B < A, B, A)
    mn = np.where(C < mn, C, mn)
    mx = np.where(A < B, B, A)
    mx = np.where(mx < C, C, mx)
    return np.concatenate([mn - F(0.001), mx + F(0.001)]).astype(F)


def np_refit(v, tris, depth, leaves):
    """The host refit restated: nodes (2^(d+1) - 1, 6) from the vertices, the triangles and the leaves."""
    nl = 1 << depth
    nodes = np.zeros((2 * nl - 1, 6), F)
    if depth == 0:
        nodes[0] = np_tri_box(v, tris[0])
        return nodes
    for k in range(nl):
        if leaves[k] >= 0:
            nodes[nl - 1 + k] = np_tri_box(v, tris[leaves[k]])
    for k in range(nl):
        if leaves[k] < 0:
            nodes[nl - 1 + k] = nodes[nl - 1 + (k ^ 1)]
    for k in range(2 * nl - 2, 1, -2):   # kd_build's merge: c1 the right child, c2 the left
        c1, c2 = nodes[k], nodes[k - 1]
        p = (k - 2) // 2
        nodes[p, :3] = np.where(c2[:3] < c1[:3], c2[:3], c1[:3])   # std::min(c1, c2)
        nodes[p, 3:] = np.where(c1[3:] < c2[3:], c2[3:], c1[3:])   # std::max(c1, c2)
    return nodes


def one_mesh_scene(mcpt_mod, v, n, t, bb):
    s = mcpt_mod.Scene()
    mid = s.add_mesh(v, n, t, bb)
    s.place_mesh(mid, np.eye(4, dtype=F), mcpt_mod.material([1, 1, 1, 1]))
    s.finalize()
    return s, mid


def same_buffers(a, b):
    return all(np.array_equal(np.ascontiguousarray(a[k]).view(np.uint32), np.ascontiguousarray(b[k]).view(np.uint32))
               for k in a)


@pytest.mark.parametrize("name", sorted(CASES))
def test_update_matches_restatement(mcpt_mod, name):
    v, n, t, bb = CASES[name]
    s, mid = one_mesh_scene(mcpt_mod, v, n, t, bb)
    before = s.mesh_buffers()
    v2, n2 = deform(v, n)
    s.update_mesh(mid, v2, n2)
    mb = s.mesh_buffers()
    d = int(mb["info"][0, 2])
    assert np.array_equal(mb["info"], before["info"]) and np.array_equal(mb["leaves"], before["leaves"])
    assert np.array_equal(mb["tris"], before["tris"])
    assert np.array_equal(bits(mb["verts"]), bits(v2)) and np.array_equal(bits(mb["normals"]), bits(n2))
    want = np_refit(v2, t.astype(np.int64), d, mb["leaves"])
    assert np.array_equal(bits(mb["nodes"]), bits(want))
    assert not np.array_equal(bits(mb["nodes"]), bits(before["nodes"]))
    assert s.mesh_vertex_range(mid) == (0, len(v))


@pytest.mark.parametrize("name", sorted(CASES))
def test_update_with_own_vertices_is_identity(mcpt_mod, name):
    v, n, t, bb = CASES[name]
    s, mid = one_mesh_scene(mcpt_mod, v, n, t, bb)
    before = s.mesh_buffers()
    s.update_mesh(mid, v, n)
    assert same_buffers(before, s.mesh_buffers())


def test_second_of_two_meshes(mcpt_mod):
    T = mcpt_mod.Transfo
    (v0, n0, t0, _), (v1, n1, t1, _) = CASES["sphere"], CASES["torus"]
    s = mcpt_mod.Scene()
    a, b = s.add_mesh(v0, n0, t0, ROOMY), s.add_mesh(v1, n1, t1, ROOMY)
    s.place_mesh(a, T.translate(-3, 0, 0), mcpt_mod.material([1, 1, 1, 1]))
    s.place_mesh(b, T.translate(3, 0, 0), mcpt_mod.material([1, 0, 0, 1]))
    s.add_sphere(T.scale(0.5), mcpt_mod.light([1, 1, 1, 1], 5))
    s.finalize()
    scene_before, before = s.buffers(), s.mesh_buffers()
    v2, n2 = deform(v1, n1, 0.7)
    s.update_mesh(b, v2, n2)
    mb = s.mesh_buffers()
    assert s.mesh_vertex_range(a) == (0, len(v0)) and s.mesh_vertex_range(b) == (len(v0), len(v1))
    assert all(np.array_equal(bits(x), bits(y)) for x, y in zip(scene_before[:2], s.buffers()[:2]))   # (still finalized)
    assert np.array_equal(scene_before[2], s.buffers()[2])
    no, lo = int(mb["info"][1, 0]), int(mb["info"][1, 1])
    assert np.array_equal(bits(mb["nodes"][:no]), bits(before["nodes"][:no]))
    assert np.array_equal(bits(mb["verts"][:len(v0)]), bits(v0)) and np.array_equal(bits(mb["normals"][:len(v0)]), bits(n0))
    assert np.array_equal(mb["leaves"], before["leaves"]) and np.array_equal(mb["tris"], before["tris"])
    want = np_refit(v2, t1.astype(np.int64), int(mb["info"][1, 2]), mb["leaves"][lo:])
    assert np.array_equal(bits(mb["nodes"][no:]), bits(want))
    assert np.array_equal(bits(mb["verts"][len(v0):]), bits(v2))


def test_refusals_change_nothing(mcpt_mod):
    v, n, t, _ = CASES["sphere"]
    s, mid = one_mesh_scene(mcpt_mod, v, n, t, meshes.uv_sphere(24, 12)[3])   # bb = [-1, 1]^3
    before = s.mesh_buffers()
    L = mcpt_mod.lib()
    fp = lambda a: a.ctypes.data_as(mcpt_mod._c_float_p)
    out = v.copy()
    out[17, 1] = F(1.5)                                   # outside the bb the mesh was added with
    assert L.mcpt_scene_update_mesh(s._h, mid, fp(out), fp(n), len(v)) == -6        # MCPT_ERR_BAD_SCENE
    nan = v.copy()
    nan[3, 0] = np.nan
    assert L.mcpt_scene_update_mesh(s._h, mid, fp(nan), fp(n), len(v)) == -6
    assert L.mcpt_scene_update_mesh(s._h, mid, fp(v), fp(n), len(v) - 1) == -1      # MCPT_ERR_INVALID_ARG
    assert L.mcpt_scene_update_mesh(s._h, mid + 1, fp(v), fp(n), len(v)) == -1
    assert L.mcpt_scene_update_mesh(s._h, mid, None, fp(n), len(v)) == -1
    with pytest.raises(mcpt_mod.MCPTError):
        s.update_mesh(mid, out, n)
    with pytest.raises(mcpt_mod.MCPTError):
        s.mesh_vertex_range(mid + 1)
    assert same_buffers(before, s.mesh_buffers())


def test_signed_zeros(mcpt_mod):
    """Coordinates of +0 and -0 in every order: the comparisons keep the first of equals, as the
    restatement's do, and the bits agree (min({+0, -0}) is +0, min({-0, +0}) is -0)."""
    v, n, t, bb = strip(5, 11)
    s, mid = one_mesh_scene(mcpt_mod, v, n, t, bb)
    z = np.array([0.0, -0.0], F)
    v2 = v.copy()
    for i in range(len(v2)):
        v2[i, 0] = z[i & 1]
        v2[i, 1] = z[(i >> 1) & 1]
        v2[i, 2] = z[(i // 3) & 1] if i % 2 else F(0.25 * i)
    s.update_mesh(mid, v2, n)
    mb = s.mesh_buffers()
    want = np_refit(v2, t.astype(np.int64), int(mb["info"][0, 2]), mb["leaves"])
    assert np.array_equal(bits(mb["nodes"]), bits(want))
    assert np.array_equal(bits(mb["verts"]), bits(v2))   # (the zeros' signs are kept)


def test_oracle_traversal_of_refitted_boxes(mcpt_mod, oracle_mod):
    """The refitted boxes still enclose their triangles: the oracle's closest hit through them is
    the brute-force closest triangle of the deformed mesh, triangle and distance bits."""
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
    import gen_golden as g
    T = mcpt_mod.Transfo
    v, n, t, _ = CASES["torus"]
    s = mcpt_mod.Scene()
    mid = s.add_mesh(v, n, t, ROOMY)
    trf = T.mul(T.translate(5, -3, 2), T.rotateX(40), T.scale(20))
    s.place_mesh(mid, trf, mcpt_mod.material([1, 1, 1, 1]))
    s.place_mesh(mid, T.mul(T.translate(500, 0, 0), T.scale(1)), mcpt_mod.material([1, 1, 1, 1]))
    s.finalize()
    v2, n2 = deform(v, n, 0.3)
    s.update_mesh(mid, v2, n2)
    prims, nodes, leaves = s.buffers()
    mv = oracle_mod.MeshView(s.mesh_buffers())
    rng = np.random.default_rng(4)
    o = rng.uniform(-60, 60, (60, 3)).astype(F)
    tgt = rng.uniform(-15, 15, (60, 3)).astype(F)
    d = (tgt - o).astype(F)
    oi, of = oracle_mod.trace(prims, nodes, leaves, s.depth(), o, d, meshes=mv)
    k = [i for i in range(len(prims)) if np.array_equal(bits(prims[i][32:48]), bits(trf))][0]
    rec = prims[k]
    hits = 0
    for i in range(len(o)):
        Oi = g.xpoint(rec[16:32], list(o[i]))
        Di = g.normalize(g.xdir(rec[16:32], list(d[i])))
        dist, tri = _np_closest_triangle(v2, t, Oi, Di, [F(x) for x in o[i]], rec[32:48])
        if tri >= 0:
            hits += 1
            assert oi[i, 0] == 0 and oi[i, 1] == k and oi[i, 2] == tri, i
            assert bits(of[i, 0]) == bits(dist), i
        else:
            assert oi[i, 0] == -1, i
    assert hits > 15
