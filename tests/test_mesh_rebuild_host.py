"""Rebuilding a mesh's tree on the CPU: Scene.rebuild_mesh, the specification of the
device rebuild, against a numpy restatement of kd_build_stable written here (np.argsort(kind="stable")
per range on float32 keys), the triangle sets of add_mesh's tree, its refusals, and the oracle's
traversal of the rebuilt buffers."""
import numpy as np
import pytest

from test_mesh_refit_host import ROOMY, bits, np_refit, np_tri_box, one_mesh_scene, same_buffers, strip

F = np.float32


def jitter_mesh(n_tris, seed, size=0.05):
    """n_tris triangles of extent `size` at random places of [-1, 1]^3, their rows in a random order:
    every centre key distinct (asserted where it matters)."""
    rng = np.random.default_rng(seed)
    c = rng.uniform(-1, 1, (n_tris, 1, 3))
    v = (c + rng.uniform(-size, size, (n_tris, 3, 3))).reshape(-1, 3).astype(F)
    n = rng.normal(size=v.shape).astype(F)
    t = np.arange(3 * n_tris, dtype=np.uint32).reshape(-1, 3)[rng.permutation(n_tris)]
    return v, n, t, ROOMY


def grid_mesh(nx=9, ny=7):
    """Two triangles per cell of a regular grid in z = 0: whole columns share a centre x, whole rows a
    centre y, every centre z is equal — ties in every round."""
    xs, ys = np.meshgrid(np.arange(nx + 1), np.arange(ny + 1), indexing="ij")
    v = np.stack([xs.ravel() / nx - 0.5, ys.ravel() / ny - 0.5, np.zeros(xs.size)], 1).astype(F)
    idx = lambda i, j: i * (ny + 1) + j
    t = []
    for i in range(nx):
        for j in range(ny):
            t += [[idx(i, j), idx(i + 1, j), idx(i + 1, j + 1)], [idx(i, j), idx(i + 1, j + 1), idx(i, j + 1)]]
    n = np.tile(np.array([0, 0, 1], F), (len(v), 1))
    return v, n, np.array(t, np.uint32), ROOMY


def copies_mesh(k=37):
    """k copies of one triangle: all keys equal, so the order must stay 0 .. k-1."""
    v = np.array([[0, 0, 0], [0.5, 0, 0.1], [0, 0.5, -0.1]], F)
    return v, np.tile(np.array([0, 0, 1], F), (3, 1)), np.tile(np.array([0, 1, 2], np.uint32), (k, 1)), ROOMY


def cases():
    out = {f"strip{k}": strip(k, 100 + k) for k in (1, 2, 3, 4, 5, 7, 257, 1000)}
    out["grid"] = grid_mesh()
    out["copies37"] = copies_mesh()
    return out


CASES = cases()


def np_centres(v, tris):
    box = np.stack([np_tri_box(v, t) for t in tris])
    return ((box[:, :3] + box[:, 3:]) / F(2.0)).astype(F)


def np_bounds(n, rounds):
    b = [0, n]
    for _ in range(rounds):
        nxt = [b[0]]
        for s in range(1, len(b)):
            nxt += [(b[s - 1] + b[s]) // 2, b[s]]
        b = nxt
    return b


def np_build_stable(v, tris):
    """kd_build_stable restated: (depth, leaves)."""
    n = len(tris)
    depth = int(np.ceil(np.log2(F(n))))
    if depth == 0:
        return 0, np.array([-1], np.int32)
    c = np_centres(v, tris)
    order = np.arange(n)
    for rnd in range(1, depth):
        key = c[:, (rnd - 1) % 3]
        b = np_bounds(n, rnd - 1)
        for s in range(len(b) - 1):
            seg = order[b[s]:b[s + 1]]
            order[b[s]:b[s + 1]] = seg[np.argsort(key[seg], kind="stable")]
    b = np_bounds(n, depth - 1)
    leaves = np.full(1 << depth, -1, np.int32)
    for s in range(len(b) - 1):
        leaves[2 * s] = order[b[s]]
        if b[s + 1] - b[s] == 2:
            leaves[2 * s + 1] = order[b[s] + 1]
        assert 1 <= b[s + 1] - b[s] <= 2
    return depth, leaves


def want_buffers(v, t):
    depth, leaves = np_build_stable(v, t.astype(np.int64))
    return depth, leaves, np_refit(v, t.astype(np.int64), depth, leaves)


@pytest.mark.parametrize("name", sorted(CASES))
def test_rebuild_matches_restatement(mcpt_mod, name):
    v, n, t, bb = CASES[name]
    s, mid = one_mesh_scene(mcpt_mod, v, n, t, bb)
    before = s.mesh_buffers()
    s.rebuild_mesh(mid)
    mb = s.mesh_buffers()
    depth, leaves, nodes = want_buffers(v, t)
    assert int(mb["info"][0, 2]) == depth and np.array_equal(mb["info"], before["info"])
    assert np.array_equal(mb["leaves"], leaves)
    assert np.array_equal(bits(mb["nodes"]), bits(nodes))
    assert np.array_equal(mb["tris"], t.astype(np.int32)) and np.array_equal(bits(mb["verts"]), bits(v))
    if name == "copies37":
        assert np.array_equal(mb["leaves"][mb["leaves"] >= 0], np.arange(37))   # (the leaves' triangles, in order)
    again = s.mesh_buffers()
    s.rebuild_mesh(mid)                                  # idempotent
    assert same_buffers(again, s.mesh_buffers())
    s.buffers()                                          # (still finalized)


@pytest.mark.parametrize("name", ["strip5", "strip257", "grid"])
def test_rebuild_after_update(mcpt_mod, name):
    from test_mesh_refit_host import deform
    v, n, t, bb = CASES[name]
    s, mid = one_mesh_scene(mcpt_mod, v, n, t, bb)
    v2, n2 = deform(v, n, 0.2)
    s.update_mesh(mid, v2, n2)
    s.rebuild_mesh(mid)
    mb = s.mesh_buffers()
    _, leaves, nodes = want_buffers(v2, t)
    assert np.array_equal(mb["leaves"], leaves) and np.array_equal(bits(mb["nodes"]), bits(nodes))


def subtree_sets(leaves, depth):
    """the triangle-id set under every internal node, heap order"""
    level = [frozenset([int(x)]) - {-1} for x in leaves]
    out = []
    for _ in range(depth):
        level = [level[2 * k] | level[2 * k + 1] for k in range(len(level) // 2)]
        out = level + out
    return out


@pytest.mark.parametrize("n_tris", [2, 3, 5, 7, 100, 257, 1000])
def test_triangle_sets_of_add_mesh(mcpt_mod, n_tris):
    v, n, t, bb = jitter_mesh(n_tris, n_tris)
    c = np_centres(v, t.astype(np.int64))
    for a in range(3):   # the condition under which the two builders must agree
        assert len(np.unique(c[:, a])) == n_tris
    s, mid = one_mesh_scene(mcpt_mod, v, n, t, bb)
    before = s.mesh_buffers()
    s.rebuild_mesh(mid)
    mb = s.mesh_buffers()
    d = int(mb["info"][0, 2])
    assert subtree_sets(before["leaves"], d) == subtree_sets(mb["leaves"], d)
    assert np.array_equal(mb["leaves"] < 0, before["leaves"] < 0)
    # internal boxes are merges of the same sets: the same bits (min / max do not depend on the order)
    assert np.array_equal(bits(mb["nodes"][:(1 << d) - 1]), bits(before["nodes"][:(1 << d) - 1]))


@pytest.mark.parametrize("name", ["strip1", "strip2", "strip7", "strip257", "grid"])
def test_new_triangle_rows(mcpt_mod, name):
    """tris= with the same rows in another order gives the tree of the permuted mesh."""
    v, n, t, bb = CASES[name]
    rng = np.random.default_rng(8)
    t2 = t[rng.permutation(len(t))][:, [1, 2, 0]]
    s, mid = one_mesh_scene(mcpt_mod, v, n, t, bb)
    s.rebuild_mesh(mid, t2)
    s2, mid2 = one_mesh_scene(mcpt_mod, v, n, t2, bb)
    s2.rebuild_mesh(mid2)
    assert same_buffers(s.mesh_buffers(), s2.mesh_buffers())
    depth, leaves, nodes = want_buffers(v, t2)
    mb = s.mesh_buffers()
    assert np.array_equal(mb["tris"], t2.astype(np.int32)) and np.array_equal(mb["leaves"], leaves)
    assert np.array_equal(bits(mb["nodes"]), bits(nodes))


def test_second_of_two_meshes(mcpt_mod):
    T = mcpt_mod.Transfo
    (v0, n0, t0, _), (v1, n1, t1, _) = CASES["strip7"], CASES["grid"]
    s = mcpt_mod.Scene()
    a, b = s.add_mesh(v0, n0, t0, ROOMY), s.add_mesh(v1, n1, t1, ROOMY)
    s.place_mesh(a, T.translate(-3, 0, 0), mcpt_mod.material([1, 1, 1, 1]))
    s.place_mesh(b, T.translate(3, 0, 0), mcpt_mod.material([1, 0, 0, 1]))
    s.finalize()
    scene_before, before = s.buffers(), s.mesh_buffers()
    t2 = t1[::-1].copy()
    s.rebuild_mesh(b, t2)
    mb = s.mesh_buffers()
    assert all(np.array_equal(bits(x), bits(y)) for x, y in zip(scene_before[:2], s.buffers()[:2]))
    no, lo, to = (int(x) for x in mb["info"][1, [0, 1, 3]])
    for k in ("nodes", "leaves", "tris"):
        cut = {"nodes": no, "leaves": lo, "tris": to}[k]
        assert np.array_equal(mb[k][:cut].view(np.uint32), before[k][:cut].view(np.uint32))
    depth, leaves, nodes = want_buffers(v1, t2)
    assert np.array_equal(mb["leaves"][lo:], leaves) and np.array_equal(bits(mb["nodes"][no:]), bits(nodes))
    assert np.array_equal(mb["tris"][to:], t2.astype(np.int32) + len(v0))   # (global vertex ids)


def test_refusals_change_nothing(mcpt_mod):
    v, n, t, bb = CASES["strip257"]
    s, mid = one_mesh_scene(mcpt_mod, v, n, t, bb)
    s.rebuild_mesh(mid)
    before = s.mesh_buffers()
    L = mcpt_mod.lib()
    import ctypes
    up = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_uint))
    INVALID = -1
    t2 = np.ascontiguousarray(t[::-1])
    assert L.mcpt_scene_rebuild_mesh(s._h, mid + 1, None, 0) == INVALID
    assert L.mcpt_scene_rebuild_mesh(s._h, -1, None, 0) == INVALID
    assert L.mcpt_scene_rebuild_mesh(s._h, mid, up(t2), len(t2) - 1) == INVALID
    assert L.mcpt_scene_rebuild_mesh(s._h, mid, up(t2), len(t2) + 1) == INVALID
    bad = t2.copy()
    bad[200, 1] = len(v)                                  # the first index outside the vertices
    assert L.mcpt_scene_rebuild_mesh(s._h, mid, up(bad), len(bad)) == INVALID
    with pytest.raises(mcpt_mod.MCPTError):
        s.rebuild_mesh(mid, bad)
    assert same_buffers(before, s.mesh_buffers())
    s.buffers()                                           # (still finalized)


def test_oracle_traversal_of_rebuilt_tree(mcpt_mod, oracle_mod):
    """The oracle's closest hits over the rebuilt buffers are those over add_mesh's buffers (a jittered
    mesh: no two hits of a ray tie, so the answer does not depend on the visit order)."""
    T = mcpt_mod.Transfo
    v, n, t, bb = jitter_mesh(600, 21, size=0.2)          # (larger triangles: more hits)
    rng = np.random.default_rng(22)
    s = mcpt_mod.Scene()
    mid = s.add_mesh(v, n, t, ROOMY)
    s.place_mesh(mid, T.mul(T.translate(2, -1, 3), T.rotateX(25), T.scale(30)), mcpt_mod.material([1, 1, 1, 1]))
    s.add_sphere(T.mul(T.translate(0, 0, 300), T.scale(5)), mcpt_mod.light([1, 1, 1, 1], 5))   # (a scene of one primitive has no leaf)
    s.finalize()
    prims, nodes, leaves = s.buffers()
    o = rng.uniform(-90, 90, (3000, 3)).astype(F)
    d = (rng.uniform(-25, 25, (3000, 3)) - o).astype(F)
    oi0, of0 = oracle_mod.trace(prims, nodes, leaves, s.depth(), o, d, meshes=oracle_mod.MeshView(s.mesh_buffers()))
    s.rebuild_mesh(mid)
    oi1, of1 = oracle_mod.trace(prims, nodes, leaves, s.depth(), o, d, meshes=oracle_mod.MeshView(s.mesh_buffers()))
    assert np.array_equal(oi0, oi1) and np.array_equal(bits(of0), bits(of1))
    assert (oi0[:, 0] == 0).sum() > 300
