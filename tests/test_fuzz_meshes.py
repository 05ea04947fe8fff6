"""The mesh fuzz on CPU: the generators of fuzz_meshes.py reach what they claim (the pair
record's out-of-range flag, mesh BVH depths 0 and 1, several depths in one upload), and the host
producer and the oracle are pinned on every family before any GPU is involved."""
import os
import sys

import numpy as np
import pytest

import fuzz_meshes as fm
from test_meshes import _np_closest_triangle

GPU_SEEDS = list(range(48)) + list(range(100, 116)) + list(range(200, 212))   # test_gpu_fuzz_meshes.py


def bits(a):
    return np.asarray(a, np.float32).view(np.uint32)


def _golden():
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
    import gen_golden as g
    return g


def _one_mesh_buffers(mcpt_mod, mesh):
    s = mcpt_mod.Scene()
    mid = s.add_mesh(*mesh)
    s.place_mesh(mid, np.eye(4, dtype=np.float32), mcpt_mod.material([1, 1, 1, 1]))
    s.finalize()
    return s.mesh_buffers()


@pytest.mark.parametrize("seed", range(8))
@pytest.mark.parametrize("family", fm.FAMILIES)
def test_fuzz_mesh_bvh_matches_oracle(mcpt_mod, oracle_mod, family, seed):
    v, n, t, bb = fm.random_mesh(seed, family)
    mb = _one_mesh_buffers(mcpt_mod, (v, n, t, bb))
    d, nodes, leaves = oracle_mod.mesh_bvh(v, t)
    assert mb["info"].tolist() == [[0, 0, d, 0]]
    assert np.array_equal(bits(mb["nodes"]), bits(nodes))
    assert np.array_equal(mb["leaves"], leaves)
    if len(t) > 1:
        assert sorted(leaves[leaves >= 0].tolist()) == list(range(len(t)))
    else:
        assert d == 0 and leaves.tolist() == [-1]
    assert np.array_equal(mb["tris"], t.astype(np.int32))
    assert np.array_equal(bits(mb["verts"]), bits(v)) and np.array_equal(bits(mb["normals"]), bits(n))


def test_one_and_two_triangle_meshes(mcpt_mod, oracle_mod):
    """kd_build's n == 1 case: depth 0, the root is the only leaf and keeps id -1 (as the
    reference does), so none of the mesh's triangles is reachable; n == 2: depth 1, both ids."""
    for n, depth, want in ((1, 0, [-1]), (2, 1, [0, 1])):
        v, nr, t, bb = fm.random_mesh(5, "soup", n)
        mb = _one_mesh_buffers(mcpt_mod, (v, nr, t, bb))
        d, nodes, leaves = oracle_mod.mesh_bvh(v, t)
        assert d == depth and mb["info"].tolist() == [[0, 0, depth, 0]]
        assert np.array_equal(mb["leaves"], leaves) and np.array_equal(bits(mb["nodes"]), bits(nodes))
        assert sorted(mb["leaves"].tolist()) == want


def half_width_flags(nodes, depth):
    """pack_mesh_pairs' range test restated: per internal node, whether all six half-widths
    0.5f * (max - min) of its two children lie in [2^-126, 2^126)."""
    nodes = np.asarray(nodes, np.float32).reshape(-1, 6)
    out = []
    for i in range((1 << depth) - 1):
        hw = np.concatenate([np.float32(0.5) * (nodes[c, 3:] - nodes[c, :3]) for c in (2 * i + 1, 2 * i + 2)])
        assert hw.dtype == np.float32
        a = np.abs(hw)
        out.append(bool(((a >= np.float32(2.0 ** -126)) & (a < np.float32(2.0 ** 126))).all()))
    return np.array(out, bool)


@pytest.mark.parametrize("seed", range(8))
def test_far_meshes_reach_the_out_of_range_flag(mcpt_mod, seed):
    mb = _one_mesh_buffers(mcpt_mod, fm.random_mesh(seed, "far"))
    ok = half_width_flags(mb["nodes"], int(mb["info"][0, 2]))
    assert (~ok).any() and ok.any(), ok


@pytest.mark.parametrize("family", [f for f in fm.FAMILIES if f not in ("far", "planar")])
def test_other_families_stay_in_range(mcpt_mod, family):
    for seed in range(8):
        mb = _one_mesh_buffers(mcpt_mod, fm.random_mesh(seed, family))
        assert half_width_flags(mb["nodes"], int(mb["info"][0, 2])).all(), (family, seed)


def test_scene_flags_follow_the_families(mcpt_mod):
    """In the GPU tests' scenes: every far mesh has a flag-0 pair record, no other mesh but a
    planar one may."""
    for seed in GPU_SEEDS:
        sc, spec = fm.random_mesh_scene(mcpt_mod, seed)
        mb = sc.mesh_buffers()
        if seed % 6 == 0:
            assert "far" in spec["families"], seed
        for fam, (no, lo, d, to) in zip(spec["families"], mb["info"].tolist()):
            ok = half_width_flags(mb["nodes"][no:no + (2 << d) - 1], d)
            if fam == "far":
                assert (~ok).any() and ok.any(), seed
            elif fam != "planar":
                assert ok.all(), (seed, fam)


def test_scene_depths_and_slots(mcpt_mod):
    depths = []
    for seed in GPU_SEEDS:
        sc, spec = fm.random_mesh_scene(mcpt_mod, seed)
        info = sc.mesh_buffers()["info"]
        assert len(info) == len(spec["families"]) and 1 <= len(info) <= 4
        assert 1 <= len(spec["placements"]) <= 8
        if seed % 6 == 1:
            nt = sorted(len(m[2]) for m in spec["meshes"])
            assert nt[:2] == [1, 2], seed
        depths.append(info[:, 2].tolist())
    flat = [d for ds in depths for d in ds]
    assert 0 in flat and 1 in flat and max(flat) >= 6
    assert any(ds[-1] in (0, 1) for ds in depths)                       # the last mesh's slots: 1 or 2
    assert any(len(set(ds)) >= 3 for ds in depths)                      # three or more different depths


def _small_mesh(family, first_seed):
    for seed in range(first_seed, first_seed + 200):
        m = fm.random_mesh(seed, family)
        if 2 <= len(m[2]) <= 64:
            return m
    raise AssertionError(family)


def _placed(mcpt_mod, mesh, trf):
    """A scene of one instance of `mesh` under trf and a far-away second one (a scene of one
    primitive has a one-leaf BVH, whose only leaf keeps id -1)."""
    T = mcpt_mod.Transfo
    s = mcpt_mod.Scene()
    mid = s.add_mesh(*mesh)
    s.place_mesh(mid, trf, mcpt_mod.material([1, 1, 1, 1]))
    s.place_mesh(mid, T.mul(T.translate(5000, 0, 0), T.scale(1)), mcpt_mod.material([1, 1, 1, 1]))
    s.finalize()
    return s


def _placements(mcpt_mod):
    T = mcpt_mod.Transfo
    return {"plain": T.mul(T.translate(5, -3, 2), T.rotateX(40), T.rotateY(25), T.scale(20, 12, 30)),
            "mirrored": T.mul(T.translate(-8, 4, 1), T.rotateZ(70), T.rotateX(-20), T.scale(-15, 20, 10)),
            "tiny": T.mul(T.translate(1, 2, 3), T.rotateY(50), T.scale(0.05))}


@pytest.mark.parametrize("kind", ["plain", "mirrored", "tiny"])
@pytest.mark.parametrize("family", ["soup", "grid", "degenerate", "stock"])
def test_oracle_traversal_vs_brute_force_on_families(mcpt_mod, oracle_mod, family, kind):
    """Every half-width of these families' boxes is positive, so the boxes only cull: the oracle's
    closest hit is the brute-force closest triangle's distance, bit for bit.  Where several
    triangles give that same distance (exact duplicates, a ray through a shared edge) the
    brute force keeps the lowest index and the traversal the first one visited, so the oracle's
    triangle is required to give the best distance, not to be the lowest such index."""
    g = _golden()
    mesh = _small_mesh(family, {"plain": 0, "mirrored": 40, "tiny": 80}[kind])
    v, _, t, _ = mesh
    trf = _placements(mcpt_mod)[kind]
    s = _placed(mcpt_mod, mesh, trf)
    prims, nodes, leaves = s.buffers()
    mv = oracle_mod.MeshView(s.mesh_buffers())
    rng = np.random.default_rng([7, fm.FAMILIES.index(family), len(kind)])
    spec = {"placements": [(0, trf, None)], "meshes": [mesh]}
    o, d, _ = fm.aimed_rays(rng, spec, 40)
    d[20:] += (rng.normal(size=(20, 3)) * np.linalg.norm(d[20:], axis=1, keepdims=True) * 0.02).astype(np.float32)
    oi, of = oracle_mod.trace(prims, nodes, leaves, s.depth(), o, d, meshes=mv)
    k = [i for i in range(len(prims)) if np.array_equal(bits(prims[i][32:48]), bits(trf))][0]
    rec = prims[k]
    hits = 0
    for i in range(len(o)):
        Oi = g.xpoint(rec[16:32], list(o[i]))
        Di = g.normalize(g.xdir(rec[16:32], list(d[i])))
        Ol = [np.float32(x) for x in o[i]]
        dist, tri = _np_closest_triangle(v, t, Oi, Di, Ol, rec[32:48])
        if tri >= 0:
            hits += 1
            assert oi[i, 0] == 0 and oi[i, 1] == k, i
            assert bits(of[i, 0]) == bits(dist), i
            own, _ = _np_closest_triangle(v, t[oi[i, 2]:oi[i, 2] + 1], Oi, Di, Ol, rec[32:48])
            assert bits(own) == bits(dist), (i, int(oi[i, 2]), tri)
        else:
            assert oi[i, 0] == -1, i
    assert hits > 10


@pytest.mark.parametrize("seed", range(4))
def test_oracle_sees_far_and_planar_meshes(mcpt_mod, oracle_mod, seed):
    """far and planar meshes are not compared with the brute force: a box of zero width is the
    reference's behaviour, whatever it culls.  What is asserted is that they stay visible: the
    oracle hits the mesh with more than 10 % of the rays aimed at the far mesh's tilted patch
    (triangles 12.., whose own boxes are not flat) and at the planar mesh.  Measured: 93-96 % for the
    patch (the cube's faces, whose boxes are flat, are never entered: reference behaviour) and
    91-95 % for the planar meshes, which are therefore visible in the reference: their triangle
    boxes are grown by 0.001, only the instance box is flat."""
    T = mcpt_mod.Transfo
    for family, tri_from in (("far", 12), ("planar", 0)):
        mesh = fm.random_mesh(seed, family)
        trf = T.mul(T.translate(5, -3, 2), T.rotateX(40), T.rotateY(25), T.scale(0.1 if family == "far" else 20))
        if family == "far":
            trf = T.mul(trf, T.translate(*(-fm.far_centre(mesh[0]))))
        s = _placed(mcpt_mod, mesh, trf)
        prims, nodes, leaves = s.buffers()
        mv = oracle_mod.MeshView(s.mesh_buffers())
        rng = np.random.default_rng([11, seed])
        o, d, _ = fm.aimed_rays(rng, {"placements": [(0, trf, None)], "meshes": [mesh]}, 200, tri_from=tri_from)
        oi, _ = oracle_mod.trace(prims, nodes, leaves, s.depth(), o, d, meshes=mv)
        frac = float((oi[:, 0] == 0).mean())
        print(f"{family} seed {seed}: {frac:.3f} of the aimed rays hit the mesh")
        assert frac > 0.10, (family, seed, frac)


def test_instance_records_of_mirrored_and_computed_bb(mcpt_mod):
    """place_mesh's rule (test_meshes.test_instance_record) on a mirrored placement of a mesh with
    its own bb6 and on a placement of a mesh whose box is computed from its vertices (bb6 = None):
    rows 0..15 = trf . BB.matrix(), rows 32..47 = trf, field 49 = the mesh id; rows 16..31 are
    trf's inverse: their product with trf is the identity to 1e-5 of the products summed."""
    T = mcpt_mod.Transfo
    stock, soup = fm.random_mesh(3, "stock"), fm.random_mesh(2, "soup", 33)
    assert stock[3] is not None and soup[3] is None
    pl = _placements(mcpt_mod)
    s = mcpt_mod.Scene()
    ids = [s.add_mesh(*stock), s.add_mesh(*soup)]
    s.place_mesh(ids[0], pl["mirrored"], mcpt_mod.material([1, 1, 1, 1]))
    s.place_mesh(ids[1], pl["plain"], mcpt_mod.material([1, 1, 1, 1]))
    s.finalize()
    prims, _, _ = s.buffers()
    assert (prims[:, 48] == 0).sum() == 2
    for mid, (mesh, trf) in enumerate(((stock, pl["mirrored"]), (soup, pl["plain"]))):
        rec = [r for r in prims if np.array_equal(bits(r[32:48]), bits(trf))][0]
        bb = mesh[3] if mesh[3] is not None else np.concatenate([mesh[0].min(0), mesh[0].max(0)]).astype(np.float32)
        c = (bb[:3] + bb[3:]) / np.float32(2)
        sc = (bb[3:] - bb[:3]) / np.float32(2)
        assert np.array_equal(bits(rec[:16]), bits(T.mul(trf, T.mul(T.translate(*c), T.scale(*sc)))))
        assert rec[49] == float(mid) and rec[59] == 0.0
        inv, m = (np.asarray(x, np.float64).reshape(4, 4).T for x in (rec[16:32], rec[32:48]))
        err = np.abs(inv @ m - np.eye(4))
        assert (err <= 1e-5 * (np.abs(inv) @ np.abs(m))).all(), err
    assert np.linalg.det(np.asarray(pl["mirrored"], np.float64).reshape(4, 4)) < 0   # it is a mirror
