"""Random triangle meshes and mesh scenes for the mesh fuzz tests (test_fuzz_meshes.py on CPU,
test_gpu_fuzz_meshes.py on the GPU), modelled on fuzz_scenes.py: everything is deterministic from
a seed and goes through the public scene API only (Scene.add_mesh, place_mesh, add_*, finalize).

Every input is valid: finite float32 positions, indices in range, no zero-length normal.  Nothing
here is meant to be refused or to fault; the families are the awkward but legal meshes the stock
generators (cube, uv_sphere, torus) never produce:

* soup        unshared random triangles, 1..200 of them (mesh BVH depth 0..8, padded leaves),
              non-unit vertex normals, some pointing backwards;
* grid        an open k x m height field with shared vertices and smooth normals;
* planar      a grid lying exactly in a coordinate plane: Mesh::BB() has zero extent there;
* degenerate  a soup or grid plus a repeated-index triangle, collinear triangles, exact
              duplicates (some with reversed winding) and a sliver of aspect ratio about 1e6;
* far         a cube and a tilted patch authored 2^15..2^16 units from the origin on integer
              coordinates: the 0.001 the triangle boxes grow by is below half an ulp there, so
              the cube's axis-aligned faces have boxes of half-width exactly 0;
* stock       uv_sphere / torus at small odd tessellations, with their own bb6.

Out of scope, on purpose: emissive mesh instances (the reference gives them area 0) and
non-finite vertex data.
"""
import numpy as np

from mcpt import meshes

from fuzz_scenes import ADD, random_ops

FAMILIES = ("soup", "grid", "planar", "degenerate", "far", "stock")
SOUP_SIZES = (1, 2, 3, 4, 5, 7, 8, 9, 31, 33, 200)


def _rng(seed, family):
    return np.random.default_rng([int(seed), FAMILIES.index(family)])


def _unit(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def _face_normals(v, t):
    a, b, c = (v[t[:, k]].astype(np.float64) for k in range(3))
    return np.cross(b - a, c - a)


def _random_units(rng, n):
    return _unit(rng.normal(size=(n, 3)))


def _soup(rng, n):
    v = rng.uniform(-1, 1, (n * 3, 3)).astype(np.float32)
    t = np.arange(n * 3, dtype=np.uint32).reshape(n, 3)
    fn = _unit(_face_normals(v, t)) * np.where(rng.random(n) < 0.5, -1.0, 1.0)[:, None]
    nrm = np.repeat(fn, 3, axis=0) * rng.uniform(0.5, 2.0, (n * 3, 1))
    return v, nrm.astype(np.float32), t


def _grid_tris(k, m):
    i, j = np.meshgrid(np.arange(k - 1), np.arange(m - 1), indexing="ij")
    a, b = i * m + j, i * m + j + 1
    c, d = a + m, b + m
    return np.stack([np.stack([a, c, b], -1), np.stack([b, c, d], -1)], 2).reshape(-1, 3).astype(np.uint32)


def _smooth_normals(v, t):
    fn = _face_normals(v, t)
    acc = np.zeros((len(v), 3))
    for k in range(3):
        np.add.at(acc, t[:, k], fn)
    return _unit(acc).astype(np.float32)


def _grid(rng, k, m, height=0.4):
    x, y = np.meshgrid(np.linspace(-1, 1, k), np.linspace(-1, 1, m), indexing="ij")
    z = rng.uniform(-height, height, (k, m))
    v = np.stack([x, y, z], -1).reshape(-1, 3).astype(np.float32)
    t = _grid_tris(k, m)
    return v, _smooth_normals(v, t), t


def _planar(rng):
    k, m = (int(x) for x in rng.integers(2, 13, 2))
    v, _, t = _grid(rng, k, m, height=0.0)
    axis = int(rng.integers(0, 3))              # the plane x = 0, y = 0 or z = 0
    v = np.roll(v, axis + 1, axis=1)            # (the grid's zero column moves to `axis`)
    nrm = np.zeros_like(v)
    nrm[:, axis] = 1.0
    assert not v[:, axis].any()
    return v, nrm, t


def _degenerate(rng):
    if rng.random() < 0.5:
        v, nrm, t = _soup(rng, int(rng.choice([5, 8, 20, 31, 60])))
    else:
        v, nrm, t = _grid(rng, int(rng.integers(2, 8)), int(rng.integers(2, 8)))
    n0, nv = len(t), len(v)
    ev, et = [], []                             # extra vertices (appended after nv), extra triangles

    def push(points):
        ev.extend(points)
        return list(range(nv + len(ev) - len(points), nv + len(ev)))
    # one triangle that repeats a vertex index
    i, j = (int(x) for x in rng.choice(nv, 2, replace=False))
    et.append([i, i, j])
    # collinear triangles: P, P + d, P + 2 d on a 1/64 lattice (exact in binary32)
    for _ in range(int(rng.integers(2, 5))):
        p = rng.integers(-32, 33, 3) / 64.0
        d = rng.integers(-16, 17, 3) / 64.0
        d[int(rng.integers(0, 3))] = 0.25
        et.append(push([p, p + d, p + 2 * d]))
    # a sliver: base 1, height 1e-6
    p = rng.uniform(-0.5, 0.5, 3)
    u, w = _random_units(rng, 2)
    w = _unit(np.cross(u, w))
    et.append(push([p - 0.5 * u, p + 0.5 * u, p + 1e-6 * w]))
    # exact duplicates of the mesh's own triangles, 10-30 % of the final count, some reversed
    base = np.concatenate([t, np.array(et, np.uint32)])
    frac = float(rng.uniform(0.1, 0.3))
    nd = max(1, int(np.ceil(frac * len(base) / (1.0 - frac))))
    dup = base[rng.integers(0, n0, nd)].copy()
    rev = rng.random(nd) < 0.4
    dup[rev] = dup[rev][:, ::-1]
    t2 = np.concatenate([base, dup]).astype(np.uint32)
    t2 = t2[rng.permutation(len(t2))]           # the extras anywhere in the triangle order
    v2 = np.concatenate([v, np.array(ev, np.float32)]).astype(np.float32)
    n2 = np.concatenate([nrm, _random_units(rng, len(ev)).astype(np.float32)]).astype(np.float32)
    return v2, n2, t2


def _far(rng):
    cv, cn, ct, _ = meshes.cube()
    k, m = (int(x) for x in rng.integers(3, 7, 2))
    gv, _, gt = _grid(rng, k, m, height=0.3)
    ax, ay = np.radians(rng.uniform(20, 70, 2))  # tilt about x then y: no axis-aligned edge is left
    rx = np.array([[1, 0, 0], [0, np.cos(ax), -np.sin(ax)], [0, np.sin(ax), np.cos(ax)]])
    ry = np.array([[np.cos(ay), 0, np.sin(ay)], [0, 1, 0], [-np.sin(ay), 0, np.cos(ay)]])
    gv = gv.astype(np.float64) @ (ry @ rx).T + np.array([2.6, 0.0, 0.0])   # beside the cube
    s = float(rng.integers(40, 100))                  # the mesh spans a few hundred units
    off = rng.integers(2 ** 15 + 2048, 2 ** 16 - 2048, 3) * np.where(rng.random(3) < 0.5, -1, 1)
    v = np.round(np.concatenate([cv.astype(np.float64), gv]) * s) + off
    assert (np.abs(v) >= 2 ** 15).all() and (np.abs(v) < 2 ** 16).all()
    v32 = v.astype(np.float32)
    assert np.array_equal(v32.astype(np.float64), v)                       # integer-valued floats
    t = np.concatenate([ct, gt + len(cv)]).astype(np.uint32)
    gn = _smooth_normals((v - off)[len(cv):], gt)
    return v32, np.concatenate([cn, gn]).astype(np.float32), t


def _stock(rng):
    a, b = (int(x) for x in rng.choice(np.arange(3, 16, 2), 2))
    if rng.random() < 0.5:
        return meshes.uv_sphere(a, b)
    return meshes.torus(a, b, float(rng.uniform(0.15, 0.5)))


def random_mesh(seed, family, n=None):
    """(verts, normals, tris, bb6 or None) of one mesh of `family`; `n` fixes a soup's size."""
    rng = _rng(seed, family)
    if family == "soup":
        v, nrm, t = _soup(rng, int(n if n is not None else rng.choice(SOUP_SIZES)))
    elif family == "grid":
        v, nrm, t = _grid(rng, int(rng.integers(2, 13)), int(rng.integers(2, 13)))
    elif family == "planar":
        v, nrm, t = _planar(rng)
    elif family == "degenerate":
        v, nrm, t = _degenerate(rng)
    elif family == "far":
        v, nrm, t = _far(rng)
    elif family == "stock":
        return _stock(rng)
    else:
        raise ValueError(family)
    assert np.isfinite(v).all() and (np.linalg.norm(nrm, axis=1) > 0.1).all() and t.max() < len(v)
    return v, nrm, t, None


def far_centre(verts):
    """The integer point a `far` mesh was authored around (the centre of its box, rounded)."""
    return np.round((verts.min(0).astype(np.float64) + verts.max(0).astype(np.float64)) / 2)


def random_material(rng):
    """fuzz_scenes.random_ops' material distribution, emissivity 0."""
    col = [*rng.uniform(0, 1, 3).round(3), 1.0 if rng.random() < 0.5 else float(rng.uniform(0.02, 0.98))]
    shin = 0.0 if rng.random() < 0.3 else float(rng.uniform(0.05, 1.0))
    return np.array(col + [shin, float(rng.uniform(0, 1)), 0.0], np.float32)


def random_placement(mcpt_mod, rng, verts, family):
    """translate . rotateZ . rotateX . rotateY . scale: per-axis scales in [0.05, 60] for the
    unit-sized families (each axis uniform, or log-uniform with probability 0.3: most instances
    fill many pixels, some are far below one), one negative (a mirrored instance) with probability 0.3.
    A `far` mesh's transform ends with a scale of about 0.1 and the opposite of its translation,
    so that the instance lands in the usual scene volume."""
    T = mcpt_mod.Transfo
    if family == "far":
        sc = 0.1 * np.exp(rng.uniform(np.log(0.5), np.log(2.0), 3))
    else:
        sc = np.where(rng.random(3) < 0.3, np.exp(rng.uniform(np.log(0.05), np.log(60.0), 3)), rng.uniform(0.05, 60.0, 3))
    if rng.random() < 0.3:
        sc[int(rng.integers(0, 3))] *= -1.0
    trf = T.mul(T.translate(*rng.uniform(-80, 80, 3).round(2)), T.rotateZ(float(rng.uniform(0, 360))),
                T.rotateX(float(rng.uniform(0, 360))), T.rotateY(float(rng.uniform(0, 360))),
                T.scale(*sc.round(4)))
    return T.mul(trf, T.translate(*(-far_centre(verts)))) if family == "far" else trf


def random_mesh_scene_spec(mcpt_mod, seed):
    """The scene of `seed` as data: {"families", "meshes" [(v, n, t, bb6)], "placements"
    [(mesh index, trf16, material7)], "ops" (analytic primitives, fuzz_scenes form), "light"}."""
    rng = np.random.default_rng([int(seed), 99])
    fams = [str(f) for f in rng.choice(FAMILIES, int(rng.integers(1, 5)))]
    sizes = [None] * len(fams)
    if seed % 6 == 0 and "far" not in fams:
        fams[int(rng.integers(0, len(fams)))] = "far"
    if seed % 6 == 1:                           # a one-triangle and a two-triangle soup, anywhere
        while len(fams) < 2:
            fams.append("soup")
        i, j = (int(x) for x in rng.choice(len(fams), 2, replace=False))
        fams[i], fams[j], sizes = "soup", "soup", [None] * len(fams)
        sizes[i], sizes[j] = 1, 2
    ms = [random_mesh(1000 * seed + k, f, sizes[k]) for k, f in enumerate(fams)]
    n_place = int(rng.integers(1, 9))
    which = list(range(len(ms))) + [int(x) for x in rng.integers(0, len(ms), 8)]   # each mesh first
    placements = [(which[p], random_placement(mcpt_mod, rng, ms[which[p]][0], fams[which[p]]), random_material(rng))
                  for p in range(n_place)]
    n_prim = int(rng.integers(0, 11))
    ops = random_ops(mcpt_mod, 7000 + seed, n_prim, n_prim) if n_prim else random_ops(mcpt_mod, 7000 + seed, 1, 1)[1:]
    T = mcpt_mod.Transfo
    light = (5, T.mul(T.translate(0, 0, 160), T.rotateX(180), T.scale(70, 70, 1)),
             mcpt_mod.light([0.9, 0.9, 0.9, 1], 24))
    return {"seed": seed, "families": fams, "meshes": ms, "placements": placements, "ops": ops, "light": light}


def build_scene(mcpt_mod, spec, with_meshes=True):
    """The finalized Scene of a spec; with_meshes=False leaves the meshes and their placements out."""
    s = mcpt_mod.Scene()
    for t, trf, mat in spec["ops"] + [spec["light"]]:
        getattr(s, ADD[t])(trf, mat)
    if with_meshes:
        ids = [s.add_mesh(*m) for m in spec["meshes"]]
        for k, trf, mat in spec["placements"]:
            s.place_mesh(ids[k], trf, mat)
    s.finalize()
    return s


def random_mesh_scene(mcpt_mod, seed):
    """(finalized Scene, its spec): 1-4 meshes of random families (a far one when seed % 6 == 0, a
    one-triangle and a two-triangle soup when seed % 6 == 1), 1-8 placements with non-emissive
    materials, 0-10 analytic primitives and the ground slab of fuzz_scenes.random_ops, and an
    emissive quad above the scene."""
    spec = random_mesh_scene_spec(mcpt_mod, seed)
    return build_scene(mcpt_mod, spec), spec


def aimed_rays(rng, spec, n, which=None, tri_from=0):
    """n rays aimed at points of the placed meshes: a random placement (of `which`, default all), a
    random triangle, a random barycentric point (a quarter of them a vertex or an edge midpoint
    exactly), an origin within 300 units; tri_from: only triangles from that index on.  Returns (origins, dirs, placement index per ray)."""
    pl = spec["placements"]
    which = list(range(len(pl))) if which is None else list(which)
    o = np.zeros((n, 3), np.float32)
    d = np.zeros((n, 3), np.float32)
    pi = np.zeros(n, np.int64)
    for i in range(n):
        p = which[int(rng.integers(0, len(which)))]
        k, trf, _ = pl[p]
        v, _, t, _ = spec["meshes"][k]
        tri = v[t[int(rng.integers(tri_from, len(t)))]].astype(np.float64)
        if rng.random() < 0.25:
            w = np.array([[1, 0, 0], [0, 1, 0], [0, 0, 1], [.5, .5, 0], [0, .5, .5], [.5, 0, .5]])[int(rng.integers(0, 6))]
        else:
            w = rng.dirichlet([1, 1, 1])
        M = np.asarray(trf, np.float64).reshape(4, 4).T
        tgt = M[:3, :3] @ (w @ tri) + M[:3, 3]
        org = tgt + _random_units(rng, 1)[0] * rng.uniform(5, 300)
        o[i], pi[i] = org, p
        d[i] = tgt - o[i].astype(np.float64)
    return o, d, pi
