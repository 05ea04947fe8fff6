"""Guide buffers (mcpt_render_guides) on the GPU: every pixel's primary hit, bit for bit against
the oracle's ray query and the device's own (Renderer.trace) on camera rays computed by the
independent restatement tests/golden/gen_golden.camera_dir — scenes 1..8 and a mesh scene
(smooth and flat normals) at 45x37 (partial tiles in both axes), and a row shard."""
import os
import sys

import numpy as np
import pytest

from test_meshes import mesh_scene

pytestmark = pytest.mark.gpu

W, H = 45, 37
FLT_MAX = np.float32(3.402823e38)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def renderer(mcpt_mod):
    r = mcpt_mod.Renderer(0)
    yield r
    r.close()


@pytest.fixture(scope="module")
def rays(mcpt_mod):
    """(origins, dirs) of every pixel of the W x H frame, row-major (row 0 = bottom); computed once."""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
    import gen_golden as g
    ipv, iv = mcpt_mod.camera_canonical(W, H)
    o = np.zeros((H, W, 3), np.float32)
    d = np.zeros((H, W, 3), np.float32)
    for y in range(H):
        for x in range(W):
            ori, dr, _, _ = g.camera_dir(ipv, iv, W, H, x, y)
            o[y, x], d[y, x] = ori, dr
    return ipv, iv, o, d


def check_guides(g, oi, of, hits, shape_hw):
    """guides dict (rows x W) against the oracle's (oi, of) and the device's trace records."""
    n = shape_hw[0] * shape_hw[1]
    key = g["key"].reshape(n)
    hit = oi[:, 0] >= 0
    assert hit.any()
    want_key = np.where(hit, (oi[:, 0] << 28) | oi[:, 1], -1).astype(np.int32)
    assert np.array_equal(key, want_key)
    assert np.array_equal(bits(g["normal"].reshape(n, 3)), bits(of[:, 7:10]))
    assert np.array_equal(bits(g["position"].reshape(n, 3)), bits(of[:, 10:13]))
    assert np.array_equal(bits(g["dist"].reshape(n)), bits(of[:, 0]))
    assert np.array_equal(bits(g["albedo"].reshape(n, 4)), bits(of[:, 13:17]))
    # a miss: N = P = colour = 0, dist = FLT_MAX
    assert (g["dist"].reshape(n)[~hit] == FLT_MAX).all() and not g["normal"].reshape(n, 3)[~hit].any()
    assert not g["position"].reshape(n, 3)[~hit].any() and not g["albedo"].reshape(n, 4)[~hit].any()
    # the device's own ray query on the same rays
    assert np.array_equal(np.where(hits["shape"] >= 0, (hits["shape"] << 28) | hits["prim"], -1).astype(np.int32), key)
    assert np.array_equal(bits(hits["N"]), bits(g["normal"].reshape(n, 3)))
    assert np.array_equal(bits(hits["P"]), bits(g["position"].reshape(n, 3)))
    assert np.array_equal(bits(hits["dist"]), bits(g["dist"].reshape(n)))
    assert np.array_equal(bits(hits["color"]), bits(g["albedo"].reshape(n, 4)))


@pytest.mark.parametrize("scene_id", range(1, 9))
def test_guides_reference_scenes(mcpt_mod, oracle_mod, renderer, rays, scene_id):
    ipv, iv, o, d = rays
    sc = mcpt_mod.Scene.reference(scene_id)
    prims, nodes, leaves = sc.buffers()
    renderer.upload_scene(sc)
    renderer.set_target(W, H)
    renderer.render_guides(ipv, iv)
    g = renderer.read_guides()
    assert g["normal"].shape == (H, W, 3) and g["key"].dtype == np.int32 and g["albedo"].shape == (H, W, 4)
    oi, of = oracle_mod.trace(prims, nodes, leaves, sc.depth(), o, d)
    check_guides(g, oi, of, renderer.trace(o, d), (H, W))
    assert renderer.last_denoise_ms()[0] > 0.0


@pytest.mark.parametrize("flat", [False, True])
def test_guides_mesh_scene(mcpt_mod, oracle_mod, renderer, rays, flat):
    ipv, iv, o, d = rays
    sc = mesh_scene(mcpt_mod)
    prims, nodes, leaves = sc.buffers()
    renderer.upload_scene(sc)
    renderer.set_flat_face(flat)
    renderer.set_target(W, H)
    renderer.render_guides(ipv, iv)
    g = renderer.read_guides()
    hits = renderer.trace(o, d)
    renderer.set_flat_face(False)
    mv = oracle_mod.MeshView(sc.mesh_buffers(), flat_face=flat)
    oi, of = oracle_mod.trace(prims, nodes, leaves, sc.depth(), o, d, meshes=mv)
    check_guides(g, oi, of, hits, (H, W))
    assert ((g["key"] >> 28) == 0).sum() > 50          # mesh hits (shape code 0)


def test_guides_row_shard(mcpt_mod, renderer, rays):
    """A row-shard target's guides are the full frame's guides of those rows."""
    ipv, iv, _, _ = rays
    rows = [3, 4, 20, 36]
    renderer.upload_scene(mcpt_mod.Scene.reference(6))
    renderer.set_target(W, H)
    renderer.render_guides(ipv, iv)
    full = renderer.read_guides()
    renderer.set_target_rows(W, H, rows)
    with pytest.raises(mcpt_mod.MCPTError):               # the new target has no guides yet
        renderer.read_guides()
    renderer.render_guides(ipv, iv)
    part = renderer.read_guides()
    for k in ("normal", "position", "dist", "albedo"):
        assert part[k].shape[0] == len(rows)
        assert np.array_equal(bits(part[k]), bits(full[k][rows])), k
    assert np.array_equal(part["key"], full["key"][rows])
