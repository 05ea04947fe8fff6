"""Lifetimes of what a context holds on the device (ownership by type, groups by
lifetime): a context that has allocated every group and then changes its target behaves as a fresh
one does, bit for bit, and closing a context with work queued is safe.

No memory is measured (the device is shared): what is asserted is what a caller can see -- the modes
off, the guides gone, no error map, the timing queries answering as a fresh context's, and the same
bits as a fresh context and as the oracle after the target shrinks and grows again.

The gathered-planes case reads `read_sample_counts` "falling back to the pass count" as the library
implements it: after `set_target` the frame holds no per-pixel counts (the query refuses), and a
counted gather *from* that frame carries its pass count for every pixel, not the old plane's counts."""
import numpy as np
import pytest

from test_gpu_work_items import B_ROWS, MB, MIOR, MW, oracle_rows
from test_meshes import mesh_scene

pytestmark = pytest.mark.gpu

W0, H0, W1, H1, S, B = 24, 19, 17, 9, 70, 8
NO_GUIDES, NO_ADAPTIVE = -7, -9


def bits(a):
    return np.asarray(a, np.float32).view(np.uint32)


def status(mcpt_mod, call, *args):
    try:
        call(*args)
    except mcpt_mod.MCPTError as e:
        return str(e)
    return "ok"


def render_frame(mcpt_mod, r, W, H, passes=S, rows=None, ior=1.0):
    if rows is None:
        r.set_target(W, H)
    else:
        r.set_target_rows(W, H, rows)
    ipv, iv = mcpt_mod.camera_canonical(W, H)
    r.render(ipv, iv, 1, passes, 0.0, B, ior, 0)
    acc, n = r.read_accum()
    assert n == passes
    return acc


def fresh_frame(mcpt_mod, sc, W, H, passes=S, rows=None, ior=1.0):
    r = mcpt_mod.Renderer(0)
    try:
        r.set_traversal(1)
        r.upload_scene(sc)
        return render_frame(mcpt_mod, r, W, H, passes, rows, ior), r.last_denoise_ms(), r.last_stats_ms()
    finally:
        r.close()


def assert_as_fresh(mcpt_mod, r, fresh_denoise_ms, fresh_stats_ms):
    assert not r.stats_info()["on"] and not r.adaptive_info()["on"] and not r.temporal_info()["on"]
    assert f"({NO_GUIDES})" in status(mcpt_mod, r.read_guides)
    assert r.error_map_source() == 0
    assert r.last_denoise_ms() == fresh_denoise_ms and r.last_stats_ms() == fresh_stats_ms


def test_churn_is_invisible(mcpt_mod, oracle_mod, monkeypatch):
    """24 x 19, the LDS-scene reference scene, the walk pinned (lane launches) and the pass split off
    (launches of several segments steal): statistics, adaptive and temporal modes on, guides, 70-pass
    renders of three segments on both lanes (segment sums and steal store; a frame this small has too
    few work items for the item order, which the mesh case allocates), a variance filter and a temporal
    accumulate; then set_target(17, 9)."""
    monkeypatch.setenv("MCPT_PASS_SPLIT", "0")
    monkeypatch.setenv("MCPT_SEG_PER_ITEM", "1")
    sc = mcpt_mod.Scene.reference(1)
    small, fresh_dn, fresh_st = fresh_frame(mcpt_mod, sc, W1, H1)
    r = mcpt_mod.Renderer(0)
    try:
        r.set_traversal(1)
        r.upload_scene(sc)
        r.set_target(W0, H0)
        ipv, iv = mcpt_mod.camera_canonical(W0, H0)
        r.stats_begin()
        r.adaptive_begin(0)
        r.temporal_begin()
        r.render_guides(ipv, iv)
        r.render(ipv, iv, 1, S, 0.0, B, 1.0, 0)       # the 70-pass call: lane 0
        r.render(ipv, iv, 71, S, 0.0, B, 1.0, 0)      # (a second batch for the error map: lane 1)
        assert r.debug_counters(reset=True)[62] > 0   # (passes were stolen: the steal store is in use)
        r.convergence(0.05)
        r.denoise_variance(2)
        rec = r.temporal_accumulate(None)
        assert rec["frames"] == 1 and r.stats_info()["on"] and r.adaptive_info()["on"] and r.temporal_info()["on"]
        assert r.error_map_source() == 1 and r.last_denoise_ms()[1] > 0.0 and r.last_stats_ms()[0] > 0.0

        r.set_target(W1, H1)
        assert_as_fresh(mcpt_mod, r, fresh_dn, fresh_st)
        assert np.array_equal(bits(render_frame(mcpt_mod, r, W1, H1)), bits(small))
        big = render_frame(mcpt_mod, r, W0, H0)
    finally:
        r.close()
    ref = oracle_rows(oracle_mod, sc, W0, H0, S, B, 1.0, [0, 7, 8, 18])
    for y, row in ref.items():
        assert row.any() and np.array_equal(bits(big[y]), bits(row)), f"row {y}"


def test_mesh_churn_is_invisible(mcpt_mod, oracle_mod):
    """The same with meshes: the row shard of test_gpu_work_items.py's case B (43 rows of 253 x 131,
    704-pass calls of 4,224 items: the order, split items and stealing), shrunk to 17 x 9, regrown."""
    sc = mesh_scene(mcpt_mod)
    small, _, _ = fresh_frame(mcpt_mod, sc, W1, H1, ior=MIOR)
    r = mcpt_mod.Renderer(0)
    try:
        r.set_traversal(1)
        r.upload_scene(sc)
        r.set_target_rows(MW, 131, B_ROWS)
        ipv, iv = mcpt_mod.camera_canonical(MW, 131)
        r.render(ipv, iv, 1, 704, 0.0, MB, MIOR, 0)
        r.render(ipv, iv, 705, 704, 0.0, MB, MIOR, 0)   # (the second call runs the measured order, split items)
        assert np.array_equal(bits(render_frame(mcpt_mod, r, W1, H1, ior=MIOR)), bits(small))
        big = render_frame(mcpt_mod, r, MW, 131, 704, rows=B_ROWS, ior=MIOR)
    finally:
        r.close()
    rows = [int(B_ROWS[0]), int(B_ROWS[-1])]
    ref = oracle_rows(oracle_mod, sc, MW, 131, 704, MB, MIOR, rows, meshes=oracle_mod.MeshView(sc.mesh_buffers()))
    for i, y in ((0, rows[0]), (42, rows[1])):
        assert ref[y].any() and np.array_equal(bits(big[i]), bits(ref[y])), f"image row {y}"


def test_gathered_planes_end_with_the_target(mcpt_mod):
    """A counted gather and a gathered error map into a frame, then set_target on the frame."""
    sc = mcpt_mod.Scene.reference(1)
    ipv, iv = mcpt_mod.camera_canonical(W0, H0)
    made = []
    try:
        shards = []
        for k, rows in enumerate((list(range(0, 10)), list(range(10, H0)))):
            s = mcpt_mod.Renderer(0)
            made.append(s)
            s.upload_scene(sc)
            s.set_target_rows(W0, H0, rows)
            s.stats_begin()
            for b in range(2 + k):   # (shard 1 holds more passes: the counts differ between the shards)
                s.render(ipv, iv, 1 + 8 * b, 8, 0.0, B, 1.0, 0)
            s.convergence(0.05)
            shards.append(s)
        frame, other = mcpt_mod.Renderer(0), mcpt_mod.Renderer(0)
        made += [frame, other]
        for f in (frame, other):
            f.upload_scene(sc)
            f.set_target(W0, H0)
        frame.gather_rows_counted(shards)
        frame.gather_error_map(shards)
        cnt = frame.read_sample_counts()
        assert (cnt[:10] == 16).all() and (cnt[10:] == 24).all() and frame.error_map_source() == 2

        frame.set_target(W0, H0)
        assert frame.error_map_source() == 0
        assert f"({NO_ADAPTIVE})" in status(mcpt_mod, frame.read_sample_counts)
        frame.render(ipv, iv, 1, 3, 0.0, B, 1.0, 0)
        other.gather_rows_counted([frame])      # the frame's counts: its pass count for every pixel
        assert (other.read_sample_counts() == 3).all() and other.error_map_source() == 0
    finally:
        for r in made:
            r.close()


def test_destroy_with_work_queued(mcpt_mod, oracle_mod):
    """mcpt_destroy's ordinary shutdown path: a 70-pass render queued, the context closed without a
    wait; a new context then renders one pass equal to the oracle's."""
    sc = mcpt_mod.Scene.reference(1)
    ipv, iv = mcpt_mod.camera_canonical(W0, H0)
    r = mcpt_mod.Renderer(0)
    r.set_traversal(1)
    r.upload_scene(sc)
    r.set_target(W0, H0)
    r.render(ipv, iv, 1, S, 0.0, B, 1.0, 0)
    r.close()
    acc, _, _ = fresh_frame(mcpt_mod, sc, W0, H0, passes=1)
    prims, nodes, leaves = sc.buffers()
    oipv, oiv = oracle_mod.camera(W0, H0)
    ref, _ = oracle_mod.render(prims, nodes, leaves, sc.depth(), oipv, oiv, W0, H0, 1, 1, 0.0, B, 1.0, 0)
    assert ref.any() and np.array_equal(bits(acc), bits(ref))
