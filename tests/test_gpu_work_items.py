"""The work-item order, split items, pass stealing, tail pieces and the render lanes on frames
whose size is no multiple of the tile, against the oracle (closes ADVICE.md's third finding).

Every other "same bits" test of these mechanisms (test_gpu_parity.py, test_gpu_full_size.py) runs
at 1920x1080 or 960x540, multiples of 8, 16 and 32: every tile of every kernel lies wholly inside
the frame, and "on" is compared with "off", never with the oracle.  Here the frames are 253 x 131
(mesh kernels, 8x8 tiles: a last tile column 5 px wide, a last tile row 3 px tall) and 517 x 253
(scene kernels, 16- and 32-wide tiles: a last column and row of 5 px), each launch holds at least
4,096 work items (kOrderMinItems), so the mechanisms are on, and the MCPT_ITEM_ORDER=0 frame they
are compared with is itself compared with the oracle on rows that cross the partial tiles.  What
runs here and nowhere else in the suite: steal_next's skip of units whose pixel lies outside the
frame, the combines' pixel -> (tile, thread) mapping with tiles_x = ceil(W / TW), a split item's
pieces on a partial tile, tail pieces on a partial tile, and all of it on a row shard whose row
count is no multiple of 8.  Bits are compared everywhere; there is no tolerance."""
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from test_meshes import mesh_scene

pytestmark = pytest.mark.gpu

SLOT_STOLEN, SLOT_SPLIT = 62, 63   # debug counters: passes rendered for another lane's pixel, items split
ENV = ("MCPT_ITEM_ORDER", "MCPT_SPLIT_ITEMS", "MCPT_STEAL", "MCPT_SEG_PER_ITEM", "MCPT_TAIL_PIECES", "MCPT_PASS_SPLIT")

# mesh cases: 32 x 17 tiles of 8x8
MW, MH, MB, MIOR = 253, 131, 8, 1.2
A_CALLS = [256, 256, 256, 72]   # 3 x (544 tiles x 8 segments = 4,352 items), then 1,632 items (combine_kernel)
A_ROWS = [0, 7, 8, 64, 127, 128, 129, 130]   # tile-row edges, an interior row, the 3-row top tile row
B_ROWS = np.arange(1, 131, 3)[:43]           # 43 local rows (43 % 8 == 3), not contiguous in the image
B_CALLS = [704, 704]                         # 192 tiles x 22 segments = 4,224 items per call


def bits(a):
    return np.asarray(a, np.float32).view(np.uint32)


def set_env(mp, **on):
    """The scheduling switches the library reads per launch: those named, the others unset."""
    for k in ENV:
        mp.delenv(k, raising=False)
    for k, v in on.items():
        mp.setenv(k, str(v))


@pytest.fixture(scope="module")
def renderer(mcpt_mod):
    r = mcpt_mod.Renderer(0)
    yield r
    r.close()


@pytest.fixture(scope="module")
def mesh(mcpt_mod):
    return mesh_scene(mcpt_mod)


def run_calls(mcpt_mod, r, sc, W, H, calls, B, ior, traversal, rows=None, snap=()):
    """Upload, set the target (a row shard with `rows`) and render `calls` (pass counts, from pass
    1) with the walk pinned.  Returns the final accumulator, the accumulators read after the calls
    whose index is in `snap`, each call's sub-launch count, and debug slots 62 / 63 of the run."""
    ipv, iv = mcpt_mod.camera_canonical(W, H)
    r.set_traversal(traversal)
    try:
        r.upload_scene(sc)
        if rows is None:
            r.set_target(W, H)
        else:
            r.set_target_rows(W, H, rows)
        r.debug_counters(reset=True)
        p, snaps, launches = 1, {}, []
        for k, n in enumerate(calls):
            r.render(ipv, iv, p, n, 0.0, B, ior, 0)
            launches.append(r.last_launch_count())
            p += n
            if k in snap:
                snaps[k] = r.read_accum()[0]
        acc, cnt = r.read_accum()
        # (read once the run is over, so that no host wait separates the calls: slot 63 is written by
        # the sort after the first call, slot 62 is summed by every stealing launch)
        dbg = r.debug_counters(reset=True)
    finally:
        r.set_traversal(0)
    assert cnt == sum(calls)
    return acc, snaps, launches, (int(dbg[SLOT_STOLEN]), int(dbg[SLOT_SPLIT]))


def oracle_rows(oracle_mod, sc, W, H, S, B, ior, rows, meshes=None):
    """{image row: its W x 3 sums of passes 1..S} from the oracle, one single-threaded render per
    row (row_step = H), the rows side by side."""
    prims, nodes, leaves = sc.buffers()
    ipv, iv = oracle_mod.camera(W, H)

    def one(y):
        ref, _ = oracle_mod.render(prims, nodes, leaves, sc.depth(), ipv, iv, W, H, 1, S, 0.0, B, ior, 0,
                                   row_step=H, row_offset=int(y), n_threads=1, meshes=meshes)
        return ref[int(y)].copy()

    rows = [int(y) for y in rows]
    with ThreadPoolExecutor(max_workers=min(len(rows), 8)) as ex:
        return dict(zip(rows, ex.map(one, rows)))


@pytest.fixture(scope="module")
def mesh_baseline(mcpt_mod, renderer, mesh):
    """Case A's baseline: the four calls with MCPT_ITEM_ORDER=0 (launch order, no split items, no
    stealing, combine_kernel: the path test_gpu_meshes.py pins at 64x48), read after 256, 768 and
    all 840 passes."""
    with pytest.MonkeyPatch.context() as mp:
        set_env(mp, MCPT_ITEM_ORDER=0)
        acc, snaps, launches, (stolen, _) = run_calls(mcpt_mod, renderer, mesh, MW, MH, A_CALLS, MB, MIOR, 1,
                                                      snap=(0, 2))
    assert launches == [1, 1, 1, 1] and stolen == 0
    return {256: snaps[0], 768: snaps[2], 840: acc}


def test_mesh_baseline_equals_oracle(oracle_mod, mesh, mesh_baseline):
    """The baseline against the oracle: after the first 256-pass call on rows that are a tile
    row's edges, an interior row and the three rows of the partial top tile row (every row also
    crosses the 5-px last tile column), and after all 840 passes on the partial tile row."""
    mv = oracle_mod.MeshView(mesh.mesh_buffers())
    ref = oracle_rows(oracle_mod, mesh, MW, MH, 256, MB, MIOR, A_ROWS, meshes=mv)
    assert all(ref[y].any() for y in A_ROWS)
    for y in A_ROWS:
        assert np.array_equal(bits(mesh_baseline[256][y]), bits(ref[y])), f"256 passes, row {y}"
    ref = oracle_rows(oracle_mod, mesh, MW, MH, 840, MB, MIOR, [128, 129, 130], meshes=mv)
    assert all(ref[y].any() for y in ref)
    for y in ref:
        assert np.array_equal(bits(mesh_baseline[840][y]), bits(ref[y])), f"840 passes, row {y}"


@pytest.mark.parametrize("name,env,steals,splits", [
    ("defaults", {}, True, True),                              # order, split items, stealing
    ("no stealing", {"MCPT_STEAL": 0}, False, True),           # combine_items_kernel
    ("no split items", {"MCPT_SPLIT_ITEMS": 0}, False, None),  # the order alone (stealing needs split launches)
], ids=["defaults", "no_stealing", "no_split_items"])
def test_mesh_partial_tiles_same_bits(mcpt_mod, renderer, mesh, mesh_baseline, monkeypatch, name, env, steals, splits):
    """Case A: 253 x 131, three 256-pass calls (4,352 items each: the second and third run the
    measured order with split items) and one of 72 passes (1,632 items, not whole segments: back to
    combine_kernel) equal the baseline over the whole frame, with stealing (combine_steal_kernel),
    without it (combine_items_kernel) and with the order alone."""
    set_env(monkeypatch, **env)
    acc, _, launches, (stolen, n_split) = run_calls(mcpt_mod, renderer, mesh, MW, MH, A_CALLS, MB, MIOR, 1)
    print(f"case A, {name}: slot 62 (stolen passes) {stolen}, slot 63 (items split) {n_split}, launches {launches}")
    # one launch per call: were the steal store's budget to cut one, the items per launch would
    # fall below the order's threshold
    assert launches == [1, 1, 1, 1]
    assert (stolen > 0) if steals else (stolen == 0)
    if splits:
        assert n_split > 0
    same = bits(acc) == bits(mesh_baseline[840])
    assert same.all(), f"{name}: {int((~same).any(axis=2).sum())} pixels differ, rows {np.unique(np.nonzero(~same)[0])[:12]}"


@pytest.fixture(scope="module")
def mesh_full_1408(mcpt_mod, renderer, mesh):
    """Case B's unsharded frame: the shard's two 704-pass calls on the whole frame, launch order."""
    with pytest.MonkeyPatch.context() as mp:
        set_env(mp, MCPT_ITEM_ORDER=0)
        acc, _, _, _ = run_calls(mcpt_mod, renderer, mesh, MW, MH, B_CALLS, MB, MIOR, 1)
    return acc


@pytest.fixture(scope="module")
def mesh_oracle_1408(oracle_mod, mesh):
    """Oracle rows of case B: the first and the last three local rows of the shard in both orders."""
    rows = sorted({int(B_ROWS[i]) for i in (0, 1, 2, -3, -2, -1)})
    return oracle_rows(oracle_mod, mesh, MW, MH, sum(B_CALLS), MB, MIOR, rows,
                       meshes=oracle_mod.MeshView(mesh.mesh_buffers()))


@pytest.mark.parametrize("reverse", [False, True])
def test_mesh_row_shard_same_bits(mcpt_mod, renderer, mesh, mesh_full_1408, mesh_oracle_1408, monkeypatch, reverse):
    """Case B: a row shard of 43 image rows (1, 4, ..., 127, and reversed): 6 tile rows, the last of
    3 local rows, 192 tiles x 22 segments = 4,224 items per call.  Order, split items and stealing
    equal launch order; the shard's rows equal the same image rows of the unsharded frame and the
    oracle's (the last three local rows, which form the partial tile row, and the first)."""
    rows = B_ROWS[::-1].copy() if reverse else B_ROWS
    assert len(rows) == 43 and len(rows) % 8 == 3
    set_env(monkeypatch)
    on, _, launches, (stolen, n_split) = run_calls(mcpt_mod, renderer, mesh, MW, MH, B_CALLS, MB, MIOR, 1, rows=rows)
    print(f"case B, reverse={reverse}: slot 62 (stolen passes) {stolen}, slot 63 (items split) {n_split}, launches {launches}")
    set_env(monkeypatch, MCPT_ITEM_ORDER=0)
    off, _, _, _ = run_calls(mcpt_mod, renderer, mesh, MW, MH, B_CALLS, MB, MIOR, 1, rows=rows)
    assert launches == [1, 1]
    assert stolen > 0
    assert on.shape == (43, MW, 3)
    assert np.array_equal(bits(on), bits(off))
    assert np.array_equal(bits(off), bits(mesh_full_1408[rows]))
    for i in (0, 40, 41, 42):
        ref = mesh_oracle_1408[int(rows[i])]
        assert ref.any()
        assert np.array_equal(bits(off[i]), bits(ref)), f"local row {i} (image row {rows[i]})"


def test_render_lanes_partial_tiles_same_bits(mcpt_mod, mesh, mesh_baseline, monkeypatch):
    """Case C: the render lanes (MCPT_OVERLAP, read when a Renderer is created) at 253 x 131 with
    order, split items and stealing on: three 256-pass calls, then the same 768 passes as one call
    cut into three sub-launches by the segment-sum budget (the lanes alternate inside the call).
    Lanes on and off give the same frames, and both are the baseline's after 768 passes."""
    ipv, iv = mcpt_mod.camera_canonical(MW, MH)
    set_env(monkeypatch)
    out = {}
    for ov in ("1", "0"):
        monkeypatch.setenv("MCPT_OVERLAP", ov)
        r = mcpt_mod.Renderer(0)
        try:
            r.set_traversal(1)
            r.upload_scene(mesh)
            r.set_target(MW, MH)
            for k in range(3):
                r.render(ipv, iv, 1 + 256 * k, 256, 0.0, MB, MIOR, 0)
            a, n = r.read_accum()
            r.clear_accum()
            r.set_partial_budget(MW * MH * 12 * 8)   # eight segments per sub-launch
            r.render(ipv, iv, 1, 768, 0.0, MB, MIOR, 0)
            launches = r.last_launch_count()
            b, n2 = r.read_accum()
        finally:
            r.close()
        assert n == 768 and n2 == 768 and launches == 3
        out[ov] = (a, b)
    for k in range(2):
        assert np.array_equal(bits(out["1"][k]), bits(out["0"][k])), k
        assert np.array_equal(bits(out["1"][k]), bits(mesh_baseline[768])), k


# a frame one tile wide: 17 tiles of 8x8, every one with the partial column, the last 3 px tall
E_W, E_H = 5, 131
E_ROWS = np.arange(3, 131, 12)   # 11 image rows: two tiles, of 8 and of 3 local rows


@pytest.mark.parametrize("rows,segs", [(None, 256), (E_ROWS, 2048)], ids=["frame", "row_shard"])
def test_mesh_one_tile_column_same_bits(mcpt_mod, mesh, monkeypatch, rows, segs):
    """Case E: 5 x 131, the mesh kernels' value store where the tile index is the tile row alone
    (tiles_x = 1) and no tile is whole.  One call of 2 x `segs` segments, cut by the segment-sum
    budget into two sub-launches of `segs` segments: 17 x 256 = 4,352 items on the frame, 2 x 2,048 =
    4,096 on an 11-row shard (kOrderMinItems: split-item launches, which steal; the second sub-launch
    starts at chunk `segs` and runs the order the first one measured).  The frame equals launch
    order's (MCPT_ITEM_ORDER=0: no stealing, combine_kernel) bit for bit."""
    n_rows = E_H if rows is None else len(rows)
    assert -(-n_rows // 8) * segs >= 4096
    r = mcpt_mod.Renderer(0)
    try:
        r.set_partial_budget(E_W * n_rows * 12 * segs)
        set_env(monkeypatch)
        on, _, launches, (stolen, n_split) = run_calls(mcpt_mod, r, mesh, E_W, E_H, [2 * segs * 32], MB, MIOR, 1, rows=rows)
        set_env(monkeypatch, MCPT_ITEM_ORDER=0)
        off, _, launches_off, (stolen_off, _) = run_calls(mcpt_mod, r, mesh, E_W, E_H, [2 * segs * 32], MB, MIOR, 1, rows=rows)
    finally:
        r.close()
    print(f"case E, {n_rows} rows: slot 62 (stolen passes) {stolen}, slot 63 (items split) {n_split}, launches {launches}")
    assert launches == [2] and launches_off == [2]
    assert stolen > 0 and stolen_off == 0
    assert on.shape == (n_rows, E_W, 3) and off.any()
    same = bits(on) == bits(off)
    assert same.all(), f"{int((~same).any(axis=2).sum())} pixels differ, rows {np.unique(np.nonzero(~same)[0])[:12]}"


D_W, D_H, D_B = 517, 253, 4   # 32 tile rows, the last 5 px tall; the last tile column 5 px wide at 16 and at 32
D_ROWS = [0, 100, 247, 248, 252]
# (scene, walk, tile width (mcpt_internal.h tile_w_for), passes per call of the tail-piece runs).
# Scenes 6, 8 and 3 all run 16-wide tiles (33 x 32 = 1,056 of them); scene 1 is a scene whose
# staged copy is too large for the 16-wide LDS kernel: the 32-wide one (17 x 32 = 544 tiles).
# Scene 8's tail-piece calls are 512 passes (16 segments in 4 groups: 4,224 items), the others'
# 1,024 (8 groups): its oracle rows cost 10 CPU-seconds per 1,024 passes each.
D_CASES = [(6, 1, 16, 1024), (8, 1, 16, 512), (3, 2, 16, 1024), (1, 1, 32, 1024)]


def oracle_pixel_rows(oracle_mod, sc, W, H, S, B, rows):
    """{image row: its W x 3 sums of passes 1..S}: the oracle's chunked sums for an explicit pixel
    list (bit-equal to its render() on those pixels), the pixels dealt to the CPUs."""
    import os
    prims, nodes, leaves = sc.buffers()
    ipv, iv = oracle_mod.camera(W, H)
    xy = np.array([(x, y) for y in rows for x in range(W)], np.int32)
    cpus = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    out = oracle_mod.render_pixels(prims, nodes, leaves, sc.depth(), ipv, iv, W, H, xy, 1, S, 0.0, B, 1.0, 0,
                                   n_threads=min(16, cpus))
    return dict(zip(rows, out.reshape(len(rows), W, 3)))


@pytest.mark.parametrize("mode", ["tail_pieces", "order"])
@pytest.mark.parametrize("scene_id,traversal,tile_w,tail_passes", D_CASES)
def test_scene_partial_tiles_same_bits(mcpt_mod, oracle_mod, renderer, monkeypatch, scene_id, traversal, tile_w,
                                       tail_passes, mode):
    """Case D: the scene kernels (scene 6 staged in LDS in 16-wide tiles, scene 1 in 32-wide ones,
    scene 8 read through L1/L2, scene 3 with the wave walk) at 517 x 253.  Three calls of at least
    4,096 items each, the second and third in the measured order — with MCPT_SEG_PER_ITEM=4 their
    cheapest items as tail pieces (seg_only) — equal launch order over the whole frame, and launch
    order equals the oracle after the first call on rows that include the partial top tile row."""
    sc = mcpt_mod.Scene.reference(scene_id)
    tail = mode == "tail_pieces"
    seg = {"MCPT_SEG_PER_ITEM": 4} if tail else {}
    passes = tail_passes if tail else 256
    tiles = -(-D_W // tile_w) * -(-D_H // 8)
    assert tiles * -(-(passes // 32) // (4 if tail else 1)) >= 4096   # kOrderMinItems: the order applies
    calls = [passes] * 3
    set_env(monkeypatch, MCPT_ITEM_ORDER=1, **seg)
    on, _, launches, _ = run_calls(mcpt_mod, renderer, sc, D_W, D_H, calls, D_B, 1.0, traversal)
    set_env(monkeypatch, MCPT_ITEM_ORDER=0, **seg)
    off, snaps, _, _ = run_calls(mcpt_mod, renderer, sc, D_W, D_H, calls, D_B, 1.0, traversal, snap=(0,))
    assert launches == [1, 1, 1]
    same = bits(on) == bits(off)
    assert same.all(), f"{int((~same).any(axis=2).sum())} pixels differ, rows {np.unique(np.nonzero(~same)[0])[:12]}"
    ref = oracle_pixel_rows(oracle_mod, sc, D_W, D_H, passes, D_B, D_ROWS)
    assert all(ref[y].any() for y in D_ROWS)
    for y in D_ROWS:
        assert np.array_equal(bits(snaps[0][y]), bits(ref[y])), f"scene {scene_id}, row {y}"
