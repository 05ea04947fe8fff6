"""Fuzz of pass stealing inside the waves of the LDS-scene render kernels against the
oracle: what tests/test_gpu_scene_steal.py (one frame size, aligned calls, three reference scenes,
default walk knobs, date 0) leaves out.

Every case is the same check (`check`): the calls rendered with stealing on and with MCPT_STEAL=0
and the oracle's frame for the same calls are equal bit for bit, MCPT_STEAL=0 reports no stolen
pass in debug slot 62, and -- wherever the launch can steal -- stealing on reports some.  The walk
is pinned per lane, the pass split off and MCPT_SEG_PER_ITEM set, so that a launch of two or more
segments of a staged scene is a stealing launch at any frame size.  There is no tolerance anywhere.

A. 64 random cases (`SEEDS`, `draw`): random scenes of all five primitive types small enough to be
   staged in LDS, half in 16-wide and half in 32-wide tiles; frames of 9..48 x 8..40, one in four a
   row shard; two or three consecutive calls that start and end inside 32-pass chunks; 1, 2, 3, 4 or
   8 segments per item; B, IOR, shader variant, a non-zero date in half of them; walk_exit and
   leaf_batch, which select the SUSPEND twins of the stealing kernels.  `test_seed_list_covers_the_kernels`
   (no GPU) counts over the seed list that all four STEAL instantiations get at least 16 cases.
B. Named edges: pass ranges whose head or tail chunk holds one or two passes, frames with one live
   column or row in their last wave or tile, variants 1 and 2, B = 0, a date, the SUSPEND twins on
   the reference scenes, stealing launches cut into sub-launches by the partial budget (a
   one-segment sub-launch, which does not steal, next to stealing ones), the render lanes, and two
   negative controls (a one-segment call; a scene too large to stage).

Which kernel a scene gets (`tile_width`) is restated here from the staged scene's size, not read
from the library.

Out of scope: stealing in the mesh kernels (it needs >= 4,096 work items for the item order;
tests/test_gpu_work_items.py covers it at 253 x 131, and plan::items aligns its launches), the
L1/L2 scene kernels (C4: they do not steal), anything that reads a kernel's assembly, and sanitizer
runs."""
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from fuzz_scenes import build_product, random_ops

gpu = pytest.mark.gpu

SLOT_STOLEN = 62
CHUNK = 32   # passes per accumulation chunk (= pass segment)
ENV = ("MCPT_ITEM_ORDER", "MCPT_SPLIT_ITEMS", "MCPT_STEAL", "MCPT_SEG_PER_ITEM", "MCPT_TAIL_PIECES", "MCPT_PASS_SPLIT",
       "MCPT_WALK_MIN_DONE", "MCPT_PARTIAL_BYTES")

# The random cases.  Debug slot 62 cannot be predicted on the CPU (a frame whose paths all have one
# length steals nothing), so the list is a literal: range(64) with the seeds that stole nothing on
# the first GPU run replaced by the next unused seed of their parity (at most 8).  An even seed draws
# a scene for 16-wide tiles, an odd one for 32-wide tiles.
# The three that stole nothing were frames of variants 1 and 2, whose passes all take one render
# round: the lanes of a wave end their passes together and claim their next units in lane order, so
# a wave whose live lanes repeat with a period that divides 64 hands every lane its own pixel again.
REPLACED = {   # seed taken out -> (seed put in, what the frame looked like)
    30: (64, "variant 2, 32 wide, a shard of 12 rows: every wave is full or has its first 32 lanes live"),
    48: (66, "variant 1, 48 x 16: every wave full"),
    51: (65, "variant 2, 48 x 18: every wave is full or has its first 16 lanes live"),
}
SEEDS = [REPLACED.get(s, (s,))[0] for s in range(64)]


def bits(a):
    return np.asarray(a, np.float32).view(np.uint32)


def segments(first, n):
    """Accumulation chunks that passes first .. first + n - 1 touch."""
    return (first + n - 2) // CHUNK - (first - 1) // CHUNK + 1


def staged_bytes(depth, n_prims):
    """The scene's copy in LDS: nodes (3 float4) and primitives (8 float4), leaves and type codes."""
    return (3 * ((2 << depth) - 1) + 8 * n_prims) * 16 + ((1 << depth) + n_prims) * 4


def tile_width(depth, n_prims):
    """16 / 32: the LDS-scene kernel's tile width for a scene; 0: not staged (the L1/L2 kernel)."""
    b = staged_bytes(depth, n_prims)
    return 16 if b <= 1968 else (32 if b <= 3584 else 0)


def test_tile_width_thresholds():
    d = lambda n: int(np.ceil(np.log2(n))) if n > 1 else 0   # noqa: E731
    assert staged_bytes(d(8), 8) == 1808 and staged_bytes(d(15), 15) == 3532 and staged_bytes(d(16), 16) == 3664
    assert [tile_width(d(n), n) for n in (1, 8, 9, 15, 16)] == [16, 16, 32, 32, 0]


def set_env(mp, seg, steal):
    for k in ENV:
        mp.delenv(k, raising=False)
    mp.setenv("MCPT_PASS_SPLIT", "0")
    mp.setenv("MCPT_SEG_PER_ITEM", str(seg))
    if not steal:
        mp.setenv("MCPT_STEAL", "0")


@pytest.fixture(scope="module")
def renderer(mcpt_mod):
    """The file's renderer, both render lanes' value stores filled.  A store only grows and is not
    cleared, and a fresh one may hold zeros, which a combine that summed slots its launch did not write
    (a chunk's passes before the call's first or after its last) would add without a trace.  Two
    aligned ten-segment stealing launches of the widest frame in 32-wide tiles, one per lane, are as
    large as any store the tests need and leave a pass's value in every slot of a live pixel."""
    r = mcpt_mod.Renderer(0)
    try:
        with pytest.MonkeyPatch.context() as mp:
            set_env(mp, 4, True)
            _, stolen, launches = gpu_frame(mcpt_mod, r, mcpt_mod.Scene.reference(1), 48, 40, None, [(1, 320), (321, 320)],
                                            8, 1.0, 0, 0.0)
        assert stolen > 0 and launches == [1, 1]
        yield r
    finally:
        r.close()


def gpu_frame(mcpt_mod, r, sc, W, H, rows, calls, B, ior, variant, date, walk_exit=-1, leaf_batch=-1):
    """The accumulator after `calls` ((first pass, passes) each), debug slot 62 of the run and each
    call's sub-launch count."""
    ipv, iv = mcpt_mod.camera_canonical(W, H)
    r.set_traversal(1)
    r.set_walk_exit(walk_exit)
    r.set_leaf_batch(leaf_batch)
    try:
        r.upload_scene(sc)
        if rows is None:
            r.set_target(W, H)
        else:
            r.set_target_rows(W, H, rows)
        r.debug_counters(reset=True)
        launches = []
        for first, n in calls:
            r.render(ipv, iv, first, n, date, B, ior, variant)
            launches.append(r.last_launch_count())
        acc, cnt = r.read_accum()
        stolen = int(r.debug_counters(reset=True)[SLOT_STOLEN])
    finally:
        r.set_traversal(0)
        r.set_walk_exit(-1)
        r.set_leaf_batch(-1)
    assert cnt == sum(n for _, n in calls)
    return acc, stolen, launches


_ORACLE = {}
_THREADS = min(16, len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1))


def oracle_frame(oracle_mod, key, buffers, W, H, rows, calls, B, ior, variant, date):
    """The oracle's frame after the same calls (`accum=` carried across them), computed once per case
    and left read-only; of a row shard only its rows, one single-threaded render per row side by side."""
    key = (key, W, H, None if rows is None else tuple(rows), tuple(calls), B, ior, variant, date)
    if key not in _ORACLE:
        prims, nodes, leaves, depth = buffers()
        ipv, iv = oracle_mod.camera(W, H)

        def run(**kw):
            acc = None
            for first, n in calls:
                acc, _ = oracle_mod.render(prims, nodes, leaves, depth, ipv, iv, W, H, first, n, date, B, ior, variant,
                                           accum=acc, **kw)
            return acc

        if rows is None:
            ref = run(n_threads=_THREADS)
        else:
            with ThreadPoolExecutor(max_workers=min(len(rows), _THREADS)) as ex:
                ref = np.stack(list(ex.map(lambda y: run(row_step=H, row_offset=int(y), n_threads=1)[int(y)], rows)))
        ref.setflags(write=False)
        _ORACLE[key] = ref
    return _ORACLE[key]


def reference_scene(mcpt_mod, oracle_mod, scene_id):
    """(oracle key, the product's scene, the oracle's own buffers of it)"""
    return (("reference", scene_id), mcpt_mod.Scene.reference(scene_id),
            lambda: oracle_mod.scene(scene_id)[:4])


def random_scene(mcpt_mod, seed, n_min, n_max):
    sc = build_product(mcpt_mod, random_ops(mcpt_mod, seed, n_min, n_max))
    return ("random", seed, n_min, n_max), sc, lambda: (*sc.buffers(), sc.depth())


def check(mcpt_mod, oracle_mod, r, mp, scene, W, H, calls, seg, B=8, ior=1.0, variant=0, date=0.0, rows=None,
          walk_exit=-1, leaf_batch=-1, stolen="some", lit=True, what=""):
    """The common check.  stolen: "some" (slot 62 > 0 with stealing on), "none" (== 0) or "any"
    (printed only).  lit=False: the frame is all zeros (B = 0), in both modes and in the oracle."""
    key, sc, buffers = scene
    what = (f"{what or key}: W {W} H {H} rows {rows} calls {calls} seg {seg} B {B} ior {ior} variant {variant} "
            f"date {date} walk_exit {walk_exit} leaf_batch {leaf_batch} depth {sc.depth()} prims {sc.nb_prim()}")
    args = (mcpt_mod, r, sc, W, H, rows, calls, B, ior, variant, date, walk_exit, leaf_batch)
    set_env(mp, seg, True)
    on, stolen_on, launches = gpu_frame(*args)
    set_env(mp, seg, False)
    off, stolen_off, _ = gpu_frame(*args)
    ref = oracle_frame(oracle_mod, key, buffers, W, H, rows, calls, B, ior, variant, date)
    print(f"{what}: slot 62 on {stolen_on}, off {stolen_off}")
    assert ref.shape == on.shape == off.shape, what
    if lit:
        assert ref.any(), what
    else:
        assert not ref.any() and not on.any() and not off.any(), what
    same = bits(on) == bits(off)
    assert same.all(), f"{int((~same).any(axis=2).sum())} pixels differ between stealing on and off ({what})"
    bad_off, bad_on = int((bits(off) != bits(ref)).sum()), int((bits(on) != bits(ref)).sum())
    assert bad_off == 0, f"MCPT_STEAL=0 differs from the oracle in {bad_off} channels ({what})"
    assert bad_on == 0, f"stealing differs from the oracle in {bad_on} channels ({what})"
    assert stolen_off == 0, what
    if stolen == "some":
        assert stolen_on > 0, f"nothing stolen ({what})"
    elif stolen == "none":
        assert stolen_on == 0, what
    return launches


# ---- A. random cases

def draw(mcpt_mod, seed):
    """Everything one random case renders, from its seed alone."""
    rng = np.random.default_rng(7000 + seed)
    scene = random_scene(mcpt_mod, seed, *((9, 14) if seed % 2 else (1, 7)))   # (+ a ground slab: <= 8 / <= 15)
    W, H = int(rng.integers(9, 49)), int(rng.integers(8, 41))
    rows = None
    if rng.random() < 0.25:
        rows = sorted(int(y) for y in rng.choice(H, min(int(rng.integers(3, 14)), H), replace=False))
    calls, first = [], int(rng.integers(1, 81))
    for _ in range(int(rng.integers(2, 4))):
        n = int(rng.integers(33, 151))
        calls.append((first, n))
        first += n
    return dict(scene=scene, W=W, H=H, rows=rows, calls=calls,
                seg=int(rng.choice([1, 2, 3, 4, 8])), B=int(rng.integers(1, 11)),
                ior=1.0 if rng.random() < 0.4 else float(rng.uniform(1.05, 2.0)),
                variant=0 if rng.random() < 0.7 else int(rng.integers(1, 3)),
                date=0.0 if rng.random() < 0.5 else float(np.float32(rng.uniform(0.05, 50.0))),
                walk_exit=int(rng.choice([-1, 0, 4, 16, 40])), leaf_batch=int(rng.choice([-1, 0, 2, 8, 64])))


def test_seed_list_covers_the_kernels(mcpt_mod):
    """No GPU: over the seed list both tile widths get at least 16 cases, and at least 16 of each width
    run the SUSPEND twin (walk_exit > 0 or leaf_batch > 0; the default -1 is 0 below BVH depth 8), so
    all four STEAL instantiations run; the plain twins run in the rest and in the named edges.  Every
    call touches two chunks or more, and the frames stay within 48 x 40 and 450 passes."""
    assert len(SEEDS) == len(set(SEEDS)) == 64 and len(REPLACED) <= 8
    assert all(s in range(64) and s not in SEEDS and new % 2 == s % 2 for s, (new, _) in REPLACED.items())
    n = {(tw, susp): 0 for tw in (16, 32) for susp in (False, True)}
    seen = {k: set() for k in ("seg", "variant", "depth")}
    shards = dated = 0
    for seed in SEEDS:
        c = draw(mcpt_mod, seed)
        sc = c["scene"][1]
        tw = tile_width(sc.depth(), sc.nb_prim())
        assert tw in (16, 32), (seed, sc.depth(), sc.nb_prim())
        assert sc.depth() < 8
        n[tw, c["walk_exit"] > 0 or c["leaf_batch"] > 0] += 1
        assert 9 <= c["W"] <= 48 and 8 <= c["H"] <= 40 and sum(k for _, k in c["calls"]) <= 450
        assert 1 <= c["calls"][0][0] <= 80 and len(c["calls"]) in (2, 3)
        for (first, k), nxt in zip(c["calls"], c["calls"][1:] + [None]):
            assert 33 <= k <= 150 and (first + k - 2) // 32 - (first - 1) // 32 >= 1
            assert nxt is None or nxt[0] == first + k
        assert c["rows"] is None or (3 <= len(c["rows"]) <= 13 and len(set(c["rows"])) == len(c["rows"]))
        shards += c["rows"] is not None
        dated += c["date"] != 0.0
        seen["seg"].add(c["seg"]); seen["variant"].add(c["variant"]); seen["depth"].add(sc.depth())
    print(n, seen, shards, dated)
    for tw in (16, 32):
        assert n[tw, False] + n[tw, True] >= 16 and n[tw, True] >= 16 and n[tw, False] >= 1, n
    assert seen["seg"] == {1, 2, 3, 4, 8} and seen["variant"] == {0, 1, 2} and {0, 4} <= seen["depth"]
    assert shards >= 8 and dated >= 16


@gpu
@pytest.mark.parametrize("seed", SEEDS)
def test_random_case(mcpt_mod, oracle_mod, renderer, monkeypatch, seed):
    check(mcpt_mod, oracle_mod, renderer, monkeypatch, what=f"seed {seed}", **draw(mcpt_mod, seed))


# ---- B. named edges

W0, H0 = 40, 24   # where the frame is not the subject (2.5 16-wide tiles, 1.25 32-wide ones)
TWO_CALLS = [(7, 100), (107, 60)]


def test_reference_scenes_tile_widths(mcpt_mod):
    """Scene 6 runs in 16-wide tiles, scene 1 in 32-wide ones."""
    s6, s1 = mcpt_mod.Scene.reference(6), mcpt_mod.Scene.reference(1)
    assert tile_width(s6.depth(), s6.nb_prim()) == 16 and tile_width(s1.depth(), s1.nb_prim()) == 32


@gpu
@pytest.mark.parametrize("seg", [1, 2, 4])
@pytest.mark.parametrize("first,n", [(1, 33), (32, 2), (31, 66), (20, 150), (33, 64), (5, 300)])
def test_pass_ranges(mcpt_mod, oracle_mod, renderer, monkeypatch, first, n, seg):
    """(1, 33): the second segment holds one pass; (32, 2): two segments of one pass; (31, 66): a
    two-pass head chunk; (33, 64): aligned, not from pass 1; (5, 300): ten segments, so four-segment
    items of 4, 4 and 2."""
    assert segments(first, n) >= 2
    # (32, 2) at one segment per item: every item is one pass per pixel, 64 units per wave that its
    # 64 lanes start with, so no unit is left to claim -- nothing can be stolen
    stolen = "none" if (first, n, seg) == (32, 2, 1) else "some"
    check(mcpt_mod, oracle_mod, renderer, monkeypatch, reference_scene(mcpt_mod, oracle_mod, 6), W0, H0, [(first, n)], seg,
          stolen=stolen)


@gpu
@pytest.mark.parametrize("scene_id", [6, 1])
@pytest.mark.parametrize("W,H", [(9, 9), (17, 8), (33, 9)])
def test_one_live_column_or_row(mcpt_mod, oracle_mod, renderer, monkeypatch, W, H, scene_id):
    """A second wave or tile with one live column (9, 17, 33 wide) or row (9 high)."""
    check(mcpt_mod, oracle_mod, renderer, monkeypatch, reference_scene(mcpt_mod, oracle_mod, scene_id), W, H, TWO_CALLS, 2)


@gpu
@pytest.mark.parametrize("W,H", [(7, 3), (1, 1)])
def test_tiny_frames(mcpt_mod, oracle_mod, renderer, monkeypatch, W, H):
    """21 pixels and one: at 1 x 1 one lane renders every unit, so slot 62 may be 0 (printed)."""
    check(mcpt_mod, oracle_mod, renderer, monkeypatch, reference_scene(mcpt_mod, oracle_mod, 6), W, H, TWO_CALLS, 2,
          stolen="any")


@gpu
@pytest.mark.parametrize("scene_id", [6, 1])
@pytest.mark.parametrize("variant", [1, 2])
def test_variants(mcpt_mod, oracle_mod, renderer, monkeypatch, variant, scene_id):
    """Variants 1 and 2 at B = 3.  Their passes take one render round each, so the lanes of a full wave
    claim in step and each gets its own pixel again (40 x 24 steals nothing); at 37 x 21 the last
    waves have 5 live columns or 5 live rows, the units of the pixels outside are skipped, and the
    live lanes render each other's pixels."""
    check(mcpt_mod, oracle_mod, renderer, monkeypatch, reference_scene(mcpt_mod, oracle_mod, scene_id), 37, 21, TWO_CALLS, 2,
          B=3, variant=variant)


@gpu
def test_no_bounces(mcpt_mod, oracle_mod, renderer, monkeypatch):
    """Variant 0 with B = 0: no pass runs (`run` is false), the store holds zeros, the frame is black."""
    check(mcpt_mod, oracle_mod, renderer, monkeypatch, reference_scene(mcpt_mod, oracle_mod, 6), W0, H0, TWO_CALLS, 2,
          B=0, stolen="any", lit=False)


@gpu
def test_date(mcpt_mod, oracle_mod, renderer, monkeypatch):
    """A stolen pass's seed takes the date with the pixel's (u, v) from LDS."""
    check(mcpt_mod, oracle_mod, renderer, monkeypatch, reference_scene(mcpt_mod, oracle_mod, 6), W0, H0, TWO_CALLS, 2,
          date=0.37)


@gpu
@pytest.mark.parametrize("ior", [1.0, 1.5])
@pytest.mark.parametrize("walk_exit,leaf_batch", [(8, 0), (0, 8), (40, 64)])
@pytest.mark.parametrize("scene_id", [6, 1])
def test_suspend_twins(mcpt_mod, oracle_mod, renderer, monkeypatch, scene_id, walk_exit, leaf_batch, ior):
    """render_kernel<.., LDSS, SUSPEND, 16 | 32, .., STEAL>: a stolen pass starts beside suspended walks."""
    check(mcpt_mod, oracle_mod, renderer, monkeypatch, reference_scene(mcpt_mod, oracle_mod, scene_id), W0, H0, TWO_CALLS, 2,
          ior=ior, walk_exit=walk_exit, leaf_batch=leaf_batch)


@gpu
@pytest.mark.parametrize("seg", [1, 2, 4])
@pytest.mark.parametrize("budget", [2, 3])
@pytest.mark.parametrize("first,n", [(20, 150), (20, 140)])
def test_sub_launches(mcpt_mod, oracle_mod, renderer, monkeypatch, first, n, budget, seg):
    """Stealing launches cut by the partial budget (2 and 3 segments of W x H x 12 bytes).  Passes
    20..169 touch six chunks (sub-launches of 2, 2, 2 and 3, 3 segments), passes 20..159 five: 2, 2, 1
    and 3, 2, so at budget 2 the last sub-launch has one segment and does not steal beside two that do."""
    W, H = 24, 16
    renderer.set_partial_budget(budget * W * H * 12)
    try:
        launches = check(mcpt_mod, oracle_mod, renderer, monkeypatch, reference_scene(mcpt_mod, oracle_mod, 6), W, H,
                         [(first, n)], seg)
    finally:
        renderer.set_partial_budget(4 << 30)   # (the default)
    assert segments(20, 150) == 6 and segments(20, 140) == 5
    assert launches == [-(-segments(first, n) // budget)]


@gpu
def test_one_segment_steals_nothing(mcpt_mod, oracle_mod, renderer, monkeypatch):
    check(mcpt_mod, oracle_mod, renderer, monkeypatch, reference_scene(mcpt_mod, oracle_mod, 6), W0, H0, [(1, 32)], 2,
          stolen="none")


@gpu
def test_unstaged_scene_steals_nothing(mcpt_mod, oracle_mod, renderer, monkeypatch):
    """16 primitives or more: the L1/L2 kernel, which does not steal, at several segments per item."""
    scene = random_scene(mcpt_mod, 3, 16, 24)
    assert tile_width(scene[1].depth(), scene[1].nb_prim()) == 0
    check(mcpt_mod, oracle_mod, renderer, monkeypatch, scene, W0, H0, TWO_CALLS, 2, stolen="none")


@gpu
def test_render_lanes(mcpt_mod, oracle_mod, monkeypatch):
    """Three consecutive unaligned calls with the render lanes on and off, each in a fresh Renderer:
    with the lanes on a lane's value store is used twice."""
    calls = [(23, 70), (93, 45), (138, 101)]
    assert all(segments(f, n) >= 2 and (f - 1) % CHUNK and (f + n - 1) % CHUNK for f, n in calls)
    key, sc, buffers = reference_scene(mcpt_mod, oracle_mod, 6)
    set_env(monkeypatch, 2, True)
    out = {}
    for lanes in (True, False):
        r = mcpt_mod.Renderer(0)
        try:
            r.set_render_lanes(lanes)
            out[lanes] = gpu_frame(mcpt_mod, r, sc, W0, H0, None, calls, 8, 1.0, 0, 0.0)
        finally:
            r.close()
    ref = oracle_frame(oracle_mod, key, buffers, W0, H0, None, calls, 8, 1.0, 0, 0.0)
    assert ref.any()
    for lanes in (True, False):
        acc, stolen, _ = out[lanes]
        assert stolen > 0, f"render lanes {lanes}"
        assert np.array_equal(bits(acc), bits(ref)), f"render lanes {lanes}"
