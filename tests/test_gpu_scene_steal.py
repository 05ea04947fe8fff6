"""Pass stealing inside the waves of the LDS-scene render kernel: the frame with
stealing on is the frame with MCPT_STEAL=0 and the oracle's, bit for bit, and debug slot 62 shows
that passes were in fact rendered by other lanes than their pixel's.

The frames are 40 x 24: 16-wide tiles (scene 6) are partial in x (40 = 2.5 tiles), 32-wide ones
(scenes 1 and 2) too, and no tile is partial in y, so the row shard of five rows adds the partial
tile row: waves with 8 live pixels of 64.  Passes per call are 96 (three chunks) and 160 (five: with
two and four segments per item an item boundary falls inside the call); every run is two calls, from
pass 1 and from pass 97, so the second adds into a non-zero accumulator.  The launches are small, so
the pass split is pinned off (it would run one pass per item: nothing to steal) and the walk is
pinned per lane (AUTO's trials do not steal).  Bits are compared everywhere; there is no tolerance."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

W, H = 40, 24
SLOT_STOLEN = 62
ENV = ("MCPT_ITEM_ORDER", "MCPT_SPLIT_ITEMS", "MCPT_STEAL", "MCPT_SEG_PER_ITEM", "MCPT_TAIL_PIECES", "MCPT_PASS_SPLIT")
SHARD_ROWS = [1, 5, 10, 17, 22]


def bits(a):
    return np.asarray(a, np.float32).view(np.uint32)


def set_env(mp, seg, steal):
    for k in ENV:
        mp.delenv(k, raising=False)
    mp.setenv("MCPT_PASS_SPLIT", "0")
    mp.setenv("MCPT_SEG_PER_ITEM", str(seg))
    if not steal:
        mp.setenv("MCPT_STEAL", "0")


@pytest.fixture(scope="module")
def renderer(mcpt_mod):
    r = mcpt_mod.Renderer(0)
    yield r
    r.close()


def calls_of(n, k=2):
    """k calls of n passes: from pass 1, then from pass 97, 193, ..."""
    return [(1 + 96 * i, n) for i in range(k)]


def gpu_frame(mcpt_mod, r, scene_id, calls, B, ior, rows=None):
    """The accumulator after `calls` ((first pass, passes) each) and debug slot 62 of the run."""
    ipv, iv = mcpt_mod.camera_canonical(W, H)
    r.set_traversal(1)
    try:
        r.upload_scene(mcpt_mod.Scene.reference(scene_id))
        if rows is None:
            r.set_target(W, H)
        else:
            r.set_target_rows(W, H, rows)
        r.debug_counters(reset=True)
        for first, n in calls:
            r.render(ipv, iv, first, n, 0.0, B, ior, 0)
        acc, cnt = r.read_accum()
        stolen = int(r.debug_counters(reset=True)[SLOT_STOLEN])
    finally:
        r.set_traversal(0)
    assert cnt == sum(n for _, n in calls)
    return acc, stolen


_ORACLE = {}


def oracle_frame(oracle_mod, scene_id, calls, B, ior):
    """The oracle's whole frame after the same calls, computed once per (scene, calls, B, ior)."""
    key = (scene_id, tuple(calls), B, ior)
    if key not in _ORACLE:
        prims, nodes, leaves, depth, _ = oracle_mod.scene(scene_id)
        ipv, iv = oracle_mod.camera(W, H)
        acc = None
        for first, n in calls:
            acc, _ = oracle_mod.render(prims, nodes, leaves, depth, ipv, iv, W, H, first, n, 0.0, B, ior, 0, accum=acc)
        acc.setflags(write=False)
        _ORACLE[key] = acc
    return _ORACLE[key]


def on_off_oracle(mcpt_mod, oracle_mod, r, mp, scene_id, seg, calls, B=8, ior=1.0, rows=None):
    set_env(mp, seg, True)
    on, stolen_on = gpu_frame(mcpt_mod, r, scene_id, calls, B, ior, rows)
    set_env(mp, seg, False)
    off, stolen_off = gpu_frame(mcpt_mod, r, scene_id, calls, B, ior, rows)
    ref = oracle_frame(oracle_mod, scene_id, calls, B, ior)
    if rows is not None:
        ref = ref[rows]
    print(f"scene {scene_id} seg {seg} calls {calls} B {B} ior {ior}: slot 62 on {stolen_on}, off {stolen_off}")
    assert ref.any()
    same = bits(on) == bits(off)
    assert same.all(), f"{int((~same).any(axis=2).sum())} pixels differ between stealing on and off"
    assert np.array_equal(bits(off), bits(ref)), "MCPT_STEAL=0 differs from the oracle"
    assert np.array_equal(bits(on), bits(ref)), "stealing differs from the oracle"
    assert stolen_on > 0 and stolen_off == 0


@pytest.mark.parametrize("passes", [96, 160])
@pytest.mark.parametrize("seg", [1, 2, 4])
def test_scene6_steal_same_bits(mcpt_mod, oracle_mod, renderer, monkeypatch, seg, passes):
    on_off_oracle(mcpt_mod, oracle_mod, renderer, monkeypatch, 6, seg, calls_of(passes))


def test_refraction_inner_walk(mcpt_mod, oracle_mod, renderer, monkeypatch):
    """IOR 1.5: stolen passes run the inner-walk phase, whose saved N / P rows stay the rendering lane's."""
    on_off_oracle(mcpt_mod, oracle_mod, renderer, monkeypatch, 6, 2, calls_of(96), ior=1.5)


@pytest.mark.parametrize("scene_id", [1, 2])
def test_other_lds_scenes(mcpt_mod, oracle_mod, renderer, monkeypatch, scene_id):
    """Scenes 1 and 2: staged copies too large for 16-wide tiles, so four waves per workgroup."""
    on_off_oracle(mcpt_mod, oracle_mod, renderer, monkeypatch, scene_id, 2, calls_of(96))


def test_one_bounce(mcpt_mod, oracle_mod, renderer, monkeypatch):
    """B = 1: every non-emissive hit ends black at the first bounce (B = 8 is every other case)."""
    on_off_oracle(mcpt_mod, oracle_mod, renderer, monkeypatch, 6, 2, calls_of(96), B=1)


def test_row_shard(mcpt_mod, oracle_mod, renderer, monkeypatch):
    """Five scattered rows of the 40-wide frame: one tile row of five local rows, 8-40 live pixels per wave."""
    on_off_oracle(mcpt_mod, oracle_mod, renderer, monkeypatch, 6, 2, calls_of(96), rows=SHARD_ROWS)


def test_render_lanes(mcpt_mod, oracle_mod, monkeypatch):
    """Three consecutive 96-pass calls with the render lanes on and off: each lane's own value buffer is
    used twice with the lanes on.  Same frames, and the oracle's."""
    calls = calls_of(96, 3)
    set_env(monkeypatch, 2, True)
    out = {}
    for lanes in (True, False):
        r = mcpt_mod.Renderer(0)
        try:
            r.set_render_lanes(lanes)
            out[lanes] = gpu_frame(mcpt_mod, r, 6, calls, 8, 1.0)
        finally:
            r.close()
    ref = oracle_frame(oracle_mod, 6, calls, 8, 1.0)
    for lanes in (True, False):
        acc, stolen = out[lanes]
        assert stolen > 0
        assert np.array_equal(bits(acc), bits(ref)), f"render lanes {lanes}"
