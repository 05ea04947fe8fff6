"""Adaptive sampling of 8x8 blocks, restated in numpy float32 on top of
test_stats_restate's error / record, so that tests/test_gpu_adaptive.py can pin the HIP kernels bit
for bit.  CPU checks of the restatement itself on synthetic states: block maxima, retirement,
monotone active sets, stale map entries, the record over mixed fresh and stored values, samples and
the resolve."""
import numpy as np

import test_stats_restate as st

F = np.float32
bits = st.bits


def grid(W, rows):
    """(blocks_x, blocks_y) of a local grid of `rows` rows."""
    return (W + 7) // 8, (rows + 7) // 8


def block_ids(W, rows):
    """(rows, W) int: every local pixel's block id by * blocks_x + bx."""
    bx, _ = grid(W, rows)
    return (np.arange(rows)[:, None] // 8) * bx + np.arange(W)[None, :] // 8


def begin(W, rows, p0, min_passes=0):
    """Adaptive mode on: every block active with zero passes; p0 = the accumulator's pass count."""
    bx, by = grid(W, rows)
    return {"W": W, "rows": rows, "p0": int(p0), "min_passes": int(min_passes),
            "active": np.ones(bx * by, bool), "passes": np.zeros(bx * by, np.int64),
            "map": np.zeros((rows, W, 2), np.float32), "ids": block_ids(W, rows)}


def active_list(ad):
    return np.flatnonzero(ad["active"]).astype(np.int32)


def rendered(ad, n, every_block=False):
    """n passes went into the active blocks (render_adaptive) or into every block (plain render)."""
    if every_block:
        ad["passes"] += n
    else:
        ad["passes"][ad["active"]] += n


def select(ad, state, threshold, mu_floor):
    """§3.9's select on a test_stats_restate state: the error map entries of the active blocks'
    pixels, the new active set and the record (fresh values for active blocks, stored map values
    for retired ones)."""
    se, r, _ = st.error(state, mu_floor)
    fresh = ad["active"][ad["ids"]]                      # pixels of blocks active before the select
    ad["map"][fresh, 0] = se[fresh]
    ad["map"][fresh, 1] = r[fresh]
    n_blocks = ad["active"].size
    bmax = np.zeros(n_blocks, np.float32)                # r >= 0; every block holds an in-frame pixel
    np.maximum.at(bmax, ad["ids"].ravel(), ad["map"][..., 1].ravel())
    stay = ad["active"] & ((bmax > F(threshold)) | (ad["passes"] < ad["min_passes"]))
    ad["active"] = stay
    rr = ad["map"][..., 1]
    with np.errstate(all="ignore"):
        q = (rr * st.Q_SCALE).astype(np.uint32)
    rec = st.record(rr, q, threshold)
    rec["passes"], rec["batches"] = state["N"], state["B"]
    rec["n_active_blocks"], rec["n_blocks"] = int(stay.sum()), int(n_blocks)
    rec["samples"] = int(counts(ad).astype(np.int64).sum())
    return rec


def counts(ad):
    """(rows, W) int32: a pixel's sample count p0 + its block's passes."""
    return (ad["p0"] + ad["passes"][ad["ids"]]).astype(np.int32)


def resolve(accum, cnt):
    """accum / (float)count per channel (mcpt_average's division with the pixel's own count)."""
    with np.errstate(all="ignore"):
        out = np.asarray(accum, np.float32) / np.asarray(cnt).astype(np.float32)[..., None]
    assert out.dtype == np.float32
    return out


# ---- CPU checks of the restatement -------------------------------------------------------------
def _state(rows, W, sigma, n_batches=4, n=8, seed=0, mean=1.0):
    """A statistics state from synthetic accumulator snapshots: per pass a pixel gains
    mean + sigma[pixel] * gauss on every channel."""
    rng = np.random.default_rng(seed)
    acc = np.zeros((rows, W, 3), np.float32)
    s = st.begin(acc)
    snaps = []
    for _ in range(n_batches):
        inc = (n * mean + np.sqrt(n) * sigma * rng.standard_normal((rows, W))).astype(np.float32)
        acc = (acc + inc[..., None]).astype(np.float32)
        st.batch(s, acc, n)
        snaps.append(acc.copy())
    return s, acc


def test_grid_and_block_ids_with_partial_blocks():
    assert grid(45, 37) == (6, 5) and grid(1, 1) == (1, 1) and grid(8, 8) == (1, 1) and grid(9, 16) == (2, 2)
    ids = block_ids(45, 37)
    assert ids[0, 0] == 0 and ids[7, 7] == 0 and ids[8, 0] == 6 and ids[0, 8] == 1
    assert ids[36, 44] == 29 and (ids[32:, 40:] == 29).all()       # the 5 x 5 corner block
    assert np.array_equal(np.unique(ids), np.arange(30))


def test_block_max_and_retirement_at_partial_edges():
    """45x37: noise only in the one-lane-wide right column and in the top (last) partial row block;
    exactly the blocks that hold such a pixel stay."""
    W, rows = 45, 37
    sigma = np.zeros((rows, W))
    sigma[3, 44] = 2.0          # block 5 (right edge, 5 columns wide)
    sigma[36, 10] = 2.0         # block 25 (last block row, 5 rows high)
    sigma[36, 44] = 2.0         # block 29 (the corner)
    s, _ = _state(rows, W, sigma)
    ad = begin(W, rows, 0)
    rendered(ad, 32)
    rec = select(ad, s, 0.05, 0.01)
    assert active_list(ad).tolist() == [5, 25, 29]
    assert rec["n_active_blocks"] == 3 and rec["n_blocks"] == 30 and rec["n_above"] == 3
    assert rec["samples"] == 32 * W * rows and rec["n_px"] == W * rows
    _, r, q = st.error(s, 0.01)
    ref = st.record(r, q, 0.05)           # first select: every block fresh = the whole-frame record
    assert all(rec[k] == ref[k] for k in ("n_px", "n_above", "sum_q", "mean_r"))
    assert bits(rec["max_r"]) == bits(ref["max_r"])


def test_monotone_sets_stale_map_and_mixed_record():
    """A retired block keeps its map entries and its count, never returns (even when its pixels
    would now exceed the threshold), and the record mixes stored and fresh values."""
    W, rows = 20, 12
    quiet = np.zeros((rows, W)); quiet[:, 8:] = 1.0
    s1, acc1 = _state(rows, W, quiet, seed=1)
    ad = begin(W, rows, 5)
    rendered(ad, 32)
    select(ad, s1, 0.02, 0.01)
    first = active_list(ad).tolist()
    assert first == [1, 2, 4, 5]          # blocks 0 and 3 (columns 0..7) retired
    stale = ad["map"].copy()
    loud = np.full((rows, W), 3.0)        # now every pixel is noisy, the retired ones too
    s2, _ = _state(rows, W, loud, seed=2)
    rendered(ad, 32)
    rec = select(ad, s2, 0.02, 0.01)
    assert set(active_list(ad).tolist()) <= set(first) and not ad["active"][[0, 3]].any()
    assert np.array_equal(bits(ad["map"][:, :8]), bits(stale[:, :8]))          # stale entries kept
    se, r, q = st.error(s2, 0.01)
    assert np.array_equal(bits(ad["map"][:, 8:, 1]), bits(r[:, 8:]))           # fresh entries written
    a = st.record(stale[:, :8, 1], (stale[:, :8, 1] * st.Q_SCALE).astype(np.uint32), 0.02)
    b = st.record(r[:, 8:], q[:, 8:], 0.02)
    ref = st.add_records(a, b)
    assert all(rec[k] == ref[k] for k in ("n_px", "n_above", "sum_q", "mean_r"))
    assert bits(rec["max_r"]) == bits(F(ref["max_r"]))
    c = counts(ad)
    assert (c[:, :8] == 5 + 32).all() and (c[:, 8:] == 5 + 64).all()
    assert rec["samples"] == int(c.sum()) == 12 * 8 * 37 + 12 * 12 * 69
    rendered(ad, 4, every_block=True)     # a plain render reaches the retired blocks too
    assert (counts(ad)[:, :8] == 41).all() and (counts(ad)[:, 8:] == 73).all()


def test_one_pixel_frame():
    s, acc = _state(1, 1, np.full((1, 1), 0.5))
    ad = begin(1, 1, 0)
    rendered(ad, 32)
    rec = select(ad, s, 1e-6, 0.01)
    assert rec["n_blocks"] == 1 and rec["n_active_blocks"] == 1 and rec["n_px"] == 1 and rec["samples"] == 32
    rec = select(ad, s, 60.0, 0.01)
    assert rec["n_active_blocks"] == 0 and active_list(ad).size == 0
    assert np.array_equal(bits(resolve(acc, counts(ad))), bits(acc / F(32)))


def test_block_whose_only_pixel_overflowed():
    """9x1: block 1 holds one in-frame pixel; overflowed, it counts r = 64 and keeps the block."""
    s, acc = _state(1, 9, np.zeros((1, 9)))
    s["S2"][0, 8] = np.inf
    ad = begin(9, 1, 0)
    rendered(ad, 32)
    rec = select(ad, s, 63.0, 0.01)
    assert active_list(ad).tolist() == [1]
    assert bits(rec["max_r"]) == bits(st.R_MAX) and rec["n_above"] == 1
    assert bits(ad["map"][0, 8, 1]) == bits(F(64.0))


def test_min_passes_holds_a_converged_block():
    s, _ = _state(8, 16, np.zeros((8, 16)))
    ad = begin(16, 8, 0, min_passes=40)
    rendered(ad, 32)
    rec = select(ad, s, 0.5, 0.01)
    assert rec["n_above"] == 0 and rec["n_active_blocks"] == 2          # converged, but 32 < 40
    rendered(ad, 8)
    rec = select(ad, s, 0.5, 0.01)
    assert rec["n_active_blocks"] == 0 and rec["samples"] == 40 * 128


def test_resolve_divides_by_the_pixels_own_count():
    acc = np.arange(2 * 16 * 3, dtype=np.float32).reshape(2, 16, 3) / F(7)
    ad = begin(16, 2, 3)
    ad["active"][0] = False
    rendered(ad, 10)
    c = counts(ad)
    assert (c[:, :8] == 3).all() and (c[:, 8:] == 13).all()
    out = resolve(acc, c)
    assert np.array_equal(bits(out[:, :8]), bits(acc[:, :8] / F(3)))
    assert np.array_equal(bits(out[:, 8:]), bits(acc[:, 8:] / F(13)))


def test_binding_declares_the_adaptive_calls():
    """The binding's table carries every adaptive entry point of include/mcpt.h."""
    import os
    import re
    here = os.path.dirname(os.path.abspath(__file__))
    hdr = open(os.path.join(here, "..", "include", "mcpt.h")).read()
    py = open(os.path.join(here, "..", "montecarlo-pathtracing_amd", "mcpt", "__init__.py")).read()
    names = set(re.findall(r"^int (mcpt_(?:adaptive_\w+|render_adaptive|read_sample_counts|read_resolved|"
                           r"read_active_blocks|last_adaptive_ms))\(", hdr, re.M))
    assert len(names) == 9, names
    for n in names:
        assert f'"{n}"' in py, n
    assert "MCPT_ERR_NO_ADAPTIVE = -9" in hdr
