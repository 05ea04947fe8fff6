"""Where a pixel's sample count comes from: the count plane of a counted gather,
else p0 + the block's passes while the adaptive mode is on, else the context's pass count.  Every
call that reads a count must see the same one: mcpt_read_sample_counts, the fourth word of
mcpt_pack_counted_device's records, the plane a second frame gets from mcpt_gather_rows_counted,
mcpt_read_resolved and the first step of mcpt_denoise_resolved.

Scene 6 at 24x19 (3 x 3 blocks, partial on both axes), 4 bounces, calls of 4 passes.  The threshold
is a value between two blocks' largest r of the GPU's own map after the second batch, so the select
retires some blocks but not all; that is asserted on the select's record.  Everything is compared
bit for bit.  The second test sends two non-contiguous row shards through both gathers (in process,
and pack + load with FrameGather's padded layout, whose index is checked against
dist.frame_row_index on a partition it knows) and compares the two frames."""
import numpy as np
import pytest
import torch

import test_adaptive_restate as ar
import test_denoise_restate as rs
from test_gpu_adaptive import BOUNCES, FLOOR
from test_gpu_adaptive_pipeline import new_renderer, status

pytestmark = pytest.mark.gpu

bits = rs.bits
W, H, N = 24, 19, 4
NO_ADAPTIVE = -9
ROWS_A = list(range(0, 5)) + list(range(8, 11)) + list(range(16, 19))
ROWS_B = [y for y in range(H) if y not in ROWS_A]


def split_threshold(r, rows):
    """A value between two blocks' largest r of the map r (rows x W)."""
    ids = ar.block_ids(W, rows)
    bmax = np.zeros(ids.max() + 1, np.float32)
    np.maximum.at(bmax, ids.ravel(), r.ravel())
    v = np.unique(bmax)
    assert v.size >= 2, v
    k = v.size // 2
    return float(np.float32(0.5) * (v[k - 1] + v[k]))


def adaptive(mcpt_mod, rows=None):
    """An adaptive render of three calls whose second select retires some blocks (not asserted here);
    returns (renderer, camera, the select's record)."""
    r, cam = new_renderer(mcpt_mod, rows, W, H)
    r.stats_begin()
    r.adaptive_begin(0)
    for first in (1, 1 + N):
        r.render_adaptive(cam[0], cam[1], first, N, 0.0, BOUNCES, 1.0, 0)
    r.adaptive_select(1e-30, FLOOR)                       # every pixel's r into the map
    n_rows = H if rows is None else len(rows)
    rec = r.adaptive_select(split_threshold(r.read_error_map()[..., 1], n_rows), FLOOR)
    r.render_adaptive(cam[0], cam[1], 1 + 2 * N, N, 0.0, BOUNCES, 1.0, 0)
    return r, cam, rec


def packed_counts(r):
    """(accumulator words, counts) of mcpt_pack_counted_device's records."""
    buf = torch.zeros((r.n_local_rows, W, 4), dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    r.pack_counted_device(buf.data_ptr(), r.n_local_rows * W * 16)
    r.synchronize()
    host = buf.cpu().numpy()
    return host[..., :3].view(np.uint32), host[..., 3]


def resolve(acc, cnt):
    return acc / cnt.astype(np.float32)[..., None]


@pytest.fixture(scope="module")
def contexts(mcpt_mod):
    made = []
    a, cam = new_renderer(mcpt_mod, None, W, H)                          # (a) uniform
    made.append(a)
    for first in (1, 1 + N, 1 + 2 * N):
        a.render(cam[0], cam[1], first, N, 0.0, BOUNCES, 1.0, 0)
    b, _, rec = adaptive(mcpt_mod)                                       # (b) adaptive, blocks retired
    made.append(b)
    c, _ = new_renderer(mcpt_mod, None, W, H)                            # (c) the counts are the plane
    made.append(c)
    c.gather_rows_counted([b])
    yield dict(a=a, b=b, c=c, cam=cam, rec=rec)
    for r in made:
        r.close()


@pytest.mark.parametrize("which", ["a", "b", "c"])
def test_one_count_everywhere(mcpt_mod, contexts, which):
    r, cam, rec = contexts[which], contexts["cam"], contexts["rec"]
    assert 0 < rec["n_active_blocks"] < rec["n_blocks"], rec
    acc, n = r.read_accum()
    assert n == 3 * N
    if which == "a":
        cnt = np.full((H, W), 3 * N, np.int32)
        assert f"({NO_ADAPTIVE})" in status(mcpt_mod, r.read_sample_counts)
        assert f"({NO_ADAPTIVE})" in status(mcpt_mod, r.read_resolved)
    else:
        cnt = r.read_sample_counts()
        assert sorted(np.unique(cnt).tolist()) == [2 * N, 3 * N]
        assert np.array_equal(cnt, contexts["b"].read_sample_counts())
    words, packed = packed_counts(r)
    assert np.array_equal(packed, cnt) and np.array_equal(words, bits(acc))
    want = resolve(acc, cnt)
    frame, _ = new_renderer(mcpt_mod, None, W, H)
    try:
        frame.gather_rows_counted([r])
        assert np.array_equal(frame.read_sample_counts(), cnt)
        assert np.array_equal(bits(frame.read_accum()[0]), bits(acc)) and frame.read_accum()[1] == 3 * N
        for x in (frame,) if which == "a" else (r, frame):
            res = x.read_resolved()
            assert np.array_equal(bits(res), bits(want))
            x.render_guides(*cam)
            assert np.array_equal(bits(x.denoise_resolved(0, 1.5, 0.75)), bits(res))
    finally:
        frame.close()


def padded_index(row_sets, n_rows):
    """FrameGather's layout: shard k at rows k * m .. of [n * m, W, ...] (m the longest shard)."""
    m = max(len(rows) for rows in row_sets)
    src = np.full(n_rows, -1, np.int64)
    for k, rows in enumerate(row_sets):
        src[np.asarray(rows)] = k * m + np.arange(len(rows))
    assert (src >= 0).all()
    return m, src


def test_non_contiguous_shards_both_routes(mcpt_mod):
    from mcpt.dist import frame_row_index, local_rows
    balanced = [local_rows(H, 8, 2, k, "balanced").tolist() for k in range(2)]
    assert np.array_equal(padded_index(balanced, H)[1], frame_row_index(H, 8, 2, "balanced"))
    row_sets = [ROWS_A, ROWS_B]
    assert sorted(ROWS_A + ROWS_B) == list(range(H))
    m, src = padded_index(row_sets, H)
    made = []
    try:
        shards, recs = [], []
        for rows in row_sets:
            r, _, rec = adaptive(mcpt_mod, rows)
            made.append(r)
            shards.append(r)
            recs.append(rec)
        assert any(0 < rec["n_active_blocks"] < rec["n_blocks"] for rec in recs), recs
        a, _ = new_renderer(mcpt_mod, None, W, H)
        b, _ = new_renderer(mcpt_mod, None, W, H)
        made += [a, b]
        a.gather_rows_counted(shards)
        a.gather_error_map(shards)
        rows_buf = torch.zeros((2 * m, W, 4), dtype=torch.int32, device="cuda:0")
        map_buf = torch.zeros((2 * m, W, 2), dtype=torch.int32, device="cuda:0")
        torch.cuda.synchronize()
        for k, s in enumerate(shards):
            s.pack_counted_device(rows_buf[k * m].data_ptr(), s.n_local_rows * W * 16)
            s.pack_error_map_device(map_buf[k * m].data_ptr(), s.n_local_rows * W * 8)
            s.synchronize()
        b.load_rows_counted(rows_buf.data_ptr(), rows_buf.shape[0], src.astype(np.int32), max(s.pass_count() for s in shards))
        b.load_rows_error_map(map_buf.data_ptr(), map_buf.shape[0], src.astype(np.int32))
        acc, n = a.read_accum()
        cnt, emap = a.read_sample_counts(), a.read_error_map()
        assert n == b.read_accum()[1] == 3 * N
        assert np.array_equal(bits(acc), bits(b.read_accum()[0]))
        assert np.array_equal(cnt, b.read_sample_counts())
        assert np.array_equal(bits(emap), bits(b.read_error_map()))
        assert a.error_map_source() == b.error_map_source() == 2
        for s, rows in zip(shards, row_sets):                 # ... and both equal the shards' own rows
            assert np.array_equal(bits(acc[rows]), bits(s.read_accum()[0]))
            assert np.array_equal(cnt[rows], s.read_sample_counts())
            assert np.array_equal(bits(emap[rows]), bits(s.read_error_map()))
        assert np.unique(cnt).size >= 2, np.unique(cnt)
    finally:
        for r in made:
            r.close()
