"""Per-pixel sample counts through the multi-process gather: the pack and load
kernels (mcpt_pack_counted_device, mcpt_load_rows_counted), ShardedRenderer's adaptive calls, the
merged select record and gather_counted().

Scene 6 at 45x37 (partial blocks on both axes), 4 bounces, thresholds from choose_threshold on the
oracle's snapshots of each shard's rows.  The reference throughout is the in-process counted gather
(mcpt_gather_rows_counted) of the same shards driven by the same calls: the frame the new path
delivers must equal it bit for bit.  On the oracle: the calls of SIZES leave the balanced shards with
counts {8, 16, 19 / 51, 91}, the explicit shards A, B, C with {8, 16, 51}, {8, 16, 19}, {8, 16, 51, 91};
calls of 4 passes up to 24 leave blocks active and blocks retired on every balanced shard of world 1,
2 and 3.  Every test asserts such a condition on the GPU's own results."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import test_adaptive_restate as ar
import test_denoise_restate as rs
import test_gpu_adaptive as tga
from test_gpu_adaptive import BOUNCES, FLOOR, H0, SHARD, SIZES, W0, choose_threshold, oracle_snapshots
from test_gpu_adaptive_pipeline import balanced_rows, begin, new_renderer, run_calls, status

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
bits = rs.bits
NO_ADAPTIVE, NO_STATS, NO_TARGET, INVALID = -9, -8, -3, -1
SHARD_B = [35, 0, 19, 12, 28, 5, 21]
SHARD_C = [y for y in range(H0) if y not in SHARD and y not in SHARD_B]
BATCH, CAP = 4, 24              # ShardedRenderer.render_adaptive_until's calls in the process tests
SUMS = ("n_px", "n_above", "sum_q", "samples", "n_active_blocks", "n_blocks")


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def shard_threshold(mcpt_mod, oracle_mod, rows):
    snaps = oracle_snapshots(mcpt_mod, oracle_mod, 6, W0, H0)
    return choose_threshold([s[rows] for s in snaps], W0, len(rows))


def partly_retired(r):
    info = r.adaptive_info()
    return 0 < info["n_active"] < info["n_blocks"]


def packed_layout(row_sets):
    """FrameGather's layout of the shards' packed rows: shard k at rows k * m .. of [n * m, W, 4]
    (m the longest shard); the source row of every frame row."""
    m = max(len(rows) for rows in row_sets)
    src = np.full(H0, -1, np.int32)
    for k, rows in enumerate(row_sets):
        src[np.asarray(rows)] = k * m + np.arange(len(rows))
    assert (src >= 0).all()
    return m, src


def pack_all(shards, m):
    buf = torch.zeros((len(shards) * m, W0, 4), dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    for k, s in enumerate(shards):
        n = s.n_local_rows
        s.pack_counted_device(buf[k * m].data_ptr(), n * W0 * 16)
        s.synchronize()
    return buf


# ---- 1. pack + load against the in-process counted gather ---------------------------------------
@pytest.mark.parametrize("layout", ["balanced2", "explicit3"])
def test_pack_load_equals_gather_rows_counted(mcpt_mod, oracle_mod, layout):
    from mcpt.dist import frame_row_index
    if layout == "balanced2":
        row_sets = [balanced_rows(mcpt_mod, H0, 2, k, 8) for k in range(2)]
    else:
        row_sets = [SHARD, SHARD_B, SHARD_C]
    assert sorted(sum(row_sets, [])) == list(range(H0))
    m, src = packed_layout(row_sets)
    if layout == "balanced2":
        assert np.array_equal(src, frame_row_index(H0, 8, 2, "balanced"))
    made = []
    try:
        shards = []
        for k, rows in enumerate(row_sets):
            r, cam = new_renderer(mcpt_mod, rows)
            made.append(r)
            begin(r)
            run_calls(r, cam, shard_threshold(mcpt_mod, oracle_mod, rows), range(4 if k == 1 else 6), 1)   # shard 1 stops early
            shards.append(r)
        assert any(partly_retired(s) for s in shards)
        counts = [s.pass_count() for s in shards]      # (a shard whose blocks have all retired stops counting)
        assert counts[1] == 19 and max(counts) == 91, counts
        a, cam = new_renderer(mcpt_mod)
        b, _ = new_renderer(mcpt_mod)
        made += [a, b]
        a.gather_rows_counted(shards)
        buf = pack_all(shards, m)
        host = buf.cpu().numpy()
        for k, s in enumerate(shards):          # the records themselves: the accumulator's bits and the counts
            n = s.n_local_rows
            assert np.array_equal(host[k * m: k * m + n, :, :3].view(np.uint32), bits(s.read_accum()[0]))
            assert np.array_equal(host[k * m: k * m + n, :, 3], s.read_sample_counts())
            assert not host[k * m + n: (k + 1) * m].any()                     # padding rows untouched
        b.load_rows_counted(buf.data_ptr(), buf.shape[0], src, max(s.pass_count() for s in shards))
        acc_a, n_a = a.read_accum()
        acc_b, n_b = b.read_accum()
        cnt = b.read_sample_counts()
        assert n_a == n_b == 91
        assert np.array_equal(bits(acc_a), bits(acc_b)) and np.array_equal(a.read_sample_counts(), cnt)
        assert np.unique(cnt).size >= 3
        assert np.array_equal(bits(a.read_resolved()), bits(b.read_resolved()))
        assert np.array_equal(bits(b.read_resolved()), bits(ar.resolve(acc_b, cnt)))
        a.render_guides(*cam)
        b.render_guides(*cam)
        assert np.array_equal(bits(a.denoise_resolved(3)), bits(b.denoise_resolved(3)))
        # a shard with the adaptive mode off packs its pass count for every pixel
        s, rows = shards[1], row_sets[1]
        cam1 = tga.target(mcpt_mod, s, 6, W0, H0, rows)
        for first in (1, 5):
            s.render(cam1[0], cam1[1], first, 4, 0.0, BOUNCES, 1.0, 0)
        assert s.adaptive_info()["on"] is False and s.pass_count() == 8
        host = pack_all(shards, m).cpu().numpy()[m: m + len(rows)]
        assert (host[..., 3] == 8).all() and np.array_equal(host[..., :3].view(np.uint32), bits(s.read_accum()[0]))
    finally:
        for r in made:
            r.close()


# ---- 2. processes sharing cuda:0 over staged gloo ---------------------------------------------
def reference_loop(mcpt_mod, row_sets, thrs, first=1, threshold=None, mu_floor=FLOOR):
    """The shards as plain Renderers driven by ShardedRenderer.render_adaptive_until's calls; returns
    (renderers, the last records merged by hand, rounds)."""
    made = []
    for rows in row_sets:
        r, cam = new_renderer(mcpt_mod, rows)
        begin(r)
        made.append(r)
    done, calls, recs = 0, 0, None
    while done < CAP:
        for r in made:
            r.render_adaptive(cam[0], cam[1], first + done, BATCH, 0.0, BOUNCES, 1.0, 0)
        done += BATCH
        calls += 1
        if calls >= 2:
            recs = [r.adaptive_select(thr if threshold is None else threshold, mu_floor) for r, thr in zip(made, thrs)]
            if sum(x["n_active_blocks"] for x in recs) == 0:
                break
    merged = {k: sum(x[k] for x in recs) for k in SUMS}
    merged.update(passes=max(x["passes"] for x in recs), batches=max(x["batches"] for x in recs),
                  max_r_bits=max(int(np.float32(x["max_r"]).view(np.uint32)) for x in recs))
    merged["mean_r"] = merged["sum_q"] / 65536.0 / merged["n_px"]
    return made, merged, calls


def record_key(rec):
    out = {k: rec[k] for k in SUMS + ("passes", "batches", "mean_r")}
    out["max_r_bits"] = int(np.float32(rec["max_r"]).view(np.uint32))
    return out


def _gloo_worker(rank, world, port, thrs, q):
    import sys
    for p in (os.path.join(REPO, "tests"), REPO, os.path.join(REPO, "montecarlo-pathtracing_amd")):
        sys.path.insert(0, p)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        import mcpt
        from mcpt.dist import ShardedRenderer, local_rows
        ipv, iv = mcpt.camera_canonical(W0, H0)
        sr = ShardedRenderer(W0, H0, 8, world, rank, 0)
        sr.upload_scene(mcpt.Scene.reference(6))
        rec = sr.render_adaptive_until(ipv, iv, thrs[rank], batch=BATCH, max_passes=CAP, bounces=BOUNCES, mu_floor=FLOOR)
        frame = sr.gather_counted()
        out = {"rank": rank, "rounds": rec["rounds"], "rec": record_key(rec), "partly": partly_retired(sr.r),
               "local_ok": rec["local"]["n_px"] == sr.r.n_local_rows * W0, "is_frame": (frame is not None) == (rank == 0)}
        if rank == 0:
            row_sets = [local_rows(H0, 8, world, k, "balanced").tolist() for k in range(world)]
            made, merged, calls = reference_loop(mcpt, row_sets, thrs)
            ref, _ = new_renderer(mcpt)
            ref.gather_rows_counted(made)
            acc, n = frame.read_accum()
            want, n_want = ref.read_accum()
            out.update(acc=bool(np.array_equal(bits(acc), bits(want))), n=(n, n_want),
                       cnt=bool(np.array_equal(frame.read_sample_counts(), ref.read_sample_counts())),
                       n_counts=int(np.unique(frame.read_sample_counts()).size),
                       resolved=bool(np.array_equal(bits(frame.read_resolved()), bits(ref.read_resolved()))),
                       merged=merged, ref_rounds=calls)
            for r in made + [ref]:
                r.close()
        # a second window in which every block retires at the first select: the loop ends there on every rank
        rec2 = sr.render_adaptive_until(ipv, iv, 60.0, batch=BATCH, max_passes=CAP, first_pass=CAP + 1, bounces=BOUNCES,
                                        mu_floor=10.0)
        out["rounds2"], out["active2"] = rec2["rounds"], rec2["n_active_blocks"]
        q.put(out)
        sr.close()
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 3])
def test_sharded_adaptive_gather_counted(mcpt_mod, oracle_mod, world):
    from mcpt.dist import local_rows
    thrs = [shard_threshold(mcpt_mod, oracle_mod, local_rows(H0, 8, world, k, "balanced").tolist()) for k in range(world)]
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    mp.start_processes(_gloo_worker, args=(world, _free_port(), thrs, q), nprocs=world, join=True, start_method="spawn")
    outs = sorted((q.get(timeout=120) for _ in range(world)), key=lambda o: o["rank"])
    zero = outs[0]
    assert any(o["partly"] for o in outs), outs                      # blocks retired and blocks still active
    assert all(o["is_frame"] and o["local_ok"] for o in outs)
    assert len({o["rounds"] for o in outs}) == 1 and zero["rounds"] == zero["ref_rounds"] == CAP // BATCH
    assert all(o["rec"] == zero["merged"] for o in outs), (zero["merged"], [o["rec"] for o in outs])
    assert zero["n"] == (CAP, CAP) and zero["n_counts"] >= 3
    assert zero["acc"] and zero["cnt"] and zero["resolved"], zero
    assert [(o["rounds2"], o["active2"]) for o in outs] == [(2, 0)] * world


# ---- 3. world 1 over RCCL ----------------------------------------------------------------------
def _nccl_worker(rank, port, thr, q):
    import sys
    for p in (os.path.join(REPO, "tests"), REPO, os.path.join(REPO, "montecarlo-pathtracing_amd")):
        sys.path.insert(0, p)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    torch.cuda.set_device(0)
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
    try:
        import mcpt
        from mcpt.dist import ShardedRenderer
        ipv, iv = mcpt.camera_canonical(W0, H0)
        sr = ShardedRenderer(W0, H0, 8, 1, 0, 0, force_collective=True)
        sr.upload_scene(mcpt.Scene.reference(6))
        rec = sr.render_adaptive_until(ipv, iv, thr, batch=BATCH, max_passes=CAP, bounces=BOUNCES, mu_floor=FLOOR)
        frame = sr.gather_counted()
        acc, n = frame.read_accum()
        want, n_want = sr.r.read_accum()
        cnt = frame.read_sample_counts()
        ptr = frame.accum_device_ptr()[0]
        q.put({"backend": dist.get_backend(), "n": (n, n_want, sr.r.pass_count()), "partly": partly_retired(sr.r),
               "acc": bool(np.array_equal(bits(acc), bits(want))),
               "cnt": bool(np.array_equal(cnt, sr.r.read_sample_counts())), "n_counts": int(np.unique(cnt).size),
               "resolved": bool(np.array_equal(bits(frame.read_resolved()), bits(sr.r.read_resolved()))),
               "separate": ptr not in (sr.gc.send.data_ptr(), sr.gc.recv.data_ptr()) and ptr != sr.r.accum_device_ptr()[0],
               "merged": record_key(rec) == record_key(rec["local"])})
        sr.close()
    finally:
        dist.destroy_process_group()


def test_rccl_world1_gather_counted(mcpt_mod, oracle_mod):
    thr = shard_threshold(mcpt_mod, oracle_mod, list(range(H0)))
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    mp.start_processes(_nccl_worker, args=(_free_port(), thr, q), nprocs=1, join=True, start_method="spawn")
    o = q.get(timeout=120)
    assert o["backend"] == "nccl" and o["partly"] and o["n_counts"] >= 3, o
    assert o["n"] == (CAP, CAP, CAP)
    assert o["acc"] and o["cnt"] and o["resolved"] and o["merged"], o
    assert o["separate"], "the frame context's accumulator must not alias the gather's buffers"


# ---- 4. error and invalidation returns ---------------------------------------------------------
def test_errors_and_invalidation(mcpt_mod, oracle_mod):
    made = []
    try:
        bare = mcpt_mod.Renderer(0)
        made.append(bare)
        buf = torch.zeros((H0, W0, 4), dtype=torch.int32, device="cuda:0")
        torch.cuda.synchronize()
        nbytes = H0 * W0 * 16
        assert f"({NO_TARGET})" in status(mcpt_mod, bare.pack_counted_device, buf.data_ptr(), nbytes)
        assert f"({NO_TARGET})" in status(mcpt_mod, bare.pass_count)
        frame, cam = new_renderer(mcpt_mod)
        shard, scam = new_renderer(mcpt_mod, SHARD)
        made += [frame, shard]
        ident = np.arange(H0, dtype=np.int32)
        # pass_count() is read_accum()'s count: plain renders, adaptive renders, an empty active list
        assert frame.pass_count() == 0
        frame.render(cam[0], cam[1], 1, 4, 0.0, BOUNCES, 1.0, 0)
        assert frame.pass_count() == frame.read_accum()[1] == 4
        thr = shard_threshold(mcpt_mod, oracle_mod, SHARD)
        begin(shard)
        run_calls(shard, scam, thr, range(3), 1)
        assert shard.pass_count() == shard.read_accum()[1] == 16 and partly_retired(shard)
        assert shard.adaptive_select(60.0, 10.0)["n_active_blocks"] == 0           # every block retires
        shard.render_adaptive(scam[0], scam[1], 17, 8, 0.0, BOUNCES, 1.0, 0)        # an empty list: nothing changes
        assert shard.pass_count() == shard.read_accum()[1] == 16
        # pack: a short buffer
        assert f"({INVALID})" in status(mcpt_mod, frame.pack_counted_device, buf.data_ptr(), nbytes - 16)
        assert f"({INVALID})" in status(mcpt_mod, shard.pack_counted_device, buf.data_ptr(), len(SHARD) * W0 * 16 - 1)
        frame.pack_counted_device(buf.data_ptr(), nbytes)                           # mode off: the pass count
        frame.synchronize()
        assert (buf.cpu().numpy()[..., 3] == 4).all()
        # load: a shard target, an index out of range, pass_count 0; the frame keeps what it has
        assert "is a shard" in status(mcpt_mod, shard.load_rows_counted, buf.data_ptr(), H0, ident, 4)
        assert f"({INVALID})" in status(mcpt_mod, shard.load_rows_counted, buf.data_ptr(), H0, ident, 4)
        for bad in (np.where(ident == 7, H0, ident), np.where(ident == 30, -1, ident)):
            assert f"({INVALID})" in status(mcpt_mod, frame.load_rows_counted, buf.data_ptr(), H0, bad.astype(np.int32), 4)
        assert f"({INVALID})" in status(mcpt_mod, frame.load_rows_counted, buf.data_ptr(), H0, ident, 0)
        assert f"({INVALID})" in status(mcpt_mod, frame.load_rows_counted, buf.data_ptr(), H0 - 1, ident, 4)
        assert f"({NO_ADAPTIVE})" in status(mcpt_mod, frame.read_sample_counts)
        # a good load, rows reversed; then what the loaded frame serves and what invalidates it
        want = frame.read_accum()[0]
        frame.load_rows_counted(buf.data_ptr(), H0, ident[::-1], 9)
        acc, n = frame.read_accum()
        assert n == frame.pass_count() == 9 and np.array_equal(bits(acc), bits(want[::-1]))
        assert (frame.read_sample_counts() == 4).all()
        assert np.array_equal(bits(frame.read_resolved()), bits(ar.resolve(acc, frame.read_sample_counts())))
        frame.render_guides(*cam)
        assert frame.denoise_resolved(2).shape == (H0, W0, 3)
        assert f"({NO_STATS})" in status(mcpt_mod, frame.denoise_resolved_guided, 2)
        frame.render(cam[0], cam[1], 10, 2, 0.0, BOUNCES, 1.0, 0)
        assert f"({NO_ADAPTIVE})" in status(mcpt_mod, frame.read_sample_counts)
        assert f"({NO_ADAPTIVE})" in status(mcpt_mod, frame.read_resolved)
        for undo in (frame.clear_accum, lambda: frame.write_accum(want, 4), lambda: frame.set_target(W0, H0)):
            frame.load_rows_counted(buf.data_ptr(), H0, ident, 4)
            assert frame.read_sample_counts().shape == (H0, W0)
            undo()
            assert f"({NO_ADAPTIVE})" in status(mcpt_mod, frame.read_sample_counts)
    finally:
        for r in made:
            r.close()


# ---- 5. ordering: render + gather_counted rounds back to back ----------------------------------
def test_gather_counted_rounds_ordered(mcpt_mod, oracle_mod):
    """Two render_adaptive + gather_counted rounds with no host synchronization between them (world
    1: pack, load and the renders share the private stream, and nothing in gather_counted waits) give
    what the same calls give without the first gather."""
    from mcpt.dist import ShardedRenderer
    thr = shard_threshold(mcpt_mod, oracle_mod, list(range(H0)))
    ipv, iv = mcpt_mod.camera_canonical(W0, H0)
    sr = ShardedRenderer(W0, H0, 8, 1, 0, 0)
    ref, cam = new_renderer(mcpt_mod)
    try:
        sr.upload_scene(mcpt_mod.Scene.reference(6))
        sr.stats_begin()
        sr.adaptive_begin(0)
        begin(ref)
        first = 1
        for k in range(4):                      # the selects synchronize: they come before the two rounds
            for r in (sr, ref):
                r.render_adaptive(ipv, iv, first, SIZES[k], 0.0, BOUNCES, 1.0, 0)
            first += SIZES[k]
            if k >= 1:
                rec = sr.adaptive_select(thr, FLOOR)
                assert record_key(rec) == record_key(ref.adaptive_select(thr, FLOOR)) and rec["local"]["n_px"] == W0 * H0
        assert partly_retired(sr.r)
        for k in (4, 5):                        # 32 and 40 passes: each round's render is still running at its gather
            sr.render_adaptive(ipv, iv, first, SIZES[k], 0.0, BOUNCES, 1.0, 0)
            frame = sr.gather_counted()
            ref.render_adaptive(ipv, iv, first, SIZES[k], 0.0, BOUNCES, 1.0, 0)
            first += SIZES[k]
        assert frame is sr.frame_r
        acc, n = frame.read_accum()
        want, n_want = ref.read_accum()
        assert n == n_want == 91
        assert np.array_equal(bits(acc), bits(want))
        assert np.array_equal(frame.read_sample_counts(), ref.read_sample_counts())
        assert np.unique(frame.read_sample_counts()).size >= 3
        assert np.array_equal(bits(frame.read_resolved()), bits(ref.read_resolved()))
        frame.render_guides(ipv, iv)            # the frame context holds the scene: the filter runs on it
        ref.render_guides(ipv, iv)
        assert np.array_equal(bits(frame.denoise_resolved(3)), bits(ref.denoise_resolved(3)))
    finally:
        sr.close()
        ref.close()
