"""The gathered error map without a GPU: the binding's table and the NULL-context
returns of the five new entry points, mcpt.dist.FrameGather with the map's record (2 int32 words per
pixel) over gloo, and the merge of the uniform shards' convergence records.

The map's words {se, r} travel as bits: se may be inf or NaN for an overflowed pixel.  The payload
therefore holds what a float path could alter: NaNs with distinct mantissas (quiet and signalling,
both signs), +-inf, denormals and -0.0, every pattern in both channels."""
import ctypes
import os
import re
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = 20, 29       # H is no multiple of band_rows x world in any case below
SPECIAL = np.array([0x7FC00000, 0x7FC00001, 0x7FD2345B, 0xFFC00321, 0x7F800001, 0xFF8ABCDE,   # NaNs
                    0x7F800000, 0xFF800000, 0x80000000, 0x00000001, 0x00000002, 0x007FFFFF,   # inf, -0.0, denormals
                    0x3F800000, 0x42800000], np.uint32)
NEW_CALLS = ("mcpt_gather_error_map", "mcpt_pack_error_map_device", "mcpt_load_rows_error_map", "mcpt_error_map_record",
             "mcpt_error_map_source")
INVALID = -1


def test_binding_declares_the_error_map_calls():
    """The header declares the five entry points and the binding's table carries each of them."""
    hdr = open(os.path.join(REPO, "include", "mcpt.h")).read()
    py = open(os.path.join(REPO, "montecarlo-pathtracing_amd", "mcpt", "__init__.py")).read()
    names = set(re.findall(r"^int (mcpt_(?:gather_error_map|pack_error_map_device|load_rows_error_map|"
                           r"error_map_record|error_map_source))\(", hdr, re.M))
    assert names == set(NEW_CALLS), names
    for n in names:
        assert f'"{n}"' in py, n
    for method in ("gather_error_map", "pack_error_map_device", "load_rows_error_map", "error_map_record",
                   "error_map_source"):
        assert f"    def {method}(self" in py, method
    assert "Out of scope: the shards' error maps do not travel" not in hdr


def test_null_context_is_an_invalid_argument(mcpt_mod):
    """Every new call refuses a NULL context before it touches a device."""
    L = mcpt_mod.lib()
    rec, src = mcpt_mod.Convergence(), ctypes.c_int(7)
    idx = (ctypes.c_int * 4)(0, 1, 2, 3)
    buf = ctypes.c_void_p(64)                    # (never dereferenced)
    assert L.mcpt_gather_error_map(None, None, 0) == INVALID
    assert L.mcpt_pack_error_map_device(None, buf, 1024) == INVALID
    assert L.mcpt_load_rows_error_map(None, buf, 4, idx) == INVALID
    assert L.mcpt_error_map_record(None, 0.1, ctypes.byref(rec)) == INVALID
    assert L.mcpt_error_map_source(None, ctypes.byref(src)) == INVALID
    assert src.value == 7 and rec.n_px == 0


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def payload():
    """[H, W, 2] uint32: the words walk through SPECIAL (every pattern in both channels), every third
    pixel instead a NaN whose mantissa names (row, column, channel)."""
    y, x, c = np.meshgrid(np.arange(H), np.arange(W), np.arange(2), indexing="ij")
    k = (y * W + x) * 2 + c
    out = SPECIAL[(k + y) % SPECIAL.size]
    unique = (0x7F800000 | (k.astype(np.uint32) + 1)).astype(np.uint32)
    return np.where((y * W + x) % 3 == 1, unique, out).astype(np.uint32)


def _setup(rank, world, port):
    import sys
    sys.path.insert(0, REPO)
    sys.path.insert(0, os.path.join(REPO, "montecarlo-pathtracing_amd"))
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)


def _map_worker(rank, world, port, band_rows, partition, q):
    _setup(rank, world, port)
    try:
        from mcpt.dist import FrameGather, frame_row_index, local_rows, max_local_rows
        full = payload()
        rows = local_rows(H, band_rows, world, rank, partition)
        g = FrameGather(H, W, band_rows, world, rank, torch.device("cpu"), partition=partition, channels=2,
                        dtype=torch.int32, assemble=False)
        ok = {"send": (tuple(g.send.shape), g.send.dtype) == ((g.m, W, 2), torch.int32), "no_frame": g.frame is None}
        raw = g.gather_raw(torch.from_numpy(np.ascontiguousarray(full[rows]).view(np.int32)))
        if rank == 0:
            m = max_local_rows(H, band_rows, world, partition)
            idx = frame_row_index(H, band_rows, world, partition)
            got = raw.numpy().view(np.uint32)
            ok["raw"] = (tuple(raw.shape), raw.dtype) == ((world * m, W, 2), torch.int32)
            ok["frame"] = bool(np.array_equal(got[idx], full))
            ok["ranks"], padding = True, []
            for r in range(world):
                rr = local_rows(H, band_rows, world, r, partition)
                ok["ranks"] &= bool(np.array_equal(got[r * m: r * m + len(rr)], full[rr]))
                padding += list(range(r * m + len(rr), (r + 1) * m))
            ok["padding"] = len(padding) > 0 and not set(padding) & set(idx.tolist())
            q.put(ok)
        else:
            assert raw is None
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world,band_rows,partition",
                         [(2, 4, "bands"), (2, 8, "balanced"), (3, 4, "bands"), (3, 2, "balanced")])
def test_map_rows_bit_equal(world, band_rows, partition):
    assert H % (band_rows * world) != 0
    p = payload()
    f = p.view(np.float32)
    assert np.isnan(f).sum() > 100 and np.isinf(f).any() and (p == 0x80000000).any() and (p == 0x007FFFFF).any()
    assert np.unique(p[np.isnan(f)] & 0x7FFFFF).size > 100                    # distinct mantissas
    for c in range(2):
        assert set(SPECIAL.tolist()) <= set(p[..., c].ravel().tolist())      # every pattern in both channels
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    mp.start_processes(_map_worker, args=(world, _free_port(), band_rows, partition, q), nprocs=world, join=True,
                       start_method="spawn")
    ok = q.get(timeout=60)
    assert all(ok.values()), ok


RECORDS = [
    dict(n_px=900, n_above=17, sum_q=2 ** 53 + 1, max_r=0.75, mean_r=0.0, passes=43, batches=3),
    dict(n_px=765, n_above=5, sum_q=2, max_r=1.5000001, mean_r=0.0, passes=43, batches=3),
]


def _merge_worker(rank, world, port, q):
    _setup(rank, world, port)
    try:
        from mcpt.dist import merge_convergence_records
        q.put((rank, merge_convergence_records(RECORDS[rank])))
    finally:
        dist.destroy_process_group()


def test_merge_convergence_records():
    """ShardedRenderer.convergence's merge: the sums add exactly, max_r takes the largest bit pattern,
    mean_r is recomputed, and the record keeps mcpt_convergence's fields."""
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    mp.start_processes(_merge_worker, args=(2, _free_port(), q), nprocs=2, join=True, start_method="spawn")
    got = dict(q.get(timeout=60) for _ in range(2))
    a, b = RECORDS
    for rank in (0, 1):
        m = got[rank]
        assert m.pop("local") == RECORDS[rank]
        for k in ("n_px", "n_above", "sum_q"):
            assert m[k] == a[k] + b[k] and isinstance(m[k], int), k
        assert m["sum_q"] == 2 ** 53 + 3 and float(m["sum_q"]) != m["sum_q"]      # past a double's integers, exact
        assert (m["passes"], m["batches"]) == (43, 3)
        assert np.float32(m["max_r"]).view(np.uint32) == np.float32(1.5000001).view(np.uint32)
        assert m["mean_r"] == (2 ** 53 + 3) / 65536.0 / 1665
        assert set(m) == set(a)
