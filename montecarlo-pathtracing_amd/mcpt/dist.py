"""Multi-GPU rendering: interleaved row-band shards + one gather to rank 0.

One process per GPU (torch.distributed; backend "nccl" = RCCL over xGMI on ROCm).  Every
pixel×pass is independent and the RNG seed is a pure function of (screen_tc, pass, date),
so splitting the frame by rows is bit-identical to one GPU: each rank renders its rows for
ALL passes, into a compact local accumulator, and rank 0 gathers the shards (one RCCL
gather of fp32 RGB rows, padded to the largest shard) and scatters them back into frame
order.  Partitions: "balanced" (default; mcpt_balanced_rows: 8-row bands dealt with a
per-period rotation, leftover rows dealt singly, row counts equal within one) and "bands"
(``(y // band_rows) % world == rank``, mcpt_set_target).  No collective runs on the
data path of the render itself; the gather is the frame's only exchange step.

The gather/reassembly here is device-agnostic torch code so the N>1 path is covered by
world_size-2 ``gloo`` tests on CPU (tests/test_dist_gloo.py).

Adaptive renders: ShardedRenderer passes the statistics and adaptive calls to
its shard, merges the shards' select records over the process group (merge_adaptive_records) and
gathers the frame WITH its per-pixel sample counts (gather_counted: 16 B/px int32 records, one
gather, one load kernel into a full-frame context on rank 0; tests/test_dist_counted_gloo.py,
tests/test_gpu_dist_adaptive.py).  With ``error_map=True`` both gathers also move the shards' error maps
(8 B/px int32 records through a second FrameGather, mcpt_load_rows_error_map on rank 0), so that the
noise-guided filters serve the gathered frame; ShardedRenderer.convergence merges the uniform shards'
records (tests/test_emap_gather_host.py, tests/test_gpu_emap_gather.py).
"""
from __future__ import annotations

from typing import Optional

import numpy as np
import torch
import torch.distributed as dist


PARTITIONS = ("balanced", "bands")


def band_owner(H: int, band_rows: int, world: int) -> np.ndarray:
    """Owner rank of every row, interleaved bands: band (y // band_rows) % world — mcpt_set_target."""
    return (np.arange(H) // band_rows) % world


def balanced_owner(H: int, band_rows: int, world: int) -> np.ndarray:
    """Owner rank of every row, balanced partition — mcpt_balanced_rows (include/mcpt.h).

    Whole periods of `world` bands: in period j, rank r takes band j·world + (r + j) % world,
    so every rank holds every band position of a period equally often (no rank always gets
    the top band of each period); the rows after the last whole period are dealt one at a
    time with the same rotation, so row counts differ by at most one.
    """
    y = np.arange(H)
    periods = (H // band_rows) // world
    rest0 = periods * world * band_rows
    b = y // band_rows
    owner = ((b % world) - (b // world) % world) % world
    tail = y >= rest0
    owner[tail] = ((y[tail] - rest0) + periods) % world
    return owner


def local_rows(H: int, band_rows: int, world: int, rank: int, partition: str = "bands") -> np.ndarray:
    """Global row ids (increasing) owned by `rank` under `partition` ("bands": mcpt_set_target,
    "balanced": mcpt_balanced_rows)."""
    if partition not in PARTITIONS:
        raise ValueError(f"partition must be one of {PARTITIONS}")
    owner = (balanced_owner if partition == "balanced" else band_owner)(H, band_rows, world)
    return np.nonzero(owner == rank)[0]


def max_local_rows(H: int, band_rows: int, world: int, partition: str = "bands") -> int:
    return max(len(local_rows(H, band_rows, world, r, partition)) for r in range(world))


def frame_row_index(H: int, band_rows: int, world: int, partition: str = "bands") -> np.ndarray:
    """For the padded gather buffer [world, max_rows, ...]: flat source index of each frame row."""
    m = max_local_rows(H, band_rows, world, partition)
    src = np.empty(H, np.int64)
    for r in range(world):
        rows = local_rows(H, band_rows, world, r, partition)
        src[rows] = r * m + np.arange(len(rows))
    return src


class FrameGather:
    """Pre-allocated buffers + index for gathering row-band shards into a frame on `dst`.

    ``gather(local)``: local is [n_local_rows, W, C] on this rank's device; returns the
    assembled [H, W, C] frame on `dst` (None on other ranks).  ``gather_raw(local)`` runs the same
    exchange and returns the receive buffer itself, [world * max_rows, W, C] in rank order (frame
    row y is its row ``index[y]``; the padding rows of shorter shards are never indexed), for a
    caller that scatters the rows itself (ShardedRenderer.gather_counted).

    ``channels`` and ``dtype`` give the per-pixel record: the default, 3 float32, is the
    accumulator's sums; 4 int32 is the counted gather's packed record {r, g, b bits, sample count}
    (DESIGN.md §3.9.1), carried as integers so that no step of the exchange reads the words as floats.
    ``assemble=False`` leaves the frame tensor out (gather_raw only).

    At world 1 the send buffer is the frame and no collective runs, unless
    ``force_collective``: then the world-1 gather goes through the process group like any other
    (the test that drives the RCCL branch on a one-GPU box, tests/test_gpu_dist.py).
    """

    def __init__(self, H: int, W: int, band_rows: int, world: int, rank: int, device: torch.device,
                 dst: int = 0, group=None, use_gather: bool = True, partition: str = "bands",
                 force_collective: bool = False, channels: int = 3, dtype: torch.dtype = torch.float32,
                 assemble: bool = True):
        self.collective = world > 1 or force_collective
        self.H, self.W, self.band_rows, self.world, self.rank = H, W, band_rows, world, rank
        self.dst, self.group, self.device, self.partition = dst, group, device, partition
        self.C = C = int(channels)
        self.m = max_local_rows(H, band_rows, world, partition)
        self.n_local = len(local_rows(H, band_rows, world, rank, partition))
        self.send = torch.zeros((self.m, W, C), dtype=dtype, device=device)
        self.use_gather = use_gather
        if rank == dst or not use_gather:
            self.recv = torch.empty((world * self.m, W, C), dtype=dtype, device=device)
            self.recv_list = list(self.recv.view(world, self.m, W, C).unbind(0))
        else:
            self.recv, self.recv_list = None, None
        self.index = torch.as_tensor(frame_row_index(H, band_rows, world, partition), device=device)
        self.frame = (torch.empty((H, W, C), dtype=dtype, device=device)
                      if rank == dst and self.collective and assemble else None)

    def gather_raw(self, local: Optional[torch.Tensor] = None) -> Optional[torch.Tensor]:
        """The exchange alone: the receive buffer [world * max_rows, W, C] on `dst` (the send buffer
        at world 1 without force_collective), None on other ranks.  A buffer this object reuses."""
        if local is not None:
            self.send[: self.n_local].copy_(local)
        if not self.collective:
            return self.send
        staged = self.device.type != "cpu" and dist.get_backend(self.group) == "gloo"
        if staged:   # rehearsal of the N>1 path on one GPU (gloo collectives need host tensors)
            send, recv = self.send.cpu(), (self.recv.cpu() if self.recv is not None else None)
            recv_list = list(recv.view(self.world, self.m, self.W, self.C).unbind(0)) if recv is not None else None
        else:
            send, recv, recv_list = self.send, self.recv, self.recv_list
        if self.use_gather:
            dist.gather(send, recv_list if self.rank == self.dst else None, dst=self.dst, group=self.group)
        else:
            dist.all_gather_into_tensor(recv, send, group=self.group)
        if self.rank != self.dst:
            return None
        if staged:
            self.recv.copy_(recv)
        return self.recv

    def gather(self, local: Optional[torch.Tensor] = None) -> Optional[torch.Tensor]:
        recv = self.gather_raw(local)
        if not self.collective or recv is None:
            return recv
        torch.index_select(recv, 0, self.index, out=self.frame)
        return self.frame


# ---- the frame record of an adaptive select over row shards (include/mcpt.h: "the records of shards
# add ... and max")
RECORD_SUMS = ("n_px", "n_above", "sum_q", "samples", "n_active_blocks", "n_blocks")
RECORD_MAXES = ("passes", "batches")


def _f32_bits(x: float) -> int:
    return int(np.array([x], np.float32).view(np.uint32)[0])


def _merge_records(local: dict, sums, maxes, group=None, device: Optional[torch.device] = None) -> dict:
    """One all-gather of the record's integer fields plus max_r's bit pattern (r >= 0, so the bits
    order as the values) as int64 words per rank, reduced with Python integers: exact, a sum_q past
    2^53 included.  The fields of `sums` add, those of `maxes` and max_r take the largest, mean_r is
    recomputed as sum_q / 65536 / n_px."""
    keys = tuple(sums) + tuple(maxes)
    words = [int(local[k]) for k in keys] + [_f32_bits(local["max_r"])]
    if not all(0 <= w < 2 ** 63 for w in words):
        raise ValueError(f"merge of shard records: a field does not fit int64: {local}")
    world = dist.get_world_size(group)
    if dist.get_backend(group) == "gloo":
        device = torch.device("cpu")
    elif device is None:
        device = torch.device("cuda", torch.cuda.current_device())
    mine = torch.tensor(words, dtype=torch.int64, device=device)
    parts = [torch.empty_like(mine) for _ in range(world)]
    dist.all_gather(parts, mine, group=group)
    rows = [p.tolist() for p in parts]
    out = {}
    for j, k in enumerate(keys):
        col = [r[j] for r in rows]
        out[k] = sum(col) if k in sums else max(col)
    out["max_r"] = float(np.array([max(r[-1] for r in rows)], np.uint32).view(np.float32)[0])
    out["mean_r"] = out["sum_q"] / 65536.0 / out["n_px"] if out["n_px"] > 0 else 0.0
    out["local"] = dict(local)
    return out


def merge_adaptive_records(local: dict, group=None, device: Optional[torch.device] = None) -> dict:
    """The frame's adaptive_select record from every rank's shard record: the integer fields of
    RECORD_SUMS add, those of RECORD_MAXES and max_r take the largest, and mean_r is recomputed
    as sum_q / 65536 / n_px (mcpt_adaptive_select's arithmetic).  One all-gather of nine int64 words
    per rank (max_r travels as its bit pattern: r >= 0, so the bits order as the values), reduced
    with Python integers: exact, a sum_q past 2^53 included.  Every rank returns the merged record,
    with its own under "local".  `device`: where the collective's tensors live (default: the host
    for gloo, else the current cuda device); needs no GPU over gloo."""
    return _merge_records(local, RECORD_SUMS, RECORD_MAXES, group, device)


CONVERGENCE_SUMS = ("n_px", "n_above", "sum_q")


def merge_convergence_records(local: dict, group=None, device: Optional[torch.device] = None) -> dict:
    """merge_adaptive_records for the smaller record of mcpt_convergence (uniform shards): n_px,
    n_above and sum_q add, passes, batches and max_r take the largest, mean_r is recomputed."""
    return _merge_records(local, CONVERGENCE_SUMS, RECORD_MAXES, group, device)


class ShardedRenderer:
    """mcpt.Renderer for this rank's rows + the RCCL gather (GPU path).

    partition "balanced" (default): mcpt_balanced_rows — equal row counts (±1) and rotated
    band positions; "bands": the plain interleaved bands of mcpt_set_target.
    """

    def __init__(self, W: int, H: int, band_rows: int = 8, world: int = 1, rank: int = 0,
                 local_rank: int = 0, group=None, partition: str = "balanced", force_collective: bool = False):
        import mcpt
        self.device = torch.device("cuda", local_rank)
        self.r = mcpt.Renderer(local_rank)
        # The renderer's kernels, the D2D copy into the send buffer and the collective are
        # ordered on ONE stream: a torch stream created here and handed to the library.  (Handing
        # over torch's default stream, handle 0, would leave the library on its own non-blocking
        # stream, and the gather would read the send buffer before the copy landed.)
        # (the greatest priority: with the library's render lanes, the combines and the gather on
        # this stream are dispatched ahead of the next render's waiting workgroups)
        self.stream = torch.cuda.Stream(self.device, priority=torch.cuda.Stream.priority_range()[1])
        self.r.set_stream(self.stream.cuda_stream)
        if partition == "bands":
            self.r.set_target(W, H, band_rows, world, rank)
        else:
            self.r.set_target_rows(W, H, local_rows(H, band_rows, world, rank, partition))
        self.W, self.H, self.band_rows, self.world, self.rank = W, H, band_rows, world, rank
        self.partition, self.local_rank, self.group, self.force_collective = partition, local_rank, group, force_collective
        self.scene = None
        self.gc = None            # the counted gather's buffers and frame context: made on first use
        self.gm = None            # the error map's gather buffers: made on first use
        self.frame_r = None
        self.g = FrameGather(H, W, band_rows, world, rank, self.device, group=group, partition=partition,
                             force_collective=force_collective)
        # the gather buffers were allocated (and zero-filled) on the caller's stream
        self.stream.wait_stream(torch.cuda.current_stream(self.device))

    def upload_scene(self, scene) -> None:
        self.r.upload_scene(scene)
        self.scene = scene
        if self.frame_r is not None:
            self.frame_r.upload_scene(scene)

    def render(self, invPV, invV, first_pass, n_passes, date=0.0, bounces=3, refract_ind=1.0, variant=0):
        self.r.render(invPV, invV, first_pass, n_passes, date, bounces, refract_ind, variant)

    def gather(self, error_map: bool = False):
        """Copy the local accumulator into the send buffer and gather the frame to rank 0, both
        on `self.stream` after the queued renders; the caller's current stream is then made to
        wait for it, so the returned frame is safe to use there.

        The returned tensor is a buffer this renderer reuses (the frame on rank 0, the send
        buffer at world 1): the next gather overwrites it.  That gather's writes are ordered
        after everything the caller has queued on its current stream by then (the private
        stream waits for it first), so work the caller queued that reads the previous frame
        completes before the buffer changes; keep a copy (``frame.clone()``) to hold a frame
        across gathers.

        ``error_map=True`` (a uniform render with statistics on, after convergence()): the frame is
        delivered into a full-frame mcpt.Renderer on rank 0 together with the shards' error maps, as
        gather_counted(error_map=True) does, and that renderer is returned in place of a tensor
        (None on other ranks).  The rows travel as packed records whose count is the pass count for
        every pixel, so its denoise_resolved_guided gives accum / pass_count filtered with the
        gathered map: denoise_guided's bits on one context."""
        if error_map:
            return self.gather_counted(error_map=True)
        n = self.g.n_local
        caller = torch.cuda.current_stream(self.device)
        self.stream.wait_stream(caller)   # the caller's reads of the previous frame come first
        with torch.cuda.stream(self.stream):
            if n:
                self.r.copy_accum_device(self.g.send.data_ptr(), n * self.W * 3 * 4)
            frame = self.g.gather(None)
        caller.wait_stream(self.stream)
        return frame

    # ---- adaptive sampling over the shards: the shard context's calls, the
    # frame's record merged over the group, and the counted gather
    def stats_begin(self) -> None:
        self.r.stats_begin()

    def convergence(self, threshold: float, mu_floor: Optional[float] = None) -> dict:
        """The uniform counterpart of adaptive_select: the local mcpt_convergence (which writes the
        shard's error map), then the shards' records merged over the process group
        (merge_convergence_records): the frame's record on every rank, this rank's under "local"."""
        import mcpt
        local = self.r.convergence(threshold, mcpt.ERROR_MU_FLOOR if mu_floor is None else mu_floor)
        if self.world == 1 and not self.force_collective:
            return dict(local, local=dict(local))
        return merge_convergence_records(local, self.group, self.device)

    def adaptive_begin(self, min_passes: int = 0) -> None:
        self.r.adaptive_begin(min_passes)

    def adaptive_end(self) -> None:
        self.r.adaptive_end()

    def render_adaptive(self, invPV, invV, first_pass, n_passes, date=0.0, bounces=3, refract_ind=1.0, variant=0):
        self.r.render_adaptive(invPV, invV, first_pass, n_passes, date, bounces, refract_ind, variant)

    def adaptive_select(self, threshold: float, mu_floor: Optional[float] = None) -> dict:
        """The local select, then the shards' records merged over the process group
        (merge_adaptive_records): the frame's record on every rank, this rank's under "local"."""
        import mcpt
        local = self.r.adaptive_select(threshold, mcpt.ERROR_MU_FLOOR if mu_floor is None else mu_floor)
        if self.world == 1 and not self.force_collective:
            return dict(local, local=dict(local))
        return merge_adaptive_records(local, self.group, self.device)

    def render_adaptive_until(self, invPV, invV, threshold: float, batch: int = 32, max_passes: int = 4096,
                              min_passes: int = 0, check_every: int = 1, first_pass: int = 1, date: float = 0.0,
                              bounces: int = 3, refract_ind: float = 1.0, variant: int = 0,
                              mu_floor: Optional[float] = None) -> dict:
        """mcpt.Renderer.render_adaptive_until over the shards: every rank renders its active blocks
        in calls of `batch` passes and the loop ends on the MERGED record (no active block on any
        rank, or `max_passes`), so every rank leaves it in the same round; a rank whose blocks have
        all retired keeps calling (an empty list launches nothing).  Returns the last merged record
        plus "rendered" (passes) and "rounds" (render calls); the mode stays on for gather_counted()."""
        if batch <= 0 or check_every <= 0 or max_passes <= 0 or not threshold > 0:
            raise ValueError("render_adaptive_until: batch, check_every, max_passes and threshold must be positive")
        import mcpt
        self.stats_begin()
        self.adaptive_begin(min_passes)
        render = lambda p, n: self.render_adaptive(invPV, invV, p, n, date, bounces, refract_ind, variant)
        select = lambda: self.adaptive_select(threshold, mu_floor)     # (merged: the same answer on every rank)
        rec, done, calls = mcpt._adaptive_until(render, select, None, first_pass, batch, max_passes, check_every)
        rec["rendered"], rec["rounds"] = done, calls
        return rec

    def _counted_setup(self) -> None:
        import mcpt
        self.gc = FrameGather(self.H, self.W, self.band_rows, self.world, self.rank, self.device, group=self.group,
                              partition=self.partition, force_collective=self.force_collective, channels=4,
                              dtype=torch.int32, assemble=False)
        self.src_row = frame_row_index(self.H, self.band_rows, self.world, self.partition).astype(np.int32)
        self.most = torch.zeros(1, dtype=torch.int32, device=self.device)
        if self.rank == self.gc.dst:
            # the frame context shares the shard context's stream: its load is ordered after the
            # collective, and its reads (read_accum, denoise_resolved, ...) after the load
            self.frame_r = mcpt.Renderer(self.local_rank)
            self.frame_r.set_stream(self.stream.cuda_stream)
            self.frame_r.set_target(self.W, self.H)
            if self.scene is not None:
                self.frame_r.upload_scene(self.scene)

    def gather_counted(self, error_map: bool = False):
        """gather() for an adaptive render: the frame WITH its per-pixel sample counts.  Every rank
        packs its rows into 16 B/px records {r, g, b bits, int32 count} (mcpt_pack_counted_device;
        with the adaptive mode off the count is the pass count), one gather moves them to rank 0 as
        int32 words, and there one kernel (mcpt_load_rows_counted) scatters the rows into a
        full-frame mcpt.Renderer on the same device and stream, which is returned (None on other
        ranks): read_accum, read_sample_counts, read_resolved and denoise_resolved (after
        render_guides) serve it exactly as after the in-process gather_rows_counted.  That renderer
        is created on first use, reused by later calls and closed by close().

        The frame's pass count is the largest over the ranks: a 1-element MAX reduction in the same
        group and, on rank 0, ONE host read of it (a stream wait).  The call ends a render and does
        not belong in a timed loop of launches; gather() stays free of host waits.

        Stream discipline as gather(): the private stream first waits for the caller's current
        stream, pack, collective and load run on it, and the caller's stream then waits for it.

        ``error_map=True``: every rank also packs its error map (the last adaptive_select's or
        convergence()'s; mcpt_pack_error_map_device, 8 B/px {se, r} carried as two int32 words) into
        a second FrameGather, the same collective moves it, and rank 0 loads it behind the rows with
        the same row index (mcpt_load_rows_error_map: the index is uploaded once for the pair).  The
        returned renderer then serves denoise_resolved_guided, read_error_map and error_map_record."""
        if self.gc is None:
            self._counted_setup()
        if error_map and self.gm is None:
            self.gm = FrameGather(self.H, self.W, self.band_rows, self.world, self.rank, self.device, group=self.group,
                                  partition=self.partition, force_collective=self.force_collective, channels=2,
                                  dtype=torch.int32, assemble=False)
        g, n = self.gc, self.gc.n_local
        most = self.r.pass_count()
        caller = torch.cuda.current_stream(self.device)
        self.stream.wait_stream(caller)   # (also orders the first call's buffer fills before the pack)
        with torch.cuda.stream(self.stream):
            if n:
                self.r.pack_counted_device(g.send.data_ptr(), n * self.W * 16)
            raw = g.gather_raw(None)
            if g.collective:
                if dist.get_backend(self.group) == "gloo":   # host tensors (the staged rehearsal on one GPU)
                    t = torch.tensor([most], dtype=torch.int32)
                    dist.reduce(t, g.dst, op=dist.ReduceOp.MAX, group=self.group)
                    most = int(t.item())
                else:
                    self.most.fill_(most)
                    dist.reduce(self.most, g.dst, op=dist.ReduceOp.MAX, group=self.group)
                    if self.rank == g.dst:
                        most = int(self.most.item())   # the one host read
            if raw is not None:
                self.frame_r.load_rows_counted(raw.data_ptr(), raw.shape[0], self.src_row, most)
            if error_map:
                if n:
                    self.r.pack_error_map_device(self.gm.send.data_ptr(), n * self.W * 8)
                raw_map = self.gm.gather_raw(None)
                if raw_map is not None:
                    self.frame_r.load_rows_error_map(raw_map.data_ptr(), raw_map.shape[0], self.src_row)
        caller.wait_stream(self.stream)
        return self.frame_r if raw is not None else None

    def close(self) -> None:
        if self.frame_r is not None:
            self.frame_r.close()
            self.frame_r = None
        self.r.close()
