// mcpt_capi_gather.hip — C ABI, device half: everything that moves a shard into a frame (DESIGN.md
// §3.9, §3.9.1).  In one process the peer copies of a shard's planes (accumulator, counts, error
// map) into the frame's, all through copy_shard_planes; across processes the two ends of the same
// gathers, mcpt_pack_* on the shard and mcpt_load_rows_* on the frame (the collective between them
// is the caller's: mcpt/dist.py).  The row plan is mcpt_gather_plan.h's.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "mcpt_ctx.h"

namespace plan = mcpt::plan;

namespace {
// the gathers' guards: the calling thread's current device is restored on every return path
struct DeviceGuard {
  int prev = -1;
  DeviceGuard() { if (hipGetDevice(&prev) != hipSuccess) prev = -1; }
  ~DeviceGuard() { if (prev >= 0) (void)hipSetDevice(prev); }
};
// direct xGMI reads/writes between a frame's device and a shard's (once per process)
int enable_peer_access(const mcpt_ctx* frame, const mcpt_ctx* s) {
  int ok = 0;
  if (s->device != frame->device) HIP_OR_RETURN(hipDeviceCanAccessPeer(&ok, frame->device, s->device));
  if (ok) {
    HIP_OR_RETURN(hipSetDevice(frame->device));
    const hipError_t e = hipDeviceEnablePeerAccess(s->device, 0);
    if (e != hipSuccess && e != hipErrorPeerAccessAlreadyEnabled) return set_err(MCPT_ERR_HIP, "hipDeviceEnablePeerAccess", e);
    (void)hipGetLastError();
  }
  return MCPT_OK;
}
// the error of call `who`: "<who>: <what>"
int refuse(int status, const char* who, const char* what, hipError_t e = hipSuccess) {
  char msg[200];
  std::snprintf(msg, sizeof(msg), "%s: %s", who, what);
  return set_err(status, msg, e);
}
// the checks both in-process gathers make of one shard
int check_shard(const char* who, const mcpt_ctx* frame, const mcpt_ctx* s) {
  if (!s || s == frame) return refuse(MCPT_ERR_INVALID_ARG, who, "bad shard context");
  if (!s->has_target) return refuse(MCPT_ERR_NO_TARGET, who, "shard has no target");
  if (s->W != frame->W || s->H != frame->H) return refuse(MCPT_ERR_INVALID_ARG, who, "shard size differs");
  return MCPT_OK;
}
bool shards_hold_rows_once(const mcpt_ctx* frame, mcpt_ctx* const* shards, int n_shards) {
  std::vector<const std::vector<int>*> lists;
  for (int k = 0; k < n_shards; ++k) lists.push_back(&shards[k]->rows);
  return plan::rows_held_once(lists.data(), n_shards, frame->H);
}
// one plane of a peer copy: frame row y at dst + y * row_bytes, the shard's local row i at src + i * row_bytes
struct Plane { void* dst; const void* src; size_t row_bytes; };

// One shard's planes into the frame's, a contiguous copy per run of consecutive global rows and
// plane (the planes of a run in list order), all on the frame's stream: (1) it waits for the shard's
// queued work (the kernels that wrote the planes), (2) the shard's later work (a progressive
// caller's next render adds into its accumulator in place, its next select rewrites its map) waits
// for the copies.  Leaves the shard's device current.
int copy_shard_planes(const char* who, mcpt_ctx* frame, mcpt_ctx* s, const Plane* planes, int n_planes) {
  OK_OR_RETURN(enable_peer_access(frame, s));
  HIP_OR_RETURN(hipSetDevice(s->device));
  // (destroyed on every return path: HIP releases an event once the waits on it are satisfied)
  Event done;
  HIP_OR_RETURN(done.ensure(hipEventDisableTiming));
  HIP_OR_RETURN(hipEventRecord(done, s->stream));
  HIP_OR_RETURN(hipSetDevice(frame->device));
  HIP_OR_RETURN(hipStreamWaitEvent(frame->stream, done, 0));
  for (const plan::RowRun& run : plan::row_runs(s->rows))
    for (int p = 0; p < n_planes; ++p) {
      const Plane& pl = planes[p];
      const hipError_t e = hipMemcpyPeerAsync((char*)pl.dst + (size_t)run.global_first * pl.row_bytes, frame->device,
                                              (const char*)pl.src + (size_t)run.local_first * pl.row_bytes, s->device,
                                              (size_t)run.n * pl.row_bytes, frame->stream);
      if (e != hipSuccess) return refuse(MCPT_ERR_HIP, who, "peer copy", e);
    }
  Event copied;
  HIP_OR_RETURN(copied.ensure(hipEventDisableTiming));
  HIP_OR_RETURN(hipEventRecord(copied, frame->stream));
  HIP_OR_RETURN(hipSetDevice(s->device));
  HIP_OR_RETURN(hipStreamWaitEvent(s->stream, copied, 0));
  return MCPT_OK;
}

// mcpt_gather_rows (counted false: equal pass counts, no counts carried) and
// mcpt_gather_rows_counted (counted true: each shard's per-pixel counts travel with its rows into
// frame's count plane; every frame row from exactly one shard)
int gather_rows(mcpt_ctx* frame, mcpt_ctx* const* shards, int n_shards, bool counted) {
  const char* who = "mcpt_gather_rows";
  if (!frame || n_shards < 0 || (n_shards > 0 && !shards)) return refuse(MCPT_ERR_INVALID_ARG, who, "bad arguments");
  if (!frame->has_target) return refuse(MCPT_ERR_NO_TARGET, who, "frame has no target");
  if (frame->n_local_rows != frame->H) return refuse(MCPT_ERR_INVALID_ARG, who, "frame target is a shard");
  for (int k = 0; k < n_shards; ++k) {
    OK_OR_RETURN(check_shard(who, frame, shards[k]));
    if (!counted && shards[k]->pass_count != shards[0]->pass_count)
      return refuse(MCPT_ERR_INVALID_ARG, who, "shards hold different pass counts");
  }
  if (counted) {
    // conditions, so that no pixel is left with count 0
    if (!plan::is_full_frame(frame->rows, frame->H))
      return set_err(MCPT_ERR_INVALID_ARG, "mcpt_gather_rows_counted: frame target is not in row order");
    if (!shards_hold_rows_once(frame, shards, n_shards))
      return set_err(MCPT_ERR_INVALID_ARG, "mcpt_gather_rows_counted: every frame row must be held by exactly one shard");
  }
  invalidate_planes(frame);   // (the accumulator is replaced: a plain gather carries no counts)
  DeviceGuard device_guard;
  const size_t row_bytes = (size_t)frame->W * 3 * sizeof(float);
  const size_t row_counts = (size_t)frame->W * sizeof(int);
  if (counted && !frame->planes.d_count_plane) {
    HIP_OR_RETURN(hipSetDevice(frame->device));
    HIP_OR_RETURN(frame->planes.d_count_plane.alloc((size_t)frame->H * frame->W));
  }
  int most = 0;
  for (int k = 0; k < n_shards; ++k) {
    mcpt_ctx* s = shards[k];
    if (counted && s->n_local_rows > 0) {
      // the shard's counts on its stream (which waited for the previous gather's copies of this buffer)
      const size_t n_px = (size_t)s->n_local_rows * s->W;
      HIP_OR_RETURN(hipSetDevice(s->device));
      HIP_OR_RETURN(s->planes.d_gather_counts.ensure(n_px));
      HIP_OR_RETURN(mcpt_launch_counts(count_source(s), s->planes.d_gather_counts, (long long)n_px, s->stream));
    }
    const Plane planes[2] = {{frame->target.d_accum, s->target.d_accum, row_bytes}, {frame->planes.d_count_plane, s->planes.d_gather_counts, row_counts}};
    OK_OR_RETURN(copy_shard_planes(who, frame, s, planes, counted ? 2 : 1));
    most = std::max(most, s->pass_count);
  }
  if (n_shards > 0) frame->pass_count = most;   // (a plain gather's shards hold one pass count)
  frame->planes.plane_valid = counted;
  return MCPT_OK;
}

constexpr size_t kPackedBytes = 16;            // {r, g, b, count} per pixel
constexpr size_t kMapBytes = sizeof(float2);   // {se, r} per pixel

// the loads' row index (H ints) on the device: uploaded when it differs from the host copy of the
// previous load's, so mcpt_load_rows_counted and mcpt_load_rows_error_map with one index upload it once
int upload_load_index(mcpt_ctx* c, const int* src_row) {
  const size_t index_bytes = (size_t)c->H * sizeof(int);
  if (!c->planes.d_load_index) {
    HIP_OR_RETURN(c->planes.d_load_index.alloc((size_t)c->H));
    c->planes.load_index.clear();
  }
  if (c->planes.load_index.size() != (size_t)c->H || std::memcmp(c->planes.load_index.data(), src_row, index_bytes) != 0) {
    // on the stream after the loads that read the previous index; a queued upload of the previous
    // index may still read the host copy, so replacing one waits for it (a first upload does not)
    if (!c->planes.load_index.empty()) HIP_OR_RETURN(hipStreamSynchronize(c->stream));
    c->planes.load_index.assign(src_row, src_row + c->H);
    const hipError_t e = hipMemcpyAsync(c->planes.d_load_index, c->planes.load_index.data(), index_bytes, hipMemcpyHostToDevice, c->stream);
    if (e != hipSuccess) {
      c->planes.load_index.clear();
      return set_err(MCPT_ERR_HIP, "mcpt_load_rows: index upload", e);
    }
  }
  return MCPT_OK;
}

// the checks both loads make of their frame and index, after their own argument checks
int check_load(const char* who, const mcpt_ctx* c, long long src_rows, const int* src_row) {
  if (!c->has_target) return refuse(MCPT_ERR_NO_TARGET, who, "frame has no target");
  if (c->n_local_rows != c->H) return refuse(MCPT_ERR_INVALID_ARG, who, "frame target is a shard");
  if (!plan::is_full_frame(c->rows, c->H)) return refuse(MCPT_ERR_INVALID_ARG, who, "frame target is not in row order");
  if (!plan::src_rows_in_range(src_row, c->H, src_rows))
    return refuse(MCPT_ERR_INVALID_ARG, who, "a source row lies outside the packed buffer");
  return MCPT_OK;
}
}  // namespace

extern "C" {

int mcpt_copy_accum_device(mcpt_ctx* c, void* dst, size_t bytes) {
  if (!c || (!dst && bytes)) return mcpt_err_bare(MCPT_ERR_INVALID_ARG);
  if (!c->has_target) return mcpt_err_bare(MCPT_ERR_NO_TARGET);
  if (bytes < c->target.d_accum.bytes()) return set_err(MCPT_ERR_INVALID_ARG, "destination smaller than the accumulator");
  HIP_OR_RETURN(hipSetDevice(c->device));
  if (c->target.d_accum.bytes())
    HIP_OR_RETURN(hipMemcpyAsync(dst, c->target.d_accum, c->target.d_accum.bytes(), hipMemcpyDeviceToDevice, c->stream));
  return MCPT_OK;
}

int mcpt_gather_rows(mcpt_ctx* frame, mcpt_ctx* const* shards, int n_shards) {
  return gather_rows(frame, shards, n_shards, false);
}

int mcpt_gather_rows_counted(mcpt_ctx* frame, mcpt_ctx* const* shards, int n_shards) {
  return gather_rows(frame, shards, n_shards, true);
}

// The shards' error maps into the frame's gathered map plane.  The rows were
// gathered before (a row gather invalidates the plane); on any error the plane is left invalid.
int mcpt_gather_error_map(mcpt_ctx* frame, mcpt_ctx* const* shards, int n_shards) {
  const char* who = "mcpt_gather_error_map";
  if (!frame || n_shards < 0 || (n_shards > 0 && !shards)) return refuse(MCPT_ERR_INVALID_ARG, who, "bad arguments");
  frame->planes.emap_plane_valid = false;
  if (!frame->has_target) return refuse(MCPT_ERR_NO_TARGET, who, "frame has no target");
  if (frame->n_local_rows != frame->H) return refuse(MCPT_ERR_INVALID_ARG, who, "frame target is a shard");
  if (!plan::is_full_frame(frame->rows, frame->H)) return refuse(MCPT_ERR_INVALID_ARG, who, "frame target is not in row order");
  for (int k = 0; k < n_shards; ++k) OK_OR_RETURN(check_shard(who, frame, shards[k]));
  if (!shards_hold_rows_once(frame, shards, n_shards))
    return refuse(MCPT_ERR_INVALID_ARG, who, "every frame row must be held by exactly one shard");
  for (int k = 0; k < n_shards; ++k)
    if (!has_own_error_map(shards[k]))
      return refuse(MCPT_ERR_NO_STATS, who, "a shard holds no error map of its current statistics window");
  DeviceGuard device_guard;
  const size_t row_bytes = (size_t)frame->W * kMapBytes;
  if (!frame->planes.d_emap_plane && frame->H > 0 && frame->W > 0) {
    HIP_OR_RETURN(hipSetDevice(frame->device));
    HIP_OR_RETURN(frame->planes.d_emap_plane.alloc((size_t)frame->H * frame->W));
  }
  for (int k = 0; k < n_shards; ++k) {
    const Plane map = {frame->planes.d_emap_plane, shards[k]->stats.d_emap, row_bytes};
    OK_OR_RETURN(copy_shard_planes(who, frame, shards[k], &map, 1));
  }
  frame->planes.emap_plane_valid = true;
  return MCPT_OK;
}

// ---- the multi-process gathers' two ends
int mcpt_pass_count(mcpt_ctx* c, int* pass_count) {
  if (!c || !pass_count) return mcpt_err_bare(MCPT_ERR_INVALID_ARG);
  if (!c->has_target) return mcpt_err_bare(MCPT_ERR_NO_TARGET);
  *pass_count = c->pass_count;
  return MCPT_OK;
}

int mcpt_pack_counted_device(mcpt_ctx* c, void* dst, size_t bytes) {
  if (!c) return mcpt_err_bare(MCPT_ERR_INVALID_ARG);
  if (!c->has_target) return mcpt_err_bare(MCPT_ERR_NO_TARGET);
  const size_t need = (size_t)c->n_local_rows * c->W * kPackedBytes;
  if (bytes < need) return set_err(MCPT_ERR_INVALID_ARG, "mcpt_pack_counted_device: destination smaller than local pixels x 16 bytes");
  if (need == 0) return MCPT_OK;
  if (!dst || ((uintptr_t)dst & (kPackedBytes - 1)))
    return set_err(MCPT_ERR_INVALID_ARG, "mcpt_pack_counted_device: destination must be a 16-byte aligned device pointer");
  HIP_OR_RETURN(hipSetDevice(c->device));
  HIP_OR_RETURN(mcpt_launch_pack_counted(count_source(c), c->n_local_rows, c->target.d_accum, dst, c->stream));
  return MCPT_OK;
}

int mcpt_load_rows_counted(mcpt_ctx* c, const void* src, long long src_rows, const int* src_row, int pass_count) {
  if (!c || !src || !src_row || pass_count <= 0 || ((uintptr_t)src & (kPackedBytes - 1)))
    return set_err(MCPT_ERR_INVALID_ARG, "mcpt_load_rows_counted: bad arguments (16-byte aligned source, pass_count > 0)");
  OK_OR_RETURN(check_load("mcpt_load_rows_counted", c, src_rows, src_row));
  invalidate_planes(c);   // (the accumulator is replaced)
  if (c->H == 0 || c->W == 0) return MCPT_OK;
  HIP_OR_RETURN(hipSetDevice(c->device));
  const size_t n_px = (size_t)c->H * c->W;
  HIP_OR_RETURN(c->planes.d_count_plane.ensure(n_px));
  OK_OR_RETURN(upload_load_index(c, src_row));
  HIP_OR_RETURN(mcpt_launch_load_rows_counted(src, c->planes.d_load_index, c->W, c->H, c->target.d_accum, c->planes.d_count_plane, c->stream));
  c->pass_count = pass_count;
  c->planes.plane_valid = true;
  return MCPT_OK;
}

// (a shard's end: the map of its own statistics window; a gathered plane is a frame's and is not packed)
int mcpt_pack_error_map_device(mcpt_ctx* c, void* dst, size_t bytes) {
  if (!c) return mcpt_err_bare(MCPT_ERR_INVALID_ARG);
  if (!c->has_target) return mcpt_err_bare(MCPT_ERR_NO_TARGET);
  if (!has_own_error_map(c))
    return set_err(MCPT_ERR_NO_STATS, "mcpt_pack_error_map_device: no error map of the current statistics window");
  const size_t need = (size_t)c->n_local_rows * c->W * kMapBytes;
  if (bytes < need) return set_err(MCPT_ERR_INVALID_ARG, "mcpt_pack_error_map_device: destination smaller than local pixels x 8 bytes");
  if (need == 0) return MCPT_OK;
  if (!dst || ((uintptr_t)dst & (kMapBytes - 1)))
    return set_err(MCPT_ERR_INVALID_ARG, "mcpt_pack_error_map_device: destination must be an 8-byte aligned device pointer");
  HIP_OR_RETURN(hipSetDevice(c->device));
  // (the map is contiguous in local row order already: a copy on the stream, behind the select)
  HIP_OR_RETURN(hipMemcpyAsync(dst, c->stats.d_emap, need, hipMemcpyDeviceToDevice, c->stream));
  return MCPT_OK;
}

int mcpt_load_rows_error_map(mcpt_ctx* c, const void* src, long long src_rows, const int* src_row) {
  if (!c) return mcpt_err_bare(MCPT_ERR_INVALID_ARG);
  c->planes.emap_plane_valid = false;   // (on any error the frame holds no gathered map)
  if (!src || !src_row || ((uintptr_t)src & (kMapBytes - 1)))
    return set_err(MCPT_ERR_INVALID_ARG, "mcpt_load_rows_error_map: bad arguments (8-byte aligned source)");
  OK_OR_RETURN(check_load("mcpt_load_rows_error_map", c, src_rows, src_row));
  if (c->H == 0 || c->W == 0) return MCPT_OK;
  HIP_OR_RETURN(hipSetDevice(c->device));
  HIP_OR_RETURN(c->planes.d_emap_plane.ensure((size_t)c->H * c->W));
  OK_OR_RETURN(upload_load_index(c, src_row));
  HIP_OR_RETURN(mcpt_launch_load_rows_error_map(src, c->planes.d_load_index, c->W, c->H, c->planes.d_emap_plane, c->stream));
  c->planes.emap_plane_valid = true;
  return MCPT_OK;
}

}  // extern "C"
