// mcpt_ctx.h — the context of the C ABI's device half and the helpers its three translation units
// share (mcpt_capi.hip: lifetime, uploads, target, render, queries; mcpt_capi_post.hip: guides and
// denoiser, noise statistics, adaptive sampling; mcpt_capi_gather.hip: what moves a shard into a
// frame), among them where a pixel's sample count comes from (count_source) and which error map the
// context holds (held_error_map): each chosen here, once.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdlib>
#include <vector>

#include "../../include/mcpt.h"
#include "mcpt_adaptive_run_plan.h"
#include "mcpt_gather_plan.h"
#include "mcpt_internal.h"
#include "mcpt_plan.h"

// records the calling thread's error detail (mcpt_capi.hip: mcpt_error_string hands it out once)
int set_err(int status, const char* what, hipError_t e = hipSuccess);

#define HIP_OR_RETURN(call)                                         \
  do {                                                              \
    hipError_t e_ = (call);                                         \
    if (e_ != hipSuccess) return set_err(MCPT_ERR_HIP, #call, e_);  \
  } while (0)

#define OK_OR_RETURN(call)                     \
  do {                                         \
    const int st_ = (call);                    \
    if (st_ != MCPT_OK) return st_;            \
  } while (0)

// render calls whose events a context keeps (mcpt_kernel_ms_back)
constexpr int kTimingRing = 64;

struct mcpt_ctx {
  int device = 0;
  hipStream_t own_stream = nullptr;
  hipStream_t stream = nullptr;
  // scene (device records)
  float4* d_nodes = nullptr;
  int* d_leaves = nullptr;
  int* d_ptype = nullptr;
  float4* d_prims = nullptr;
  int n_prims = 0, depth = 0, nb_emissive = 0;
  bool has_scene = false;
  // triangle meshes
  int4* d_minfo = nullptr;
  float4* d_mpairs = nullptr;      // mesh BVH child-pair records (SceneT::mpairs)
  float4* d_mleaftris = nullptr;   // mesh leaf triangle records (SceneT::mleaftris)
  int4* d_mtris = nullptr;
  float4* d_mverts = nullptr;
  float4* d_mnorms = nullptr;
  int n_meshes = 0, flat_face = 0;
  std::vector<int> mesh_ids;     // per primitive: mesh id of a CODE_MESH record, else -1
  // framebuffer
  float* d_accum = nullptr;
  size_t accum_bytes = 0;
  int W = 0, H = 0, band_rows = 1, world = 1, rank = 0, n_local_rows = 0;
  int* d_rows = nullptr;            // global row of each local row (n_local_rows)
  std::vector<int> rows;
  int pass_count = 0;
  bool has_target = false;
  unsigned long long* d_events = nullptr;
  // per sub-launch of a render call: (start, after the path-tracing kernel, after the combine
  // kernel); a call is split into sub-launches at chunk boundaries (partial_budget).  The last
  // kTimingRing calls keep their events (mcpt_kernel_ms_back), so a caller can time a run of
  // calls without waiting after each; ring_pos = the last call's slot.
  std::vector<hipEvent_t> evs[kTimingRing];
  int ring_n_sub[kTimingRing] = {};
  std::vector<char> ring_lane[kTimingRing];   // per sub-launch: a lane launch
  int ring_pos = 0;
  long long n_timed = 0;            // render calls timed so far
  int n_sub = 0;                    // sub-launches of the last render call
  int pass_split = 0;               // the last render call ran one segment per pass (launch())
  bool timed = false;
  size_t partial_budget = mcpt::plan::kDefaultPartialBudget;
  int traversal = MCPT_TRAVERSAL_AUTO;
  mcpt::plan::Tuner tuner;          // AUTO schedule: its trials and decision (mcpt_plan.h), overlap, BVH depth
  int walk_exit = -1;               // mcpt_set_walk_exit; -1: by BVH depth
  int leaf_batch = -1;              // MCPT_LEAF_BATCH env (tuning); -1: default
  // stream schedule (MCPT_TRAVERSAL_STREAM): slot pool, payload queues, counters
  int n_cu = 0;                     // compute units of the device (persistent grids)
  float* d_slots = nullptr;         // SF_COUNT x slot capacity
  float* d_queue = nullptr;         // 2 x QF_COUNT x slot capacity
  unsigned* d_sctr = nullptr;       // SC_COUNT counters per pool
  long long slot_cap = 0;           // slots of d_slots / d_queue
  unsigned* h_sctr = nullptr;       // pinned: each pool's counters read back after each batch (2 x pools x SC_COUNT)
  hipEvent_t batch_ev[2] = {nullptr, nullptr};
  hipStream_t pool_stream[2] = {nullptr, nullptr};   // the pools' iterations overlap on two streams
  hipEvent_t pool_ev[3] = {nullptr, nullptr, nullptr};   // fork / join of the pool streams
  int stream_slots = 0;             // MCPT_STREAM_SLOTS env / mcpt_set_stream_pool (0: default)
  int stream_refill = -1;           // MCPT_STREAM_REFILL env / mcpt_set_stream_pool (-1: default)
  long long stream_iters = 0;       // iterations of the last stream render (diagnostics)
  // Render lanes (round 6): the sub-launches of render calls alternate between two lanes, each with
  // its own HIP stream, segment-sum buffer and work-item order state, so that a launch's render
  // kernel can start while the previous launch's last workgroups still run (its tail).  The
  // combines stay in call order on `stream`; a lane's next render waits for the lane's previous
  // combine (its buffers free).  Lane launches are only used once AUTO has settled, for launches
  // of several pass segments (a one-segment launch adds into the accumulator itself).
  struct Lane {
    hipStream_t stream = nullptr;
    hipEvent_t freed = nullptr;     // on `stream` after the lane's last combine: its buffers are free
    bool freed_stale = false;       // launches in order on `stream` used the lane since (not recorded:
                                    // launch-bound calls skip the record; the next waiter records it)
    hipEvent_t tail = nullptr;      // on the lane's stream after its last operation
    float* d_partial = nullptr;     // pass-segment sums (launches spanning > 1 chunk)
    size_t partial_bytes = 0;
    // work-item order (mcpt_order.hip): item costs of the lane's last ordered launch, the order
    // sorted from them (costliest first) and the launch shape it belongs to
    unsigned* d_item_cost = nullptr;
    unsigned* d_cost_sorted = nullptr;
    int* d_item_iota = nullptr;
    int* d_item_perm = nullptr;
    int* d_split_of = nullptr;      // split items: item -> split index (-1: whole)
    float* d_split_pass = nullptr;  // split items: the later pieces' per-pass values
    float* d_steal = nullptr;       // pass stealing: every pass's value (RenderParams::steal_vals)
    size_t steal_bytes = 0;
    int* d_split_n = nullptr;       // split items: how many (from the last sort)
    void* d_sort_tmp = nullptr;
    size_t sort_tmp_bytes = 0;
    long long item_cap = 0;
    long long order_key[8] = {};
    bool order_valid = false;
    int order_age = 0;              // launches since the order was last sorted
  };
  Lane lanes[2];
  // guide buffers and the à-trous denoiser (mcpt_denoise.hip): 80 B per local pixel, allocated by
  // the first mcpt_render_guides / mcpt_denoise after a mcpt_set_target*, freed by the next one
  float4* d_guide = nullptr;        // 2 per pixel: {N, key} {P, dist}
  float4* d_albedo = nullptr;
  float4* d_dn[2] = {nullptr, nullptr};   // the filter's ping-pong colour buffers
  bool guides_valid = false;        // rendered since the last change of target, scene, meshes, flat_face
  int dn_result = -1;               // which of d_dn holds the last mcpt_denoise's result (-1: none)
  int dn_iters = -1;                // its iterations (-1: none timed)
  int dn_lds_mask = 0;              // bit s: its iteration s ran the LDS-tile kernel
  bool dn_variance = false;         // it was a mcpt_denoise*_variance: the result's .w holds the variance
  bool guides_timed = false;
  hipEvent_t guide_ev[2] = {nullptr, nullptr};
  hipEvent_t dn_ev[10] = {};        // before the first iteration, then after each (<= 8); [9]: before the average
  // noise statistics (mcpt_stats.hip): 24 B per local pixel, allocated by the first
  // mcpt_stats_begin after a mcpt_set_target*, freed by mcpt_stats_end and the next mcpt_set_target*
  float4* d_stats = nullptr;        // per pixel {Yacc, S2, Ybase, 0}
  float2* d_emap = nullptr;         // per pixel {se, r} of the last mcpt_convergence
  unsigned long long* d_conv = nullptr;   // the partial frame records the error kernel reduces into
  bool stats_on = false;
  long long stats_passes = 0;       // N: passes in the window
  int stats_batches = 0;            // B: batches in the window
  bool emap_valid = false;          // d_emap was written in this window
  bool stats_update_timed = false, stats_error_timed = false;
  hipEvent_t stats_ev[4] = {};      // around the last batch update [0, 1] and the last error kernel [2, 3]
  // adaptive sampling of 8x8 blocks (mcpt_adaptive.hip): 12 B per block, allocated
  // by mcpt_adaptive_begin, freed by mcpt_adaptive_end, mcpt_stats_end, the next mcpt_set_target*
  // and mcpt_destroy
  bool ad_on = false;
  int* d_ad_flags = nullptr;        // per block: 1 active, 0 retired
  int* d_ad_passes = nullptr;       // per block: passes since mcpt_adaptive_begin
  int* d_ad_list = nullptr;         // the active block ids, ascending; [n_blocks]: the list's length
  int ad_blocks_x = 0, ad_n_blocks = 0;
  int ad_n_list = 0;                // the list's length (read back by the last select)
  int ad_p0 = 0;                    // the accumulator's pass count at mcpt_adaptive_begin
  int ad_min_passes = 0;
  bool ad_select_timed = false, ad_render_timed = false;
  bool ad_select_split = false;     // the last select was a filtered one: its time is [0, 1] + [4, 5]
  // around the last select [0, 1] and the last adaptive render [2, 3]; a filtered select
  // (DESIGN.md §3.9.2): [0, 1] around its step A, [4, 5] around its step C and the scan
  hipEvent_t ad_ev[6] = {};
  unsigned long long* d_conv_f = nullptr;   // the filtered select's partial records (as d_conv; its lifetime)
  // a queued adaptive run (mcpt_adaptive_run*): every select of a run reduces into
  // its own slice of a ring of kAdaptiveRunMaxRounds x kStatsRecWords words (the filtered selects'
  // step C into a second ring) and its list length is copied into d_run_len beside them; allocated
  // by the first run, the statistics buffers' lifetime.  run_ev: around the last run.
  unsigned long long* d_run_rec = nullptr;
  unsigned long long* d_run_rec_f = nullptr;
  int* d_run_len = nullptr;
  hipEvent_t run_ev[2] = {nullptr, nullptr};
  // per-pixel sample counts of a gathered frame (mcpt_gather_rows_counted): the
  // count plane, 4 B per local pixel, allocated by the first counted gather after a
  // mcpt_set_target*, freed by the next one and mcpt_destroy; valid until the accumulator changes
  int* d_count_plane = nullptr;
  bool plane_valid = false;
  // a shard's own counts for a counted gather (4 B per local pixel, same lifetime): the peer copies
  // read them, and the shard's stream waits for those copies before its next work
  int* d_gather_counts = nullptr;
  // mcpt_load_rows_counted's row index (H ints, same lifetime): uploaded when it differs from the
  // host copy kept here
  int* d_load_index = nullptr;
  std::vector<int> load_index;
  // the gathered error map of a frame (mcpt_gather_error_map, mcpt_load_rows_error_map; DESIGN.md
  // §3.9.1): H x W x {se, r}, 8 B per pixel, allocated by the first call that fills it after a
  // mcpt_set_target*, freed with the count plane; valid until the accumulator changes
  float2* d_emap_plane = nullptr;
  bool emap_plane_valid = false;
  // mcpt_error_map_record's partial records (as d_conv; the plane's lifetime)
  unsigned long long* d_emap_rec = nullptr;
  // temporal reprojection (mcpt_temporal.hip): per pixel of a full frame the
  // integrated {rgb, variance} (16 B), the history length (4 B) and the guides of the frame the history
  // was made with (32 B), the first two twice (the kernel reads one set and writes the other), the
  // guides twice in the ping-pong form and once in the copy form: 104 / 72 B per pixel.  Allocated by
  // mcpt_temporal_begin, freed by mcpt_temporal_end, the next mcpt_set_target* and mcpt_destroy.
  bool tp_on = false;
  bool tp_copy = false;             // the history's guides are copied behind the kernel (else ping-pong)
  float4* d_tp_c[2] = {nullptr, nullptr};
  int* d_tp_len[2] = {nullptr, nullptr};
  float4* d_tp_g[2] = {nullptr, nullptr};   // [1] null in the copy form
  int tp_cur = 0;                   // which set holds the history
  long long tp_frames = 0;          // accumulates since the history was last empty (0: it is empty)
  unsigned long long* d_tp_rec = nullptr;   // the accumulate kernel's partial records (as d_conv)
  bool tp_timed = false;
  hipEvent_t tp_ev[3] = {};         // before the kernel, behind it, behind the guides' copy
  int next_lane = 0;               // the lane of the next sub-launch
  int prev_lane = -1;               // the lane of the previous sub-launch if it was a lane launch, else -1
};

inline int env_int(const char* name, int dflt) {
  const char* v = std::getenv(name);
  return v ? std::atoi(v) : dflt;
}

inline void free_denoise(mcpt_ctx* c) {
  (void)hipFree(c->d_guide); (void)hipFree(c->d_albedo); (void)hipFree(c->d_dn[0]); (void)hipFree(c->d_dn[1]);
  c->d_guide = nullptr; c->d_albedo = nullptr; c->d_dn[0] = nullptr; c->d_dn[1] = nullptr;
  c->guides_valid = false; c->dn_result = -1; c->dn_iters = -1; c->dn_variance = false; c->guides_timed = false;
}

inline void free_stats(mcpt_ctx* c) {
  (void)hipFree(c->d_stats); (void)hipFree(c->d_emap); (void)hipFree(c->d_conv); (void)hipFree(c->d_conv_f);
  c->d_stats = nullptr; c->d_emap = nullptr; c->d_conv = nullptr; c->d_conv_f = nullptr;
  (void)hipFree(c->d_run_rec); (void)hipFree(c->d_run_rec_f); (void)hipFree(c->d_run_len);
  c->d_run_rec = nullptr; c->d_run_rec_f = nullptr; c->d_run_len = nullptr;
  c->stats_on = false; c->stats_passes = 0; c->stats_batches = 0; c->emap_valid = false;
  c->stats_update_timed = false; c->stats_error_timed = false;
}

inline void free_adaptive(mcpt_ctx* c) {
  (void)hipFree(c->d_ad_flags); (void)hipFree(c->d_ad_passes); (void)hipFree(c->d_ad_list);
  c->d_ad_flags = nullptr; c->d_ad_passes = nullptr; c->d_ad_list = nullptr;
  c->ad_on = false; c->ad_n_blocks = 0; c->ad_n_list = 0;
  c->ad_select_timed = false; c->ad_render_timed = false; c->ad_select_split = false;
}

inline void free_count_plane(mcpt_ctx* c) {
  (void)hipFree(c->d_count_plane); (void)hipFree(c->d_gather_counts); (void)hipFree(c->d_load_index);
  (void)hipFree(c->d_emap_plane); (void)hipFree(c->d_emap_rec);
  c->d_count_plane = nullptr; c->d_gather_counts = nullptr; c->d_load_index = nullptr;
  c->d_emap_plane = nullptr; c->d_emap_rec = nullptr;
  c->load_index.clear();
  c->plane_valid = false;
  c->emap_plane_valid = false;
}

inline void free_temporal(mcpt_ctx* c) {
  for (int k = 0; k < 2; ++k) {
    (void)hipFree(c->d_tp_c[k]); (void)hipFree(c->d_tp_len[k]); (void)hipFree(c->d_tp_g[k]);
    c->d_tp_c[k] = nullptr; c->d_tp_len[k] = nullptr; c->d_tp_g[k] = nullptr;
  }
  (void)hipFree(c->d_tp_rec);
  c->d_tp_rec = nullptr;
  c->tp_on = false; c->tp_cur = 0; c->tp_frames = 0; c->tp_timed = false;
}

// the accumulator changes: what a gather stored about its pixels (the count plane, the gathered
// error map) no longer describes it
inline void invalidate_planes(mcpt_ctx* c) { c->plane_valid = false; c->emap_plane_valid = false; }

// a context has per-pixel sample counts: (b) a counted gather filled the count
// plane, or (a) the adaptive mode is on; the plane describes the accumulator as long as it is valid
inline bool has_pixel_counts(const mcpt_ctx* c) { return c->plane_valid || c->ad_on; }
// ... and where they come from: the valid count plane, else the blocks' passes over p0 while the
// adaptive mode is on, else the pass count for every pixel (mcpt_internal.h: count_at)
inline mcpt::CountSource count_source(const mcpt_ctx* c) {
  mcpt::CountSource src;
  src.plane = c->plane_valid ? c->d_count_plane : nullptr;
  src.passes = !c->plane_valid && c->ad_on ? c->d_ad_passes : nullptr;
  src.W = c->W; src.blocks_x = c->ad_blocks_x;
  src.base = src.passes ? c->ad_p0 : c->pass_count;
  return src;
}

// the error map a context holds: 2 the gathered plane while it is valid, else 1
// its own statistics window's, else 0 none; held_error_map: that map (null: none, or no pixels)
inline bool has_own_error_map(const mcpt_ctx* c) { return c->stats_on && c->emap_valid; }
inline int error_map_source(const mcpt_ctx* c) { return c->emap_plane_valid ? 2 : has_own_error_map(c) ? 1 : 0; }
inline const float2* held_error_map(const mcpt_ctx* c) {
  const int source = error_map_source(c);
  return source == 2 ? c->d_emap_plane : source == 1 ? c->d_emap : nullptr;
}

// identity of a context's target for its checkpoints: FNV-1a (64 bit) over its image row ids
inline unsigned long long rows_hash(const mcpt_ctx* c) {
  unsigned long long h = 1469598103934665603ULL;
  for (int y : c->rows)
    for (int b = 0; b < 4; ++b) {
      h ^= (unsigned long long)(((unsigned)y >> (8 * b)) & 0xFFu);
      h *= 1099511628211ULL;
    }
  return h ? h : 1;   // 0 means "no identity" in the file
}

inline hipError_t ensure_timing_events(hipEvent_t* ev, int n) {
  for (int i = 0; i < n; ++i)
    if (!ev[i]) {
      const hipError_t e = hipEventCreate(&ev[i]);
      if (e != hipSuccess) return e;
    }
  return hipSuccess;
}

inline mcpt::AdaptiveTarget adaptive_target(const mcpt_ctx* c) {
  mcpt::AdaptiveTarget t;
  t.W = c->W; t.n_local_rows = c->n_local_rows; t.blocks_x = c->ad_blocks_x; t.n_blocks = c->ad_n_blocks;
  t.flags = c->d_ad_flags; t.passes = c->d_ad_passes; t.p0 = c->ad_p0;
  return t;
}

// a lane buffer of at least `need` bytes (grown on demand; a failed allocation leaves have = 0)
inline int ensure_lane_bytes(mcpt_ctx* c, float*& buf, size_t& have, size_t need) {
  if (need <= have) return MCPT_OK;
  HIP_OR_RETURN(hipStreamSynchronize(c->stream));   // (ordered after every lane's work)
  (void)hipFree(buf);
  buf = nullptr;
  have = 0;
  HIP_OR_RETURN(hipMalloc(&buf, need));
  have = need;
  return MCPT_OK;
}

// mcpt_capi.hip: the checks every render entry point starts with (`who`: its name, for the
// detail of a bad argument; args_ok: its own argument checks), a launch's scene / target / camera
// fields and its pass range and constants, the checked build's wait after a sub-launch
int check_renderable(const mcpt_ctx* c, bool args_ok, const char* who);
void scene_params(const mcpt_ctx* c, const float* invPV, const float* invV, mcpt::RenderParams& p);
void pass_params(int first_pass, int n_passes, float date, int bounces, float refract_ind, int variant,
                 mcpt::RenderParams& p);
int checked_sub_launch(mcpt_ctx* c, int k, int n_sub, const mcpt::RenderParams& p);
// mcpt_capi_post.hip: one batch of the noise statistics behind the last combine (d_count: the counted
// twin of a queued adaptive run, reading the list's length there; timed false: no events)
hipError_t stats_batch(mcpt_ctx* c, int n, const int* d_count = nullptr, bool timed = true);
