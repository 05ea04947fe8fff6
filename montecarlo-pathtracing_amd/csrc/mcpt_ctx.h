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
#include "mcpt_launch_seq.h"
#include "mcpt_owned.h"
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

using mcpt::DevBuf, mcpt::Event, mcpt::HostBuf, mcpt::Stream;

// The context.  What it holds on the device is owned by type (mcpt_owned.h), one nested struct per
// lifetime with the plain state that ends with it: ending a lifetime is `c->group = {}`.  Members are
// destroyed last to first, so the streams (own_stream, the lanes', the pools') stand before the buffers.
struct mcpt_ctx {
  int device = 0;
  Stream own_stream;
  hipStream_t stream = nullptr;     // own_stream, or the caller's (mcpt_set_stream): borrowed
  // Render lanes (round 6): the sub-launches of render calls alternate between two lanes, each with
  // its own HIP stream, segment-sum buffer and work-item order state, so that a launch's render can
  // start while the previous launch's tail still runs.  Lane i's stream and events, and what orders it
  // against `stream`: seq.lane[i] (mcpt_launch_seq.h), the context's; its buffers: to the next mcpt_set_target*.
  mcpt::LaneSeq seq;
  struct Lane {
    DevBuf<float> d_partial;        // pass-segment sums (launches spanning > 1 chunk)
    DevBuf<float> d_split_pass;     // split items: the later pieces' per-pass values
    DevBuf<float> d_steal;          // pass stealing: every pass's value (RenderParams::steal_vals)
    // work-item order (mcpt_order.hip): item costs of the lane's last ordered launch, the order
    // sorted from them (costliest first) and the launch shape it belongs to; built as a whole
    // (ensure_item_order)
    struct Order {
      DevBuf<unsigned> d_item_cost, d_cost_sorted;
      DevBuf<int> d_item_iota, d_item_perm;
      DevBuf<int> d_split_of;       // split items: item -> split index (-1: whole)
      DevBuf<int> d_split_n;        // split items: how many (from the last sort)
      DevBuf<char> d_sort_tmp;
      long long key[8] = {};
      bool valid = false;
      int age = 0;                  // launches since the order was last sorted
      long long cap() const { return (long long)d_item_perm.size(); }   // items it holds room for
    } order;
    void drop_target_sized() { d_partial.reset(); d_split_pass.reset(); d_steal.reset(); order = {}; }
  };
  Lane lanes[2];
  // stream schedule (MCPT_TRAVERSAL_STREAM): slot pool, payload queues, counters.  Lifetime: the
  // context's, but the slots and queues (4 GB by default) go once the schedule is deselected.
  struct Pools {
    Stream pool_stream[2];          // the pools' iterations overlap on two streams
    Event pool_ev[3];               // fork / join of the pool streams
    Event batch_ev[2];
    DevBuf<float> d_slots;          // SF_COUNT x slot capacity
    DevBuf<float> d_queue;          // 2 x QF_COUNT x slot capacity
    DevBuf<unsigned> d_sctr;        // SC_COUNT counters per pool
    HostBuf<unsigned> h_sctr;       // pinned: each pool's counters read back after each batch (2 x pools x SC_COUNT)
  } pools;
  int n_cu = 0;                     // compute units of the device (persistent grids)
  int stream_slots = 0;             // MCPT_STREAM_SLOTS env / mcpt_set_stream_pool (0: default)
  int stream_refill = -1;           // MCPT_STREAM_REFILL env / mcpt_set_stream_pool (-1: default)
  long long stream_iters = 0;       // iterations of the last stream render (diagnostics)
  // scene (device records).  Lifetime: one mcpt_upload_scene to the next.
  struct Scene {
    DevBuf<float4> d_nodes;
    DevBuf<int> d_leaves, d_ptype;
    DevBuf<float4> d_prims;
    bool has_scene = false;
  } scene;
  int n_prims = 0, depth = 0, nb_emissive = 0;
  // triangle meshes.  Lifetime: one mcpt_upload_meshes to the next, or the next mcpt_upload_scene.
  struct Meshes {
    DevBuf<int4> d_minfo;
    DevBuf<float4> d_mpairs;        // mesh BVH child-pair records (SceneT::mpairs), then the leaf records
    float4* d_mleaftris = nullptr;  // mesh leaf triangle records (SceneT::mleaftris): points into d_mpairs
    DevBuf<int4> d_mtris;
    DevBuf<float4> d_mverts, d_mnorms;
    int n_meshes = 0;
    // what a refit (mcpt_refit.hip) needs of the upload: per mesh the device info
    // (first pair slot, first leaf, depth, first triangle), how many leaves hold a triangle and
    // whether some leaf pair holds none (such a mesh cannot be refitted); the records' sizes
    std::vector<int4> info;
    std::vector<int> leaf_tris;
    std::vector<char> empty_pair;
    size_t n_pair_f4 = 0, n_leaf_f4 = 0;
    DevBuf<float4> d_refit_scratch; // subtree roots between a refit's stages: sized at the first refit
    DevBuf<float> d_vert_staging;   // mcpt_update_mesh_vertices: the host arrays on their way
    Event refit_ev[2];              // around the last refit that asked for its record
    // what a rebuild (mcpt_rebuild.hip) needs of the upload: per mesh its triangle
    // count, the smallest and largest vertex id its triangles use, and its vertex range (first,
    // count; count 0 until mcpt_set_mesh_vertex_counts); the sort's scratch, sized at the first
    // rebuild for the largest mesh
    std::vector<int> n_tris, vert_lo, vert_hi, vert_first, vert_count;
    DevBuf<unsigned> d_sort_ckey;   // 3 x n: the centre keys per axis, by triangle id
    DevBuf<unsigned long long> d_sort_key;   // n: (range << 32) | axis key of the round, by triangle id
    DevBuf<int> d_sort_ids[2];      // the order, ping-pong
    DevBuf<unsigned> d_sort_hist;   // 256 digits x workgroups, digit-major
    DevBuf<int> d_tri_staging;      // mcpt_rebuild_mesh: the host's triangle rows on their way
    Event rebuild_ev[3];            // start / sort end / refit end of the last rebuild that asked for its record
  } meshes;
  int flat_face = 0;
  std::vector<int> mesh_ids;     // per primitive: mesh id of a CODE_MESH record, else -1
  // framebuffer.  Lifetime: the context's, resized by mcpt_set_target*.
  struct Target {
    DevBuf<float> d_accum;          // 3 floats per local pixel
    DevBuf<int> d_rows;             // global row of each local row (n_local_rows)
  } target;
  int W = 0, H = 0, band_rows = 1, world = 1, rank = 0, n_local_rows = 0;
  std::vector<int> rows;
  int pass_count = 0;
  bool has_target = false;
  DevBuf<unsigned long long> d_events;
  mcpt::TimingRing ring;            // the events of the last render calls (mcpt_launch_seq.h)
  int pass_split = 0;               // the last render call ran one segment per pass (launch())
  size_t partial_budget = mcpt::plan::kDefaultPartialBudget;
  int traversal = MCPT_TRAVERSAL_AUTO;
  mcpt::plan::Tuner tuner;          // AUTO schedule: its trials and decision (mcpt_plan.h), overlap, BVH depth
  int walk_exit = -1;               // mcpt_set_walk_exit; -1: by BVH depth
  int leaf_batch = -1;              // MCPT_LEAF_BATCH env (tuning); -1: default
  // guide buffers and the à-trous denoiser (mcpt_denoise.hip), 80 B per local pixel.  Lifetime: the
  // first mcpt_render_guides / mcpt_denoise after a mcpt_set_target* to the next mcpt_set_target*.
  struct Denoise {
    DevBuf<float4> d_guide;         // 2 per pixel: {N, key} {P, dist}
    DevBuf<float4> d_albedo;
    DevBuf<float4> d_dn[2];         // the filter's ping-pong colour buffers
    bool guides_valid = false;      // rendered since the last change of target, scene, meshes, flat_face
    int dn_result = -1;             // which of d_dn holds the last mcpt_denoise's result (-1: none)
    int dn_iters = -1;              // its iterations (-1: none timed)
    int dn_lds_mask = 0;            // bit s: its iteration s ran the LDS-tile kernel
    bool dn_variance = false;       // it was a mcpt_denoise*_variance: the result's .w holds the variance
    bool guides_timed = false;
    Event guide_ev[2];
    Event dn_ev[10];                // before the first iteration, then after each (<= 8); [9]: before the average
  } denoise;
  // noise statistics (mcpt_stats.hip), 24 B per local pixel, with the rings of a
  // queued adaptive run.  Lifetime: mcpt_stats_begin to mcpt_stats_end or the next mcpt_set_target*.
  struct Stats {
    DevBuf<float4> d_stats;         // per pixel {Yacc, S2, Ybase, 0}
    DevBuf<float2> d_emap;          // per pixel {se, r} of the last mcpt_convergence
    DevBuf<unsigned long long> d_conv;     // the partial frame records the error kernel reduces into
    DevBuf<unsigned long long> d_conv_f;   // the filtered select's partial records (as d_conv)
    // a queued adaptive run (mcpt_adaptive_run*): every select of a run reduces into
    // its own slice of a ring of kAdaptiveRunMaxRounds x kStatsRecWords words (the filtered selects'
    // step C into a second ring) and its list length is copied into d_run_len beside them
    DevBuf<unsigned long long> d_run_rec, d_run_rec_f;
    DevBuf<int> d_run_len;
    bool stats_on = false;
    long long stats_passes = 0;     // N: passes in the window
    int stats_batches = 0;          // B: batches in the window
    bool emap_valid = false;        // d_emap was written in this window
    bool stats_update_timed = false, stats_error_timed = false;
    Event stats_ev[4];              // around the last batch update [0, 1] and the last error kernel [2, 3]
    Event run_ev[2];                // around the last queued run
  } stats;
  // adaptive sampling of 8x8 blocks (mcpt_adaptive.hip), 12 B per block.  Lifetime:
  // mcpt_adaptive_begin to mcpt_adaptive_end, mcpt_stats_end or the next mcpt_set_target*.
  struct Adaptive {
    bool ad_on = false;
    DevBuf<int> d_ad_flags;         // per block: 1 active, 0 retired
    DevBuf<int> d_ad_passes;        // per block: passes since mcpt_adaptive_begin
    DevBuf<int> d_ad_list;          // the active block ids, ascending; [n_blocks]: the list's length
    int ad_blocks_x = 0, ad_n_blocks = 0;
    int ad_n_list = 0;              // the list's length (read back by the last select)
    int ad_p0 = 0;                  // the accumulator's pass count at mcpt_adaptive_begin
    int ad_min_passes = 0;
    bool ad_select_timed = false, ad_render_timed = false;
    bool ad_select_split = false;   // the last select was a filtered one: its time is [0, 1] + [4, 5]
    // around the last select [0, 1] and the last adaptive render [2, 3]; a filtered select
    // (DESIGN.md §3.9.2): [0, 1] around its step A, [4, 5] around its step C and the scan
    Event ad_ev[6];
  } adaptive;
  // what the gathers store about a frame's pixels, each allocated by the first
  // call that fills it.  Lifetime: to the next mcpt_set_target*; valid until the accumulator changes.
  struct Planes {
    DevBuf<int> d_count_plane;      // per-pixel sample counts of a gathered frame (mcpt_gather_rows_counted)
    bool plane_valid = false;
    // a shard's own counts for a counted gather: the peer copies read them, and the shard's stream
    // waits for those copies before its next work
    DevBuf<int> d_gather_counts;
    // mcpt_load_rows_counted's row index (H ints): uploaded when it differs from the host copy kept here
    DevBuf<int> d_load_index;
    std::vector<int> load_index;
    DevBuf<float2> d_emap_plane;    // the gathered error map (mcpt_gather_error_map, mcpt_load_rows_error_map)
    bool emap_plane_valid = false;
    DevBuf<unsigned long long> d_emap_rec;   // mcpt_error_map_record's partial records (as d_conv)
  } planes;
  // temporal reprojection (mcpt_temporal.hip): per pixel of a full frame the
  // integrated {rgb, variance} (16 B), the history length (4 B) and the guides of the frame the history
  // was made with (32 B), the first two twice (the kernel reads one set and writes the other), the
  // guides twice in the ping-pong form and once in the copy form: 104 / 72 B per pixel.  Lifetime:
  // mcpt_temporal_begin to mcpt_temporal_end or the next mcpt_set_target*.
  struct Temporal {
    bool tp_on = false;
    bool tp_copy = false;           // the history's guides are copied behind the kernel (else ping-pong)
    DevBuf<float4> d_tp_c[2];
    DevBuf<int> d_tp_len[2];
    DevBuf<float4> d_tp_g[2];       // [1] empty in the copy form
    int tp_cur = 0;                 // which set holds the history
    long long tp_frames = 0;        // accumulates since the history was last empty (0: it is empty)
    DevBuf<unsigned long long> d_tp_rec;   // the accumulate kernel's partial records (as d_conv)
    bool tp_timed = false;
    Event tp_ev[3];                 // before the kernel, behind it, behind the guides' copy
  } temporal;
};

inline int env_int(const char* name, int dflt) {
  const char* v = std::getenv(name);
  return v ? std::atoi(v) : dflt;
}

// the accumulator changes: what a gather stored about its pixels (the count plane, the gathered
// error map) no longer describes it
inline void invalidate_planes(mcpt_ctx* c) { c->planes.plane_valid = false; c->planes.emap_plane_valid = false; }

// a context has per-pixel sample counts: (b) a counted gather filled the count
// plane, or (a) the adaptive mode is on; the plane describes the accumulator as long as it is valid
inline bool has_pixel_counts(const mcpt_ctx* c) { return c->planes.plane_valid || c->adaptive.ad_on; }
// ... and where they come from: the valid count plane, else the blocks' passes over p0 while the
// adaptive mode is on, else the pass count for every pixel (mcpt_internal.h: count_at)
inline mcpt::CountSource count_source(const mcpt_ctx* c) {
  mcpt::CountSource src;
  src.plane = c->planes.plane_valid ? c->planes.d_count_plane : nullptr;
  src.passes = !c->planes.plane_valid && c->adaptive.ad_on ? c->adaptive.d_ad_passes : nullptr;
  src.W = c->W; src.blocks_x = c->adaptive.ad_blocks_x;
  src.base = src.passes ? c->adaptive.ad_p0 : c->pass_count;
  return src;
}

// the error map a context holds: 2 the gathered plane while it is valid, else 1
// its own statistics window's, else 0 none; held_error_map: that map (null: none, or no pixels)
inline bool has_own_error_map(const mcpt_ctx* c) { return c->stats.stats_on && c->stats.emap_valid; }
inline int error_map_source(const mcpt_ctx* c) { return c->planes.emap_plane_valid ? 2 : has_own_error_map(c) ? 1 : 0; }
inline const float2* held_error_map(const mcpt_ctx* c) {
  const int source = error_map_source(c);
  return source == 2 ? c->planes.d_emap_plane : source == 1 ? c->stats.d_emap : nullptr;
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

inline hipError_t ensure_timing_events(Event* ev, int n) {
  hipError_t e = hipSuccess;
  for (int i = 0; i < n && e == hipSuccess; ++i) e = ev[i].ensure();
  return e;
}

inline mcpt::AdaptiveTarget adaptive_target(const mcpt_ctx* c) {
  mcpt::AdaptiveTarget t;
  t.W = c->W; t.n_local_rows = c->n_local_rows; t.blocks_x = c->adaptive.ad_blocks_x; t.n_blocks = c->adaptive.ad_n_blocks;
  t.flags = c->adaptive.d_ad_flags; t.passes = c->adaptive.d_ad_passes; t.p0 = c->adaptive.ad_p0;
  return t;
}

// a lane buffer of at least `need` bytes (grown on demand behind a wait for the stream's work)
inline int ensure_lane_bytes(mcpt_ctx* c, DevBuf<float>& buf, size_t need) {
  if (need <= buf.bytes()) return MCPT_OK;
  HIP_OR_RETURN(hipStreamSynchronize(c->stream));   // (ordered after every lane's work)
  HIP_OR_RETURN(buf.ensure((need + sizeof(float) - 1) / sizeof(float)));
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
// mcpt_refit.hip: what a refit and a rebuild (mcpt_rebuild.hip) share — the refusals and the scratch
// for meshes m0 .. m1 - 1 (`who`: the caller's name, for the detail), the refit stages of mesh m
// queued on the context's stream (*root: its root's {min, has} {max, 0} on the device, untouched for
// a mesh of depth 0), and the state a change of geometry behind the queued renders leaves
#if defined(__HIPCC__)
// std::min(a, b) / std::max(a, b): the first operand unless the comparison says otherwise
__device__ __forceinline__ float min_ab(float a, float b) { return b < a ? b : a; }
__device__ __forceinline__ float max_ab(float a, float b) { return a < b ? b : a; }
// SceneMesh::prim_bb as the host's tri_box evaluates it (std::min / std::max over {A, B, C}, then -+ 0.001)
__device__ __forceinline__ void tri_box_dev(const float4 A, const float4 B, const float4 C, float mn[3], float mx[3]) {
  mn[0] = min_ab(min_ab(A.x, B.x), C.x) - 0.001f; mx[0] = max_ab(max_ab(A.x, B.x), C.x) + 0.001f;
  mn[1] = min_ab(min_ab(A.y, B.y), C.y) - 0.001f; mx[1] = max_ab(max_ab(A.y, B.y), C.y) + 0.001f;
  mn[2] = min_ab(min_ab(A.z, B.z), C.z) - 0.001f; mx[2] = max_ab(max_ab(A.z, B.z), C.z) + 0.001f;
}
#endif
int refit_prepare(mcpt_ctx* c, int mesh_id, const char* who, int& m0, int& m1);
int refit_launch(mcpt_ctx* c, int m, const float4** root);
void geometry_changed(mcpt_ctx* c);
// mcpt_capi_post.hip: one batch of the noise statistics behind the last combine (d_count: the counted
// twin of a queued adaptive run, reading the list's length there; timed false: no events)
hipError_t stats_batch(mcpt_ctx* c, int n, const int* d_count = nullptr, bool timed = true);
