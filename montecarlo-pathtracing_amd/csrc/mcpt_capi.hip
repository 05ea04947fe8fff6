// mcpt_capi.hip — C ABI, device half: context, scene upload (repack to device records),
// framebuffer / row-band sharding, render launches, accumulator read-back.  (What runs on a
// rendered accumulator: mcpt_capi_post.hip; what moves a shard into a frame: mcpt_capi_gather.hip.)
//
// Replaces the GL state of the reference's render path: Texture2D uploads
// (bvh_gpu/gpu_bvh_scene.cpp:143-160), the RGB32F FBO + blend (MontecarloGPU/montecarlo.cpp:
// 384-386, 420-467), the uniform ABI (montecarlo.cpp:439-453) and the corner-ray vertex
// shader (shaders/raytracer.vert:9-22, evaluated here once per launch on the host).
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <new>

#include "mcpt_ctx.h"
#include "mcpt_math.h"

namespace plan = mcpt::plan;
static_assert(plan::kCandLane == MCPT_TRAVERSAL_LANE && plan::kCandWave == MCPT_TRAVERSAL_WAVE &&
              plan::kCandStream == MCPT_TRAVERSAL_STREAM, "candidates 1..3 are the traversal modes");

// The detail of the calling thread's last failed call (set_err), with its status.  "fresh"
// until mcpt_error_string hands it out once or a later call fails without a detail (every bare
// error return goes through mcpt_err_bare, which drops it), so a detail is never attached to a
// later error that did not set one (HIP errors keep theirs: mcpt_error_string(MCPT_ERR_HIP)
// always returns it).
static thread_local char g_last_error[256] = "";
static thread_local char g_detail[320] = "";
static thread_local int g_last_status = 0;
static thread_local bool g_fresh = false;

int set_err(int status, const char* what, hipError_t e) {
  if (e != hipSuccess)
    std::snprintf(g_last_error, sizeof(g_last_error), "%s: %s", what, hipGetErrorString(e));
  else
    std::snprintf(g_last_error, sizeof(g_last_error), "%s", what);
  g_last_status = status;
  g_fresh = true;
  return status;
}

int mcpt_err_bare(int status) {
  g_fresh = false;
  return status;
}

// schedule candidate of the next launch (`segs`: its pass segments; mcpt_plan.h)
static int resolve_candidate(const mcpt_ctx* c, long long segs) {
  return c->traversal != MCPT_TRAVERSAL_AUTO ? c->traversal : c->tuner.next_candidate(segs);
}
static bool schedule_settled(const mcpt_ctx* c) { return c->traversal != MCPT_TRAVERSAL_AUTO || c->tuner.tune_choice != 0; }

static void reset_tuning(mcpt_ctx* c) {
  for (auto& L : c->lanes) L.order.valid = false;   // a new scene / target: item costs start over
  c->tuner.reset();
}

// collect the timing of the oldest pending trial (waits for it) while more than `keep` are
// pending (plan::Tuner::collect decides)
static hipError_t collect_tuning(mcpt_ctx* c, int keep) {
  while (c->tuner.n_pend > keep) {
    const plan::Tuner::Pending t0 = c->tuner.pop_oldest();
    float ms = 0.0f, ms_combine = 0.0f;
    hipError_t e = c->ring.launch_ms(t0.slot, &ms, &ms_combine);
    if (e != hipSuccess) return e;
    c->tuner.collect(t0.cand, t0.shape, (double)ms * 1e6 / t0.samples);
  }
  return hipSuccess;
}

extern "C" {

const char* mcpt_error_string(int status) {
  if (status != MCPT_ERR_HIP && status != MCPT_OK && g_fresh && g_last_status == status) {
    g_fresh = false;
    const char* base = status == MCPT_ERR_INVALID_ARG ? "invalid argument"
                       : status == MCPT_ERR_NO_SCENE  ? "no scene uploaded"
                       : status == MCPT_ERR_NO_TARGET ? "no render target"
                       : status == MCPT_ERR_BAD_SCENE ? "malformed scene buffers"
                       : status == MCPT_ERR_NO_GUIDES ? "no current guide buffers"
                       : status == MCPT_ERR_NO_STATS  ? "no noise statistics"
                       : status == MCPT_ERR_NO_ADAPTIVE ? "adaptive mode is off"
                       : status == MCPT_ERR_NO_TEMPORAL ? "temporal mode is off"
                                                      : "error";
    std::snprintf(g_detail, sizeof(g_detail), "%s (%s)", base, g_last_error);
    return g_detail;
  }
  switch (status) {
    case MCPT_OK: return "ok";
    case MCPT_ERR_INVALID_ARG: return "invalid argument";
    case MCPT_ERR_NO_SCENE: return "no scene uploaded";
    case MCPT_ERR_NO_TARGET: return "no render target (call mcpt_set_target)";
    case MCPT_ERR_HIP: return g_last_error[0] ? g_last_error : "HIP runtime error";
    case MCPT_ERR_NOT_FINALIZED: return "scene not finalized";
    case MCPT_ERR_BAD_SCENE: return "malformed scene buffers";
    case MCPT_ERR_NO_GUIDES: return "no current guide buffers (call mcpt_render_guides)";
    case MCPT_ERR_NO_STATS: return "no noise statistics (mcpt_stats_begin, two batches, mcpt_convergence)";
    case MCPT_ERR_NO_ADAPTIVE: return "adaptive mode is off (mcpt_adaptive_begin)";
    case MCPT_ERR_NO_TEMPORAL: return "temporal mode is off (mcpt_temporal_begin)";
    default: return "unknown status";
  }
}

int mcpt_version(void) { return 2; }

int mcpt_build_flags(void) {
  int f = 0;
#ifdef MCPT_CHECKED
  f |= MCPT_BUILD_CHECKED;
#endif
#ifdef MCPT_STAMPS
  f |= MCPT_BUILD_STAMPS;
#endif
#ifdef MCPT_LANESTATS
  f |= MCPT_BUILD_LANESTATS;
#endif
#ifdef MCPT_BLOCKTIMES
  f |= MCPT_BUILD_BLOCKTIMES;
#endif
#if MCPT_DRIVER_MATH   // (mcpt_math.h: 0 in the shipped build)
  f |= MCPT_BUILD_DRIVER_MATH;
#endif
  return f;
}

int mcpt_create(int device_ordinal, mcpt_ctx** out) {
  if (!out) return mcpt_err_bare(MCPT_ERR_INVALID_ARG);
  *out = nullptr;
  int n = 0;
  HIP_OR_RETURN(hipGetDeviceCount(&n));
  if (device_ordinal < 0 || device_ordinal >= n) return set_err(MCPT_ERR_INVALID_ARG, "device ordinal out of range");
  HIP_OR_RETURN(hipSetDevice(device_ordinal));
  mcpt_ctx* c = new (std::nothrow) mcpt_ctx();
  if (!c) return mcpt_err_bare(MCPT_ERR_INVALID_ARG);
  c->leaf_batch = env_int("MCPT_LEAF_BATCH", -1);   // tuning hook (same results for any value)
  c->stream_slots = env_int("MCPT_STREAM_SLOTS", 0);
  c->stream_refill = env_int("MCPT_STREAM_REFILL", -1);
  c->device = device_ordinal;
  if (hipDeviceGetAttribute(&c->n_cu, hipDeviceAttributeMultiprocessorCount, device_ordinal) != hipSuccess ||
      c->n_cu <= 0)
    c->n_cu = 256;
  // the context's own stream (combines, copies) at the device's greatest priority: with render
  // lanes its short kernels are dispatched ahead of the next render's waiting workgroups
  int prio_least = 0, prio_greatest = 0;
  if (hipDeviceGetStreamPriorityRange(&prio_least, &prio_greatest) != hipSuccess) prio_greatest = 0;
  hipError_t e = c->own_stream.ensure_with_priority(hipStreamNonBlocking, prio_greatest);
  if (e == hipSuccess) e = c->seq.create(c->own_stream);
  c->tuner.overlap = env_int("MCPT_OVERLAP", 1);
  if (const char* pb = std::getenv("MCPT_PARTIAL_BYTES")) c->partial_budget = (size_t)std::strtoull(pb, nullptr, 10);
#ifdef MCPT_BLOCKTIMES
  // diagnostic build: per-wave (start, end) clock pairs after the debug slots
  static_assert(mcpt::kBlockTimeBase == MCPT_DEBUG_SLOTS, "block times follow the debug slots");
  constexpr size_t kEventSlots = MCPT_DEBUG_SLOTS + mcpt::kBlockTimeSlots;
#else
  constexpr size_t kEventSlots = MCPT_DEBUG_SLOTS;
#endif
  if (e == hipSuccess) e = c->d_events.alloc(kEventSlots);
  if (e == hipSuccess) e = hipMemset(c->d_events, 0, sizeof(unsigned long long) * kEventSlots);
  if (e != hipSuccess) { mcpt_destroy(c); return set_err(MCPT_ERR_HIP, "mcpt_create", e); }
  c->stream = c->own_stream;
  *out = c;
  return MCPT_OK;
}

int mcpt_destroy(mcpt_ctx* c) {
  if (!c) return MCPT_OK;
  (void)hipSetDevice(c->device);
  if (c->stream) (void)hipStreamSynchronize(c->stream);
  for (auto& L : c->seq.lane) if (L.stream) (void)hipStreamSynchronize(L.stream);
  delete c;   // (every member frees what it owns: mcpt_owned.h)
  return MCPT_OK;
}

int mcpt_upload_scene(mcpt_ctx* c, const float* prims, int n_prims, const float* nodes, const int* leaves,
                      int depth, int nb_emissives) {
  // n_prims < 2^24: the kernel packs a hit's primitive index, shape and face in one word
  if (!c || !prims || !nodes || !leaves || n_prims <= 0 || n_prims >= (1 << 24) || depth < 0 || depth > 24)
    return set_err(MCPT_ERR_INVALID_ARG, "mcpt_upload_scene: bad arguments");
  const int n_leaf = 1 << depth, n_node = 2 * n_leaf - 1;
  for (int i = 0; i < n_leaf; ++i)
    if (leaves[i] < -1 || leaves[i] >= n_prims) return set_err(MCPT_ERR_BAD_SCENE, "leaf id out of range");
  // subtree-holds-a-primitive flags (bottom-up over the implicit heap): empty subtrees
  // are never visited by the kernel (they cannot change the closest hit)
  std::vector<char> has(n_node, 0);
  for (int i = n_node - 1; i >= 0; --i)
    has[i] = (i >= n_leaf - 1) ? (leaves[i - (n_leaf - 1)] >= 0) : (has[2 * i + 1] || has[2 * i + 2]);
  // nodes → (centre, has-prim flag) (half-width, 0) (1/half-width, 0): raytracer_func.frag:319-320
  // hoisted to upload
  std::vector<float4> hn((size_t)n_node * mcpt::kNodeF4);
  for (int i = 0; i < n_node; ++i) {
    const float* b = nodes + (size_t)i * 6;
    float cx = (b[0] + b[3]) / 2.0f, cy = (b[1] + b[4]) / 2.0f, cz = (b[2] + b[5]) / 2.0f;
    float wx = 0.5f * (b[3] - b[0]), wy = 0.5f * (b[4] - b[1]), wz = 0.5f * (b[5] - b[2]);
    hn[(size_t)i * 3 + 0] = make_float4(cx, cy, cz, has[i] ? 1.0f : 0.0f);
    hn[(size_t)i * 3 + 1] = make_float4(wx, wy, wz, 0.0f);
    hn[(size_t)i * 3 + 2] = make_float4(1.0f / wx, 1.0f / wy, 1.0f / wz, 0.0f);
  }
  // prims → rows of the inverse and of the transform (the shader uses .xyz of mat4·v).  A
  // CODE_MESH record's transform rows are its mesh transform (texel 8-11, read_mesh_transfo:
  // the only transform Mesh_intersect / mesh_inter_geom_info use); its mesh id (texel 12 .y,
  // "mesh_line") goes into ptype's high bits.
  std::vector<int> ht(n_prims), mesh_ids(n_prims, -1);
  std::vector<float4> hp((size_t)n_prims * mcpt::kPrimF4);
  for (int i = 0; i < n_prims; ++i) {
    const float* r = prims + (size_t)i * 64;
    float tcode = r[48];
    if (!(tcode >= 0.0f && tcode <= 5.0f) || tcode != (float)(int)tcode)
      return set_err(MCPT_ERR_BAD_SCENE, "primitive type code not in 0..5");
    ht[i] = (int)tcode;
    const float* trf = r;
    if (ht[i] == 0) {
      const float ml = r[49];
      if (!(ml >= 0.0f && ml < (float)(1 << 26)) || ml != (float)(int)ml)
        return set_err(MCPT_ERR_BAD_SCENE, "mesh primitive without a valid mesh id");
      mesh_ids[i] = (int)ml;
      ht[i] |= mesh_ids[i] << 4;
      trf = r + 32;
    }
    float4* o = &hp[(size_t)i * mcpt::kPrimF4];
    for (int row = 0; row < 3; ++row) {
      const float* inv = r + 16;
      o[row] = make_float4(inv[row], inv[4 + row], inv[8 + row], inv[12 + row]);
      o[3 + row] = make_float4(trf[row], trf[4 + row], trf[8 + row], trf[12 + row]);
    }
    o[6] = make_float4(r[52], r[53], r[54], r[55]);
    o[7] = make_float4(r[56], r[57], r[58], r[59]);
  }
  HIP_OR_RETURN(hipSetDevice(c->device));
  HIP_OR_RETURN(hipStreamSynchronize(c->stream));
  c->scene = {};   // (the previous scene goes first: the two need not fit side by side)
  mcpt_ctx::Scene sc;
  HIP_OR_RETURN(sc.d_nodes.alloc(hn.size()));
  HIP_OR_RETURN(sc.d_leaves.alloc((size_t)n_leaf));
  HIP_OR_RETURN(sc.d_ptype.alloc((size_t)n_prims));
  HIP_OR_RETURN(sc.d_prims.alloc(hp.size()));
  HIP_OR_RETURN(hipMemcpy(sc.d_nodes, hn.data(), sc.d_nodes.bytes(), hipMemcpyHostToDevice));
  HIP_OR_RETURN(hipMemcpy(sc.d_leaves, leaves, sc.d_leaves.bytes(), hipMemcpyHostToDevice));
  HIP_OR_RETURN(hipMemcpy(sc.d_ptype, ht.data(), sc.d_ptype.bytes(), hipMemcpyHostToDevice));
  HIP_OR_RETURN(hipMemcpy(sc.d_prims, hp.data(), sc.d_prims.bytes(), hipMemcpyHostToDevice));
  sc.has_scene = true; c->scene = std::move(sc);
  c->n_prims = n_prims; c->depth = c->tuner.depth = depth; c->nb_emissive = nb_emissives;
  c->mesh_ids = mesh_ids;
  c->denoise.guides_valid = false;
  c->temporal.tp_frames = 0;      // (temporal mode: the history shows another scene)
  c->meshes = {};                 // a new scene drops the previous meshes (upload them again)
  reset_tuning(c);
  return MCPT_OK;
}

// nodes (bbmin, bbmax) → device node records with the subtree-holds-an-item flag
static void pack_nodes(const float* nodes, const int* leaves, int depth, float4* out) {
  const int n_leaf = 1 << depth, n_node = 2 * n_leaf - 1;
  std::vector<char> has(n_node, 0);
  for (int i = n_node - 1; i >= 0; --i)
    has[i] = (i >= n_leaf - 1) ? (leaves[i - (n_leaf - 1)] >= 0) : (has[2 * i + 1] || has[2 * i + 2]);
  for (int i = 0; i < n_node; ++i) {
    const float* b = nodes + (size_t)i * 6;
    float cx = (b[0] + b[3]) / 2.0f, cy = (b[1] + b[4]) / 2.0f, cz = (b[2] + b[5]) / 2.0f;
    float wx = 0.5f * (b[3] - b[0]), wy = 0.5f * (b[4] - b[1]), wz = 0.5f * (b[5] - b[2]);
    out[(size_t)i * 3 + 0] = make_float4(cx, cy, cz, has[i] ? 1.0f : 0.0f);
    out[(size_t)i * 3 + 1] = make_float4(wx, wy, wz, 0.0f);
    out[(size_t)i * 3 + 2] = make_float4(1.0f / wx, 1.0f / wy, 1.0f / wz, 0.0f);
  }
}

static float int_bits_f(int v) {
  float f;
  std::memcpy(&f, &v, sizeof f);
  return f;
}

// A mesh BVH's child-pair records: internal node i -> 4 rows (the device's one 64-byte fetch per
// visit): (c_left, has_left) (w_left, 0) (c_right, has_right) (w_right, 0), c and w computed as
// pack_nodes does; 1/w is recomputed on the device (rcp_rn, correctly rounded: the bits of the
// host's 1/w)
static void pack_mesh_pairs(const float* nodes, const int* leaves, int depth, float4* out) {
  const int n_leaf = 1 << depth, n_node = 2 * n_leaf - 1;
  std::vector<float4> rec((size_t)n_node * 3);
  pack_nodes(nodes, leaves, depth, rec.data());
  for (int i = 0; i + 1 < n_leaf; ++i) {   // internal nodes 0 .. n_leaf - 2
    const float4* l = &rec[(size_t)(2 * i + 1) * 3];
    const float4* r = &rec[(size_t)(2 * i + 2) * 3];
    float4* o = out + (size_t)mcpt::mesh_pair_slot((unsigned)i) * 4;
    // row 1's w: 1 when all six half-widths lie in rcp_core's exact range (rcp6_rn then skips
    // its six range tests), else 0
    bool in_range = true;
    for (float v : {l[1].x, l[1].y, l[1].z, r[1].x, r[1].y, r[1].z}) {
      const float a = std::fabs(v);
      in_range = in_range && a >= 0x1p-126f && a < 0x1p126f;
    }
    o[0] = l[0];
    o[1] = make_float4(l[1].x, l[1].y, l[1].z, in_range ? 1.0f : 0.0f);
    o[2] = r[0];
    o[3] = make_float4(r[1].x, r[1].y, r[1].z, 0.0f);
  }
}

int mcpt_upload_meshes(mcpt_ctx* c, int n_meshes, const int* info, int n_nodes, const float* nodes, int n_leaves,
                       const int* leaves, int n_tris, const int* tris, int n_verts, const float* verts,
                       const float* normals) {
  if (!c || n_meshes < 0) return set_err(MCPT_ERR_INVALID_ARG, "mcpt_upload_meshes: bad arguments");
  if (!c->scene.has_scene) return set_err(MCPT_ERR_NO_SCENE, "upload the scene before its meshes");
  HIP_OR_RETURN(hipSetDevice(c->device));
  HIP_OR_RETURN(hipStreamSynchronize(c->stream));
  c->meshes = {};
  c->denoise.guides_valid = false;
  c->temporal.tp_frames = 0;
  if (n_meshes == 0) {
    for (int id : c->mesh_ids)
      if (id >= 0) return set_err(MCPT_ERR_BAD_SCENE, "the scene has mesh instances but no meshes were uploaded");
    return MCPT_OK;
  }
  if (!info || !nodes || !leaves || !tris || !verts || !normals || n_nodes <= 0 || n_leaves <= 0 || n_tris <= 0 ||
      n_verts <= 0)
    return set_err(MCPT_ERR_INVALID_ARG, "mcpt_upload_meshes: bad arguments");
  // validate the layout: each mesh's BVH within the node / leaf arrays, leaf triangle ids
  // within the mesh's triangles, vertex ids within the vertex array
  // pair records: each mesh's in its own run of slots (mesh_pair_slot), the run starting at an
  // even slot so that two-slot lines are 128-byte aligned; leaf triangle records indexed by the
  // global leaf index
  std::vector<unsigned> pair_base(n_meshes);
  size_t n_slots = 0;
  for (int m = 0; m < n_meshes; ++m) {
    const int d = info[4 * m + 2];
    if (d < 0 || d > 24) return set_err(MCPT_ERR_BAD_SCENE, "bad mesh info");
    pair_base[m] = (unsigned)n_slots;
    n_slots = (n_slots + mcpt::mesh_pair_slots(d) + 1) & ~(size_t)1;
  }
  if (n_slots * 4 >= (size_t(1) << 31)) return set_err(MCPT_ERR_BAD_SCENE, "mesh BVHs too large");
  std::vector<float4> hn(std::max<size_t>(n_slots, 2) * 4, make_float4(0.0f, 0.0f, 0.0f, 0.0f));
  for (int m = 0; m < n_meshes; ++m) {
    const int no = info[4 * m], lo = info[4 * m + 1], d = info[4 * m + 2], to = info[4 * m + 3];
    if (d < 0 || d > 24 || no < 0 || lo < 0 || to < 0) return set_err(MCPT_ERR_BAD_SCENE, "bad mesh info");
    const int nl = 1 << d, nn = 2 * nl - 1;
    if (no + nn > n_nodes || lo + nl > n_leaves) return set_err(MCPT_ERR_BAD_SCENE, "mesh BVH out of range");
    const int nt = (m + 1 < n_meshes ? info[4 * (m + 1) + 3] : n_tris) - to;
    if (nt <= 0 || to + nt > n_tris) return set_err(MCPT_ERR_BAD_SCENE, "mesh triangles out of range");
    for (int k = 0; k < nl; ++k)
      if (leaves[lo + k] < -1 || leaves[lo + k] >= nt) return set_err(MCPT_ERR_BAD_SCENE, "mesh leaf id out of range");
    pack_mesh_pairs(nodes + (size_t)no * 6, leaves + lo, d, &hn[(size_t)pair_base[m] * 4]);
  }
  for (int id : c->mesh_ids)
    if (id >= n_meshes) return set_err(MCPT_ERR_BAD_SCENE, "mesh instance refers to a missing mesh");
  std::vector<int4> hi(n_meshes), ht(n_tris);
  // device mesh info: (first pair slot, first leaf, depth, first triangle)
  for (int m = 0; m < n_meshes; ++m) hi[m] = make_int4((int)pair_base[m], info[4 * m + 1], info[4 * m + 2], info[4 * m + 3]);
  for (int t = 0; t < n_tris; ++t) {
    const int* v = tris + (size_t)t * 3;
    for (int k = 0; k < 3; ++k)
      if (v[k] < 0 || v[k] >= n_verts) return set_err(MCPT_ERR_BAD_SCENE, "vertex id out of range");
    ht[t] = make_int4(v[0], v[1], v[2], 0);
  }
  std::vector<float4> hv(n_verts), hm(n_verts);
  for (int i = 0; i < n_verts; ++i) {
    hv[i] = make_float4(verts[3 * i], verts[3 * i + 1], verts[3 * i + 2], 0.0f);
    hm[i] = make_float4(normals[3 * i], normals[3 * i + 1], normals[3 * i + 2], 0.0f);
  }
  // leaf triangle records (one 64-byte fetch per leaf visit, no index -> vertex indirection):
  // (A, t) (B - A, 0) (C - A, 0) (0): Triangle_intersect's vertex A and its two edges, computed
  // with the binary32 subtractions the device did (same bits), and the mesh-local triangle id t
  // (-1: an empty leaf) as int bits
  std::vector<float4> hl((size_t)n_leaves * 4, make_float4(0.0f, 0.0f, 0.0f, 0.0f));
  for (int k = 0; k < n_leaves; ++k) hl[(size_t)k * 4].w = int_bits_f(-1);
  std::vector<int> leaf_tris(n_meshes, 0);
  std::vector<char> empty_pair(n_meshes, 0);
  for (int m = 0; m < n_meshes; ++m) {
    const int lo = info[4 * m + 1], d = info[4 * m + 2], to = info[4 * m + 3];
    for (int k = 0; k < (1 << d); ++k) {
      const int t = leaves[lo + k];
      // (a leaf pair without a triangle has no box to refit from: mcpt_refit_mesh refuses the mesh)
      if (t < 0 && d >= 1 && leaves[lo + (k ^ 1)] < 0) empty_pair[m] = 1;
      if (t < 0) continue;
      ++leaf_tris[m];
      const int4 vi = ht[to + t];
      const float4 A = hv[vi.x], B = hv[vi.y], C = hv[vi.z];
      float4* r = &hl[(size_t)(lo + k) * 4];
      r[0] = make_float4(A.x, A.y, A.z, int_bits_f(t));
      r[1] = make_float4(B.x - A.x, B.y - A.y, B.z - A.z, 0.0f);
      r[2] = make_float4(C.x - A.x, C.y - A.y, C.z - A.z, 0.0f);
    }
  }
  // one allocation: the pair slots, then the leaf records (walk_run_mesh addresses both by 32-bit
  // byte offsets from d_mpairs)
  if ((hn.size() + hl.size()) * sizeof(float4) > (size_t(1) << 32))
    return set_err(MCPT_ERR_BAD_SCENE, "mesh BVH records exceed 4 GiB");
  mcpt_ctx::Meshes ms;
  HIP_OR_RETURN(ms.d_minfo.alloc(hi.size()));
  HIP_OR_RETURN(ms.d_mpairs.alloc(hn.size() + hl.size()));
  ms.d_mleaftris = ms.d_mpairs + hn.size();
  HIP_OR_RETURN(ms.d_mtris.alloc(ht.size()));
  HIP_OR_RETURN(ms.d_mverts.alloc(hv.size()));
  HIP_OR_RETURN(ms.d_mnorms.alloc(hm.size()));
  HIP_OR_RETURN(hipMemcpy(ms.d_minfo, hi.data(), hi.size() * sizeof(int4), hipMemcpyHostToDevice));
  HIP_OR_RETURN(hipMemcpy(ms.d_mpairs, hn.data(), hn.size() * sizeof(float4), hipMemcpyHostToDevice));
  HIP_OR_RETURN(hipMemcpy(ms.d_mleaftris, hl.data(), hl.size() * sizeof(float4), hipMemcpyHostToDevice));
  HIP_OR_RETURN(hipMemcpy(ms.d_mtris, ht.data(), ht.size() * sizeof(int4), hipMemcpyHostToDevice));
  HIP_OR_RETURN(hipMemcpy(ms.d_mverts, hv.data(), hv.size() * sizeof(float4), hipMemcpyHostToDevice));
  HIP_OR_RETURN(hipMemcpy(ms.d_mnorms, hm.data(), hm.size() * sizeof(float4), hipMemcpyHostToDevice));
  ms.n_meshes = n_meshes;
  ms.info = std::move(hi); ms.leaf_tris = std::move(leaf_tris); ms.empty_pair = std::move(empty_pair);
  ms.n_pair_f4 = hn.size(); ms.n_leaf_f4 = hl.size();
  // a rebuild's view (mcpt_rebuild.hip): each mesh's triangle count and the vertex ids its triangles
  // use; its vertex range is not known until mcpt_set_mesh_vertex_counts tells it (count 0)
  ms.n_tris.resize(n_meshes); ms.vert_lo.assign(n_meshes, n_verts); ms.vert_hi.assign(n_meshes, 0);
  ms.vert_first.assign(n_meshes, 0); ms.vert_count.assign(n_meshes, 0);
  for (int m = 0; m < n_meshes; ++m) {
    const int to = info[4 * m + 3];
    ms.n_tris[m] = (m + 1 < n_meshes ? info[4 * (m + 1) + 3] : n_tris) - to;
    for (int t = to; t < to + ms.n_tris[m]; ++t) {
      ms.vert_lo[m] = std::min(ms.vert_lo[m], std::min(ht[t].x, std::min(ht[t].y, ht[t].z)));
      ms.vert_hi[m] = std::max(ms.vert_hi[m], std::max(ht[t].x, std::max(ht[t].y, ht[t].z)));
    }
  }
  c->meshes = std::move(ms);
  return MCPT_OK;
}

int mcpt_set_flat_face(mcpt_ctx* c, int flat_face) {
  if (!c) return mcpt_err_bare(MCPT_ERR_INVALID_ARG);
  c->flat_face = flat_face ? 1 : 0;
  c->denoise.guides_valid = false;
  c->temporal.tp_frames = 0;
  return MCPT_OK;
}

// Shard the frame by explicit row lists: `rows` = the global rows this context renders, in
// local-row order.  mcpt_set_target (interleaved bands) and mcpt_balanced_rows are row lists.
static int set_target_rows(mcpt_ctx* c, int W, int H, const int* rows, int n_rows, int band_rows, int world,
                           int rank) {
  // the kernels index a shard's pixels with 32-bit ints (render_kernel's local pixel index)
  if ((long long)n_rows * W >= (1LL << 31))
    return set_err(MCPT_ERR_INVALID_ARG, "mcpt_set_target: a shard of 2^31 pixels or more");
  HIP_OR_RETURN(hipSetDevice(c->device));
  HIP_OR_RETURN(hipStreamSynchronize(c->stream));
  c->denoise = {};    // (sized by the target; allocated again by the next guides / denoise call)
  c->stats = {};      // (statistics off: a new target begins again)
  c->adaptive = {};   // (adaptive mode off: its blocks are the old target's)
  c->planes = {};     // (a gathered frame's counts are the old target's)
  c->temporal = {};   // (temporal mode off: its history is the old target's)
  for (auto& L : c->lanes) L.drop_target_sized();   // (segment sums, steal store, item order: other pixels)
  const size_t n_accum = (size_t)n_rows * W * 3;
  if (n_accum != c->target.d_accum.size()) {
    c->target.d_accum.reset();
    if (n_accum) HIP_OR_RETURN(c->target.d_accum.alloc(n_accum));
  }
  if ((size_t)std::max(n_rows, 1) != c->target.d_rows.size()) HIP_OR_RETURN(c->target.d_rows.alloc((size_t)std::max(n_rows, 1)));
  c->rows.assign(rows, rows + n_rows);
  if (n_rows) HIP_OR_RETURN(hipMemcpy(c->target.d_rows, rows, sizeof(int) * (size_t)n_rows, hipMemcpyHostToDevice));
  c->W = W; c->H = H; c->band_rows = band_rows; c->world = world; c->rank = rank; c->n_local_rows = n_rows;
  c->has_target = true;
  return mcpt_clear_accum(c);
}

int mcpt_set_target(mcpt_ctx* c, int W, int H, int band_rows, int world, int rank) {
  if (!c || W <= 0 || H <= 0 || band_rows <= 0 || world <= 0 || rank < 0 || rank >= world)
    return set_err(MCPT_ERR_INVALID_ARG, "mcpt_set_target: bad arguments");
  std::vector<int> rows;
  for (int y = 0; y < H; ++y)
    if ((y / band_rows) % world == rank) rows.push_back(y);
  return set_target_rows(c, W, H, rows.data(), (int)rows.size(), band_rows, world, rank);
}

int mcpt_set_target_rows(mcpt_ctx* c, int W, int H, const int* rows, int n_rows) {
  if (!c || W <= 0 || H <= 0 || n_rows < 0 || n_rows > H || (n_rows > 0 && !rows))
    return set_err(MCPT_ERR_INVALID_ARG, "mcpt_set_target_rows: bad arguments");
  std::vector<char> seen((size_t)H, 0);
  for (int i = 0; i < n_rows; ++i) {
    if (rows[i] < 0 || rows[i] >= H || seen[(size_t)rows[i]])
      return set_err(MCPT_ERR_INVALID_ARG, "mcpt_set_target_rows: rows must be distinct and in [0, H)");
    seen[(size_t)rows[i]] = 1;
  }
  return set_target_rows(c, W, H, rows, n_rows, 0, 0, 0);
}

int mcpt_balanced_rows(int H, int world, int rank, int band_rows, int* rows_out, int* n_out) {
  if (H <= 0 || world <= 0 || rank < 0 || rank >= world || band_rows <= 0 || !n_out)
    return set_err(MCPT_ERR_INVALID_ARG, "mcpt_balanced_rows: bad arguments");
  // whole periods of `world` bands: in period j, rank r takes band j·world + (r + j) mod world
  // (each rank gets every band position of a period equally often); the rows after the last
  // whole period are dealt one at a time, rotated the same way
  const int periods = (H / band_rows) / world;
  const int rest0 = periods * world * band_rows;
  int n = 0;
  for (int y = 0; y < H; ++y) {
    int owner;
    if (y < rest0) {
      const int b = y / band_rows, j = b / world;
      owner = ((b % world) - j % world + world) % world;
    } else {
      owner = ((y - rest0) + periods) % world;
    }
    if (owner == rank) {
      if (rows_out) rows_out[n] = y;
      ++n;
    }
  }
  *n_out = n;
  return MCPT_OK;
}

int mcpt_local_row_ids(mcpt_ctx* c, int* rows_out) {
  if (!c || !rows_out) return mcpt_err_bare(MCPT_ERR_INVALID_ARG);
  if (!c->has_target) return mcpt_err_bare(MCPT_ERR_NO_TARGET);
  std::copy(c->rows.begin(), c->rows.end(), rows_out);
  return MCPT_OK;
}

int mcpt_local_rows(mcpt_ctx* c, int* n) {
  if (!c || !n) return mcpt_err_bare(MCPT_ERR_INVALID_ARG);
  if (!c->has_target) return mcpt_err_bare(MCPT_ERR_NO_TARGET);
  *n = c->n_local_rows;
  return MCPT_OK;
}

int mcpt_clear_accum(mcpt_ctx* c) {
  if (!c) return mcpt_err_bare(MCPT_ERR_INVALID_ARG);
  if (!c->has_target) return mcpt_err_bare(MCPT_ERR_NO_TARGET);
  HIP_OR_RETURN(hipSetDevice(c->device));
  if (c->target.d_accum.bytes()) HIP_OR_RETURN(hipMemsetAsync(c->target.d_accum, 0, c->target.d_accum.bytes(), c->stream));
  c->pass_count = 0;
  invalidate_planes(c);
  return MCPT_OK;
}

// raytracer.vert:9-22 for the 4 strip corners: Ori = invV·(0,0,0,1), Dir = normalize(Q.xyz/Q.w − Ori)
static void corner_rays(const float* invPV, const float* invV, mcpt::RenderParams& p) {
  auto matvec = [](const float* m, const float v[4], float o[4]) {
    for (int r = 0; r < 4; ++r)
      o[r] = std::fma(m[12 + r], v[3], std::fma(m[8 + r], v[2], std::fma(m[4 + r], v[1], m[r] * v[0])));
  };
  const float origin[4] = {0.0f, 0.0f, 0.0f, 1.0f};
  float o4[4];
  matvec(invV, origin, o4);
  p.ox = o4[0]; p.oy = o4[1]; p.oz = o4[2];
  for (int v = 0; v < 4; ++v) {
    float tcx = (float)(v % 2), tcy = (float)(v / 2);
    float cv[4] = {2.0f * tcx - 1.0f, 2.0f * tcy - 1.0f, 1.0f, 1.0f};
    float q[4];
    matvec(invPV, cv, q);
    float dx = q[0] / q[3] - o4[0], dy = q[1] / q[3] - o4[1], dz = q[2] / q[3] - o4[2];
    float len2 = std::fma(dz, dz, std::fma(dy, dy, dx * dx));
    float rn = 1.0f / std::sqrt(len2);
    p.cd[3 * v + 0] = dx * rn; p.cd[3 * v + 1] = dy * rn; p.cd[3 * v + 2] = dz * rn;
  }
}

// stream schedule defaults: 16 Mi path slots (2 x 92 B of queue payload + 64 B of unit data
// each: 4 GB) keep the iterations few and every trace kernel long against its tail (the last
// walks of the iteration): scene 8, 512 spp, 1080p (33 M units): 4 Mi slots 1,344 iterations
// 447 Msamples/s, 8 Mi 792 / 472, 12 Mi 624 / 482, 16 Mi 512 / 484, 32 Mi 352 / 478 (the
// units' own tail grows); a wave refills its idle lanes once 8 of them have finished their walks
constexpr int kStreamSlotsDefault = 1 << 24;
constexpr int kStreamRefillDefault = 56;
constexpr int kStreamBatch = 8;   // iterations issued between two reads of the counters
// the shade kernel compacts its output (drops dead entries) once fewer than this share of the
// queue is live
constexpr double kStreamCompactBelow = 0.6;

static bool stream_applies(const mcpt_ctx* c, int variant, int bounces, bool count) {
  (void)c;
  return !count && variant == 0 && bounces > 0;
}

// path-slot pools of a launch: each runs its own iterations on its own stream, so one pool's
// shade kernel and trace-kernel tail overlap the other pool's trace kernel
constexpr int kStreamPools = 2;

// One sub-launch (one pass range of <= max_seg segments) with the stream schedule: the slots of
// every pool set up, then iterations (trace + shade) in batches until every slot has run out of
// units.  The host reads the counters of batch b-1 while batch b runs, so the device never waits
// for the host.
static int stream_run(mcpt_ctx* c, const mcpt::RenderParams& p) {
  const unsigned long long n_units = (unsigned long long)p.n_local_px * (unsigned long long)p.n_segments;
  if (n_units == 0) return MCPT_OK;
  if (n_units >= (1ULL << 31) || p.n_local_px >= (1LL << 31))
    return set_err(MCPT_ERR_INVALID_ARG, "stream schedule: too many units in one launch");
  // the kernels address a pool's queue / slot data through one buffer resource: below 2 GiB each
  const int max_pool = (int)(((1ULL << 31) - 1) / (mcpt::QF_COUNT * sizeof(float)));
  const int n_pools = (int)std::max(1, std::min(env_int("MCPT_STREAM_POOLS", kStreamPools), kStreamPools));
  const long long want = c->stream_slots > 0 ? c->stream_slots : kStreamSlotsDefault;
  const long long n_slots = std::min<long long>((long long)n_units, std::min<long long>(want, (long long)max_pool * n_pools));
  int pool_n[kStreamPools] = {0, 0};
  int np = 0;
  for (int k = 0; k < n_pools; ++k) {
    pool_n[k] = (int)(n_slots / n_pools + (k < n_slots % n_pools ? 1 : 0));
    if (pool_n[k] > 0) np = k + 1;
  }
  const size_t slot_floats = (size_t)mcpt::SF_COUNT * n_slots, queue_floats = (size_t)2 * mcpt::QF_COUNT * n_slots;
  if (slot_floats > c->pools.d_slots.size() || queue_floats > c->pools.d_queue.size()) {
    HIP_OR_RETURN(hipStreamSynchronize(c->stream));
    c->pools.d_slots.reset(); c->pools.d_queue.reset();   // (both go before either grows)
  }
  HIP_OR_RETURN(c->pools.d_slots.ensure(slot_floats));
  HIP_OR_RETURN(c->pools.d_queue.ensure(queue_floats));
  HIP_OR_RETURN(c->pools.d_sctr.ensure(kStreamPools * mcpt::SC_COUNT));
  HIP_OR_RETURN(c->pools.h_sctr.ensure(2 * kStreamPools * mcpt::SC_COUNT));
  for (Event& e : c->pools.batch_ev) HIP_OR_RETURN(e.ensure(hipEventDisableTiming));
  for (Event& e : c->pools.pool_ev) HIP_OR_RETURN(e.ensure(hipEventDisableTiming));
  for (Stream& st : c->pools.pool_stream) HIP_OR_RETURN(st.ensure(hipStreamNonBlocking));
  // BVH nodes in the trace kernel's LDS where they fit (MCPT_STREAM_LDS_NODES=1): off by default,
  // no faster on scenes 3/7/8 (random lanes' node reads conflict in the LDS banks, 11 conflict
  // cycles per LDS instruction; gpurun_out r03e/r03f)
  const bool lds_nodes = env_int("MCPT_STREAM_LDS_NODES", 0) != 0 && p.n_meshes == 0 && mcpt_stream_lds_nodes_fit(p.depth);
  mcpt::StreamParams q[kStreamPools];
  unsigned* unit_ctr = c->pools.d_sctr + mcpt::SC_UNIT;   // pool 0's slot: shared
  {
    const unsigned first_free = (unsigned)n_slots;   // units 0 .. n_slots-1 start in the pools' slots
    HIP_OR_RETURN(hipMemcpyAsync(unit_ctr, &first_free, sizeof(unsigned), hipMemcpyHostToDevice, c->stream));
  }
  size_t slot_off = 0, queue_off = 0;
  int unit_base = 0;
  for (int k = 0; k < np; ++k) {
    mcpt::StreamParams& s = q[k];
    s.r = p;
    // leaf batching of the trace kernel's walks: 16 lanes (8 for the megakernel; scene 8: 16 is
    // +4 % over 8 and 32, 4 is -8 %)
    if (c->leaf_batch < 0) s.r.leaf_batch = 16;
    // field f of pool entry i at queue[par][f * n + i], slot data likewise: laid out per pool
    s.slots = c->pools.d_slots + slot_off;
    s.queue[0] = c->pools.d_queue + queue_off;
    s.queue[1] = s.queue[0] + (size_t)mcpt::QF_COUNT * pool_n[k];
    s.ctr = c->pools.d_sctr + k * mcpt::SC_COUNT;
    s.unit_ctr = unit_ctr;
    s.n_slots = pool_n[k];
    s.unit_base = unit_base;
    s.n_units = (unsigned)n_units;
    s.parity = 0;
    s.refill = c->stream_refill >= 0 ? c->stream_refill : kStreamRefillDefault;
    s.compact = 0;
    slot_off += (size_t)mcpt::SF_COUNT * pool_n[k];
    queue_off += (size_t)2 * mcpt::QF_COUNT * pool_n[k];
    unit_base += pool_n[k];
    HIP_OR_RETURN(mcpt_launch_stream_init(s, c->stream));
  }
  // fork: the pool streams start after the set-up (and everything before it) on the context's stream
  HIP_OR_RETURN(hipEventRecord(c->pools.pool_ev[2], c->stream));
  for (int k = 0; k < np; ++k) HIP_OR_RETURN(hipStreamWaitEvent(c->pools.pool_stream[k], c->pools.pool_ev[2], 0));
  // every iteration advances each live slot by one traversal; a unit needs at most
  // (passes) x (2 B + 1) + 1 of them, and a slot runs ceil(units / slots) units
  const long long per_unit = (long long)mcpt::kPassChunk * (2LL * p.bounces + 1) + 1;
  const long long min_pool = pool_n[np - 1];
  const long long cap = ((long long)(n_units / min_pool) + 2) * per_unit + 4 * kStreamBatch;
  long long it = 0;
  bool compact[kStreamPools] = {false, false}, done[kStreamPools] = {false, false};
  const int st = [&]() -> int {
  for (int b = 0;; ++b) {
    for (int k = 0; k < kStreamBatch; ++k, ++it)
      for (int j = 0; j < np; ++j) {
        if (done[j]) continue;
        q[j].parity = (int)(it & 1);
        q[j].compact = (k == 0 && compact[j]) ? 1 : 0;
        HIP_OR_RETURN(mcpt_launch_stream_iter(q[j], c->n_cu, lds_nodes, c->pools.pool_stream[j]));
      }
    // every pool's counters after the batch, read on pool 0's stream once all pools are there
    for (int j = 1; j < np; ++j) {
      HIP_OR_RETURN(hipEventRecord(c->pools.pool_ev[j], c->pools.pool_stream[j]));
      HIP_OR_RETURN(hipStreamWaitEvent(c->pools.pool_stream[0], c->pools.pool_ev[j], 0));
    }
    unsigned* h = c->pools.h_sctr + (b & 1) * kStreamPools * mcpt::SC_COUNT;
    HIP_OR_RETURN(hipMemcpyAsync(h, c->pools.d_sctr, (size_t)np * mcpt::SC_COUNT * sizeof(unsigned), hipMemcpyDeviceToHost,
                                 c->pools.pool_stream[0]));
    HIP_OR_RETURN(hipEventRecord(c->pools.batch_ev[b & 1], c->pools.pool_stream[0]));
    if (b >= 1) {
      HIP_OR_RETURN(hipEventSynchronize(c->pools.batch_ev[(b - 1) & 1]));
      bool all = true;
      for (int j = 0; j < np; ++j) {
        const unsigned* hp = c->pools.h_sctr + ((b - 1) & 1) * kStreamPools * mcpt::SC_COUNT + j * mcpt::SC_COUNT;
        const unsigned dead = hp[mcpt::SC_DEAD];
        done[j] = dead >= (unsigned)pool_n[j];   // every slot of the pool was done by the end of batch b-1
        all = all && done[j];
        // the queue length the iteration after batch b-1 read (in place: unchanged until compacted)
        const unsigned len = hp[mcpt::SC_CNT + (int)((it - kStreamBatch) & 1)];
        compact[j] = !done[j] && (double)(pool_n[j] - dead) < kStreamCompactBelow * (double)len;
      }
      if (all) break;
    }
    if (it > cap) return set_err(MCPT_ERR_HIP, "stream schedule did not drain its queue");
  }
  return MCPT_OK;
  }();
  // join: the context's stream (the combine kernel, the caller's next work) waits for every
  // pool stream.  Also after an error: kernels already queued on a pool stream still read and
  // write d_slots / d_queue / d_partial, which the context frees or reallocates only after
  // synchronizing its own stream, so that stream must not run ahead of them.
  bool joined = true;
  for (int j = 0; j < np; ++j)
    joined = joined && hipEventRecord(c->pools.pool_ev[j], c->pools.pool_stream[j]) == hipSuccess &&
             hipStreamWaitEvent(c->stream, c->pools.pool_ev[j], 0) == hipSuccess;
  if (!joined)   // cannot order them: wait for them here
    for (int j = 0; j < np; ++j) (void)hipStreamSynchronize(c->pools.pool_stream[j]);
  if (st != MCPT_OK) return st;
  if (!joined) return set_err(MCPT_ERR_HIP, "stream schedule: joining the pool streams failed");
  c->stream_iters += it;
  return MCPT_OK;
}

// the stream schedule's pools (4 GB at the default 16 Mi slots), once no longer selected
static int free_stream_pools(mcpt_ctx* c) {
  if (!c->pools.d_slots && !c->pools.d_queue) return MCPT_OK;
  HIP_OR_RETURN(hipSetDevice(c->device));
  HIP_OR_RETURN(hipStreamSynchronize(c->stream));
  c->pools.d_slots.reset(); c->pools.d_queue.reset();
  return MCPT_OK;
}

// Buffers of the work-item order for `items` items (grown on demand, with the identity values
// the sort permutes and its temporary storage)
static hipError_t ensure_item_order(mcpt_ctx* c, int li, long long items) {
  mcpt_ctx::Lane& L = c->lanes[li];
  if (items <= L.order.cap()) return hipSuccess;
  hipError_t e = hipStreamSynchronize(c->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(c->seq.lane[li].stream);
  if (e != hipSuccess) return e;
  L.order = {};
  mcpt_ctx::Lane::Order o;
  size_t n = (size_t)items, tmp = 0;
  if ((e = o.d_item_cost.alloc(n)) != hipSuccess) return e;
  if ((e = o.d_cost_sorted.alloc(n)) != hipSuccess) return e;
  if ((e = o.d_item_iota.alloc(n)) != hipSuccess) return e;
  if ((e = o.d_item_perm.alloc(n)) != hipSuccess) return e;
  if ((e = o.d_split_of.alloc(n)) != hipSuccess) return e;
  if ((e = o.d_split_n.alloc(1)) != hipSuccess) return e;
  if ((e = hipMemset(o.d_split_n, 0, sizeof(int))) != hipSuccess) return e;
  if ((e = mcpt_order_items(nullptr, nullptr, nullptr, nullptr, (int)items, nullptr, &tmp, c->stream)) != hipSuccess)
    return e;
  if ((e = o.d_sort_tmp.alloc(std::max<size_t>(tmp, 1))) != hipSuccess) return e;
  if ((e = mcpt_iota(o.d_item_iota, (int)items, c->stream)) != hipSuccess) return e;
  if ((e = hipStreamSynchronize(c->stream)) != hipSuccess) return e;
  L.order = std::move(o);
  return hipSuccess;
}

#ifdef MCPT_CHECKED
// checked build (mcpt_internal.h, kCheckedCountSlot): wait for sub-launch k of n_sub and report a
// HIP fault or an out-of-range index the kernels counted, naming the sub-launch and its shape
extern "C++" int checked_sub_launch(mcpt_ctx* c, int k, int n_sub, const mcpt::RenderParams& p) {
  char what[200];
  std::snprintf(what, sizeof(what),
                "checked build: sub-launch %d of %d (passes %d+%d, %d segments, %d items, K %d, tail %d, split max %d)",
                k, n_sub, p.first_pass, p.n_passes, p.n_segments, p.n_items, p.seg_per_item, p.tail_m, p.split_max);
  hipError_t e = hipStreamSynchronize(c->stream);   // (ordered after the sub-launch's lane work)
  if (e != hipSuccess) return set_err(MCPT_ERR_HIP, what, e);
  unsigned long long v[2] = {0, 0};
  e = hipMemcpy(v, c->d_events + mcpt::kCheckedCountSlot, sizeof(v), hipMemcpyDeviceToHost);
  if (e != hipSuccess) return set_err(MCPT_ERR_HIP, what, e);
  if (v[0] != 0) {
    char msg[256];
    std::snprintf(msg, sizeof(msg), "%s: %llu out-of-range indices, first at site %llu index %lld", what, v[0],
                  v[1] >> 48, (long long)(v[1] & 0xffffffffffffull));
    (void)hipMemset(c->d_events + mcpt::kCheckedCountSlot, 0, sizeof(v));
    return set_err(MCPT_ERR_HIP, msg);
  }
  return MCPT_OK;
}
#endif

// a render launch's scene, target and camera fields (launch(), mcpt_render_adaptive, mcpt_render_guides)
extern "C++" void scene_params(const mcpt_ctx* c, const float* invPV, const float* invV, mcpt::RenderParams& p) {
  std::memset(&p, 0, sizeof(p));
  p.nodes = c->scene.d_nodes; p.leaves = c->scene.d_leaves; p.ptype = c->scene.d_ptype; p.prims = c->scene.d_prims;
  p.accum = c->target.d_accum; p.events = c->d_events;
  corner_rays(invPV, invV, p);
  p.W = c->W; p.H = c->H; p.rows = c->target.d_rows;
  p.n_local_rows = c->n_local_rows; p.depth = c->depth; p.n_prims = c->n_prims;
  {
    const long long lds = ((3LL * ((2LL << c->depth) - 1) + (long long)mcpt::kPrimF4 * c->n_prims) * 16) +
                          (((1LL << c->depth) + c->n_prims) * 4);
    p.lds_scene_bytes = lds <= mcpt::kLdsSceneBytes ? (int)lds : 0;
  }
  p.minfo = c->meshes.d_minfo; p.mpairs = c->meshes.d_mpairs; p.mleaftris = c->meshes.d_mleaftris; p.mtris = c->meshes.d_mtris;
  p.mverts = c->meshes.d_mverts; p.mnorms = c->meshes.d_mnorms; p.n_meshes = c->meshes.n_meshes; p.flat_face = c->flat_face;
  p.tile_w = mcpt::tile_w_for(c->meshes.n_meshes > 0, p.lds_scene_bytes);
  p.n_local_px = (long long)c->n_local_rows * c->W;
}

// ... and its pass range and wave-uniform constants
extern "C++" void pass_params(int first_pass, int n_passes, float date, int bounces, float refract_ind, int variant,
                 mcpt::RenderParams& p) {
  p.first_pass = first_pass; p.n_passes = n_passes; p.bounces = bounces; p.variant = variant;
  p.date = date; p.ior = refract_ind;
  p.inv_ior = 1.0f / refract_ind;
  float r0 = (refract_ind - 1.0f) / (refract_ind + 1.0f);   // schlick tp/montecarlo.frag:93-94
  p.schlick_r0 = r0 * r0;
  p.schlick_1mr0 = 1.0f - p.schlick_r0;
  p.ior_sq = refract_ind * refract_ind;
  p.inv_ior_sq = p.inv_ior * p.inv_ior;
  const float fmax = mcpt::kFLTMAX, nx = std::nextafter(fmax, INFINITY);   // cull_bound_sq(FLT_MAX)
  const double m = ((double)fmax + (double)nx) * 0.5;
  p.cull2_max = m * m;
}

extern "C++" int check_renderable(const mcpt_ctx* c, bool args_ok, const char* who) {
  if (!c || !args_ok) {
    char what[64];
    std::snprintf(what, sizeof(what), "%s: bad arguments", who);
    return set_err(MCPT_ERR_INVALID_ARG, what);
  }
  if (!c->scene.has_scene) return set_err(MCPT_ERR_NO_SCENE, "no scene uploaded");
  if (!c->has_target) return set_err(MCPT_ERR_NO_TARGET, "no render target");
  if (c->meshes.n_meshes == 0)
    for (int id : c->mesh_ids)
      if (id >= 0) return set_err(MCPT_ERR_BAD_SCENE, "mesh instances present: call mcpt_upload_meshes");
  return MCPT_OK;
}

static bool holds_order(const mcpt_ctx::Lane& L, const plan::Items& it) {
  return L.order.valid && std::equal(it.key, it.key + 8, L.order.key);
}

// An ordered sub-launch s (its render and set-up on s.ws): the order it runs, its tail pieces and
// its cleared item costs
static int prepare_order(mcpt_ctx* c, const mcpt::LaneSeq::Sub& s, const plan::ItemsIn& in, const plan::Items& it,
                         mcpt::RenderParams& p) {
  mcpt_ctx::Lane &L = c->lanes[s.li], &O = c->lanes[s.li ^ 1];
  // the other lane holds this shape's order (AUTO's trials alternate candidates between the
  // lanes; a new shape's first launches): copied once its last sort is done, so that a trial
  // runs the order a settled launch of its candidate would
  if (!holds_order(L, it) && holds_order(O, it) && O.order.cap() >= it.items) {
    HIP_OR_RETURN(c->seq.before_order_copy(s));
    HIP_OR_RETURN(hipMemcpyAsync(L.order.d_item_perm, O.order.d_item_perm, sizeof(int) * (size_t)it.items, hipMemcpyDeviceToDevice, s.ws));
    HIP_OR_RETURN(hipMemcpyAsync(L.order.d_split_n, O.order.d_split_n, sizeof(int), hipMemcpyDeviceToDevice, s.ws));
    HIP_OR_RETURN(c->seq.after_order_copy(s));
    std::copy(it.key, it.key + 8, L.order.key);
    L.order.valid = true;
    L.order.age = O.order.age;
  }
  if (holds_order(L, it)) {
    p.item_perm = L.order.d_item_perm;
    p.tail_m = plan::tail_m(in, it, true);
  }
  HIP_OR_RETURN(hipMemsetAsync(L.order.d_item_cost, 0, sizeof(unsigned) * (size_t)it.items, s.ws));
  p.item_cost = L.order.d_item_cost;
  return MCPT_OK;
}

// ... its split items' buffers
static int prepare_split_items(mcpt_ctx::Lane& L, hipStream_t ws, long long items, mcpt::RenderParams& p) {
  HIP_OR_RETURN(L.d_split_pass.ensure(3 * (size_t)plan::kSplitMax * mcpt::kPassChunk * mcpt::kTileThreads));
  HIP_OR_RETURN(hipMemsetAsync(L.order.d_split_of, 0xff, sizeof(int) * (size_t)items, ws));
  p.split_of = L.order.d_split_of;
  p.split_pass = L.d_split_pass;
  p.split_max = plan::kSplitMax;
  if (p.item_perm) p.split_n = L.order.d_split_n;
  return MCPT_OK;
}

// ... and the sort of the costs it measured: after its render (outside its timed events); the
// lane's next launch of this shape reads the order in stream order, so no host wait
static int sort_order(mcpt_ctx* c, mcpt_ctx::Lane& L, hipStream_t ws, const plan::Items& it, const mcpt::RenderParams& p) {
  size_t tmp = L.order.d_sort_tmp.size();
  HIP_OR_RETURN(mcpt_order_items(L.order.d_item_cost, L.order.d_cost_sorted, L.order.d_item_iota, L.order.d_item_perm, (int)it.items,
                                 L.order.d_sort_tmp, &tmp, ws));
  // mesh scenes: how many of the costliest to split next time (the mesh kernels run 5
  // waves per SIMD: 20 per CU, in workgroups of tile_w / 8 waves)
  if (c->meshes.n_meshes > 0)
    HIP_OR_RETURN(mcpt_split_count(L.order.d_cost_sorted, (int)it.items, 20 / (p.tile_w / 8) * c->n_cu, plan::kSplitMax,
                                   L.order.d_split_n, c->d_events + kDebugSplitSlot, ws));
  std::copy(it.key, it.key + 8, L.order.key);
  L.order.valid = true;
  L.order.age = 0;
  return MCPT_OK;
}

// A render call: the plan (mcpt_plan.h: schedule candidate, limits, pass split, sub-launches),
// then per sub-launch: prepare its lane, record, render, combine, maybe sort, hand the lane back.
static int launch(mcpt_ctx* c, const float* invPV, const float* invV, int first_pass, int n_passes, float date,
                  int bounces, float refract_ind, int variant, bool count, unsigned long long* events) {
  OK_OR_RETURN(check_renderable(c, invPV && invV && n_passes >= 0 && variant >= 0 && variant <= 2, "mcpt_render"));
  invalidate_planes(c);   // (a gathered frame's counts do not describe what is rendered into it)
  HIP_OR_RETURN(hipSetDevice(c->device));
  mcpt::RenderParams p;
  scene_params(c, invPV, invV, p);
  plan::Tuner& tuner = c->tuner;
  // AUTO: the trial before the last call is collected now (its render has ended while the last
  // call's runs); all of them first when this call's shape differs from theirs
  HIP_OR_RETURN(collect_tuning(c, (tuner.pending_other_shape(p.n_local_px, n_passes) || count) ? 0 : 1));
  // (the counting build is not timed: AUTO counts with the per-lane walk)
  p.n_tiles = ((c->W + p.tile_w - 1) / p.tile_w) * ((c->n_local_rows + mcpt::kTileH - 1) / mcpt::kTileH);
  const long long total_seg = plan::pass_segments(first_pass, n_passes);
  // segment groups need segments to group; whether longer items pay (the lanes' pass-count
  // tails average out) or cost (longer grid tail) depends on the scene and the launch: timed,
  // not guessed (profiles/r01_ab44_seg_per_item.jsonl, r01_ab49_seg_groups_tail.jsonl)
  tuner.deep_auto = c->depth >= 8;
  const int cand = count ? (c->traversal == MCPT_TRAVERSAL_AUTO ? MCPT_TRAVERSAL_LANE : c->traversal)
                         : resolve_candidate(c, total_seg);
  const bool stream = cand == plan::kCandStream && stream_applies(c, variant, bounces, count);
  c->stream_iters = 0;
  p.wave_traversal = (cand == MCPT_TRAVERSAL_WAVE) ? 1 : 0;
  p.walk_exit = plan::cand_walk_exit(cand, c->walk_exit, c->meshes.n_meshes, c->depth);
  p.leaf_batch = plan::cand_leaf_batch(cand, c->leaf_batch, c->depth);
  p.walk_min_done = plan::cand_deep_knobs(cand) ? plan::kDeepMinDone : 1;
  // MCPT_WALK_MIN_DONE overrides (tuning hook; same bits for any value)
  if (const int md = env_int("MCPT_WALK_MIN_DONE", 0); md > 0) p.walk_min_done = md;
  p.seg_per_item = plan::resolved_seg_per_item(cand, env_int("MCPT_SEG_PER_ITEM", 0));
  pass_params(first_pass, n_passes, date, bounces, refract_ind, variant, p);
  const bool steal = env_int("MCPT_STEAL", 1) != 0;
  plan::LimitsIn lin;
  lin.n_local_px = p.n_local_px; lin.n_tiles = p.n_tiles; lin.tile_w = p.tile_w; lin.seg_per_item = p.seg_per_item;
  lin.n_cu = c->n_cu; lin.partial_budget = c->partial_budget; lin.mesh = c->meshes.n_meshes > 0;
  lin.wave_traversal = p.wave_traversal != 0; lin.steal = steal;
  // the LDS-scene kernel steals passes inside each wave: timed megakernel launches
  // only, and none of AUTO's trials (their plan and kernel stay the ones the candidates were
  // compared with)
  const bool scene_steal = steal && p.lds_scene_bytes > 0 && c->meshes.n_meshes == 0 && !p.wave_traversal && !count &&
                           !stream && schedule_settled(c);
  lin.lds_scene = scene_steal;
  const plan::Limits lim = plan::limits(lin);
  if (lim.too_large) return set_err(MCPT_ERR_INVALID_ARG, "render target too large for one launch");
  const bool split = plan::pass_split(lim, p.n_tiles, n_passes, total_seg, c->n_cu, stream, env_int("MCPT_PASS_SPLIT", -1));
  p.pass_split = split ? 1 : 0;
  if (split) p.seg_per_item = 1;
  const int n_sub = plan::count_sub_launches(first_pass, n_passes, lim.max_seg, split);
  const size_t seg_bytes = (size_t)p.n_local_px * 3 * sizeof(float);
  HIP_OR_RETURN(c->ring.begin(n_sub));   // this call's events: the ring's next slot, the last call's once committed
  // lane launches (mcpt_ctx::Lane) once AUTO has settled.  (AUTO's trials run in order on
  // `stream`: on the lanes a trial's period would be charged its own tail and discounted the
  // previous trial's, which favours the candidates with short items — C2 / C5 picked two segments
  // per item where four are 3 % faster on the lanes, tools/seg_ab.py, profiles/r06_seg_ab.jsonl)
  const bool lanes_ok = tuner.overlap != 0 && !count && !stream && schedule_settled(c);
  if (count) HIP_OR_RETURN(hipMemsetAsync(c->d_events, 0, sizeof(unsigned long long) * mcpt::EV_COUNT, c->stream));
  if (n_sub == 0) HIP_OR_RETURN(c->ring.record_empty(c->stream));
  plan::ItemsIn in;
  in.n_tiles = p.n_tiles; in.seg_per_item = p.seg_per_item; in.walk_exit = p.walk_exit; in.bounces = bounces;
  in.variant = variant; in.tile_w = p.tile_w; in.n_cu = c->n_cu; in.wave_traversal = p.wave_traversal != 0;
  in.pass_split = split; in.mesh = c->meshes.n_meshes > 0;
  // (MCPT_ITEM_ORDER=0: dispatch order b = item, tests and A/B; the same bits either way)
  in.orderable = !count && !stream && env_int("MCPT_ITEM_ORDER", 1) != 0;
  in.split_items_on = env_int("MCPT_SPLIT_ITEMS", 1) != 0;
  in.tail_pieces_on = env_int("MCPT_TAIL_PIECES", 1) != 0;
  int k = 0;
  for (long long lo = first_pass, end = (long long)first_pass + n_passes; lo < end; lo = in.sub.end(), ++k) {
    in.sub = plan::next_sub_launch(lo, end, lim.max_seg, split);
    const plan::Items it = plan::items(in);
    p.first_pass = in.sub.first_pass; p.n_passes = in.sub.n_passes; p.n_segments = in.sub.n_segments;
    p.item_perm = nullptr;
    p.item_cost = nullptr;
    p.split_n = nullptr; p.split_of = nullptr; p.split_pass = nullptr; p.split_max = 0;
    p.steal_vals = nullptr;
    p.n_items = (int)it.items;
    p.tail_m = 0;
#ifdef MCPT_CHECKED
    p.check_inject = env_int("MCPT_CHECKED_INJECT", 0);
#endif
    // the sub-launch's lane: its segment-sum buffer and work-item order state; a lane launch renders
    // on the lane's stream s.ws, else on `stream` (mcpt_launch_seq.h: the steps on `seq`, in its order)
    const mcpt::LaneSeq::Sub s = c->seq.pick(k, lanes_ok && p.n_segments > 1, c->stream);
    mcpt_ctx::Lane& L = c->lanes[s.li];
    if (p.n_segments > 1) OK_OR_RETURN(ensure_lane_bytes(c, L.d_partial, (size_t)p.n_segments * seg_bytes));
    p.partial = L.d_partial;
    if (it.order) HIP_OR_RETURN(ensure_item_order(c, s.li, it.items));
    HIP_OR_RETURN(c->seq.acquire(s));
    if (it.order) OK_OR_RETURN(prepare_order(c, s, in, it, p));
    if (it.split_items) OK_OR_RETURN(prepare_split_items(L, s.ws, it.items, p));
    // pass stealing (MCPT_STEAL=0: off, tests and A/B; the same bits either way): the mesh kernels
    // in split-item launches, the LDS-scene kernels in launches of several segments (launches of
    // one segment add into the accumulator themselves, pass-split ones run one pass per item:
    // neither steals); the store of every pass's value
    if (lim.may_steal && (it.split_items || (scene_steal && p.n_segments > 1 && !split))) {
      OK_OR_RETURN(ensure_lane_bytes(c, L.d_steal,
                                     (size_t)plan::steal_store_bytes(p.n_tiles, p.tile_w, p.n_segments)));
      p.steal_vals = L.d_steal;
    }
    HIP_OR_RETURN(c->seq.start(c->ring, s));
    if (stream) {
      OK_OR_RETURN(stream_run(c, p));
    } else {
      HIP_OR_RETURN(mcpt_launch_render(p, count, s.ws));
    }
    HIP_OR_RETURN(c->seq.render_done(c->ring, s));
    HIP_OR_RETURN(mcpt_launch_combine(p, c->stream));
    HIP_OR_RETURN(c->seq.combine_done(c->ring, s));
    if (it.order && (!p.item_perm || ++L.order.age >= plan::kOrderRefresh)) OK_OR_RETURN(sort_order(c, L, s.ws, it, p));
    HIP_OR_RETURN(c->seq.release(s));
#ifdef MCPT_CHECKED
    // checked build: the sub-launch (render, combine, order sort) is waited for here, so a fault
    // is reported with the sub-launch that caused it, and the kernels' bounds tests are read
    OK_OR_RETURN(checked_sub_launch(c, k, n_sub, p));
#endif
  }
  c->ring.commit();
  if (!count && c->traversal == MCPT_TRAVERSAL_AUTO)
    tuner.issue(cand, (double)p.n_local_px * n_passes, p.n_local_px, n_passes, total_seg, c->ring.pos());
  c->pass_split = split ? 1 : 0;
  c->pass_count += n_passes;
  // adaptive mode on: a plain render reaches every pixel, retired blocks included
  if (c->adaptive.ad_on && n_passes > 0)
    HIP_OR_RETURN(mcpt_launch_adaptive_add_passes(adaptive_target(c), nullptr, 0, n_passes, c->stream));
  // noise statistics on: the call is one batch, behind its last combine
  if (c->stats.stats_on && n_passes > 0) HIP_OR_RETURN(stats_batch(c, n_passes));
  if (count) {
    unsigned long long h[mcpt::EV_COUNT];
    HIP_OR_RETURN(hipMemcpyAsync(h, c->d_events, sizeof(h), hipMemcpyDeviceToHost, c->stream));
    HIP_OR_RETURN(hipStreamSynchronize(c->stream));
    for (int e = 0; e < mcpt::EV_COUNT; ++e) events[e] += h[e];
  }
  return MCPT_OK;
}

int mcpt_render(mcpt_ctx* c, const float* invPV, const float* invV, int first_pass, int n_passes, float date,
                int bounces, float refract_ind, int variant) {
  return launch(c, invPV, invV, first_pass, n_passes, date, bounces, refract_ind, variant, false, nullptr);
}

int mcpt_render_counted(mcpt_ctx* c, const float* invPV, const float* invV, int first_pass, int n_passes,
                        float date, int bounces, float refract_ind, int variant, unsigned long long* events) {
  if (!events) return mcpt_err_bare(MCPT_ERR_INVALID_ARG);
  return launch(c, invPV, invV, first_pass, n_passes, date, bounces, refract_ind, variant, true, events);
}

int mcpt_debug_counters(mcpt_ctx* c, unsigned long long* out, int n_slots, int reset) {
  if (!c || n_slots < 0 || (!out && n_slots > 0)) return mcpt_err_bare(MCPT_ERR_INVALID_ARG);
  HIP_OR_RETURN(hipSetDevice(c->device));
  const int n = n_slots < MCPT_DEBUG_SLOTS ? n_slots : MCPT_DEBUG_SLOTS;   // never past the caller's buffer
  if (n > 0)
    HIP_OR_RETURN(hipMemcpyAsync(out, c->d_events, sizeof(unsigned long long) * n, hipMemcpyDeviceToHost, c->stream));
  if (reset) HIP_OR_RETURN(hipMemsetAsync(c->d_events, 0, sizeof(unsigned long long) * MCPT_DEBUG_SLOTS, c->stream));
  HIP_OR_RETURN(hipStreamSynchronize(c->stream));
  return MCPT_OK;
}

#ifdef MCPT_BLOCKTIMES
// diagnostic build only: the per-wave (start, end) clock pairs of the last render launch
// (wave w of workgroup b at 2 (b * waves per workgroup + w)), zeroed after the copy
extern "C" int mcpt_debug_blocktimes(mcpt_ctx* c, unsigned long long* out, long long n) {
  if (!c || !out || n < 0 || (size_t)n > mcpt::kBlockTimeSlots) return mcpt_err_bare(MCPT_ERR_INVALID_ARG);
  HIP_OR_RETURN(hipSetDevice(c->device));
  HIP_OR_RETURN(hipMemcpyAsync(out, c->d_events + MCPT_DEBUG_SLOTS, sizeof(unsigned long long) * n,
                               hipMemcpyDeviceToHost, c->stream));
  HIP_OR_RETURN(hipMemsetAsync(c->d_events + MCPT_DEBUG_SLOTS, 0, sizeof(unsigned long long) * mcpt::kBlockTimeSlots, c->stream));
  HIP_OR_RETURN(hipStreamSynchronize(c->stream));
  return MCPT_OK;
}
#endif

int mcpt_event_bytes(int e) {
  if (e < 0 || e >= mcpt::EV_COUNT) return mcpt_err_bare(MCPT_ERR_INVALID_ARG);
  return mcpt::kEventBytes[e];
}

int mcpt_read_accum(mcpt_ctx* c, float* rgb_out, int* pass_count) {
  if (!c) return mcpt_err_bare(MCPT_ERR_INVALID_ARG);
  if (!c->has_target) return mcpt_err_bare(MCPT_ERR_NO_TARGET);
  HIP_OR_RETURN(hipSetDevice(c->device));
  if (rgb_out && c->target.d_accum.bytes())
    HIP_OR_RETURN(hipMemcpyAsync(rgb_out, c->target.d_accum, c->target.d_accum.bytes(), hipMemcpyDeviceToHost, c->stream));
  HIP_OR_RETURN(hipStreamSynchronize(c->stream));
  if (pass_count) *pass_count = c->pass_count;
  return MCPT_OK;
}

int mcpt_write_accum(mcpt_ctx* c, const float* rgb, int pass_count) {
  if (!c || !rgb || pass_count < 0) return mcpt_err_bare(MCPT_ERR_INVALID_ARG);
  if (!c->has_target) return mcpt_err_bare(MCPT_ERR_NO_TARGET);
  HIP_OR_RETURN(hipSetDevice(c->device));
  if (c->target.d_accum.bytes())
    HIP_OR_RETURN(hipMemcpyAsync(c->target.d_accum, rgb, c->target.d_accum.bytes(), hipMemcpyHostToDevice, c->stream));
  HIP_OR_RETURN(hipStreamSynchronize(c->stream));
  c->pass_count = pass_count;
  invalidate_planes(c);
  return MCPT_OK;
}

namespace mcpt {
namespace host {
int checkpoint_write_ex(const char* path, const float* rgb, int W, int rows, int pass_count, int next_pass,
                        const char* tag, int H, unsigned long long rows_hash);
int checkpoint_read_ex(const char* path, float* rgb_out, long long capacity, int* W, int* rows, int* pass_count,
                       int* next_pass, char* tag_out, int* H, unsigned long long* rows_hash);
}  // namespace host
}  // namespace mcpt

int mcpt_checkpoint_save(mcpt_ctx* c, const char* path, int next_pass, const char* tag) {
  if (!c || !path) return mcpt_err_bare(MCPT_ERR_INVALID_ARG);
  if (!c->has_target) return mcpt_err_bare(MCPT_ERR_NO_TARGET);
  std::vector<float> acc((size_t)c->n_local_rows * c->W * 3);
  int n = 0;
  const int st = mcpt_read_accum(c, acc.data(), &n);
  if (st != MCPT_OK) return st;
  if (mcpt::host::checkpoint_write_ex(path, acc.data(), c->W, c->n_local_rows, n, next_pass, tag, c->H, rows_hash(c)) !=
      MCPT_OK)
    return set_err(MCPT_ERR_INVALID_ARG, "mcpt_checkpoint_save: cannot write the file");
  return MCPT_OK;
}

int mcpt_checkpoint_load(mcpt_ctx* c, const char* path, const char* tag, int* next_pass) {
  if (!c || !path) return mcpt_err_bare(MCPT_ERR_INVALID_ARG);
  if (!c->has_target) return mcpt_err_bare(MCPT_ERR_NO_TARGET);
  int w = 0, rows = 0, n = 0, nxt = 0, h = 0;
  unsigned long long hash = 0;
  std::vector<char> t(MCPT_CHECKPOINT_TAG_MAX);
  std::vector<float> acc((size_t)c->n_local_rows * c->W * 3);
  if (mcpt::host::checkpoint_read_ex(path, acc.data(), (long long)acc.size(), &w, &rows, &n, &nxt, t.data(), &h,
                                     &hash) != MCPT_OK)
    return set_err(MCPT_ERR_INVALID_ARG, "mcpt_checkpoint_load: missing, foreign or truncated file, or not this target's size");
  if (h == 0 || hash == 0)
    return set_err(MCPT_ERR_INVALID_ARG,
                   "mcpt_checkpoint_load: the file carries no target identity (mcpt_checkpoint_write); "
                   "read it with mcpt_checkpoint_read and load it with mcpt_write_accum");
  if (w != c->W || rows != c->n_local_rows || h != c->H || hash != rows_hash(c))
    return set_err(MCPT_ERR_INVALID_ARG, "mcpt_checkpoint_load: the checkpoint belongs to another target or shard");
  if (tag && std::strcmp(tag, t.data()) != 0)
    return set_err(MCPT_ERR_INVALID_ARG, "mcpt_checkpoint_load: the render parameters differ (tag)");
  const int st = mcpt_write_accum(c, acc.data(), n);
  if (st != MCPT_OK) return st;
  if (next_pass) *next_pass = nxt;
  return MCPT_OK;
}

int mcpt_accum_device_ptr(mcpt_ctx* c, void** dev_ptr, size_t* bytes) {
  if (!c || !dev_ptr) return mcpt_err_bare(MCPT_ERR_INVALID_ARG);
  if (!c->has_target) return mcpt_err_bare(MCPT_ERR_NO_TARGET);
  *dev_ptr = c->target.d_accum;
  if (bytes) *bytes = c->target.d_accum.bytes();
  return MCPT_OK;
}

int mcpt_trace(mcpt_ctx* c, const float* origins, const float* dirs, int n, int any_hit, int prim, mcpt_hit* out) {
  if (!c || n < 0 || (n > 0 && (!origins || !dirs || !out))) return set_err(MCPT_ERR_INVALID_ARG, "mcpt_trace: bad arguments");
  if (!c->scene.has_scene) return set_err(MCPT_ERR_NO_SCENE, "no scene uploaded");
  if (prim >= c->n_prims) return set_err(MCPT_ERR_INVALID_ARG, "mcpt_trace: primitive index out of range");
  if (c->meshes.n_meshes == 0)
    for (int id : c->mesh_ids)
      if (id >= 0) return set_err(MCPT_ERR_BAD_SCENE, "mesh instances present: call mcpt_upload_meshes");
  if (n == 0) return MCPT_OK;
  HIP_OR_RETURN(hipSetDevice(c->device));
  const size_t n3 = (size_t)n * 3 * sizeof(float), ni = (size_t)n * 3 * sizeof(int);
  const size_t nf = (size_t)n * mcpt::kTraceFloats * sizeof(float);
  DevBuf<char> scratch;
  HIP_OR_RETURN(scratch.alloc(2 * n3 + ni + nf));
  char* buf = scratch;
  mcpt::TraceParams q;
  q.nodes = c->scene.d_nodes; q.leaves = c->scene.d_leaves; q.ptype = c->scene.d_ptype; q.prims = c->scene.d_prims; q.depth = c->depth;
  q.prim = prim < 0 ? -1 : prim;
  q.minfo = c->meshes.d_minfo; q.mpairs = c->meshes.d_mpairs; q.mleaftris = c->meshes.d_mleaftris; q.mtris = c->meshes.d_mtris;
  q.mverts = c->meshes.d_mverts; q.mnorms = c->meshes.d_mnorms; q.n_meshes = c->meshes.n_meshes; q.flat_face = c->flat_face;
  q.orig = (const float*)buf; q.dir = (const float*)(buf + n3);
  q.out_i = (int*)(buf + 2 * n3); q.out = (float*)(buf + 2 * n3 + ni); q.n = n;
  std::vector<int> hi((size_t)n * 3);
  std::vector<float> hf((size_t)n * mcpt::kTraceFloats);
  hipError_t e = hipMemcpyAsync(buf, origins, n3, hipMemcpyHostToDevice, c->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(buf + n3, dirs, n3, hipMemcpyHostToDevice, c->stream);
  if (e == hipSuccess) e = mcpt_launch_trace(q, any_hit != 0, c->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(hi.data(), q.out_i, ni, hipMemcpyDeviceToHost, c->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(hf.data(), q.out, nf, hipMemcpyDeviceToHost, c->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  if (e != hipSuccess) return set_err(MCPT_ERR_HIP, "mcpt_trace", e);
  for (int i = 0; i < n; ++i) {
    mcpt_hit& h = out[i];
    const int* a = &hi[(size_t)i * 3];
    const float* f = &hf[(size_t)i * mcpt::kTraceFloats];
    h.shape = a[0]; h.prim = a[1]; h.dir = a[2];
    h.dist = f[0];
    std::memcpy(h.pl, f + 1, 12); std::memcpy(h.pg, f + 4, 12);
    std::memcpy(h.N, f + 7, 12); std::memcpy(h.P, f + 10, 12);
    std::memcpy(h.color, f + 13, 16); std::memcpy(h.material, f + 17, 16);
  }
  return MCPT_OK;
}

int mcpt_sample_hemisphere(mcpt_ctx* c, const float* normal3, const float* fseed3, float roughness, int nb_used,
                           int n, float* out_xyz) {
  if (!c || !normal3 || !fseed3 || n < 0 || nb_used < 0 || (n > 0 && !out_xyz))
    return set_err(MCPT_ERR_INVALID_ARG, "mcpt_sample_hemisphere: bad arguments");
  if (n == 0) return MCPT_OK;
  HIP_OR_RETURN(hipSetDevice(c->device));
  mcpt::SampleParams q;
  for (int k = 0; k < 3; ++k) { q.normal[k] = normal3[k]; q.fseed[k] = fseed3[k]; }
  q.roughness = roughness; q.nb_used = (uint32_t)nb_used; q.n = n;
  DevBuf<float> out;
  HIP_OR_RETURN(out.alloc((size_t)n * 3));
  q.out = out;
  hipError_t e = mcpt_launch_sample(q, c->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(out_xyz, q.out, (size_t)n * 3 * sizeof(float), hipMemcpyDeviceToHost, c->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  if (e != hipSuccess) return set_err(MCPT_ERR_HIP, "mcpt_sample_hemisphere", e);
  return MCPT_OK;
}

int mcpt_set_traversal(mcpt_ctx* c, int mode) {
  if (!c || mode < MCPT_TRAVERSAL_AUTO || mode > MCPT_TRAVERSAL_STREAM)
    return set_err(MCPT_ERR_INVALID_ARG, "mcpt_set_traversal: bad mode");
  c->traversal = mode;
  reset_tuning(c);
  if (mode != MCPT_TRAVERSAL_STREAM) return free_stream_pools(c);
  return MCPT_OK;
}

int mcpt_set_walk_exit(mcpt_ctx* c, int lanes) {
  if (!c || lanes < -1 || lanes > 64) return set_err(MCPT_ERR_INVALID_ARG, "mcpt_set_walk_exit: bad lane count");
  c->walk_exit = lanes;
  return MCPT_OK;
}

int mcpt_set_stream_pool(mcpt_ctx* c, int slots, int refill) {
  if (!c || slots < 0 || refill < -1 || refill > 64) return set_err(MCPT_ERR_INVALID_ARG, "mcpt_set_stream_pool: bad arguments");
  c->stream_slots = slots;
  c->stream_refill = refill;
  return MCPT_OK;
}

int mcpt_stream_iterations(mcpt_ctx* c, long long* iterations) {
  if (!c || !iterations) return mcpt_err_bare(MCPT_ERR_INVALID_ARG);
  *iterations = c->stream_iters;
  return MCPT_OK;
}

int mcpt_set_render_lanes(mcpt_ctx* c, int on) {
  if (!c) return mcpt_err_bare(MCPT_ERR_INVALID_ARG);
  HIP_OR_RETURN(hipSetDevice(c->device));
  HIP_OR_RETURN(hipStreamSynchronize(c->stream));   // (ordered after every lane's work)
  c->tuner.overlap = on ? 1 : 0;
  c->seq.lanes_switched();
  return MCPT_OK;
}

int mcpt_set_partial_budget(mcpt_ctx* c, size_t bytes) {
  if (!c) return mcpt_err_bare(MCPT_ERR_INVALID_ARG);
  c->partial_budget = bytes;
  return MCPT_OK;
}

int mcpt_last_launch_count(mcpt_ctx* c, int* n_launches) {
  if (!c || !n_launches) return mcpt_err_bare(MCPT_ERR_INVALID_ARG);
  *n_launches = c->ring.n_sub();
  return MCPT_OK;
}

int mcpt_last_pass_split(mcpt_ctx* c, int* split) {
  if (!c || !split) return mcpt_err_bare(MCPT_ERR_INVALID_ARG);
  *split = c->ring.n_timed() > 0 ? c->pass_split : 0;
  return MCPT_OK;
}

int mcpt_set_leaf_batch(mcpt_ctx* c, int lanes) {
  if (!c || lanes < -1 || lanes > 64) return set_err(MCPT_ERR_INVALID_ARG, "mcpt_set_leaf_batch: bad lane count");
  c->leaf_batch = lanes;
  return MCPT_OK;
}

int mcpt_get_leaf_batch(mcpt_ctx* c, int* resolved) {
  if (!c || !resolved) return mcpt_err_bare(MCPT_ERR_INVALID_ARG);
  // the value the next launch of the last launch shape uses (an AUTO deep candidate sets its own)
  *resolved = plan::cand_leaf_batch(resolve_candidate(c, c->tuner.meas_segs), c->leaf_batch, c->depth);
  return MCPT_OK;
}

int mcpt_get_walk_exit(mcpt_ctx* c, int* resolved) {
  if (!c || !resolved) return mcpt_err_bare(MCPT_ERR_INVALID_ARG);
  *resolved = plan::cand_walk_exit(resolve_candidate(c, c->tuner.meas_segs), c->walk_exit, c->meshes.n_meshes, c->depth);
  return MCPT_OK;
}

int mcpt_get_traversal(mcpt_ctx* c, int* resolved) {
  if (!c || !resolved) return mcpt_err_bare(MCPT_ERR_INVALID_ARG);
  *resolved = plan::cand_traversal(resolve_candidate(c, c->tuner.meas_segs));
  return MCPT_OK;
}

int mcpt_get_schedule(mcpt_ctx* c, int* traversal, int* seg_per_item, int* settled) {
  if (!c) return mcpt_err_bare(MCPT_ERR_INVALID_ARG);
  const int cand = resolve_candidate(c, c->tuner.meas_segs);
  if (traversal) *traversal = plan::cand_traversal(cand);
  if (seg_per_item) *seg_per_item = plan::resolved_seg_per_item(cand, env_int("MCPT_SEG_PER_ITEM", 0));
  if (settled) *settled = schedule_settled(c) ? 1 : 0;
  return MCPT_OK;
}

int mcpt_set_stream(mcpt_ctx* c, void* s) {
  if (!c) return mcpt_err_bare(MCPT_ERR_INVALID_ARG);
  HIP_OR_RETURN(hipSetDevice(c->device));
  HIP_OR_RETURN(hipStreamSynchronize(c->stream));
  c->stream = s ? (hipStream_t)s : (hipStream_t)c->own_stream;
  return MCPT_OK;
}

int mcpt_synchronize(mcpt_ctx* c) {
  if (!c) return mcpt_err_bare(MCPT_ERR_INVALID_ARG);
  HIP_OR_RETURN(hipSetDevice(c->device));
  HIP_OR_RETURN(hipStreamSynchronize(c->stream));
  return MCPT_OK;
}

int mcpt_last_render_ms(mcpt_ctx* c, float* ms) {
  if (!c || !ms) return mcpt_err_bare(MCPT_ERR_INVALID_ARG);
  if (c->ring.n_timed() == 0) return set_err(MCPT_ERR_INVALID_ARG, "no render timed yet");
  HIP_OR_RETURN(hipSetDevice(c->device));
  HIP_OR_RETURN(c->ring.call_ms(ms));
  return MCPT_OK;
}

int mcpt_kernel_ms_back(mcpt_ctx* c, int back, float* trace_ms, float* combine_ms) {
  if (!c || !trace_ms || !combine_ms) return mcpt_err_bare(MCPT_ERR_INVALID_ARG);
  const int slot = c->ring.slot_back(back);
  if (slot < 0) return set_err(MCPT_ERR_INVALID_ARG, "mcpt_kernel_ms_back: no such call in the timing ring");
  HIP_OR_RETURN(hipSetDevice(c->device));
  HIP_OR_RETURN(c->ring.launch_ms(slot, trace_ms, combine_ms));
  return MCPT_OK;
}

int mcpt_kernel_span_ms_back(mcpt_ctx* c, int back, float* span_ms) {
  if (!c || !span_ms) return mcpt_err_bare(MCPT_ERR_INVALID_ARG);
  const int slot = c->ring.slot_back(back);
  if (slot < 0) return set_err(MCPT_ERR_INVALID_ARG, "mcpt_kernel_span_ms_back: no such call in the timing ring");
  HIP_OR_RETURN(hipSetDevice(c->device));
  HIP_OR_RETURN(c->ring.span_ms(slot, span_ms));
  return MCPT_OK;
}

int mcpt_last_kernel_ms(mcpt_ctx* c, float* trace_ms, float* combine_ms) {
  if (!c || !trace_ms || !combine_ms) return mcpt_err_bare(MCPT_ERR_INVALID_ARG);
  if (c->ring.n_timed() == 0) return set_err(MCPT_ERR_INVALID_ARG, "no render timed yet");
  return mcpt_kernel_ms_back(c, 0, trace_ms, combine_ms);
}

}  // extern "C"
