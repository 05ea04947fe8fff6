// mcpt_refit.hip — deforming meshes: new vertices into the uploaded meshes and
// the refit of their BVH records where they live, with the C ABI of both and the records' reader.
//
// The specification is the host's: mcpt_scene_update_mesh (mcpt_scene.cpp: tri_box, the lone leaf's
// sibling box, kd_build's merge) followed by mcpt_upload_meshes (mcpt_capi.hip: pack_nodes,
// pack_mesh_pairs, the leaf records).  The kernels here write the same bits: min / max are the
// comparisons std::min / std::max make, in the host's operand order, and the build has no
// contraction (-ffp-contract=off), so signed zeros and ties come out as on the host.  No atomics, no
// arithmetic whose result depends on an order the hardware chooses.
//
// The host merges level by level; the device reduces by subtree.  The heap layout makes every run of
// 2^k consecutive nodes of a level a complete subtree's bottom: a workgroup of 2^k threads takes such
// a run, keeps the boxes in LDS, walks k levels up writing each level's child-pair records, and
// leaves the subtree root's {min, max, has} in a scratch array, which the next stage takes as its
// run.  Stage one's items are the leaves (it gathers the triangles' vertices and writes the leaf
// records); depth 20 is three launches (8 + 8 + 4 levels).
#include <algorithm>
#include <cstring>

#include "mcpt_ctx.h"

namespace {

constexpr int kRefitK = 8;                    // levels a stage walks up
constexpr int kRefitThreads = 1 << kRefitK;   // ... and its workgroup

struct RefitStage {
  float4* pairs;         // the mesh's pair slots (its slot 0)
  float4* leafrec;       // the mesh's leaf records
  const int4* tris;      // the mesh's triangles (global vertex ids)
  const float4* verts;
  const float4* in;      // box stages: the items' {min, has} {max, 0}
  float4* out;           // one per workgroup: its subtree root's
  int lev;               // the items are the 2^lev nodes of level lev (>= 1)
  int up;                // levels walked: min(kRefitK, lev)
};

// a child's rows of a pair record, as pack_nodes computes them: (centre, has) (half-width)
__device__ __forceinline__ void node_rows(const float mn[3], const float mx[3], float has, float4& c, float4& w) {
  c = make_float4((mn[0] + mx[0]) / 2.0f, (mn[1] + mx[1]) / 2.0f, (mn[2] + mx[2]) / 2.0f, has);
  w = make_float4(0.5f * (mx[0] - mn[0]), 0.5f * (mx[1] - mn[1]), 0.5f * (mx[2] - mn[2]), 0.0f);
}
// pack_mesh_pairs' flag: the half-width lies in rcp_core's exact range
__device__ __forceinline__ bool rcp_in_range(float v) {
  const float a = fabsf(v);
  return a >= 0x1p-126f && a < 0x1p126f;
}

template <bool LEAF>
__global__ __launch_bounds__(kRefitThreads) void refit_stage_kernel(RefitStage p) {
  // the boxes of a level, component-major; a level reads one half and writes the other
  __shared__ float s_box[2][7][kRefitThreads];
  const unsigned j = threadIdx.x;
  const unsigned n_items = 1u << p.lev;
  const unsigned cnt = n_items < (unsigned)kRefitThreads ? n_items : (unsigned)kRefitThreads;   // items of this workgroup
  const unsigned g = blockIdx.x * cnt + j;
  const bool live = j < cnt;
  float mn[3] = {0.0f, 0.0f, 0.0f}, mx[3] = {0.0f, 0.0f, 0.0f}, has = 0.0f;
  if (LEAF) {
    int t = -1;
    if (live) t = __float_as_int(p.leafrec[(size_t)g * 4].w);
    if (t >= 0) {
      const int4 vi = p.tris[t];
      const float4 A = p.verts[vi.x], B = p.verts[vi.y], C = p.verts[vi.z];
      tri_box_dev(A, B, C, mn, mx);
      has = 1.0f;
      float4* r = p.leafrec + (size_t)g * 4;
      r[0] = make_float4(A.x, A.y, A.z, __int_as_float(t));
      r[1] = make_float4(B.x - A.x, B.y - A.y, B.z - A.z, 0.0f);
      r[2] = make_float4(C.x - A.x, C.y - A.y, C.z - A.z, 0.0f);
      r[3] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    }
    for (int q = 0; q < 3; ++q) { s_box[0][q][j] = mn[q]; s_box[0][3 + q][j] = mx[q]; }
    s_box[0][6][j] = has;
    __syncthreads();
    // an empty leaf: its sibling's box (kd_build's lone item: "its box twice"); has stays 0
    if (live && t < 0) {
      for (int q = 0; q < 6; ++q) s_box[0][q][j] = s_box[0][q][j ^ 1u];
    }
  } else {
    if (live) {
      const float4 a = p.in[(size_t)g * 2], b = p.in[(size_t)g * 2 + 1];
      mn[0] = a.x; mn[1] = a.y; mn[2] = a.z; has = a.w;
      mx[0] = b.x; mx[1] = b.y; mx[2] = b.z;
    }
    for (int q = 0; q < 3; ++q) { s_box[0][q][j] = mn[q]; s_box[0][3 + q][j] = mx[q]; }
    s_box[0][6][j] = has;
  }
  __syncthreads();
  for (int s = 1; s <= p.up; ++s) {
    const unsigned n_par = cnt >> s;
    const int rd = (s - 1) & 1, wr = s & 1;
    if (j < n_par) {
      float lmn[3], lmx[3], rmn[3], rmx[3];
      for (int q = 0; q < 3; ++q) {
        lmn[q] = s_box[rd][q][2 * j]; lmx[q] = s_box[rd][3 + q][2 * j];
        rmn[q] = s_box[rd][q][2 * j + 1]; rmx[q] = s_box[rd][3 + q][2 * j + 1];
      }
      const float lhas = s_box[rd][6][2 * j], rhas = s_box[rd][6][2 * j + 1];
      // the parent: node i of the heap, item (first item of the workgroup >> s) + j of level lev - s
      const unsigned i = ((1u << (p.lev - s)) - 1u) + ((blockIdx.x * cnt) >> s) + j;
      float4 cl, wl, cr, wrr;
      node_rows(lmn, lmx, lhas, cl, wl);
      node_rows(rmn, rmx, rhas, cr, wrr);
      wl.w = (rcp_in_range(wl.x) && rcp_in_range(wl.y) && rcp_in_range(wl.z) && rcp_in_range(wrr.x) &&
              rcp_in_range(wrr.y) && rcp_in_range(wrr.z)) ? 1.0f : 0.0f;
      float4* o = p.pairs + (size_t)mcpt::mesh_pair_slot(i) * 4;
      o[0] = cl; o[1] = wl; o[2] = cr; o[3] = wrr;
      // kd_build's merge: std::min(c1, c2), std::max(c1, c2) with c1 the right child
      for (int q = 0; q < 3; ++q) {
        mn[q] = min_ab(rmn[q], lmn[q]);
        mx[q] = max_ab(rmx[q], lmx[q]);
        s_box[wr][q][j] = mn[q]; s_box[wr][3 + q][j] = mx[q];
      }
      has = (lhas != 0.0f || rhas != 0.0f) ? 1.0f : 0.0f;
      s_box[wr][6][j] = has;
    }
    __syncthreads();
  }
  if (j == 0) {   // (thread 0 made the last merge itself)
    p.out[(size_t)blockIdx.x * 2] = make_float4(mn[0], mn[1], mn[2], has);
    p.out[(size_t)blockIdx.x * 2 + 1] = make_float4(mx[0], mx[1], mx[2], 0.0f);
  }
}

// packed n x 3 f32 positions and normals -> the float4 arrays (.w = 0) from `first` on
__global__ void widen_vertices_kernel(const float* __restrict__ v, const float* __restrict__ nrm, int n,
                                      float4* __restrict__ verts, float4* __restrict__ norms) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  verts[i] = make_float4(v[3 * (size_t)i], v[3 * (size_t)i + 1], v[3 * (size_t)i + 2], 0.0f);
  norms[i] = make_float4(nrm[3 * (size_t)i], nrm[3 * (size_t)i + 1], nrm[3 * (size_t)i + 2], 0.0f);
}

unsigned stage_groups(int lev) { return lev > kRefitK ? 1u << (lev - kRefitK) : 1u; }

// scratch of a mesh of depth d: the roots stage one leaves, then (the other half) stage two's; stage
// three writes one root into the first half again
size_t scratch_half_a(int d) { return 2 * (size_t)stage_groups(d); }
size_t scratch_half_b(int d) { return 2 * (size_t)stage_groups(std::max(d - kRefitK, 0)); }

int update_vertices(mcpt_ctx* c, int first, int n, const float* d_v, const float* d_n) {
  if (n == 0) return MCPT_OK;
  widen_vertices_kernel<<<dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream>>>(
      d_v, d_n, n, c->meshes.d_mverts + first, c->meshes.d_mnorms + first);
  HIP_OR_RETURN(hipGetLastError());
  geometry_changed(c);
  return MCPT_OK;
}

int check_vertex_range(const mcpt_ctx* c, int first, int n, const void* v, const void* nrm, const char* who) {
  char what[96];
  if (!c || !v || !nrm) {
    std::snprintf(what, sizeof(what), "%s: bad arguments", who);
    return set_err(MCPT_ERR_INVALID_ARG, what);
  }
  if (c->meshes.n_meshes == 0) return set_err(MCPT_ERR_BAD_SCENE, "no meshes uploaded");
  if (first < 0 || n < 0 || (size_t)first + (size_t)n > c->meshes.d_mverts.size()) {
    std::snprintf(what, sizeof(what), "%s: vertex range outside the uploaded vertices", who);
    return set_err(MCPT_ERR_INVALID_ARG, what);
  }
  return MCPT_OK;
}

}  // namespace

// the geometry changed behind the queued renders: what was derived from it is stale, and the render
// lanes' next launches must wait for the context's stream again (LaneSeq::used_in_order)
void geometry_changed(mcpt_ctx* c) {
  c->denoise.guides_valid = false;
  c->temporal.tp_frames = 0;
  c->seq.used_in_order(0);
  c->seq.used_in_order(1);
}

int refit_prepare(mcpt_ctx* c, int mesh_id, const char* who, int& m0, int& m1) {
  char what[96];
  if (!c) {
    std::snprintf(what, sizeof(what), "%s: bad arguments", who);
    return set_err(MCPT_ERR_INVALID_ARG, what);
  }
  mcpt_ctx::Meshes& ms = c->meshes;
  if (ms.n_meshes == 0) return set_err(MCPT_ERR_BAD_SCENE, "no meshes uploaded");
  if (mesh_id < -1 || mesh_id >= ms.n_meshes) {
    std::snprintf(what, sizeof(what), "%s: no such mesh", who);
    return set_err(MCPT_ERR_INVALID_ARG, what);
  }
  m0 = mesh_id < 0 ? 0 : mesh_id; m1 = mesh_id < 0 ? ms.n_meshes : mesh_id + 1;
  size_t half_a = 2, half_b = 2;
  for (int m = m0; m < m1; ++m) {
    if (ms.empty_pair[m]) {
      std::snprintf(what, sizeof(what), "%s: a leaf pair of the mesh holds no triangle", who);
      return set_err(MCPT_ERR_BAD_SCENE, what);
    }
    half_a = std::max(half_a, scratch_half_a(ms.info[m].z));
    half_b = std::max(half_b, scratch_half_b(ms.info[m].z));
  }
  HIP_OR_RETURN(hipSetDevice(c->device));
  if (half_a + half_b > ms.d_refit_scratch.size()) {
    HIP_OR_RETURN(hipStreamSynchronize(c->stream));   // (an earlier refit of a shallower mesh may still use it)
    HIP_OR_RETURN(ms.d_refit_scratch.alloc(half_a + half_b));
  }
  return MCPT_OK;
}

int refit_launch(mcpt_ctx* c, int m, const float4** root) {
  mcpt_ctx::Meshes& ms = c->meshes;
  const int4 mi = ms.info[m];   // (first pair slot, first leaf, depth, first triangle)
  if (mi.z == 0) return MCPT_OK;   // one triangle in a leaf with id -1: no records
  float4* const half[2] = {ms.d_refit_scratch, ms.d_refit_scratch + std::max<size_t>(2, scratch_half_a(mi.z))};
  RefitStage p;
  p.pairs = ms.d_mpairs + (size_t)mi.x * 4;
  p.leafrec = ms.d_mleaftris + (size_t)mi.y * 4;
  p.tris = ms.d_mtris + mi.w;
  p.verts = ms.d_mverts;
  p.in = nullptr;
  int side = 0;
  for (int lev = mi.z; lev > 0; side ^= 1) {
    p.lev = lev; p.up = std::min(kRefitK, lev); p.out = half[side];
    const dim3 grid(stage_groups(lev)), block(kRefitThreads);
    if (lev == mi.z) refit_stage_kernel<true><<<grid, block, 0, c->stream>>>(p);
    else refit_stage_kernel<false><<<grid, block, 0, c->stream>>>(p);
    HIP_OR_RETURN(hipGetLastError());
    lev -= p.up;
    p.in = p.out;
  }
  *root = p.in;
  return MCPT_OK;
}

extern "C" {

int mcpt_update_mesh_vertices_device(mcpt_ctx* c, int first_vertex, int n_vertices, const void* verts_dev,
                                     const void* normals_dev) {
  OK_OR_RETURN(check_vertex_range(c, first_vertex, n_vertices, verts_dev, normals_dev, "mcpt_update_mesh_vertices_device"));
  HIP_OR_RETURN(hipSetDevice(c->device));
  return update_vertices(c, first_vertex, n_vertices, (const float*)verts_dev, (const float*)normals_dev);
}

int mcpt_update_mesh_vertices(mcpt_ctx* c, int first_vertex, int n_vertices, const float* verts, const float* normals) {
  OK_OR_RETURN(check_vertex_range(c, first_vertex, n_vertices, verts, normals, "mcpt_update_mesh_vertices"));
  if (n_vertices == 0) return MCPT_OK;
  HIP_OR_RETURN(hipSetDevice(c->device));
  const size_t n3 = (size_t)n_vertices * 3;
  DevBuf<float>& st = c->meshes.d_vert_staging;
  if (2 * n3 > st.size()) {
    HIP_OR_RETURN(hipStreamSynchronize(c->stream));   // (an earlier update may still read it)
    HIP_OR_RETURN(st.alloc(2 * n3));
  }
  HIP_OR_RETURN(hipMemcpyAsync(st, verts, n3 * sizeof(float), hipMemcpyHostToDevice, c->stream));
  HIP_OR_RETURN(hipMemcpyAsync(st + n3, normals, n3 * sizeof(float), hipMemcpyHostToDevice, c->stream));
  return update_vertices(c, first_vertex, n_vertices, st, st + n3);
}

int mcpt_refit_mesh(mcpt_ctx* c, int mesh_id, mcpt_refit_t* out) {
  int m0 = 0, m1 = 0;
  OK_OR_RETURN(refit_prepare(c, mesh_id, "mcpt_refit_mesh", m0, m1));
  mcpt_ctx::Meshes& ms = c->meshes;
  if (out) {
    std::memset(out, 0, sizeof(*out));
    HIP_OR_RETURN(ensure_timing_events(ms.refit_ev, 2));
    HIP_OR_RETURN(hipEventRecord(ms.refit_ev[0], c->stream));
  }
  long long n_tris = 0, n_leaves = 0, n_internal = 0;
  const float4* root = nullptr;
  for (int m = m0; m < m1; ++m) {
    const int d = ms.info[m].z;
    if (d == 0) continue;
    OK_OR_RETURN(refit_launch(c, m, &root));
    n_tris += ms.leaf_tris[m]; n_leaves += 1LL << d; n_internal += (1LL << d) - 1;
  }
  geometry_changed(c);
  if (!out) return MCPT_OK;
  float4 rb[2] = {make_float4(0.0f, 0.0f, 0.0f, 0.0f), make_float4(0.0f, 0.0f, 0.0f, 0.0f)};
  HIP_OR_RETURN(hipEventRecord(ms.refit_ev[1], c->stream));
  const bool has_root = mesh_id >= 0 && root;
  if (has_root) HIP_OR_RETURN(hipMemcpyAsync(rb, root, sizeof(rb), hipMemcpyDeviceToHost, c->stream));
  HIP_OR_RETURN(hipStreamSynchronize(c->stream));
  HIP_OR_RETURN(hipEventElapsedTime(&out->device_ms, ms.refit_ev[0], ms.refit_ev[1]));
  out->triangles = n_tris; out->leaves = n_leaves; out->internal_nodes = n_internal;
  out->has_root = has_root ? 1 : 0;
  out->root_box[0] = rb[0].x; out->root_box[1] = rb[0].y; out->root_box[2] = rb[0].z;
  out->root_box[3] = rb[1].x; out->root_box[4] = rb[1].y; out->root_box[5] = rb[1].z;
  return MCPT_OK;
}

int mcpt_debug_mesh_record_sizes(mcpt_ctx* c, size_t* pair_floats, size_t* leaf_floats) {
  if (!c || !pair_floats || !leaf_floats) return mcpt_err_bare(MCPT_ERR_INVALID_ARG);
  *pair_floats = c->meshes.n_pair_f4 * 4;
  *leaf_floats = c->meshes.n_leaf_f4 * 4;
  return MCPT_OK;
}

int mcpt_debug_mesh_records(mcpt_ctx* c, float* pairs_out, size_t pair_floats, float* leaves_out, size_t leaf_floats) {
  if (!c) return mcpt_err_bare(MCPT_ERR_INVALID_ARG);
  const mcpt_ctx::Meshes& ms = c->meshes;
  if (ms.n_meshes == 0) return set_err(MCPT_ERR_BAD_SCENE, "no meshes uploaded");
  if ((pairs_out && pair_floats != ms.n_pair_f4 * 4) || (leaves_out && leaf_floats != ms.n_leaf_f4 * 4))
    return set_err(MCPT_ERR_INVALID_ARG, "mcpt_debug_mesh_records: sizes differ from mcpt_debug_mesh_record_sizes");
  HIP_OR_RETURN(hipSetDevice(c->device));
  if (pairs_out)
    HIP_OR_RETURN(hipMemcpyAsync(pairs_out, ms.d_mpairs, ms.n_pair_f4 * sizeof(float4), hipMemcpyDeviceToHost, c->stream));
  if (leaves_out)
    HIP_OR_RETURN(hipMemcpyAsync(leaves_out, ms.d_mleaftris, ms.n_leaf_f4 * sizeof(float4), hipMemcpyDeviceToHost, c->stream));
  HIP_OR_RETURN(hipStreamSynchronize(c->stream));
  return MCPT_OK;
}

}  // extern "C"
