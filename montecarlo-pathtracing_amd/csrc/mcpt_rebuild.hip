// mcpt_rebuild.hip — a mesh's BVH rebuilt where it lives: a new leaf order from the
// current vertices, then the refit of mcpt_refit.hip.
//
// The specification is the host's: mcpt_scene_rebuild_mesh (mcpt_scene.cpp: kd_build_stable) followed
// by mcpt_upload_meshes.  kd_build_stable stable-sorts every range of `order` by the round's axis key,
// depth - 1 rounds; here a round is one LSD radix sort of all the mesh's triangle ids by the pair
// (range of the id's position at the round's start, key), 8 bits a pass: a position never leaves its
// range, so the sort by that pair is the stable sort of every range.  The pair is one 64-bit word per
// triangle id, written at the round's start; a pass moves the ids alone and looks its digit up by id.
//
// A pass is three launches: per-workgroup digit counts (integers: their atomics' order cannot show),
// one exclusive scan over (digit, workgroup), digit-major, and the scatter.  The scatter is where such
// a sort goes wrong, so it is kept plain: a workgroup walks its tile 256 positions at a time, in
// order; a lane's rank among equal digits is the count of lower lanes of its wave with that digit (a
// match by ballots) plus the lower waves' counts, so within a step, across steps, and across
// workgroups (the scan) equal digits keep their order.  No arithmetic here depends on an order the
// hardware chooses; the keys are tri_box's centres with the refit's comparison forms, so the order,
// and with it every record, is the host's bit for bit.
#include <algorithm>
#include <cstring>

#include "mcpt_ctx.h"
#include "mcpt_rebuild_plan.h"

namespace {

namespace rb = mcpt::rebuild;

constexpr int kSortThreads = 256;
constexpr int kSortWaves = kSortThreads / 64;
constexpr int kSortTile = 4096;    // positions of a workgroup
constexpr int kScanThreads = 1024;

unsigned sort_groups(int n) { return (unsigned)((n + kSortTile - 1) / kSortTile); }

// the host's mesh-local triangle rows into d_mtris as global vertex ids (a, b, c, 0)
__global__ void tri_rows_kernel(const int* __restrict__ rows, int n, int first_vertex, int4* __restrict__ tris) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n) return;
  tris[t] = make_int4(rows[3 * (size_t)t] + first_vertex, rows[3 * (size_t)t + 1] + first_vertex,
                      rows[3 * (size_t)t + 2] + first_vertex, 0);
}

// order = 0 .. n-1 and, per axis, every triangle's centre key (tri_box: (lo + hi) / 2.0f of the grown box)
__global__ void centre_keys_kernel(const int4* __restrict__ tris, const float4* __restrict__ verts, int n,
                                   unsigned* __restrict__ ckey, int* __restrict__ ids) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n) return;
  const int4 vi = tris[t];
  float mn[3], mx[3];
  tri_box_dev(verts[vi.x], verts[vi.y], verts[vi.z], mn, mx);
  for (int q = 0; q < 3; ++q) ckey[(size_t)q * n + t] = rb::float_key((mn[q] + mx[q]) / 2.0f);
  ids[t] = t;
}

// a round's sort word of the triangle at each position: (its range after `r` rounds, its key on the axis)
__global__ void round_keys_kernel(const int* __restrict__ ids, const unsigned* __restrict__ ckey_axis, int n, int r,
                                  unsigned long long* __restrict__ key) {
  const int pos = blockIdx.x * blockDim.x + threadIdx.x;
  if (pos >= n) return;
  const int id = ids[pos];
  key[id] = ((unsigned long long)(unsigned)rb::range_of(n, r, pos) << 32) | ckey_axis[id];
}

__device__ __forceinline__ unsigned digit_of(const unsigned long long* __restrict__ key, int id, int shift) {
  return (unsigned)(key[id] >> shift) & 255u;
}

// hist[digit * n_groups + workgroup]: how many of the workgroup's positions hold that digit
__global__ __launch_bounds__(kSortThreads) void sort_count_kernel(const int* __restrict__ ids,
                                                                  const unsigned long long* __restrict__ key, int n,
                                                                  int shift, unsigned* __restrict__ hist) {
  __shared__ unsigned s_h[256];
  s_h[threadIdx.x] = 0;
  __syncthreads();
  const int first = blockIdx.x * kSortTile, end = min(n, first + kSortTile);
  for (int i = first + (int)threadIdx.x; i < end; i += kSortThreads) atomicAdd(&s_h[digit_of(key, ids[i], shift)], 1u);
  __syncthreads();
  hist[(size_t)threadIdx.x * gridDim.x + blockIdx.x] = s_h[threadIdx.x];
}

// exclusive scan of hist[0 .. n_entries) in place, one workgroup: each thread a run of entries
__global__ __launch_bounds__(kScanThreads) void sort_scan_kernel(unsigned* __restrict__ hist, int n_entries) {
  __shared__ unsigned s_sum[2][kScanThreads];
  const int tid = threadIdx.x;
  const int run = (n_entries + kScanThreads - 1) / kScanThreads;
  const int a = min(n_entries, tid * run), b = min(n_entries, a + run);
  unsigned sum = 0;
  for (int i = a; i < b; ++i) sum += hist[i];
  s_sum[0][tid] = sum;
  __syncthreads();
  int cur = 0;
  for (int off = 1; off < kScanThreads; off <<= 1, cur ^= 1) {
    unsigned v = s_sum[cur][tid];
    if (tid >= off) v += s_sum[cur][tid - off];
    s_sum[cur ^ 1][tid] = v;
    __syncthreads();
  }
  unsigned at = s_sum[cur][tid] - sum;
  for (int i = a; i < b; ++i) {
    const unsigned v = hist[i];
    hist[i] = at;
    at += v;
  }
}

// the stable scatter of a pass: position i's id goes to (scanned count of its digit and workgroup) +
// (how many earlier positions of the workgroup hold the digit)
__global__ __launch_bounds__(kSortThreads) void sort_scatter_kernel(const int* __restrict__ in, int* __restrict__ out,
                                                                    const unsigned long long* __restrict__ key, int n,
                                                                    int shift, const unsigned* __restrict__ hist) {
  __shared__ unsigned s_base[256];               // per digit: where the step's first such id goes
  __shared__ unsigned s_wcnt[kSortWaves][256];   // per wave and digit: the step's count
  const unsigned tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  s_base[tid] = hist[(size_t)tid * gridDim.x + blockIdx.x];
  for (int w = 0; w < kSortWaves; ++w) s_wcnt[w][tid] = 0;
  __syncthreads();
  const int first = blockIdx.x * kSortTile, end = min(n, first + kSortTile);
  for (int step = first; step < end; step += kSortThreads) {   // (uniform: every lane takes every ballot)
    const int i = step + (int)tid;
    const bool live = i < end;
    int id = 0;
    unsigned d = 0;
    if (live) { id = in[i]; d = digit_of(key, id, shift); }
    // the live lanes of the wave with this lane's digit
    unsigned long long same = __ballot(live);
    for (int bit = 0; bit < 8; ++bit) {
      const bool set = (d >> bit) & 1u;
      const unsigned long long have = __ballot(live && set);
      same &= set ? have : ~have;
    }
    const unsigned rank = (unsigned)__popcll(same & ((1ull << lane) - 1ull));
    if (live && rank == 0) s_wcnt[wave][d] = (unsigned)__popcll(same);
    __syncthreads();
    if (live) {
      unsigned at = s_base[d] + rank;
      for (unsigned w = 0; w < wave; ++w) at += s_wcnt[w][d];
      if (at < (unsigned)n) out[at] = id;   // (always: the counts are this walk's own)
    }
    __syncthreads();
    unsigned c = 0;
    for (int w = 0; w < kSortWaves; ++w) { c += s_wcnt[w][tid]; s_wcnt[w][tid] = 0; }
    s_base[tid] += c;
    __syncthreads();
  }
}

// the leaf records' triangle ids from the final order: range s of the last round is leaves 2s, 2s + 1.
// A leaf with a triangle gets its id word alone (the refit writes the rest from it); an empty one the
// whole record mcpt_upload_meshes writes for it.
__global__ void leaf_ids_kernel(const int* __restrict__ ids, int n, int depth, float4* __restrict__ leafrec) {
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= (1 << (depth - 1))) return;
  int first, second;
  rb::leaf_pair(n, depth, s, first, second);
  float4* const r = leafrec + (size_t)s * 8;
  const int t0 = ids[first];
  r[0].w = __int_as_float((unsigned)t0 < (unsigned)n ? t0 : 0);
  if (second >= 0) {
    const int t1 = ids[second];
    r[4].w = __int_as_float((unsigned)t1 < (unsigned)n ? t1 : 0);
  } else {
    r[4] = make_float4(0.0f, 0.0f, 0.0f, __int_as_float(-1));
    r[5] = r[6] = r[7] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  }
}

dim3 grid_for(int n, int block) { return dim3((unsigned)((n + block - 1) / block)); }

// the sort's scratch: sized once, for the largest uploaded mesh; the ids start in range so that no
// lookup by id can leave the arrays whatever a pass reads
int ensure_sort_scratch(mcpt_ctx* c) {
  mcpt_ctx::Meshes& ms = c->meshes;
  int n_max = 1;
  for (int n : ms.n_tris) n_max = std::max(n_max, n);
  if (ms.d_sort_key.size() >= (size_t)n_max) return MCPT_OK;
  HIP_OR_RETURN(ms.d_sort_ckey.alloc(3 * (size_t)n_max));
  HIP_OR_RETURN(ms.d_sort_key.alloc((size_t)n_max));
  for (auto& b : ms.d_sort_ids) {
    HIP_OR_RETURN(b.alloc((size_t)n_max));
    HIP_OR_RETURN(hipMemsetAsync(b, 0, b.bytes(), c->stream));
  }
  HIP_OR_RETURN(ms.d_sort_hist.alloc(256 * (size_t)sort_groups(n_max)));
  return MCPT_OK;
}

// mesh m's new order into its leaf records; *passes: the radix passes launched
int sort_mesh(mcpt_ctx* c, int m, int* passes) {
  mcpt_ctx::Meshes& ms = c->meshes;
  const int4 mi = ms.info[m];   // (first pair slot, first leaf, depth, first triangle)
  const int n = ms.n_tris[m], depth = mi.z;
  int* ids[2] = {ms.d_sort_ids[0], ms.d_sort_ids[1]};
  const unsigned groups = sort_groups(n);
  centre_keys_kernel<<<grid_for(n, 256), dim3(256), 0, c->stream>>>(ms.d_mtris + mi.w, ms.d_mverts, n, ms.d_sort_ckey, ids[0]);
  HIP_OR_RETURN(hipGetLastError());
  int cur = 0;
  for (int round = 1; round < depth; ++round) {
    const int axis = (round - 1) % 3, range_bits = round - 1;
    round_keys_kernel<<<grid_for(n, 256), dim3(256), 0, c->stream>>>(ids[cur], ms.d_sort_ckey + (size_t)axis * n, n,
                                                                     range_bits, ms.d_sort_key);
    HIP_OR_RETURN(hipGetLastError());
    for (int shift = 0; shift < 32 + range_bits; shift += 8, cur ^= 1, ++*passes) {
      sort_count_kernel<<<dim3(groups), dim3(kSortThreads), 0, c->stream>>>(ids[cur], ms.d_sort_key, n, shift, ms.d_sort_hist);
      HIP_OR_RETURN(hipGetLastError());
      sort_scan_kernel<<<dim3(1), dim3(kScanThreads), 0, c->stream>>>(ms.d_sort_hist, (int)(256 * groups));
      HIP_OR_RETURN(hipGetLastError());
      sort_scatter_kernel<<<dim3(groups), dim3(kSortThreads), 0, c->stream>>>(ids[cur], ids[cur ^ 1], ms.d_sort_key, n, shift,
                                                                              ms.d_sort_hist);
      HIP_OR_RETURN(hipGetLastError());
    }
  }
  leaf_ids_kernel<<<grid_for(1 << (depth - 1), 256), dim3(256), 0, c->stream>>>(ids[cur], n, depth,
                                                                                ms.d_mleaftris + (size_t)mi.y * 4);
  HIP_OR_RETURN(hipGetLastError());
  return MCPT_OK;
}

}  // namespace

extern "C" {

int mcpt_set_mesh_vertex_counts(mcpt_ctx* c, int n_meshes, const int* counts) {
  if (!c || !counts) return set_err(MCPT_ERR_INVALID_ARG, "mcpt_set_mesh_vertex_counts: bad arguments");
  mcpt_ctx::Meshes& ms = c->meshes;
  if (ms.n_meshes == 0) return set_err(MCPT_ERR_BAD_SCENE, "no meshes uploaded");
  if (n_meshes != ms.n_meshes) return set_err(MCPT_ERR_INVALID_ARG, "mcpt_set_mesh_vertex_counts: not the uploaded meshes' count");
  long long first = 0;
  for (int m = 0; m < n_meshes; first += counts[m], ++m)
    if (counts[m] <= 0 || ms.vert_lo[m] < first || ms.vert_hi[m] >= first + counts[m])
      return set_err(MCPT_ERR_INVALID_ARG, "mcpt_set_mesh_vertex_counts: a mesh's triangles reach outside its vertices");
  if ((size_t)first != ms.d_mverts.size())
    return set_err(MCPT_ERR_INVALID_ARG, "mcpt_set_mesh_vertex_counts: the counts do not add up to the uploaded vertices");
  first = 0;
  for (int m = 0; m < n_meshes; first += counts[m], ++m) { ms.vert_first[m] = (int)first; ms.vert_count[m] = counts[m]; }
  return MCPT_OK;
}

int mcpt_rebuild_mesh(mcpt_ctx* c, int mesh_id, const int* tris, int n_tris, mcpt_rebuild_t* out) {
  if (c && tris && mesh_id < 0)
    return set_err(MCPT_ERR_INVALID_ARG, "mcpt_rebuild_mesh: new triangles go to one mesh");
  int m0 = 0, m1 = 0;
  OK_OR_RETURN(refit_prepare(c, mesh_id, "mcpt_rebuild_mesh", m0, m1));
  mcpt_ctx::Meshes& ms = c->meshes;
  for (int m = m0; m < m1; ++m)
    if (ms.info[m].z != rb::depth_of(ms.n_tris[m]))
      return set_err(MCPT_ERR_BAD_SCENE, "mcpt_rebuild_mesh: the mesh's depth is not ceil(log2(triangles))");
  if (tris) {
    if (n_tris != ms.n_tris[mesh_id])
      return set_err(MCPT_ERR_INVALID_ARG, "mcpt_rebuild_mesh: the triangle count differs from the mesh's");
    if (ms.vert_count[mesh_id] <= 0)
      return set_err(MCPT_ERR_BAD_SCENE, "mcpt_rebuild_mesh: new triangles need mcpt_set_mesh_vertex_counts first");
    for (size_t i = 0; i < (size_t)n_tris * 3; ++i)
      if (tris[i] < 0 || tris[i] >= ms.vert_count[mesh_id])
        return set_err(MCPT_ERR_INVALID_ARG, "mcpt_rebuild_mesh: vertex index outside the mesh's vertices");
  }
  OK_OR_RETURN(ensure_sort_scratch(c));
  if (out) {
    std::memset(out, 0, sizeof(*out));
    HIP_OR_RETURN(ensure_timing_events(ms.rebuild_ev, 3));
    HIP_OR_RETURN(hipEventRecord(ms.rebuild_ev[0], c->stream));
  }
  if (tris) {
    const size_t n3 = (size_t)n_tris * 3;
    if (n3 > ms.d_tri_staging.size()) {
      HIP_OR_RETURN(hipStreamSynchronize(c->stream));   // (an earlier rebuild may still read it)
      HIP_OR_RETURN(ms.d_tri_staging.alloc(n3));
    }
    HIP_OR_RETURN(hipMemcpyAsync(ms.d_tri_staging, tris, n3 * sizeof(int), hipMemcpyHostToDevice, c->stream));
    tri_rows_kernel<<<grid_for(n_tris, 256), dim3(256), 0, c->stream>>>(ms.d_tri_staging, n_tris, ms.vert_first[mesh_id],
                                                                        ms.d_mtris + ms.info[mesh_id].w);
    HIP_OR_RETURN(hipGetLastError());
  }
  long long sorted = 0;
  int rounds = 0, passes = 0;
  for (int m = m0; m < m1; ++m) {
    const int d = ms.info[m].z;
    if (d == 0) continue;   // one triangle in a leaf with id -1: no order, no records
    OK_OR_RETURN(sort_mesh(c, m, &passes));
    if (d >= 2) { sorted += ms.n_tris[m]; rounds += d - 1; }
  }
  if (out) HIP_OR_RETURN(hipEventRecord(ms.rebuild_ev[1], c->stream));
  const float4* root = nullptr;
  for (int m = m0; m < m1; ++m) OK_OR_RETURN(refit_launch(c, m, &root));
  geometry_changed(c);
  if (!out) return MCPT_OK;
  float4 rbox[2] = {make_float4(0.0f, 0.0f, 0.0f, 0.0f), make_float4(0.0f, 0.0f, 0.0f, 0.0f)};
  HIP_OR_RETURN(hipEventRecord(ms.rebuild_ev[2], c->stream));
  const bool has_root = mesh_id >= 0 && root;
  if (has_root) HIP_OR_RETURN(hipMemcpyAsync(rbox, root, sizeof(rbox), hipMemcpyDeviceToHost, c->stream));
  HIP_OR_RETURN(hipStreamSynchronize(c->stream));
  HIP_OR_RETURN(hipEventElapsedTime(&out->sort_ms, ms.rebuild_ev[0], ms.rebuild_ev[1]));
  HIP_OR_RETURN(hipEventElapsedTime(&out->refit_ms, ms.rebuild_ev[1], ms.rebuild_ev[2]));
  out->triangles = sorted; out->rounds = rounds; out->sort_passes = passes;
  out->has_root = has_root ? 1 : 0;
  out->root_box[0] = rbox[0].x; out->root_box[1] = rbox[0].y; out->root_box[2] = rbox[0].z;
  out->root_box[3] = rbox[1].x; out->root_box[4] = rbox[1].y; out->root_box[5] = rbox[1].z;
  return MCPT_OK;
}

}  // extern "C"
