// mcpt_denoise.hip — primary-hit guide buffers and the edge-avoiding à-trous filter
// (no reference equivalent: the reference only averages, fs_frag).
//
//  * guide_kernel: one lane per pixel, 8x8 pixels per wave as render_kernel; the pixel's camera
//    ray (the render kernel's: same u, v, corner rays and origin), the closest hit
//    (traverse_lane) and intersection_info (geom_info) -> two float4 guide words and the hit
//    primitive's colour.  The values render_kernel memoises per segment (N0, P0, s_hit0).
//  * average4_kernel: accum / pass_count as float4 (rgb, 0): the filter's first input.
//  * atrous_*_kernel: one iteration of the filter (tap spacing `step`), one lane per pixel; all
//    three run atrous_pixel, the contract's operations in the contract's order, and differ only
//    in where a tap's three 16-byte words come from:
//      atrous_lds_kernel<STEP> (step 1, 2): the workgroup's 16x16 tile and its 2·step halo are
//        staged in LDS (colour and both guide words), the 25 taps read LDS;
//      atrous_global_kernel (step >= 4; every step with MCPT_DENOISE_NAIVE=1): every tap from
//        global memory — a wave is 64 pixels of one row, so each tap is one contiguous 1 KB read
//        per word; the taps of step >= 4 are sparse (a halo tile would be mostly unused) and
//        neighbouring rows' re-reads are served by L2.
//    Each has a noise-guided form (GUIDED, mcpt_denoise_guided): the colour term's
//    kc is not the launch's constant but a value of the centre pixel, from one extra 4-byte load
//    of its standard error (the error map of mcpt_convergence); the taps and atrous_pixel are the
//    same.  The variance-propagating form (kAtrousVariance, mcpt_denoise_variance)
//    carries each pixel's variance in the colour word's .w, which the tiles stage already: kc comes
//    from the centre's .w, the taps' .w are filtered with the squared weights, no error-map load.
//  * variance_init_kernel: that form's first input, the averaging (or the resolve) and the 3x3
//    key-aware prefilter of se^2 in one pass.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "mcpt_device.h"

namespace mcpt {

template <bool MESH>
__global__ __launch_bounds__(256) void guide_kernel(GuideParams g) {
  const RenderParams& p = g.r;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  // 32x8 tiles of four 8x8 waves side by side (kTileW x kTileH)
  const int tiles_x = (p.W + kTileW - 1) / kTileW;
  const int tile = blockIdx.x;
  const int x = (tile % tiles_x) * kTileW + wave * 8 + (lane & 7);
  const int lr = (tile / tiles_x) * kTileH + (lane >> 3);
  if (x >= p.W || lr >= p.n_local_rows) return;   // partial tiles (right / top edge)
  const int y = p.rows[lr];
  SceneT<MESH> s{p.nodes, p.leaves, p.ptype, p.prims, p.depth, p.minfo, p.mpairs, p.mleaftris, p.mtris,
                 p.mverts, p.mnorms, p.flat_face};
  Ev<false> ev;
  const float u = ((float)x + 0.5f) / (float)p.W;
  const float v = ((float)y + 0.5f) / (float)p.H;
  const f3 O = mk(p.ox, p.oy, p.oz), D = camera_dir(p, u, v);
  Hit h;
  h.pl = mk(0.0f, 0.0f, 0.0f); h.cull2 = 0.0; h.tri = 0;
  traverse_lane<false, false>(s, O, D, h, ev);
  f3 N = mk(0.0f, 0.0f, 0.0f), P = N;
  float4 col = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  if (h.hit()) {
    geom_info<false>(s, h, N, P, ev);
    col = s.prims[(size_t)h.index() * 8 + 6];
  }
  const size_t px = (size_t)lr * p.W + x;   // < n_local_px (mcpt_set_target*)
  g.guide[2 * px] = make_float4(N.x, N.y, N.z, __int_as_float(hit_key(h)));
  g.guide[2 * px + 1] = make_float4(P.x, P.y, P.z, h.hit() ? h.dist : kFLTMAX);
  g.albedo[px] = col;
}

// accum / pass_count per channel (mcpt_average's single division), padded to 16 bytes
__global__ __launch_bounds__(256) void average4_kernel(const float* __restrict__ accum, float4* __restrict__ out,
                                                       long long n_px, float nb) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n_px) return;
  out[i] = make_float4(accum[3 * i] / nb, accum[3 * i + 1] / nb, accum[3 * i + 2] / nb, 0.0f);
}

// The filter's weights h = {1/16, 1/4, 3/8, 1/4, 1/16} (their products are exact in binary32).
__host__ __device__ constexpr float atrous_h(int i) {
  return i == 2 ? 0.375f : ((i == 1 || i == 3) ? 0.25f : 0.0625f);
}

// One output pixel (x, y) of one iteration (these operations, in this order).
// fetch(qx, qy, c, g0, g1) loads the three words of the in-frame pixel (qx, qy).
// VAR (the variance-propagating form): kc is k_color^2 and the colour term's factor
// comes from the centre's carried variance cp.w; the taps' .w are summed with the squared weights.
template <bool VAR, class Fetch>
__device__ __forceinline__ float4 atrous_pixel(int x, int y, int W, int H, int step, float kc, float kp, float4 cp,
                                               float4 g0p, float4 g1p, Fetch fetch) {
  const int key_p = __float_as_int(g0p.w);
  constexpr float h22 = atrous_h(2) * atrous_h(2);
  float sx = h22 * cp.x, sy = h22 * cp.y, sz = h22 * cp.z, wsum = h22;
  float vs = 0.0f;
  if constexpr (VAR) {
    vs = (h22 * h22) * cp.w;
    kc = rcp_rn(kc * cp.w + 0x1p-40f);
  }
#pragma unroll
  for (int dy = -2; dy <= 2; ++dy) {
#pragma unroll
    for (int dx = -2; dx <= 2; ++dx) {
      if (dx == 0 && dy == 0) continue;
      const int qx = x + step * dx, qy = y + step * dy;
      if (qx < 0 || qx >= W || qy < 0 || qy >= H) continue;   // no clamping, no wrap
      float4 cq, g0q, g1q;
      fetch(qx, qy, cq, g0q, g1q);
      if (__float_as_int(g0q.w) != key_p) continue;
      const float dcx = cq.x - cp.x, dcy = cq.y - cp.y, dcz = cq.z - cp.z;
      const float a_c = ((dcx * dcx + dcy * dcy) + dcz * dcz) * kc;
      const float dPx = g1q.x - g1p.x, dPy = g1q.y - g1p.y, dPz = g1q.z - g1p.z;
      const float t = (g0p.x * dPx + g0p.y * dPy) + g0p.z * dPz;
      const float a_p = (t * t) * kp;
      float wn = 1.0f;
      if (key_p >= 0) {
        const float d = (g0p.x * g0q.x + g0p.y * g0q.y) + g0p.z * g0q.z;
        float nd = gmax(0.0f, d);
        nd = nd * nd; nd = nd * nd; nd = nd * nd; nd = nd * nd; nd = nd * nd;   // nd^32
        wn = nd;
      }
      const float r = rcp_rn(1.0f + (a_c + a_p));
      const float w = (((atrous_h(dy + 2) * atrous_h(dx + 2)) * wn) * r) * r;
      sx += w * cq.x; sy += w * cq.y; sz += w * cq.z;
      wsum += w;
      if constexpr (VAR) vs += (w * w) * cq.w;
    }
  }
  if constexpr (VAR) return make_float4(sx / wsum, sy / wsum, sz / wsum, vs / (wsum * wsum));
  return make_float4(sx / wsum, sy / wsum, sz / wsum, 0.0f);
}

// The colour term's source: the launch's constant, the error map (GUIDED), the carried variance.
enum { kAtrousFixed = 0, kAtrousGuided = 1, kAtrousVariance = 2 };

// kc of the centre pixel px.  Fixed sigma: the launch's kc.  GUIDED: kc carries k_color * 2^-s
// (formed on the host, exact) and the pixel's width is that times its standard error.  Variance:
// the launch's k_color^2, which atrous_pixel scales by the centre's own variance.
template <int MODE>
__device__ __forceinline__ float atrous_kc(float kc, const float2* __restrict__ emap, size_t px) {
  if constexpr (MODE != kAtrousGuided) return kc;
  const float sg = kc * emap[px].x;
  return rcp_rn(sg * sg + 0x1p-40f);
}

constexpr int kAtrousTile = 16;   // LDS kernels: 16x16 pixels (2x2 waves of 8x8) + the halo

template <int STEP, int MODE>
__global__ __launch_bounds__(256) void atrous_lds_kernel(const float4* __restrict__ src, float4* __restrict__ dst,
                                                         const float4* __restrict__ guide, int W, int H, float kc,
                                                         float kp, const float2* __restrict__ emap) {
  constexpr int R = 2 * STEP, TW = kAtrousTile + 2 * R, TH = kAtrousTile + 2 * R;
  __shared__ float4 s_c[TH * TW], s_g0[TH * TW], s_g1[TH * TW];
  const int tid = threadIdx.x;
  const int tx0 = blockIdx.x * kAtrousTile, ty0 = blockIdx.y * kAtrousTile;
  // stage the tile and its halo; cells outside the frame stay unwritten and are never read
  // (atrous_pixel tests the frame before it fetches)
  for (int i = tid; i < TH * TW; i += 256) {
    const int ly = i / TW, lx = i - ly * TW;
    const int gx = tx0 - R + lx, gy = ty0 - R + ly;
    if (gx >= 0 && gx < W && gy >= 0 && gy < H) {
      const size_t q = (size_t)gy * W + gx;
      s_c[i] = src[q];
      s_g0[i] = guide[2 * q];
      s_g1[i] = guide[2 * q + 1];
    }
  }
  __syncthreads();
  const int lane = tid & 63, wave = tid >> 6;
  const int lx = (wave & 1) * 8 + (lane & 7), ly = (wave >> 1) * 8 + (lane >> 3);
  const int x = tx0 + lx, y = ty0 + ly;
  if (x >= W || y >= H) return;
  const int ci = (ly + R) * TW + (lx + R);
  auto fetch = [&](int qx, int qy, float4& c, float4& g0, float4& g1) {
    const int i = (qy - ty0 + R) * TW + (qx - tx0 + R);   // |q - p| <= R per axis: inside the staged tile
    c = s_c[i]; g0 = s_g0[i]; g1 = s_g1[i];
  };
  const size_t px = (size_t)y * W + x;
  dst[px] = atrous_pixel<MODE == kAtrousVariance>(x, y, W, H, STEP, atrous_kc<MODE>(kc, emap, px), kp, s_c[ci],
                                                  s_g0[ci], s_g1[ci], fetch);
}

// 64x4 pixels per workgroup, a wave = 64 pixels of one row
template <int MODE>
__global__ __launch_bounds__(256) void atrous_global_kernel(const float4* __restrict__ src, float4* __restrict__ dst,
                                                            const float4* __restrict__ guide, int W, int H, int step,
                                                            float kc, float kp, const float2* __restrict__ emap) {
  const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
  if (x >= W || y >= H) return;
  auto fetch = [&](int qx, int qy, float4& c, float4& g0, float4& g1) {
    const size_t q = (size_t)qy * W + qx;
    c = src[q]; g0 = guide[2 * q]; g1 = guide[2 * q + 1];
  };
  const size_t px = (size_t)y * W + x;
  dst[px] = atrous_pixel<MODE == kAtrousVariance>(x, y, W, H, step, atrous_kc<MODE>(kc, emap, px), kp, src[px],
                                                  guide[2 * px], guide[2 * px + 1], fetch);
}

// The variance filter's first input: {accum / n, v0} with n the pass count
// (RESOLVED: the pixel's own count, resolve4_kernel's division) and v0 the 3x3 prefilter of the
// error map's se^2 over the neighbours of the centre's key, weights {1/4, 1/2, 1/4}^2, dy outer.
// 64x4 pixels per workgroup as atrous_global_kernel; 9 taps of 4 + 4 bytes from global memory, once.
constexpr float kVarianceMax = 0x1p60f;
__host__ __device__ constexpr float variance_g(int i) { return i == 1 ? 0.5f : 0.25f; }

template <bool RESOLVED>
__global__ __launch_bounds__(256) void variance_init_kernel(CountSource cnt, const float* __restrict__ accum,
                                                            float4* __restrict__ out,
                                                            const float4* __restrict__ guide,
                                                            const float2* __restrict__ emap, int W, int H, float nb) {
  const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
  if (x >= W || y >= H) return;
  const size_t px = (size_t)y * W + x;
  if constexpr (RESOLVED) nb = (float)count_at(cnt, (long long)px);
  const int key_p = __float_as_int(guide[2 * px].w);
  float sv = 0.0f, sg = 0.0f;
#pragma unroll
  for (int dy = -1; dy <= 1; ++dy) {
#pragma unroll
    for (int dx = -1; dx <= 1; ++dx) {
      const int qx = x + dx, qy = y + dy;
      if (qx < 0 || qx >= W || qy < 0 || qy >= H) continue;
      const size_t q = (size_t)qy * W + qx;
      if (__float_as_int(guide[2 * q].w) != key_p) continue;
      const float se = emap[q].x, t = se * se;
      const float vraw = t < kVarianceMax ? t : kVarianceMax;   // NaN and +inf: kVarianceMax
      const float gw = variance_g(dy + 1) * variance_g(dx + 1);
      sv += gw * vraw;
      sg += gw;
    }
  }
  out[px] = make_float4(accum[3 * px] / nb, accum[3 * px + 1] / nb, accum[3 * px + 2] / nb, sv / sg);
}

}  // namespace mcpt

hipError_t mcpt_launch_guides(const mcpt::GuideParams& g, hipStream_t stream) {
  const mcpt::RenderParams& p = g.r;
  if (p.n_local_px <= 0) return hipSuccess;
  const unsigned tiles = (unsigned)(((p.W + mcpt::kTileW - 1) / mcpt::kTileW) *
                                    ((p.n_local_rows + mcpt::kTileH - 1) / mcpt::kTileH));
  if (p.n_meshes > 0) hipLaunchKernelGGL((mcpt::guide_kernel<true>), dim3(tiles), dim3(256), 0, stream, g);
  else hipLaunchKernelGGL((mcpt::guide_kernel<false>), dim3(tiles), dim3(256), 0, stream, g);
  return hipGetLastError();
}

hipError_t mcpt_launch_average4(const float* accum, float4* out, long long n_px, int pass_count, hipStream_t stream) {
  if (n_px <= 0) return hipSuccess;
  hipLaunchKernelGGL(mcpt::average4_kernel, dim3((unsigned)((n_px + 255) / 256)), dim3(256), 0, stream, accum, out,
                     n_px, (float)pass_count);
  return hipGetLastError();
}

template <int MODE>
static void launch_atrous(const float4* src, float4* dst, const float4* guide, int W, int H, int step, float kc,
                          float kp, const float2* emap, bool naive, hipStream_t stream) {
  constexpr int T = mcpt::kAtrousTile;
  const dim3 tiles((unsigned)((W + T - 1) / T), (unsigned)((H + T - 1) / T));
  if (!naive && step == 1)
    hipLaunchKernelGGL((mcpt::atrous_lds_kernel<1, MODE>), tiles, dim3(256), 0, stream, src, dst, guide, W, H, kc, kp,
                       emap);
  else if (!naive && step == 2)
    hipLaunchKernelGGL((mcpt::atrous_lds_kernel<2, MODE>), tiles, dim3(256), 0, stream, src, dst, guide, W, H, kc, kp,
                       emap);
  else
    hipLaunchKernelGGL((mcpt::atrous_global_kernel<MODE>), dim3((unsigned)((W + 63) / 64), (unsigned)((H + 3) / 4)),
                       dim3(256), 0, stream, src, dst, guide, W, H, step, kc, kp, emap);
}

hipError_t mcpt_launch_atrous(const float4* src, float4* dst, const float4* guide, int W, int H, int step, float kc,
                              float kp, const float2* emap, bool naive, hipStream_t stream) {
  if (emap) launch_atrous<mcpt::kAtrousGuided>(src, dst, guide, W, H, step, kc, kp, emap, naive, stream);
  else launch_atrous<mcpt::kAtrousFixed>(src, dst, guide, W, H, step, kc, kp, nullptr, naive, stream);
  return hipGetLastError();
}

hipError_t mcpt_launch_atrous_variance(const float4* src, float4* dst, const float4* guide, int W, int H, int step,
                                       float kk, float kp, bool naive, hipStream_t stream) {
  launch_atrous<mcpt::kAtrousVariance>(src, dst, guide, W, H, step, kk, kp, nullptr, naive, stream);
  return hipGetLastError();
}

hipError_t mcpt_launch_variance_init(const mcpt::CountSource* counts, const float* accum, float4* out,
                                     const float4* guide, const float2* emap, int W, int H, int pass_count,
                                     hipStream_t stream) {
  if (W <= 0 || H <= 0) return hipSuccess;
  const dim3 grid((unsigned)((W + 63) / 64), (unsigned)((H + 3) / 4));
  if (counts)
    hipLaunchKernelGGL((mcpt::variance_init_kernel<true>), grid, dim3(256), 0, stream, *counts, accum, out, guide, emap,
                       W, H, 0.0f);
  else
    hipLaunchKernelGGL((mcpt::variance_init_kernel<false>), grid, dim3(256), 0, stream, mcpt::CountSource{}, accum, out,
                       guide, emap, W, H, (float)pass_count);
  return hipGetLastError();
}
