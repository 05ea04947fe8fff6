// mcpt_temporal.hip — temporal reprojection of a moving-camera render (no
// reference equivalent: the reference restarts its pass loop at every camera move).
//
//  * temporal_kernel: one lane per pixel of the current frame, 64x4 pixels per workgroup (a wave =
//    64 pixels of one row, as atrous_global_kernel), the workgroups stepping over the frame's tiles.
//    The pixel's own words (both guide words 16 bytes each, the accumulator's three floats, the error
//    map's se), its world position through the previous camera's P·V, then the 2x2 history taps around
//    the reprojected position from global memory: a wave's taps fall into a few rows' worth of lines
//    of the previous frame and L2 serves the overlap (no LDS tile: the footprint of a reprojected
//    wave is no fixed rectangle).  A tap counts when it shows the same primitive, lies in the
//    pixel's tangent plane and faces the same way.  The history is read from one set of buffers and
//    written to the other (no lane overwrites what another still reads); GUIDES: the kernel also
//    writes the current guides into the new history (the ping-pong form), else the host copies
//    them behind the kernel.
//    The record (integer sums and a maximum: the bits do not depend on the reduction's order) is
//    reduced as error_kernel's: wave shuffles, one LDS step, one set of atomics per workgroup into
//    slot blockIdx.x % kStatsRecSlots.
//  * temporal_init_kernel: the variance filter's first input from the temporal image, {rgb, the
//    3x3 key-aware prefilter of its variance}: variance_init_kernel's taps, weights and order.
// All of it binary32 without contraction: + - * /, comparisons, rcp_rn, an exact floor.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "mcpt_internal.h"
#include "mcpt_math.h"
#include "mcpt_stats_err.h"

namespace mcpt {

constexpr float kTemporalVarianceMax = 0x1p60f;   // variance_init_kernel's clamp (kVarianceMax)
constexpr int kTemporalMaxBlocks = 2048;          // as kErrorMaxBlocks: the record's atomics stay few
enum { kTpHistory = 0, kTpMiss = 1, kTpOffscreen = 2, kTpRejected = 3 };

// rec: kStatsRecSlots partial records of kStatsRecStride words: [0] n_history, [1] n_miss,
// [2] n_offscreen, [3] n_rejected, [4] sum_len (64-bit adds), [5] max_len (a 32-bit max on the
// word's low half).  Every lane of the workgroup calls it; idle lanes hold zeros.
__device__ __forceinline__ void reduce_temporal_record(unsigned cnt[4], unsigned long long len_sum, unsigned len_max,
                                                       unsigned long long* __restrict__ rec) {
  __shared__ unsigned s_cnt[4][4], s_max[4];
  __shared__ unsigned long long s_len[4];
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
#pragma unroll
    for (int k = 0; k < 4; ++k) cnt[k] += __shfl_down(cnt[k], off, 64);
    len_sum += __shfl_down(len_sum, off, 64);
    const unsigned o = __shfl_down(len_max, off, 64);
    len_max = o > len_max ? o : len_max;
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < 4; ++k) s_cnt[wave][k] = cnt[k];
    s_len[wave] = len_sum;
    s_max[wave] = len_max;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned long long* slot = rec + (size_t)(blockIdx.x % kStatsRecSlots) * kStatsRecStride;
    unsigned long long l = 0;
    unsigned m = 0;
    for (int w = 0; w < 4; ++w) {
      l += s_len[w];
      m = s_max[w] > m ? s_max[w] : m;
    }
    for (int k = 0; k < 4; ++k) {
      const unsigned long long a = (unsigned long long)s_cnt[0][k] + s_cnt[1][k] + s_cnt[2][k] + s_cnt[3][k];
      if (a) atomicAdd(slot + k, a);
    }
    if (l) atomicAdd(slot + 4, l);
    if (m) atomicMax(reinterpret_cast<unsigned*>(slot + 5), m);
  }
}

// One pixel of an accumulate: the current {c, v} from the accumulator's sums over nb
// samples and the map's se, the look-up through the previous camera, the 2x2 taps' tests, the blend
// and the pixel's class.  Reads the history's *_in set, writes nothing: temporal_kernel stores what it
// returns, temporal_select_kernel (§3.10.1) only looks at it.  px < W x H.
struct TemporalPixel {
  float4 out;   // {rgb, variance of the mean} the history would hold
  int len, cls;
};
__device__ __forceinline__ TemporalPixel temporal_pixel(const TemporalParams& p, size_t px, const float4 g0,
                                                        const float4 g1, float nb) {
  const float Wf = (float)p.W, Hf = (float)p.H;
  const int key_p = __float_as_int(g0.w);
  const float cr = p.accum[3 * px] / nb, cg = p.accum[3 * px + 1] / nb, cb = p.accum[3 * px + 2] / nb;
  const float se = p.emap[px].x, t2 = se * se;
  const float v = t2 < kTemporalVarianceMax ? t2 : kTemporalVarianceMax;   // NaN and +inf: the clamp
  TemporalPixel r;
  r.out = make_float4(cr, cg, cb, v);
  r.len = 1;
  r.cls = kTpMiss;
  if (!p.empty && key_p >= 0) {
    r.cls = kTpOffscreen;
    const float* M = p.M;
    const float w = ((M[3] * g1.x + M[7] * g1.y) + M[11] * g1.z) + M[15];
    const float cx = ((M[0] * g1.x + M[4] * g1.y) + M[8] * g1.z) + M[12];
    const float cy = ((M[1] * g1.x + M[5] * g1.y) + M[9] * g1.z) + M[13];
    if (0.0f < w) {
      const float iw = rcp_rn(w);
      const float sx = ((cx * iw) * 0.5f + 0.5f) * Wf - 0.5f;
      const float sy = ((cy * iw) * 0.5f + 0.5f) * Hf - 0.5f;
      if (-1.0f < sx && sx < Wf && -1.0f < sy && sy < Hf) {   // (a NaN fails)
        r.cls = kTpRejected;
        const float flx = floorf(sx), fly = floorf(sy);
        const int x0 = (int)flx, y0 = (int)fly;               // in [-1, W - 1], [-1, H - 1]
        const float fx = sx - flx, fy = sy - fly;
        const float tol = p.plane_tol * g1.w, tol2 = tol * tol;
        float bs = 0.0f, s0 = 0.0f, s1 = 0.0f, s2 = 0.0f, s3 = 0.0f;
        int lmin = 65535;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
#pragma unroll
          for (int i = 0; i < 2; ++i) {
            const int qx = x0 + i, qy = y0 + j;
            if (qx < 0 || qx >= p.W || qy < 0 || qy >= p.H) continue;
            const size_t q = (size_t)qy * p.W + qx;
            const float4 h0 = p.hg_in[2 * q];
            if (__float_as_int(h0.w) != key_p) continue;
            const float4 h1 = p.hg_in[2 * q + 1];
            const float dPx = h1.x - g1.x, dPy = h1.y - g1.y, dPz = h1.z - g1.z;
            const float t = (g0.x * dPx + g0.y * dPy) + g0.z * dPz;
            if (!(t * t <= tol2)) continue;
            const float nd = (g0.x * h0.x + g0.y * h0.y) + g0.z * h0.z;
            if (!(0.875f <= nd)) continue;
            const float b = (i ? fx : 1.0f - fx) * (j ? fy : 1.0f - fy);
            const float4 hc = p.hc_in[q];
            s0 += b * hc.x; s1 += b * hc.y; s2 += b * hc.z; s3 += b * hc.w;
            bs += b;
            const int hl = p.hl_in[q];
            lmin = hl < lmin ? hl : lmin;
          }
        }
        if (0.0f < bs) {
          r.cls = kTpHistory;
          const float h0 = s0 / bs, h1 = s1 / bs, h2 = s2 / bs, h3 = s3 / bs;
          r.len = lmin + 1 < p.max_history ? lmin + 1 : p.max_history;
          const float a = 1.0f / (float)r.len, k = 1.0f - a;
          r.out = make_float4(k * h0 + a * cr, k * h1 + a * cg, k * h2 + a * cb, (k * k) * h3 + (a * a) * v);
        }
      }
    }
  } else if (key_p >= 0) {
    r.cls = kTpRejected;   // an empty history holds no tap
  }
  return r;
}

// COUNTED: mcpt_temporal_accumulate_resolved's form, every pixel's sums divided by its own sample
// count (p.counts, count_at); else by the pass count p.nb
template <bool GUIDES, bool COUNTED>
__global__ __launch_bounds__(256) void temporal_kernel(TemporalParams p) {
  const int tiles_x = (p.W + 63) / 64, n_tiles = tiles_x * ((p.H + 3) / 4);
  // a lane's share of the record over its tiles (a lane sees at most 2^31 / (2048 x 256) pixels, each
  // of length <= 65535: the length sum is 64-bit from the start)
  unsigned cnt[4] = {0, 0, 0, 0};
  unsigned long long len_sum = 0;
  unsigned len_max = 0;
  for (int tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const int x = (tile % tiles_x) * 64 + (threadIdx.x & 63), y = (tile / tiles_x) * 4 + (threadIdx.x >> 6);
    if (x >= p.W || y >= p.H) continue;
    const size_t px = (size_t)y * p.W + x;   // < W x H, the length of every per-pixel array here
    const float4 g0 = p.guide[2 * px], g1 = p.guide[2 * px + 1];   // {N, key} {P, dist}
    const float nb = COUNTED ? (float)count_at(p.counts, (long long)px) : p.nb;
    const TemporalPixel r = temporal_pixel(p, px, g0, g1, nb);
    p.hc_out[px] = r.out;
    p.hl_out[px] = r.len;
    if constexpr (GUIDES) {
      p.hg_out[2 * px] = g0;
      p.hg_out[2 * px + 1] = g1;
    }
    cnt[r.cls] += 1u;
    len_sum += (unsigned)r.len;
    len_max = (unsigned)r.len > len_max ? (unsigned)r.len : len_max;
  }
  reduce_temporal_record(cnt, len_sum, len_max, p.rec);
}

// mcpt_adaptive_select_temporal's step T: select_kernel's geometry, one wave per
// 8x8 block of a full frame in row order, the grid capped and stepped the same way.  For every in-frame
// pixel of a block that is active on entry: `out` = what the resolved accumulate would write for it now
// (temporal_pixel on the history's current set, the map step A just wrote, the pixel's own count), then
// in binary32 without contraction, in the order written (filtered_select_kernel's arithmetic)
//   Yt = (0.2126 out.r + 0.7152 out.g) + 0.0722 out.b;  rt = sqrt_rn(out.v) / (max(0, Yt) + mu_floor);
//   rt = 64 if Yt is not finite or not rt <= 64.
// The block stays active iff its largest rt > threshold or it holds fewer than min_passes passes;
// retired blocks are not computed.  Only the flags and the record are written.  rec: select_kernel's
// partial records, [0] n_above_t, [1] sum_qt, [2] max_rt's bits, [3] n_px_t, [4] active blocks,
// [5] n_history.
__global__ __launch_bounds__(256) void temporal_select_kernel(AdaptiveTarget t, TemporalParams p, float mu_floor,
                                                              float threshold, int min_passes,
                                                              unsigned long long* __restrict__ rec) {
  __shared__ unsigned long long s_sum[4][5];   // per wave: n_above_t, sum_qt, n_px_t, active blocks, n_history
  __shared__ unsigned s_max[4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  unsigned long long above = 0, qsum = 0, n_hist = 0;   // this lane's pixels
  unsigned tmax = 0;
  unsigned long long n_px = 0, n_act = 0;   // this wave's blocks (lane 0 counts)
  for (long long blk = (long long)blockIdx.x * 4 + wave; blk < t.n_blocks; blk += (long long)gridDim.x * 4) {
    if (t.flags[blk] == 0) continue;   // (wave-uniform)
    const int bx = (int)(blk % t.blocks_x), by = (int)(blk / t.blocks_x);
    const int x = bx * 8 + (lane & 7), y = by * 8 + (lane >> 3);
    const bool in = x < p.W && y < p.H;
    const int passes = t.passes[blk];
    float rt = 0.0f;
    if (in) {
      const size_t px = (size_t)y * p.W + x;   // < W x H
      const float nb = (float)count_at(p.counts, (long long)px);
      const TemporalPixel r = temporal_pixel(p, px, p.guide[2 * px], p.guide[2 * px + 1], nb);
      const float yt = (0.2126f * r.out.x + 0.7152f * r.out.y) + 0.0722f * r.out.z;
      rt = sqrt_rn(r.out.w) / (gmax(0.0f, yt) + mu_floor);
      if (!finite32(yt) || !(rt <= 64.0f)) rt = 64.0f;
      above += (rt > threshold) ? 1u : 0u;
      qsum += error_q(rt);
      n_hist += r.cls == kTpHistory ? 1u : 0u;
    }
    unsigned bt = __float_as_uint(rt);   // rt >= 0: the bits order as the values (idle lanes: 0)
    tmax = bt > tmax ? bt : tmax;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      const unsigned o = __shfl_xor(bt, off, 64);
      bt = o > bt ? o : bt;
    }
    const bool stay = __uint_as_float(bt) > threshold || passes < min_passes;
    const unsigned n_in = (unsigned)__popcll(__ballot(in));
    if (lane == 0) {
      t.flags[blk] = stay ? 1 : 0;
      n_px += n_in;
      n_act += stay ? 1u : 0u;
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    above += __shfl_down(above, off, 64);
    qsum += __shfl_down(qsum, off, 64);
    n_hist += __shfl_down(n_hist, off, 64);
    const unsigned o = __shfl_down(tmax, off, 64);
    tmax = o > tmax ? o : tmax;
  }
  if (lane == 0) {
    s_sum[wave][0] = above; s_sum[wave][1] = qsum; s_sum[wave][2] = n_px; s_sum[wave][3] = n_act;
    s_sum[wave][4] = n_hist;
    s_max[wave] = tmax;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned long long v[5] = {0, 0, 0, 0, 0};
    unsigned m = 0;
    for (int w = 0; w < 4; ++w) {
      for (int k = 0; k < 5; ++k) v[k] += s_sum[w][k];
      m = s_max[w] > m ? s_max[w] : m;
    }
    unsigned long long* slot = rec + (size_t)(blockIdx.x % kStatsRecSlots) * kStatsRecStride;
    if (v[0]) atomicAdd(slot + 0, v[0]);
    if (v[1]) atomicAdd(slot + 1, v[1]);
    if (m) atomicMax(reinterpret_cast<unsigned*>(slot + 2), m);
    if (v[2]) atomicAdd(slot + 3, v[2]);
    if (v[3]) atomicAdd(slot + 4, v[3]);
    if (v[4]) atomicAdd(slot + 5, v[4]);
  }
}

__host__ __device__ constexpr float temporal_g(int i) { return i == 1 ? 0.5f : 0.25f; }   // variance_g

__global__ __launch_bounds__(256) void temporal_init_kernel(const float4* __restrict__ hc, float4* __restrict__ out,
                                                            const float4* __restrict__ guide, int W, int H) {
  const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
  if (x >= W || y >= H) return;
  const size_t px = (size_t)y * W + x;
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
      const float gw = temporal_g(dy + 1) * temporal_g(dx + 1);
      sv += gw * hc[q].w;
      sg += gw;
    }
  }
  const float4 c = hc[px];
  out[px] = make_float4(c.x, c.y, c.z, sv / sg);
}

}  // namespace mcpt

hipError_t mcpt_launch_temporal(const mcpt::TemporalParams& p, bool counted, hipStream_t stream) {
  if (p.W <= 0 || p.H <= 0) return hipSuccess;
  const long long tiles = (long long)((p.W + 63) / 64) * ((p.H + 3) / 4);
  const dim3 grid((unsigned)std::min<long long>(tiles, mcpt::kTemporalMaxBlocks));
  if (p.hg_out && counted) hipLaunchKernelGGL((mcpt::temporal_kernel<true, true>), grid, dim3(256), 0, stream, p);
  else if (p.hg_out) hipLaunchKernelGGL((mcpt::temporal_kernel<true, false>), grid, dim3(256), 0, stream, p);
  else if (counted) hipLaunchKernelGGL((mcpt::temporal_kernel<false, true>), grid, dim3(256), 0, stream, p);
  else hipLaunchKernelGGL((mcpt::temporal_kernel<false, false>), grid, dim3(256), 0, stream, p);
  return hipGetLastError();
}

hipError_t mcpt_launch_temporal_select(const mcpt::AdaptiveTarget& t, const mcpt::TemporalParams& p, float mu_floor,
                                       float threshold, int min_passes, unsigned long long* rec, hipStream_t stream) {
  hipError_t e = hipMemsetAsync(rec, 0, sizeof(unsigned long long) * mcpt::kStatsRecWords, stream);
  if (e != hipSuccess || t.n_blocks <= 0 || p.W <= 0 || p.H <= 0) return e;
  // select_kernel's grid: a workgroup of four waves per four blocks, capped
  const dim3 grid((unsigned)std::min<long long>(((long long)t.n_blocks + 3) / 4, mcpt::kTemporalMaxBlocks));
  hipLaunchKernelGGL(mcpt::temporal_select_kernel, grid, dim3(256), 0, stream, t, p, mu_floor, threshold, min_passes,
                     rec);
  return hipGetLastError();
}

hipError_t mcpt_launch_temporal_init(const float4* hc, float4* out, const float4* guide, int W, int H,
                                     hipStream_t stream) {
  if (W <= 0 || H <= 0) return hipSuccess;
  hipLaunchKernelGGL(mcpt::temporal_init_kernel, dim3((unsigned)((W + 63) / 64), (unsigned)((H + 3) / 4)), dim3(256), 0,
                     stream, hc, out, guide, W, H);
  return hipGetLastError();
}
