// mcpt_stats.hip — per-pixel noise statistics of a progressive render and its convergence
// metric (no reference equivalent: the reference accumulates and averages).
//
// The statistics are batch means over render calls: nothing here touches a render launch, the
// kernels read the accumulator between calls on the context's stream.
//  * stats_begin_kernel / stats_update_kernel: one lane per pixel; the pixel's state is one
//    16-byte word {Yacc, S2, Ybase, 0}.  Traffic of an update: 12 B of accumulator and 16 B of
//    state read, 16 B written.
//  * error_kernel: one lane per pixel and grid step; {se, r} per pixel and the frame record
//    (n_above, sum_q, max_r).  The record's sums are integers (q = trunc(r * 2^16), r <= 64) and
//    max_r is reduced as the bit pattern of a non-negative float, so the order of the wave
//    shuffles, the LDS step and the atomics does not show in the bits.  One set of atomics per
//    workgroup; the grid is capped (kErrorMaxBlocks: a 4K frame issues ~6,000 atomics, not
//    ~100,000) and the workgroups spread them over kStatsRecSlots partial records, one 128-byte
//    line each, which the host adds (1080p: 18 us; with every workgroup's atomics on one record
//    86 us: profiles/stats_bench.json, profiles/stats_bench_one_record.json).
// All of it binary32 without contraction: + - * /, comparisons, sqrt_rn.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "mcpt_internal.h"
#include "mcpt_math.h"
#include "mcpt_stats_err.h"

namespace mcpt {

// luminance of an accumulator pixel (the sums, not the averages)
__device__ __forceinline__ float accum_luminance(const float* __restrict__ accum, long long i) {
  return (0.2126f * accum[3 * i] + 0.7152f * accum[3 * i + 1]) + 0.0722f * accum[3 * i + 2];
}

__global__ __launch_bounds__(256) void stats_begin_kernel(const float* __restrict__ accum, float4* __restrict__ st,
                                                          long long n_px) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n_px) return;
  const float y = accum_luminance(accum, i);
  st[i] = make_float4(y, 0.0f, y, 0.0f);
}

// "the accumulator now holds n more passes than at the previous batch" (nf = (float)n)
__global__ __launch_bounds__(256) void stats_update_kernel(const float* __restrict__ accum, float4* __restrict__ st,
                                                           long long n_px, float nf) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n_px) return;
  float4 s = st[i];
  const float ynow = accum_luminance(accum, i);
  const float d = ynow - s.x;
  s.y = s.y + (d * d) / nf;
  s.x = ynow;
  st[i] = s;
}

// stats_update_kernel's twin of a queued adaptive run: no pixel changes once the
// active list is empty (count[0] == 0: the host loop stops there, and an update it never made would
// turn an overflowed pixel's inf - inf into a NaN in S2); else the same update of every pixel
__global__ __launch_bounds__(256) void stats_update_counted_kernel(const float* __restrict__ accum,
                                                                   float4* __restrict__ st, long long n_px, float nf,
                                                                   const int* __restrict__ count) {
  if (count[0] <= 0) return;
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n_px) return;
  float4 s = st[i];
  const float ynow = accum_luminance(accum, i);
  const float d = ynow - s.x;
  s.y = s.y + (d * d) / nf;
  s.x = ynow;
  st[i] = s;
}

constexpr int kErrorMaxBlocks = 2048;   // 8 workgroups per CU of a 256-CU chip

// A workgroup's share of the frame record from its lanes' sums: wave shuffles, one LDS step, one
// set of atomics into slot blockIdx.x % kStatsRecSlots.  Idle lanes (past the frame's end) hold the
// sums' neutral elements and take part in the shuffles.  Every lane of the workgroup calls it.
__device__ __forceinline__ void reduce_record(unsigned long long above, unsigned long long qsum, unsigned rmax,
                                              unsigned long long* __restrict__ rec) {
  __shared__ unsigned long long s_above[4], s_q[4];
  __shared__ unsigned s_max[4];
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    above += __shfl_down(above, off, 64);
    qsum += __shfl_down(qsum, off, 64);
    const unsigned o = __shfl_down(rmax, off, 64);
    rmax = o > rmax ? o : rmax;
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) {
    s_above[wave] = above;
    s_q[wave] = qsum;
    s_max[wave] = rmax;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned long long a = 0, q = 0;
    unsigned m = 0;
    for (int w = 0; w < 4; ++w) {
      a += s_above[w];
      q += s_q[w];
      m = s_max[w] > m ? s_max[w] : m;
    }
    unsigned long long* slot = rec + (size_t)(blockIdx.x % kStatsRecSlots) * kStatsRecStride;
    if (a) atomicAdd(slot + 0, a);
    if (q) atomicAdd(slot + 1, q);
    if (m) atomicMax(reinterpret_cast<unsigned*>(slot + 2), m);
  }
}

// rec: kStatsRecSlots partial records of kStatsRecStride words, workgroup b adds into slot
// b % kStatsRecSlots: [0] n_above, [1] sum_q (64-bit adds), [2] max_r's bits (a 32-bit max on the
// word's low half)
__global__ __launch_bounds__(256) void error_kernel(const float4* __restrict__ st, float2* __restrict__ emap,
                                                    long long n_px, float nf, float bm1f, float mu_floor,
                                                    float threshold, unsigned long long* __restrict__ rec) {
  // a lane's sums over its grid steps (q <= 2^22 per pixel, up to 2^31 / (2048 x 256) pixels per
  // lane once the grid cap binds): 64-bit from the start
  unsigned long long above = 0, qsum = 0;
  unsigned rmax = 0;
  const long long stride = (long long)gridDim.x * 256;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n_px; i += stride) {
    const float2 e = pixel_error(st[i], nf, bm1f, mu_floor);   // {se, r} (mcpt_stats_err.h)
    const float r = e.y;
    emap[i] = e;
    above += (r > threshold) ? 1u : 0u;
    qsum += error_q(r);
    const unsigned rb = __float_as_uint(r);   // r >= 0: the bits order as the values
    rmax = rb > rmax ? rb : rmax;
  }
  reduce_record(above, qsum, rmax, rec);
}

// The frame record of a STORED error map (mcpt_error_map_record): error_kernel's
// reduction over the map's r values as they are (a gathered plane, or a window's own map); neither
// se nor r is recomputed, and the map is only read.  8 B per pixel of traffic.
__global__ __launch_bounds__(256) void error_map_record_kernel(const float2* __restrict__ emap, long long n_px,
                                                               float threshold, unsigned long long* __restrict__ rec) {
  unsigned long long above = 0, qsum = 0;
  unsigned rmax = 0;
  const long long stride = (long long)gridDim.x * 256;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n_px; i += stride) {
    const float r = emap[i].y;   // 0 <= r <= 64 as pixel_error wrote it
    above += (r > threshold) ? 1u : 0u;
    qsum += error_q(r);
    const unsigned rb = __float_as_uint(r);
    rmax = rb > rmax ? rb : rmax;
  }
  reduce_record(above, qsum, rmax, rec);
}

}  // namespace mcpt

hipError_t mcpt_launch_stats_begin(const float* accum, float4* state, long long n_px, hipStream_t stream) {
  if (n_px <= 0) return hipSuccess;
  hipLaunchKernelGGL(mcpt::stats_begin_kernel, dim3((unsigned)((n_px + 255) / 256)), dim3(256), 0, stream, accum,
                     state, n_px);
  return hipGetLastError();
}

hipError_t mcpt_launch_stats_update(const float* accum, float4* state, long long n_px, int n, hipStream_t stream) {
  if (n_px <= 0) return hipSuccess;
  hipLaunchKernelGGL(mcpt::stats_update_kernel, dim3((unsigned)((n_px + 255) / 256)), dim3(256), 0, stream, accum,
                     state, n_px, (float)n);
  return hipGetLastError();
}

hipError_t mcpt_launch_stats_update_counted(const float* accum, float4* state, long long n_px, int n, const int* count,
                                            hipStream_t stream) {
  if (n_px <= 0) return hipSuccess;
  hipLaunchKernelGGL(mcpt::stats_update_counted_kernel, dim3((unsigned)((n_px + 255) / 256)), dim3(256), 0, stream,
                     accum, state, n_px, (float)n, count);
  return hipGetLastError();
}

hipError_t mcpt_launch_stats_error(const float4* state, float2* emap, long long n_px, long long passes, int batches,
                                   float mu_floor, float threshold, unsigned long long* rec, hipStream_t stream) {
  hipError_t e = hipMemsetAsync(rec, 0, sizeof(unsigned long long) * mcpt::kStatsRecWords, stream);
  if (e != hipSuccess || n_px <= 0) return e;
  const long long blocks = (n_px + 255) / 256;
  hipLaunchKernelGGL(mcpt::error_kernel, dim3((unsigned)std::min<long long>(blocks, mcpt::kErrorMaxBlocks)), dim3(256),
                     0, stream, state, emap, n_px, (float)passes, (float)(batches - 1), mu_floor, threshold, rec);
  return hipGetLastError();
}

hipError_t mcpt_launch_error_map_record(const float2* emap, long long n_px, float threshold, unsigned long long* rec,
                                        hipStream_t stream) {
  hipError_t e = hipMemsetAsync(rec, 0, sizeof(unsigned long long) * mcpt::kStatsRecWords, stream);
  if (e != hipSuccess || n_px <= 0) return e;
  const long long blocks = (n_px + 255) / 256;
  hipLaunchKernelGGL(mcpt::error_map_record_kernel, dim3((unsigned)std::min<long long>(blocks, mcpt::kErrorMaxBlocks)),
                     dim3(256), 0, stream, emap, n_px, threshold, rec);
  return hipGetLastError();
}
