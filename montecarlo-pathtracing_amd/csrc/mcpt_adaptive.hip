// mcpt_adaptive.hip — adaptive sampling of 8x8 pixel blocks guided by the error map (DESIGN.md
// §3.9; no reference equivalent: the reference renders every pixel in every pass).
//
// A block is the render kernel's wave: 8 local rows x 8 columns of the local grid, id = by *
// blocks_x + bx.  While the mode is on a block holds an active flag and the passes rendered into it
// since mcpt_adaptive_begin; blocks only ever leave the active set.
//  * select_kernel: one wave per block (grid capped, waves step over the blocks).  An active block's
//    pixels get §3.8's {se, r} from the statistics state (pixel_error, mcpt_stats_err.h: the error
//    kernel's arithmetic) written to the error map; the block stays active iff its largest r exceeds
//    the threshold or it holds fewer than min_passes passes.  A retired block's pixels are not
//    computed: their stored map entries enter the frame record.  The record's sums are integers and
//    max_r a bit pattern, reduced per wave, per workgroup and into kStatsRecSlots partial records as
//    the error kernel's are: the bits do not depend on the order.
//  * select_kernel<false> and filtered_select_kernel: the select on the denoised frame's error
//    (mcpt_adaptive_select_filtered): the first writes the map and the raw record
//    and retires nobody, the variance filter runs on that map, the second reads the filter's
//    {rgb, variance} and applies the rule.
//  * compact_kernel: the active block ids, ascending, by a single-workgroup scan over the flags
//    (ballots inside a wave, the waves' counts through LDS, a running base): no atomic append, so
//    the list does not depend on timing.  4K has 129,600 blocks: 127 steps of 1,024.
//  * combine_list_kernel: one wave per listed block adds the block's segment sums to the
//    accumulator in chunk order (combine_kernel's sequence per pixel); unlisted pixels' segment
//    slots are unwritten and are not read.
//  * add_passes / counts / resolve: the per-block pass counts, the per-pixel sample counts from the
//    context's count source (count_at, mcpt_internal.h: the count plane, p0 + passes[block] or the
//    pass count), and accum / (float)count per channel (mcpt_average's single division).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "mcpt_internal.h"
#include "mcpt_math.h"
#include "mcpt_stats_err.h"

namespace mcpt {

constexpr int kSelectMaxBlocks = 2048;   // workgroups of four waves (the error kernel's grid cap)

__global__ __launch_bounds__(256) void adaptive_reset_kernel(AdaptiveTarget t, int* __restrict__ list,
                                                             int* __restrict__ count) {
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b == 0) count[0] = t.n_blocks;
  if (b >= t.n_blocks) return;
  t.flags[b] = 1;
  t.passes[b] = 0;
  list[b] = b;
}

// kRetire false: mcpt_adaptive_select_filtered's step A: the map and the record as
// above, every flag left as it is and word 4 (the active blocks) left to filtered_select_kernel
template <bool kRetire>
__global__ __launch_bounds__(256) void select_kernel(AdaptiveTarget t, const float4* __restrict__ st,
                                                     float2* __restrict__ emap, float nf, float bm1f, float mu_floor,
                                                     float threshold, int min_passes,
                                                     unsigned long long* __restrict__ rec) {
  __shared__ unsigned long long s_sum[4][4];   // per wave: n_above, sum_q, samples, active blocks
  __shared__ unsigned s_max[4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  unsigned long long above = 0, qsum = 0;   // this lane's pixels
  unsigned rmax = 0;
  unsigned long long samples = 0, n_act = 0;   // this wave's blocks (lane 0 counts)
  for (long long blk = (long long)blockIdx.x * 4 + wave; blk < t.n_blocks; blk += (long long)gridDim.x * 4) {
    const int bx = (int)(blk % t.blocks_x), by = (int)(blk / t.blocks_x);
    const int x = bx * 8 + (lane & 7), lr = by * 8 + (lane >> 3);
    const bool in = x < t.W && lr < t.n_local_rows;
    const long long i = (long long)lr * t.W + x;
    const bool act = t.flags[blk] != 0;   // (wave-uniform)
    const int passes = t.passes[blk];
    float r = 0.0f;
    if (in) {
      if (act) {
        const float2 e = pixel_error(st[i], nf, bm1f, mu_floor);
        emap[i] = e;
        r = e.y;
      } else {
        r = emap[i].y;   // as written when the block retired
      }
      above += (r > threshold) ? 1u : 0u;
      qsum += error_q(r);
    }
    unsigned bmax = __float_as_uint(r);   // r >= 0: the bits order as the values (idle lanes: 0)
    rmax = bmax > rmax ? bmax : rmax;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      const unsigned o = __shfl_xor(bmax, off, 64);
      bmax = o > bmax ? o : bmax;
    }
    const bool stay = act && (__uint_as_float(bmax) > threshold || passes < min_passes);
    const unsigned n_in = (unsigned)__popcll(__ballot(in));
    if (lane == 0) {
      if (kRetire && act) t.flags[blk] = stay ? 1 : 0;
      samples += (unsigned long long)n_in * (unsigned long long)((long long)t.p0 + passes);
      n_act += (kRetire && stay) ? 1u : 0u;
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    above += __shfl_down(above, off, 64);
    qsum += __shfl_down(qsum, off, 64);
    const unsigned o = __shfl_down(rmax, off, 64);
    rmax = o > rmax ? o : rmax;
  }
  if (lane == 0) {
    s_sum[wave][0] = above; s_sum[wave][1] = qsum; s_sum[wave][2] = samples; s_sum[wave][3] = n_act;
    s_max[wave] = rmax;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned long long v[4] = {0, 0, 0, 0};
    unsigned m = 0;
    for (int w = 0; w < 4; ++w) {
      for (int k = 0; k < 4; ++k) v[k] += s_sum[w][k];
      m = s_max[w] > m ? s_max[w] : m;
    }
    unsigned long long* slot = rec + (size_t)(blockIdx.x % kStatsRecSlots) * kStatsRecStride;
    if (v[0]) atomicAdd(slot + 0, v[0]);
    if (v[1]) atomicAdd(slot + 1, v[1]);
    if (m) atomicMax(reinterpret_cast<unsigned*>(slot + 2), m);
    if (v[2]) atomicAdd(slot + 3, v[2]);
    if (v[3]) atomicAdd(slot + 4, v[3]);
  }
}

// mcpt_adaptive_select_filtered's step C: one wave per block, the grid capped and
// stepped as select_kernel's.  dn is the variance filter's result over the full frame in row order
// {r, g, b, v}; a pixel's filtered relative error is rf = sqrt(v) / (max(0, Y(rgb)) + mu_floor),
// clamped to 64 as pixel_error clamps r (binary32, no contraction, in the order written).  The
// filtered record {n_above_f, sum_qf, max_rf's bits} runs over every in-frame pixel, retired blocks
// included; an active block stays active iff its largest rf > threshold or its largest r (the map
// entries step A wrote) > raw_cap or it holds fewer than min_passes passes.  rec: select_kernel's
// partial records, [0] n_above_f, [1] sum_qf, [2] max_rf's bits, [4] active blocks.
__global__ __launch_bounds__(256) void filtered_select_kernel(AdaptiveTarget t, const float4* __restrict__ dn,
                                                              const float2* __restrict__ emap, float mu_floor,
                                                              float threshold, float raw_cap, int min_passes,
                                                              unsigned long long* __restrict__ rec) {
  __shared__ unsigned long long s_sum[4][3];   // per wave: n_above_f, sum_qf, active blocks
  __shared__ unsigned s_max[4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  unsigned long long above = 0, qsum = 0;   // this lane's pixels
  unsigned fmax = 0;
  unsigned long long n_act = 0;   // this wave's blocks (lane 0 counts)
  for (long long blk = (long long)blockIdx.x * 4 + wave; blk < t.n_blocks; blk += (long long)gridDim.x * 4) {
    const int bx = (int)(blk % t.blocks_x), by = (int)(blk / t.blocks_x);
    const int x = bx * 8 + (lane & 7), lr = by * 8 + (lane >> 3);
    const bool in = x < t.W && lr < t.n_local_rows;
    const long long i = (long long)lr * t.W + x;
    const bool act = t.flags[blk] != 0;   // (wave-uniform)
    const int passes = t.passes[blk];
    float rf = 0.0f, r = 0.0f;
    if (in) {
      const float4 c = dn[i];
      const float yf = (0.2126f * c.x + 0.7152f * c.y) + 0.0722f * c.z;
      const float sef = sqrt_rn(c.w);
      rf = sef / (gmax(0.0f, yf) + mu_floor);
      if (!finite32(yf) || !(rf <= 64.0f)) rf = 64.0f;
      r = emap[i].y;
      above += (rf > threshold) ? 1u : 0u;
      qsum += error_q(rf);
    }
    unsigned bf = __float_as_uint(rf), br = __float_as_uint(r);   // both >= 0: the bits order as the values
    fmax = bf > fmax ? bf : fmax;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      const unsigned of = __shfl_xor(bf, off, 64), orr = __shfl_xor(br, off, 64);
      bf = of > bf ? of : bf;
      br = orr > br ? orr : br;
    }
    const bool stay =
        act && (__uint_as_float(bf) > threshold || __uint_as_float(br) > raw_cap || passes < min_passes);
    if (lane == 0) {
      if (act) t.flags[blk] = stay ? 1 : 0;
      n_act += stay ? 1u : 0u;
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    above += __shfl_down(above, off, 64);
    qsum += __shfl_down(qsum, off, 64);
    const unsigned o = __shfl_down(fmax, off, 64);
    fmax = o > fmax ? o : fmax;
  }
  if (lane == 0) {
    s_sum[wave][0] = above; s_sum[wave][1] = qsum; s_sum[wave][2] = n_act;
    s_max[wave] = fmax;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned long long v[3] = {0, 0, 0};
    unsigned m = 0;
    for (int w = 0; w < 4; ++w) {
      for (int k = 0; k < 3; ++k) v[k] += s_sum[w][k];
      m = s_max[w] > m ? s_max[w] : m;
    }
    unsigned long long* slot = rec + (size_t)(blockIdx.x % kStatsRecSlots) * kStatsRecStride;
    if (v[0]) atomicAdd(slot + 0, v[0]);
    if (v[1]) atomicAdd(slot + 1, v[1]);
    if (m) atomicMax(reinterpret_cast<unsigned*>(slot + 2), m);
    if (v[2]) atomicAdd(slot + 4, v[2]);
  }
}

// one workgroup of 16 waves; step k scans flags [1024 k, 1024 k + 1024)
__global__ __launch_bounds__(1024) void compact_kernel(const int* __restrict__ flags, int n, int* __restrict__ list,
                                                       int* __restrict__ count) {
  __shared__ int s_wave[16];
  __shared__ int s_base;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (threadIdx.x == 0) s_base = 0;
  __syncthreads();
  for (int b0 = 0; b0 < n; b0 += 1024) {
    const int b = b0 + (int)threadIdx.x;
    const bool f = b < n && flags[b] != 0;
    const unsigned long long m = __ballot(f);
    if (lane == 0) s_wave[wave] = __popcll(m);
    __syncthreads();
    int at = s_base + __popcll(m & ((1ull << lane) - 1ull));
    for (int w = 0; w < wave; ++w) at += s_wave[w];
    if (f) list[at] = b;   // at < the flagged blocks so far <= n
    __syncthreads();
    if (threadIdx.x == 0) {
      int s = 0;
      for (int w = 0; w < 16; ++w) s += s_wave[w];
      s_base += s;
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) count[0] = s_base;
}

__global__ __launch_bounds__(256) void add_passes_kernel(int* __restrict__ passes, const int* __restrict__ list,
                                                         int n, int n_blocks, int add) {
  const int k = blockIdx.x * 256 + threadIdx.x;
  if (k >= n) return;
  const int b = list ? list[k] : k;
  if (b >= 0 && b < n_blocks) passes[b] += add;
}

// add_passes_kernel's twin of a queued adaptive run: the grid holds n_held list
// entries, the list's length is read from count[0] (compact_kernel's, behind the list)
__global__ __launch_bounds__(256) void add_passes_counted_kernel(int* __restrict__ passes,
                                                                 const int* __restrict__ list,
                                                                 const int* __restrict__ count, int n_held,
                                                                 int n_blocks, int add) {
  const int k = blockIdx.x * 256 + threadIdx.x;
  if (k >= min(max(count[0], 0), n_held)) return;
  const int b = list[k];
  if (b >= 0 && b < n_blocks) passes[b] += add;
}

__global__ __launch_bounds__(256) void counts_kernel(CountSource src, int* __restrict__ counts, long long n_px) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n_px) return;
  counts[i] = count_at(src, i);
}

__global__ __launch_bounds__(256) void resolve_kernel(CountSource src, const float* __restrict__ accum,
                                                      float* __restrict__ out, long long n_px) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n_px) return;
  const float nb = (float)count_at(src, i);
  out[3 * i] = accum[3 * i] / nb; out[3 * i + 1] = accum[3 * i + 1] / nb; out[3 * i + 2] = accum[3 * i + 2] / nb;
}

// The filter's first input from a frame with per-pixel counts (average4_kernel's twin, DESIGN.md
// §3.9): accum / (float)count per channel as float4 (rgb, 0), one lane per pixel, one 16-byte store.
// The count comes from the count plane of a counted gather (4 B per pixel) or from the block arrays
// (4 B per block, 64 lanes of a row run share at most ceil(64 / 8) + 1 words): count_at.
__global__ __launch_bounds__(256) void resolve4_kernel(CountSource src, const float* __restrict__ accum,
                                                       float4* __restrict__ out, long long n_px) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n_px) return;
  const float nb = (float)count_at(src, i);
  out[i] = make_float4(accum[3 * i] / nb, accum[3 * i + 1] / nb, accum[3 * i + 2] / nb, 0.0f);
}

// The multi-process counted gather's two ends.  A packed record is 16 bytes per
// pixel, {r, g, b, count}: the accumulator's three f32 words as they are and the pixel's int32 sample
// count.  Both kernels move words, never floats (an overflowed sum's inf / NaN payload and a count's
// denormal bit pattern pass through), one lane per pixel, a workgroup per 256 columns of a row, the
// 16-byte side as one vector access per lane.
//  * pack_counted_kernel: the shard's rows in local order, every pixel's count from count_at.
//  * load_rows_counted_kernel: frame row y from packed row src_row[y]; the sums to accum, the counts
//    to the plane (the row scatter and the split in one pass).
__global__ __launch_bounds__(256) void pack_counted_kernel(CountSource src, int n_rows,
                                                           const unsigned* __restrict__ accum,
                                                           uint4* __restrict__ out) {
  const int x = blockIdx.x * 256 + threadIdx.x;
  if (x >= src.W) return;
  for (int lr = blockIdx.y; lr < n_rows; lr += gridDim.y) {
    const long long i = (long long)lr * src.W + x;
    out[i] = make_uint4(accum[3 * i], accum[3 * i + 1], accum[3 * i + 2], (unsigned)count_at(src, i));
  }
}

__global__ __launch_bounds__(256) void load_rows_counted_kernel(const uint4* __restrict__ src,
                                                                const int* __restrict__ src_row, int W, int H,
                                                                unsigned* __restrict__ accum,
                                                                int* __restrict__ plane) {
  const int x = blockIdx.x * 256 + threadIdx.x;
  if (x >= W) return;
  for (int y = blockIdx.y; y < H; y += gridDim.y) {
    const uint4 v = src[(long long)src_row[y] * W + x];   // (the host checked 0 <= src_row[y] < src_rows)
    const long long i = (long long)y * W + x;
    accum[3 * i] = v.x; accum[3 * i + 1] = v.y; accum[3 * i + 2] = v.z;
    plane[i] = (int)v.w;
  }
}

// load_rows_counted_kernel's twin for the gathered error map: frame row y of the
// map plane from row src_row[y] of the packed 8-byte records {se, r}, one lane per pixel, the record
// as one 8-byte integer access each way (se may be inf or NaN: the words are never read as floats)
__global__ __launch_bounds__(256) void load_rows_error_map_kernel(const uint2* __restrict__ src,
                                                                  const int* __restrict__ src_row, int W, int H,
                                                                  uint2* __restrict__ plane) {
  const int x = blockIdx.x * 256 + threadIdx.x;
  if (x >= W) return;
  for (int y = blockIdx.y; y < H; y += gridDim.y)   // (the host checked 0 <= src_row[y] < src_rows)
    plane[(long long)y * W + x] = src[(long long)src_row[y] * W + x];
}

// one wave's block of the list: accum += the block's segment sums, in chunk order
__device__ __forceinline__ void combine_list_block(float* __restrict__ accum, const float* __restrict__ partial,
                                                   long long n_px, int n_seg, int W, int n_local_rows, int blocks_x,
                                                   int n_blocks, const int* __restrict__ list, long long li,
                                                   unsigned long long* ev) {
  const int lane = threadIdx.x & 63;
  const int blk = list[li];
  if (!idx_ok(ev, CK_LIST, blk, n_blocks)) return;
  const int x = (blk % blocks_x) * 8 + (lane & 7), lr = (blk / blocks_x) * 8 + (lane >> 3);
  if (x >= W || lr >= n_local_rows) return;
  const long long i = (long long)lr * W + x;
  float a0 = accum[i * 3], a1 = accum[i * 3 + 1], a2 = accum[i * 3 + 2];
  for (int s = 0; s < n_seg; ++s) {
    const float* q = partial + ((size_t)s * n_px + i) * 3;
    a0 = a0 + q[0]; a1 = a1 + q[1]; a2 = a2 + q[2];
  }
  accum[i * 3] = a0; accum[i * 3 + 1] = a1; accum[i * 3 + 2] = a2;
}

__global__ __launch_bounds__(256) void combine_list_kernel(float* __restrict__ accum, const float* __restrict__ partial,
                                                           long long n_px, int n_seg, int W, int n_local_rows,
                                                           int blocks_x, int n_blocks, const int* __restrict__ list,
                                                           int n_list, unsigned long long* ev) {
  const long long li = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (li >= n_list) return;
  combine_list_block(accum, partial, n_px, n_seg, W, n_local_rows, blocks_x, n_blocks, list, li, ev);
}

// combine_list_kernel's twin of a queued adaptive run: the grid holds n_held list
// entries, the list's length is read from list[n_blocks] (compact_kernel's count)
__global__ __launch_bounds__(256) void combine_list_counted_kernel(float* __restrict__ accum,
                                                                   const float* __restrict__ partial, long long n_px,
                                                                   int n_seg, int W, int n_local_rows, int blocks_x,
                                                                   int n_blocks, const int* __restrict__ list,
                                                                   int n_held, unsigned long long* ev) {
  const long long li = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (li >= min(max(list[n_blocks], 0), n_held)) return;
  if (!idx_ok(ev, CK_LIST, li, n_blocks)) return;
  combine_list_block(accum, partial, n_px, n_seg, W, n_local_rows, blocks_x, n_blocks, list, li, ev);
}

}  // namespace mcpt

static unsigned grid256(long long n) { return (unsigned)((n + 255) / 256); }

hipError_t mcpt_launch_adaptive_reset(const mcpt::AdaptiveTarget& t, int* list, int* count, hipStream_t stream) {
  hipLaunchKernelGGL(mcpt::adaptive_reset_kernel, dim3(std::max(1u, grid256(t.n_blocks))), dim3(256), 0, stream, t,
                     list, count);
  return hipGetLastError();
}

// the select kernels' grid: a workgroup of four waves per four blocks, capped
static dim3 select_grid(int n_blocks) {
  return dim3((unsigned)std::min<long long>(((long long)n_blocks + 3) / 4, mcpt::kSelectMaxBlocks));
}

hipError_t mcpt_launch_adaptive_select(const mcpt::AdaptiveTarget& t, const float4* state, float2* emap,
                                       long long passes, int batches, float mu_floor, float threshold, int min_passes,
                                       bool retire, unsigned long long* rec, hipStream_t stream) {
  hipError_t e = hipMemsetAsync(rec, 0, sizeof(unsigned long long) * mcpt::kStatsRecWords, stream);
  if (e != hipSuccess || t.n_blocks <= 0) return e;
  if (retire)
    hipLaunchKernelGGL(mcpt::select_kernel<true>, select_grid(t.n_blocks), dim3(256), 0, stream, t, state, emap,
                       (float)passes, (float)(batches - 1), mu_floor, threshold, min_passes, rec);
  else
    hipLaunchKernelGGL(mcpt::select_kernel<false>, select_grid(t.n_blocks), dim3(256), 0, stream, t, state, emap,
                       (float)passes, (float)(batches - 1), mu_floor, threshold, min_passes, rec);
  return hipGetLastError();
}

hipError_t mcpt_launch_adaptive_select_filtered(const mcpt::AdaptiveTarget& t, const float4* dn, const float2* emap,
                                                float mu_floor, float threshold, float raw_cap, int min_passes,
                                                unsigned long long* rec, hipStream_t stream) {
  hipError_t e = hipMemsetAsync(rec, 0, sizeof(unsigned long long) * mcpt::kStatsRecWords, stream);
  if (e != hipSuccess || t.n_blocks <= 0) return e;
  hipLaunchKernelGGL(mcpt::filtered_select_kernel, select_grid(t.n_blocks), dim3(256), 0, stream, t, dn, emap, mu_floor,
                     threshold, raw_cap, min_passes, rec);
  return hipGetLastError();
}

hipError_t mcpt_launch_adaptive_compact(const mcpt::AdaptiveTarget& t, int* list, int* count, hipStream_t stream) {
  hipLaunchKernelGGL(mcpt::compact_kernel, dim3(1), dim3(1024), 0, stream, t.flags, t.n_blocks, list, count);
  return hipGetLastError();
}

hipError_t mcpt_launch_adaptive_add_passes(const mcpt::AdaptiveTarget& t, const int* list, int n_list, int n,
                                           hipStream_t stream) {
  const int k = list ? n_list : t.n_blocks;
  if (k <= 0) return hipSuccess;
  hipLaunchKernelGGL(mcpt::add_passes_kernel, dim3(grid256(k)), dim3(256), 0, stream, t.passes, list, k, t.n_blocks, n);
  return hipGetLastError();
}

hipError_t mcpt_launch_adaptive_add_passes_counted(const mcpt::AdaptiveTarget& t, const int* list, const int* count,
                                                   int n_held, int n, hipStream_t stream) {
  if (n_held <= 0) return hipSuccess;
  hipLaunchKernelGGL(mcpt::add_passes_counted_kernel, dim3(grid256(n_held)), dim3(256), 0, stream, t.passes, list, count,
                     n_held, t.n_blocks, n);
  return hipGetLastError();
}

hipError_t mcpt_launch_counts(const mcpt::CountSource& src, int* counts, long long n_px, hipStream_t stream) {
  if (n_px <= 0) return hipSuccess;
  hipLaunchKernelGGL(mcpt::counts_kernel, dim3(grid256(n_px)), dim3(256), 0, stream, src, counts, n_px);
  return hipGetLastError();
}

hipError_t mcpt_launch_resolve(const mcpt::CountSource& src, const float* accum, float* out, long long n_px,
                               hipStream_t stream) {
  if (n_px <= 0) return hipSuccess;
  hipLaunchKernelGGL(mcpt::resolve_kernel, dim3(grid256(n_px)), dim3(256), 0, stream, src, accum, out, n_px);
  return hipGetLastError();
}

hipError_t mcpt_launch_resolve4(const mcpt::CountSource& src, const float* accum, float4* out, long long n_px,
                                hipStream_t stream) {
  if (n_px <= 0) return hipSuccess;
  hipLaunchKernelGGL(mcpt::resolve4_kernel, dim3(grid256(n_px)), dim3(256), 0, stream, src, accum, out, n_px);
  return hipGetLastError();
}

// a workgroup per 256 columns of a row; rows past the grid's y limit are stepped over
static dim3 row_grid(int W, int rows) { return dim3(grid256(W), (unsigned)std::min(rows, 65535)); }

hipError_t mcpt_launch_pack_counted(const mcpt::CountSource& src, int n_rows, const float* accum, void* out,
                                    hipStream_t stream) {
  if (src.W <= 0 || n_rows <= 0) return hipSuccess;
  hipLaunchKernelGGL(mcpt::pack_counted_kernel, row_grid(src.W, n_rows), dim3(256), 0, stream, src, n_rows,
                     reinterpret_cast<const unsigned*>(accum), static_cast<uint4*>(out));
  return hipGetLastError();
}

hipError_t mcpt_launch_load_rows_counted(const void* src, const int* src_row, int W, int H, float* accum, int* plane,
                                         hipStream_t stream) {
  if (W <= 0 || H <= 0) return hipSuccess;
  hipLaunchKernelGGL(mcpt::load_rows_counted_kernel, row_grid(W, H), dim3(256), 0, stream,
                     static_cast<const uint4*>(src), src_row, W, H, reinterpret_cast<unsigned*>(accum), plane);
  return hipGetLastError();
}

hipError_t mcpt_launch_load_rows_error_map(const void* src, const int* src_row, int W, int H, float2* plane,
                                           hipStream_t stream) {
  if (W <= 0 || H <= 0) return hipSuccess;
  hipLaunchKernelGGL(mcpt::load_rows_error_map_kernel, row_grid(W, H), dim3(256), 0, stream,
                     static_cast<const uint2*>(src), src_row, W, H, reinterpret_cast<uint2*>(plane));
  return hipGetLastError();
}

hipError_t mcpt_launch_combine_list(const mcpt::RenderParams& p, hipStream_t stream) {
  if (p.n_segments <= 1 || p.n_list == 0) return hipSuccess;   // (one segment: the render added it itself)
  if (p.n_list < 0) {   // a queued adaptive run: a grid of -n_list entries, the length read on the device
    hipLaunchKernelGGL(mcpt::combine_list_counted_kernel, dim3((unsigned)((-(long long)p.n_list + 3) / 4)), dim3(256), 0,
                       stream, p.accum, p.partial, p.n_local_px, p.n_segments, p.W, p.n_local_rows, p.blocks_x,
                       p.n_blocks, p.list, -p.n_list, p.events);
    return hipGetLastError();
  }
  hipLaunchKernelGGL(mcpt::combine_list_kernel, dim3((unsigned)(((long long)p.n_list + 3) / 4)), dim3(256), 0, stream,
                     p.accum, p.partial, p.n_local_px, p.n_segments, p.W, p.n_local_rows, p.blocks_x, p.n_blocks, p.list,
                     p.n_list, p.events);
  return hipGetLastError();
}
