// mcpt_capi_post.hip — C ABI, device half: what runs on a rendered accumulator (guide buffers and
// the à-trous denoiser, noise statistics and the convergence metric, adaptive sampling, the held
// error map's record).  The gathers that fill a frame's planes are mcpt_capi_gather.hip's.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <initializer_list>

#include "mcpt_ctx.h"

namespace plan = mcpt::plan;

static bool positive_finite(std::initializer_list<float> values) {
  for (float v : values)
    if (!(v > 0.0f) || !std::isfinite(v)) return false;
  return true;
}
// a refusal whose detail names the entry point the caller called: "<who>: <why>"
static int refuse(int status, const char* who, const char* why) {
  char what[256];
  std::snprintf(what, sizeof(what), "%s: %s", who, why);
  return set_err(status, what);
}

// One batch of the noise statistics: "the accumulator now holds n more passes than
// at the previous batch", enqueued on the context's stream (which is ordered after every queued
// render's combine), no host wait.  d_count: a queued adaptive run's batch (§3.9.3), which changes
// nothing once the list's length on the device is 0; timed false: it records no events.
hipError_t stats_batch(mcpt_ctx* c, int n, const int* d_count, bool timed) {
  const long long n_px = (long long)c->n_local_rows * c->W;
  hipError_t e = timed ? ensure_timing_events(c->stats.stats_ev, 2) : hipSuccess;
  if (e == hipSuccess && timed) e = hipEventRecord(c->stats.stats_ev[0], c->stream);
  if (e == hipSuccess)
    e = d_count ? mcpt_launch_stats_update_counted(c->target.d_accum, c->stats.d_stats, n_px, n, d_count, c->stream)
                : mcpt_launch_stats_update(c->target.d_accum, c->stats.d_stats, n_px, n, c->stream);
  if (e == hipSuccess && timed) e = hipEventRecord(c->stats.stats_ev[1], c->stream);
  if (e != hipSuccess) return e;
  c->stats.stats_passes += n;
  c->stats.stats_batches += 1;
  if (timed) c->stats.stats_update_timed = true;
  return hipSuccess;
}

// the frame's record from the kStatsRecSlots partial records of a reducing kernel: the words add,
// but word max_word is a maximum of bit patterns (max_r's bits, the longest history)
static void reduce_stats_records(const unsigned long long* part, int n_words, int max_word, unsigned long long* h) {
  for (int s = 0; s < mcpt::kStatsRecSlots; ++s) {
    const unsigned long long* q = part + (size_t)s * mcpt::kStatsRecStride;
    for (int w = 0; w < n_words; ++w) h[w] = w == max_word ? std::max(h[w], q[w] & 0xffffffffull) : h[w] + q[w];
  }
}
// a kernel's partial records back and reduced into h (zeroed by the caller), with them a second
// kernel's into hf and a list length into *len (null: none): every copy is issued, then one wait
static int read_stats_records(mcpt_ctx* c, int n_words, int max_word, const unsigned long long* d_rec,
                              unsigned long long* h, const unsigned long long* d_rec_f = nullptr,
                              unsigned long long* hf = nullptr, const int* d_len = nullptr, int* len = nullptr) {
  unsigned long long part[mcpt::kStatsRecWords] = {}, part_f[mcpt::kStatsRecWords] = {};
  HIP_OR_RETURN(hipMemcpyAsync(part, d_rec, sizeof(part), hipMemcpyDeviceToHost, c->stream));
  if (d_rec_f) HIP_OR_RETURN(hipMemcpyAsync(part_f, d_rec_f, sizeof(part_f), hipMemcpyDeviceToHost, c->stream));
  if (d_len) HIP_OR_RETURN(hipMemcpyAsync(len, d_len, sizeof(int), hipMemcpyDeviceToHost, c->stream));
  HIP_OR_RETURN(hipStreamSynchronize(c->stream));
  reduce_stats_records(part, n_words, max_word, h);
  if (d_rec_f) reduce_stats_records(part_f, n_words, max_word, hf);
  return MCPT_OK;
}
// ... into the leading fields mcpt_convergence_t and mcpt_adaptive_t share
template <class Rec>
static void fill_frame_record(const mcpt_ctx* c, const unsigned long long* h, Rec* out) {
  const long long n = (long long)c->n_local_rows * c->W;
  out->n_px = n;
  out->n_above = (long long)h[0];
  out->sum_q = h[1];
  const unsigned mb = (unsigned)(h[2] & 0xffffffffull);
  std::memcpy(&out->max_r, &mb, sizeof(float));
  out->mean_r = n > 0 ? (double)h[1] / 65536.0 / (double)n : 0.0;
  out->passes = c->stats.stats_passes;
  out->batches = c->stats.stats_batches;
}
// the filtered select's own fields from its step C's record
static void fill_filtered_record(const mcpt_ctx* c, const unsigned long long* hf, mcpt_adaptive_filtered_t* out) {
  const long long n = (long long)c->n_local_rows * c->W;
  out->n_above_f = (long long)hf[0];
  out->sum_qf = hf[1];
  const unsigned mb = (unsigned)(hf[2] & 0xffffffffull);
  std::memcpy(&out->max_rf, &mb, sizeof(float));
  out->mean_rf = n > 0 ? (double)hf[1] / 65536.0 / (double)n : 0.0;
}
// elapsed ms of an optional event pair into *out (null: not asked for): 0 unless the pair was recorded
static int pair_ms(bool timed, hipEvent_t ev_a, hipEvent_t ev_b, float* out) {
  if (!out) return MCPT_OK;
  *out = 0.0f;
  if (timed) {
    HIP_OR_RETURN(hipEventSynchronize(ev_b));
    HIP_OR_RETURN(hipEventElapsedTime(out, ev_a, ev_b));
  }
  return MCPT_OK;
}

extern "C" {

// ---- guide buffers and the à-trous denoiser (mcpt_denoise.hip)
// the kernel of the filter's steps 1 and 2 when MCPT_DENOISE_NAIVE is unset: 0 the LDS-tile
// kernels, 1 the global-tap kernel (the A/B: tools/denoise_bench.py, profiles/denoise_bench.json)
constexpr int kAtrousNaiveDefault = 0;
static hipError_t ensure_denoise_buffers(mcpt_ctx* c) {
  if (c->denoise.d_guide) return hipSuccess;
  const size_t n = (size_t)c->n_local_rows * c->W;
  if (!n) return hipSuccess;
  mcpt_ctx::Denoise g;
  hipError_t e = g.d_guide.alloc(n * 2);
  if (e == hipSuccess) e = g.d_albedo.alloc(n);
  if (e == hipSuccess) e = g.d_dn[0].alloc(n);
  if (e == hipSuccess) e = g.d_dn[1].alloc(n);
  if (e == hipSuccess) c->denoise = std::move(g);
  return e;
}
int mcpt_render_guides(mcpt_ctx* c, const float* invPV, const float* invV) {
  OK_OR_RETURN(check_renderable(c, invPV && invV, "mcpt_render_guides"));
  HIP_OR_RETURN(hipSetDevice(c->device));
  HIP_OR_RETURN(ensure_denoise_buffers(c));
  HIP_OR_RETURN(ensure_timing_events(c->denoise.guide_ev, 2));
  mcpt::GuideParams g;
  std::memset(&g, 0, sizeof(g));
  scene_params(c, invPV, invV, g.r);   // (guide_kernel reads none of accum, events, lds_scene_bytes, tile_w)
  g.guide = c->denoise.d_guide; g.albedo = c->denoise.d_albedo;
  HIP_OR_RETURN(hipEventRecord(c->denoise.guide_ev[0], c->stream));
  HIP_OR_RETURN(mcpt_launch_guides(g, c->stream));
  HIP_OR_RETURN(hipEventRecord(c->denoise.guide_ev[1], c->stream));
  c->denoise.guides_valid = true;
  c->denoise.guides_timed = true;
  return MCPT_OK;
}

int mcpt_read_guides(mcpt_ctx* c, float* guide8, float* albedo4) {
  if (!c) return mcpt_err_bare(MCPT_ERR_INVALID_ARG);
  if (!c->has_target) return mcpt_err_bare(MCPT_ERR_NO_TARGET);
  if (!c->denoise.guides_valid) return set_err(MCPT_ERR_NO_GUIDES, "mcpt_read_guides: no guides rendered for this target and scene");
  HIP_OR_RETURN(hipSetDevice(c->device));
  const size_t n = (size_t)c->n_local_rows * c->W;
  if (guide8 && n)
    HIP_OR_RETURN(hipMemcpyAsync(guide8, c->denoise.d_guide, n * 2 * sizeof(float4), hipMemcpyDeviceToHost, c->stream));
  if (albedo4 && n)
    HIP_OR_RETURN(hipMemcpyAsync(albedo4, c->denoise.d_albedo, n * sizeof(float4), hipMemcpyDeviceToHost, c->stream));
  HIP_OR_RETURN(hipStreamSynchronize(c->stream));
  return MCPT_OK;
}

// Which filter a run is: the six public forms by name, `who` for a refusal's detail.  guided false:
// sigma_color is the global width; guided true: it is k_color, the width per pixel k_color * 2^-s * se
// from the error map; resolved: the input is accum / (float)count with every pixel's own count
//  in place of accum / pass_count; variance: guided's preconditions and map, the
// first input carries the prefiltered se^2 in .w and every iteration filters it along (DESIGN.md
// §3.8); timed false: no events (a queued adaptive run's selects but its last)
struct FilterForm {
  const char* who;
  bool guided, resolved, variance;
  bool timed = true;
};
constexpr FilterForm kPlain = {"mcpt_denoise", false, false, false};
constexpr FilterForm kGuided = {"mcpt_denoise_guided", true, false, false};
constexpr FilterForm kResolved = {"mcpt_denoise_resolved", false, true, false};
constexpr FilterForm kResolvedGuided = {"mcpt_denoise_resolved_guided", true, true, false};
constexpr FilterForm kVariance = {"mcpt_denoise_variance", true, false, true};
constexpr FilterForm kResolvedVariance = {"mcpt_denoise_resolved_variance", true, true, true};

// the filter's iterations from the first input in d_dn[0] (defined behind denoise_run)
static int atrous_iterations(mcpt_ctx* c, int iterations, float sigma_color, float sigma_plane, const FilterForm& form,
                             const float2* emap, bool naive);

static int denoise_run(mcpt_ctx* c, int iterations, float sigma_color, float sigma_plane, const FilterForm& form) {
  const bool guided = form.guided, resolved = form.resolved, variance = form.variance, timed = form.timed;
  const char* who = form.who;
  if (!c || iterations < 0 || iterations > 8) return refuse(MCPT_ERR_INVALID_ARG, who, "iterations not in 0..8");
  if (!positive_finite({sigma_color, sigma_plane}))
    return refuse(MCPT_ERR_INVALID_ARG, who, "sigmas must be positive and finite");
  if (!c->has_target) return set_err(MCPT_ERR_NO_TARGET, "no render target");
  if (resolved && !has_pixel_counts(c))
    return refuse(MCPT_ERR_NO_ADAPTIVE, who, "no per-pixel sample counts (adaptive mode off, no counted gather)");
  if (!plan::is_full_frame(c->rows, c->H))
    return refuse(MCPT_ERR_INVALID_ARG, who, "needs a full-frame target (gather the shards first)");
  if (c->pass_count <= 0) return refuse(MCPT_ERR_INVALID_ARG, who, "the accumulator holds no passes");
  if (!resolved && c->adaptive.ad_on && c->adaptive.ad_n_list < c->adaptive.ad_n_blocks)
    return refuse(MCPT_ERR_INVALID_ARG, who, "adaptive mode has retired blocks (per-pixel sample counts)");
  if (!c->denoise.guides_valid) return refuse(MCPT_ERR_NO_GUIDES, who, "no guides rendered for this target and scene");
  // the guided forms' map: the one the context holds (the gathered plane, else the own window's);
  // a frame with gathered counts holds no window of its pixels, so its own map never serves the
  // resolved form of it
  const float2* emap = held_error_map(c);
  const int source = error_map_source(c);
  if (guided && (source == 0 || (resolved && c->planes.plane_valid && source != 2)))
    return refuse(MCPT_ERR_NO_STATS, who, "no error map (mcpt_convergence) of the current statistics");
  HIP_OR_RETURN(hipSetDevice(c->device));
  HIP_OR_RETURN(ensure_denoise_buffers(c));
  HIP_OR_RETURN(ensure_timing_events(c->denoise.dn_ev, 10));
  // which kernel runs steps 1 and 2 (same bits): MCPT_DENOISE_NAIVE=1 the
  // global-tap kernel, =0 the LDS-tile kernels, unset the measured default
  const bool naive = env_int("MCPT_DENOISE_NAIVE", kAtrousNaiveDefault) != 0;
  const long long n = (long long)c->H * c->W;
  // (the context's stream is ordered after all queued renders: their combines run on it)
  if (timed) HIP_OR_RETURN(hipEventRecord(c->denoise.dn_ev[9], c->stream));
  const mcpt::CountSource counts = count_source(c);
  if (variance)
    HIP_OR_RETURN(mcpt_launch_variance_init(resolved ? &counts : nullptr, c->target.d_accum, c->denoise.d_dn[0], c->denoise.d_guide, emap, c->W,
                                            c->H, c->pass_count, c->stream));
  else if (resolved)
    HIP_OR_RETURN(mcpt_launch_resolve4(count_source(c), c->target.d_accum, c->denoise.d_dn[0], n, c->stream));
  else
    HIP_OR_RETURN(mcpt_launch_average4(c->target.d_accum, c->denoise.d_dn[0], n, c->pass_count, c->stream));
  if (timed) HIP_OR_RETURN(hipEventRecord(c->denoise.dn_ev[0], c->stream));
  return atrous_iterations(c, iterations, sigma_color, sigma_plane, form, emap, naive);
}

// (denoise_run, mcpt_denoise_temporal; of the form: guided, variance, timed)
static int atrous_iterations(mcpt_ctx* c, int iterations, float sigma_color, float sigma_plane, const FilterForm& form,
                             const float2* emap, bool naive) {
  const bool guided = form.guided, variance = form.variance, timed = form.timed;
  int lds_mask = 0;
  for (int s = 0; s < iterations; ++s) {
    const int step = 1 << s;
    // the iteration's constants in binary32: 2^-s and step are exact factors
    const float sc = sigma_color * std::ldexp(1.0f, -s);
    const float sp = sigma_plane * (float)step;
    // (guided: the kernel forms kc per pixel from sc = k_color * 2^-s and the pixel's se, §3.8)
    const float kc = guided ? sc : 1.0f / (sc * sc), kp = 1.0f / (sp * sp);
    if (variance)   // (k_color^2, not halved: the width follows the variance the iteration's input has)
      HIP_OR_RETURN(mcpt_launch_atrous_variance(c->denoise.d_dn[s & 1], c->denoise.d_dn[(s + 1) & 1], c->denoise.d_guide, c->W, c->H, step,
                                                sigma_color * sigma_color, kp, naive, c->stream));
    else
      HIP_OR_RETURN(mcpt_launch_atrous(c->denoise.d_dn[s & 1], c->denoise.d_dn[(s + 1) & 1], c->denoise.d_guide, c->W, c->H, step, kc, kp,
                                       guided ? emap : nullptr, naive, c->stream));
    if (timed) HIP_OR_RETURN(hipEventRecord(c->denoise.dn_ev[s + 1], c->stream));
    if (!naive && step <= 2) lds_mask |= 1 << s;
  }
  c->denoise.dn_lds_mask = lds_mask;
  c->denoise.dn_result = iterations & 1;
  c->denoise.dn_iters = iterations;
  c->denoise.dn_variance = variance;
  return MCPT_OK;
}

int mcpt_denoise(mcpt_ctx* c, int iterations, float sigma_color, float sigma_plane) {
  return denoise_run(c, iterations, sigma_color, sigma_plane, kPlain);
}

int mcpt_denoise_guided(mcpt_ctx* c, int iterations, float k_color, float sigma_plane) {
  return denoise_run(c, iterations, k_color, sigma_plane, kGuided);
}

int mcpt_denoise_resolved(mcpt_ctx* c, int iterations, float sigma_color, float sigma_plane) {
  return denoise_run(c, iterations, sigma_color, sigma_plane, kResolved);
}

int mcpt_denoise_resolved_guided(mcpt_ctx* c, int iterations, float k_color, float sigma_plane) {
  return denoise_run(c, iterations, k_color, sigma_plane, kResolvedGuided);
}

int mcpt_denoise_variance(mcpt_ctx* c, int iterations, float k_color, float sigma_plane) {
  return denoise_run(c, iterations, k_color, sigma_plane, kVariance);
}

int mcpt_denoise_resolved_variance(mcpt_ctx* c, int iterations, float k_color, float sigma_plane) {
  return denoise_run(c, iterations, k_color, sigma_plane, kResolvedVariance);
}

// ---- noise statistics and the convergence metric (mcpt_stats.hip)
// the statistics' buffers of the current target (mcpt_stats_begin, mcpt_adaptive_checkpoint_load)
static int ensure_stats_buffers(mcpt_ctx* c) {
  const size_t n = (size_t)c->n_local_rows * c->W;
  if (!c->stats.d_conv) {
    mcpt_ctx::Stats g;
    hipError_t e = g.d_conv.alloc(mcpt::kStatsRecWords);
    if (e == hipSuccess && n) e = g.d_stats.alloc(n);
    if (e == hipSuccess && n) e = g.d_emap.alloc(n);
    if (e != hipSuccess) return set_err(MCPT_ERR_HIP, "mcpt_stats_begin: allocation", e);
    c->stats = std::move(g);
  }
  return MCPT_OK;
}

int mcpt_stats_begin(mcpt_ctx* c) {
  if (!c) return mcpt_err_bare(MCPT_ERR_INVALID_ARG);
  if (!c->has_target) return set_err(MCPT_ERR_NO_TARGET, "no render target");
  HIP_OR_RETURN(hipSetDevice(c->device));
  const size_t n = (size_t)c->n_local_rows * c->W;
  OK_OR_RETURN(ensure_stats_buffers(c));
  HIP_OR_RETURN(mcpt_launch_stats_begin(c->target.d_accum, c->stats.d_stats, (long long)n, c->stream));
  c->stats.stats_on = true;
  c->stats.stats_passes = 0;
  c->stats.stats_batches = 0;
  c->stats.emap_valid = false;
  return MCPT_OK;
}

int mcpt_stats_end(mcpt_ctx* c) {
  if (!c) return mcpt_err_bare(MCPT_ERR_INVALID_ARG);
  HIP_OR_RETURN(hipSetDevice(c->device));
  if (c->stats.d_conv) HIP_OR_RETURN(hipStreamSynchronize(c->stream));   // (queued updates still use the buffers)
  c->stats = {};
  c->adaptive = {};   // (the adaptive mode selects from the statistics: off with them)
  return MCPT_OK;
}

int mcpt_stats_add_batch(mcpt_ctx* c, int n) {
  if (!c || n <= 0) return set_err(MCPT_ERR_INVALID_ARG, "mcpt_stats_add_batch: a batch holds at least one pass");
  if (!c->stats.stats_on) return set_err(MCPT_ERR_NO_STATS, "mcpt_stats_add_batch: statistics are off (mcpt_stats_begin)");
  HIP_OR_RETURN(hipSetDevice(c->device));
  HIP_OR_RETURN(stats_batch(c, n));
  return MCPT_OK;
}

int mcpt_stats_info(mcpt_ctx* c, int* on, long long* passes, int* batches) {
  if (!c) return mcpt_err_bare(MCPT_ERR_INVALID_ARG);
  if (on) *on = c->stats.stats_on ? 1 : 0;
  if (passes) *passes = c->stats.stats_passes;
  if (batches) *batches = c->stats.stats_batches;
  return MCPT_OK;
}

int mcpt_convergence(mcpt_ctx* c, float threshold, float mu_floor, mcpt_convergence_t* out) {
  if (!c || !out) return mcpt_err_bare(MCPT_ERR_INVALID_ARG);
  if (!positive_finite({threshold, mu_floor}))
    return set_err(MCPT_ERR_INVALID_ARG, "mcpt_convergence: threshold and mu_floor must be positive and finite");
  if (!c->stats.stats_on) return set_err(MCPT_ERR_NO_STATS, "mcpt_convergence: statistics are off (mcpt_stats_begin)");
  if (c->stats.stats_batches < 2) return set_err(MCPT_ERR_NO_STATS, "mcpt_convergence: needs two batches or more");
  HIP_OR_RETURN(hipSetDevice(c->device));
  HIP_OR_RETURN(ensure_timing_events(c->stats.stats_ev + 2, 2));
  const long long n = (long long)c->n_local_rows * c->W;
  HIP_OR_RETURN(hipEventRecord(c->stats.stats_ev[2], c->stream));
  HIP_OR_RETURN(mcpt_launch_stats_error(c->stats.d_stats, c->stats.d_emap, n, c->stats.stats_passes, c->stats.stats_batches, mu_floor,
                                        threshold, c->stats.d_conv, c->stream));
  HIP_OR_RETURN(hipEventRecord(c->stats.stats_ev[3], c->stream));
  c->stats.stats_error_timed = true;
  c->stats.emap_valid = true;
  unsigned long long h[3] = {0, 0, 0};
  OK_OR_RETURN(read_stats_records(c, 3, 2, c->stats.d_conv, h));
  fill_frame_record(c, h, out);
  return MCPT_OK;
}

int mcpt_read_error_map(mcpt_ctx* c, float* se_r2) {
  if (!c || !se_r2) return mcpt_err_bare(MCPT_ERR_INVALID_ARG);
  const int source = error_map_source(c);
  if (source == 0 || (source == 1 && c->stats.stats_batches < 2))
    return set_err(MCPT_ERR_NO_STATS, "mcpt_read_error_map: no mcpt_convergence of the current statistics");
  HIP_OR_RETURN(hipSetDevice(c->device));
  const size_t n = (size_t)c->n_local_rows * c->W;
  if (n) HIP_OR_RETURN(hipMemcpyAsync(se_r2, held_error_map(c), n * sizeof(float2), hipMemcpyDeviceToHost, c->stream));
  HIP_OR_RETURN(hipStreamSynchronize(c->stream));
  return MCPT_OK;
}

int mcpt_last_stats_ms(mcpt_ctx* c, float* update_ms, float* error_ms) {
  if (!c) return mcpt_err_bare(MCPT_ERR_INVALID_ARG);
  HIP_OR_RETURN(hipSetDevice(c->device));
  OK_OR_RETURN(pair_ms(c->stats.stats_update_timed, c->stats.stats_ev[0], c->stats.stats_ev[1], update_ms));
  return pair_ms(c->stats.stats_error_timed, c->stats.stats_ev[2], c->stats.stats_ev[3], error_ms);
}

// ---- adaptive sampling of 8x8 blocks (mcpt_adaptive.hip)
// the block arrays of the current target and its block grid (mcpt_adaptive_begin,
// mcpt_adaptive_checkpoint_load)
static int ensure_adaptive_buffers(mcpt_ctx* c) {
  const int bx = (c->W + 7) / 8, by = (c->n_local_rows + 7) / 8;
  if (!c->adaptive.d_ad_flags) {
    const size_t n = (size_t)std::max(bx * by, 1);
    mcpt_ctx::Adaptive g;
    hipError_t e = g.d_ad_flags.alloc(n);
    if (e == hipSuccess) e = g.d_ad_passes.alloc(n);
    if (e == hipSuccess) e = g.d_ad_list.alloc(n + 1);
    if (e != hipSuccess) return set_err(MCPT_ERR_HIP, "mcpt_adaptive_begin: allocation", e);
    c->adaptive = std::move(g);
  }
  c->adaptive.ad_blocks_x = bx;
  c->adaptive.ad_n_blocks = bx * by;
  return MCPT_OK;
}

int mcpt_adaptive_begin(mcpt_ctx* c, int min_passes) {
  if (!c || min_passes < 0) return set_err(MCPT_ERR_INVALID_ARG, "mcpt_adaptive_begin: min_passes must not be negative");
  if (!c->has_target) return set_err(MCPT_ERR_NO_TARGET, "no render target");
  if (!c->stats.stats_on) return set_err(MCPT_ERR_NO_STATS, "mcpt_adaptive_begin: statistics are off (mcpt_stats_begin)");
  HIP_OR_RETURN(hipSetDevice(c->device));
  OK_OR_RETURN(ensure_adaptive_buffers(c));
  c->adaptive.ad_p0 = c->pass_count;
  c->adaptive.ad_min_passes = min_passes;
  HIP_OR_RETURN(mcpt_launch_adaptive_reset(adaptive_target(c), c->adaptive.d_ad_list, c->adaptive.d_ad_list + c->adaptive.ad_n_blocks, c->stream));
  c->adaptive.ad_n_list = c->adaptive.ad_n_blocks;
  c->adaptive.ad_on = true;
  return MCPT_OK;
}

int mcpt_adaptive_end(mcpt_ctx* c) {
  if (!c) return mcpt_err_bare(MCPT_ERR_INVALID_ARG);
  HIP_OR_RETURN(hipSetDevice(c->device));
  if (c->adaptive.d_ad_flags) HIP_OR_RETURN(hipStreamSynchronize(c->stream));   // (queued launches still read the list)
  c->adaptive = {};
  return MCPT_OK;
}

int mcpt_adaptive_info(mcpt_ctx* c, int* on, long long* n_active, long long* n_blocks) {
  if (!c) return mcpt_err_bare(MCPT_ERR_INVALID_ARG);
  if (on) *on = c->adaptive.ad_on ? 1 : 0;
  if (n_active) *n_active = c->adaptive.ad_on ? c->adaptive.ad_n_list : 0;
  if (n_blocks) *n_blocks = c->adaptive.ad_on ? c->adaptive.ad_n_blocks : 0;
  return MCPT_OK;
}

// ---- one select step behind mcpt_adaptive_select,
// mcpt_adaptive_select_filtered and every select of a queued run: its rule, its checks, its enqueue
// half and its host half.
// the filtered rule's own arguments; SelectRule::f null: mcpt_adaptive_select's rule on the raw error
struct RunFilter { float raw_cap; int iterations; float k_color, sigma_plane; };
// the temporal rule's own arguments: mcpt_temporal_accumulate_resolved's
struct RunTemporal { const float* prevPV16; int max_history; float plane_tol; };
struct SelectRule { float threshold, mu_floor; const RunFilter* f; const RunTemporal* t = nullptr; };
// where a select's results go on the device: the rule kernel's partial records, the filtered rule's
// step C's or the temporal rule's step T's (null for the raw rule) and a slot that receives a copy of
// the list's length (null: none)
struct SelectDest { unsigned long long *rec, *rec_f; int* len; };
// the records a select's caller receives: raw always, one of the others with its rule
struct SelectOut { mcpt_adaptive_t* raw; mcpt_adaptive_filtered_t* filtered; mcpt_adaptive_temporal_t* temporal; };

// An accumulate's launch parameters from the context (mcpt_temporal_accumulate*, the temporal select's
// dry run): the current frame, the history's current set as input and the other set as output, the
// previous camera; its preconditions have been checked
static mcpt::TemporalParams temporal_params(const mcpt_ctx* c, const float2* emap, const float* prevPV16,
                                            int max_history, float plane_tol) {
  const int in = c->temporal.tp_cur, to = in ^ 1;
  const bool empty = c->temporal.tp_frames == 0;
  mcpt::TemporalParams p;
  std::memset(&p, 0, sizeof(p));
  p.accum = c->target.d_accum; p.emap = emap; p.guide = c->denoise.d_guide;
  p.hc_in = c->temporal.d_tp_c[in]; p.hl_in = c->temporal.d_tp_len[in]; p.hg_in = c->temporal.d_tp_g[c->temporal.tp_copy ? 0 : in];
  p.hc_out = c->temporal.d_tp_c[to]; p.hl_out = c->temporal.d_tp_len[to]; p.hg_out = c->temporal.tp_copy ? nullptr : c->temporal.d_tp_g[to];
  p.rec = c->temporal.d_tp_rec;
  p.W = c->W; p.H = c->H; p.nb = (float)c->pass_count;
  p.counts = count_source(c);
  p.max_history = max_history; p.plane_tol = plane_tol; p.empty = empty ? 1 : 0;
  if (!empty) std::memcpy(p.M, prevPV16, sizeof(p.M));
  return p;
}

// The rule's preconditions, behind the caller's own MCPT_ERR_NO_ADAPTIVE.  single: one select now
// (mcpt_adaptive_select*), which needs passes and two batches on entry; a queued run's schedule
// places its selects behind both.
static int check_select_rule(const mcpt_ctx* c, const SelectRule& r, bool single, const char* who) {
  const RunFilter* f = r.f;
  const RunTemporal* t = r.t;
  if (t && !c->temporal.tp_on) return refuse(MCPT_ERR_NO_TEMPORAL, who, "temporal mode is off (mcpt_temporal_begin)");
  if (!positive_finite({r.threshold, r.mu_floor, f ? f->raw_cap : 1.0f, f ? f->k_color : 1.0f, f ? f->sigma_plane : 1.0f,
                        t ? t->plane_tol : 1.0f}))
    return refuse(MCPT_ERR_INVALID_ARG, who,
                  t         ? "threshold, mu_floor and plane_tol must be positive and finite"
                  : !single ? "threshold, mu_floor and the filter's widths must be positive and finite"
                  : f       ? "threshold, raw_cap, mu_floor, k_color and sigma_plane must be positive and finite"
                            : "threshold and mu_floor must be positive and finite");
  if (f && (f->iterations < 0 || f->iterations > 8)) return refuse(MCPT_ERR_INVALID_ARG, who, "iterations not in 0..8");
  if (t) {
    if (t->max_history < 1 || t->max_history > MCPT_TEMPORAL_MAX_HISTORY)
      return refuse(MCPT_ERR_INVALID_ARG, who, "max_history not in 1..65535");
    if (c->temporal.tp_frames > 0 && !t->prevPV16)
      return refuse(MCPT_ERR_INVALID_ARG, who, "the history needs the previous camera's P*V");
  }
  if (f || t) {
    if (!plan::is_full_frame(c->rows, c->H))
      return refuse(MCPT_ERR_INVALID_ARG, who,
                    f ? "needs a full-frame target (a shard is filtered after its gather)"
                      : "needs a full-frame target (gather the shards first)");
    // (the filter or the dry run would read a gathered frame's counts and map, the rule this window's)
    if (c->planes.plane_valid || c->planes.emap_plane_valid)
      return refuse(MCPT_ERR_INVALID_ARG, who, "the context holds a gathered frame's counts or error map");
    if (single && c->pass_count <= 0) return refuse(MCPT_ERR_INVALID_ARG, who, "the accumulator holds no passes");
  }
  if (!c->stats.stats_on) return refuse(MCPT_ERR_NO_STATS, who, "statistics are off (mcpt_stats_begin)");
  if (single && c->stats.stats_batches < 2) return refuse(MCPT_ERR_NO_STATS, who, "needs two batches or more");
  if ((f || t) && !c->denoise.guides_valid) return refuse(MCPT_ERR_NO_GUIDES, who, "no guides rendered for this target and scene");
  return MCPT_OK;
}

// the events of a select (and of the round before it), with a filter the filter's events and buffers
static int ensure_select(mcpt_ctx* c, const RunFilter* f) {
  HIP_OR_RETURN(ensure_timing_events(c->adaptive.ad_ev, 6));
  if (f) {
    HIP_OR_RETURN(ensure_denoise_buffers(c));
    HIP_OR_RETURN(ensure_timing_events(c->denoise.dn_ev, 10));
  }
  return MCPT_OK;
}

// The enqueue half, no host wait.  The raw rule: select_kernel<true> (the map, the record, the flags),
// then the scan.  The filtered rule: step A select_kernel<false>, the map and the raw
// record, no flag changes; step B denoise_run's resolved variance form on that map; step C
// filtered_select_kernel on the filter's result, then the scan.  The temporal rule:
// step A, step T temporal_select_kernel on that map and the history, then the scan.  timed: events
// [0, 1] around the raw rule (the temporal rule's steps A and T) and its scan, for the filtered rule
// [0, 1] around step A and [4, 5] around step C and the scan (mcpt_last_adaptive_ms); every
// precondition has been checked.
static int enqueue_select(mcpt_ctx* c, const SelectRule& r, const SelectDest& d, bool timed) {
  const RunFilter* f = r.f;
  const mcpt::AdaptiveTarget t = adaptive_target(c);
  int* d_count = c->adaptive.d_ad_list + c->adaptive.ad_n_blocks;
  if (timed) HIP_OR_RETURN(hipEventRecord(c->adaptive.ad_ev[0], c->stream));
  HIP_OR_RETURN(mcpt_launch_adaptive_select(t, c->stats.d_stats, c->stats.d_emap, c->stats.stats_passes, c->stats.stats_batches, r.mu_floor,
                                            r.threshold, c->adaptive.ad_min_passes, !f && !r.t, d.rec, c->stream));
  c->stats.emap_valid = true;
  if (r.t)   // step T: the dry run of the resolved accumulate on the map step A wrote (the own window's)
    HIP_OR_RETURN(mcpt_launch_temporal_select(
        t, temporal_params(c, c->stats.d_emap, r.t->prevPV16, r.t->max_history, r.t->plane_tol), r.mu_floor, r.threshold,
        c->adaptive.ad_min_passes, d.rec_f, c->stream));
  if (f) {
    if (timed) HIP_OR_RETURN(hipEventRecord(c->adaptive.ad_ev[1], c->stream));
    FilterForm form = kResolvedVariance;
    form.timed = timed;
    OK_OR_RETURN(denoise_run(c, f->iterations, f->k_color, f->sigma_plane, form));
    if (timed) HIP_OR_RETURN(hipEventRecord(c->adaptive.ad_ev[4], c->stream));
    HIP_OR_RETURN(mcpt_launch_adaptive_select_filtered(t, c->denoise.d_dn[c->denoise.dn_result], c->stats.d_emap, r.mu_floor, r.threshold,
                                                       f->raw_cap, c->adaptive.ad_min_passes, d.rec_f, c->stream));
  }
  HIP_OR_RETURN(mcpt_launch_adaptive_compact(t, c->adaptive.d_ad_list, d_count, c->stream));
  if (timed) {
    HIP_OR_RETURN(hipEventRecord(c->adaptive.ad_ev[f ? 5 : 1], c->stream));
    c->adaptive.ad_select_timed = true;
    c->adaptive.ad_select_split = f != nullptr;
  }
  if (d.len) HIP_OR_RETURN(hipMemcpyAsync(d.len, d_count, sizeof(int), hipMemcpyDeviceToDevice, c->stream));
  return MCPT_OK;
}

// The host half, from one select's reduced records (h; hf: the rule's second kernel's, step C's or
// step T's, read when o.filtered or o.temporal is given) and its list length: the length must be the
// flagged blocks the retiring kernel counted (its word 4); then the context's list length and the
// caller's record.
static int finish_select(mcpt_ctx* c, const unsigned long long* h, const unsigned long long* hf, int n_list,
                         const char* who, const SelectOut& o) {
  if (n_list < 0 || n_list > c->adaptive.ad_n_blocks || (unsigned long long)n_list != (o.filtered || o.temporal ? hf : h)[4])
    return refuse(MCPT_ERR_HIP, who, "the active list and the block flags disagree");
  c->adaptive.ad_n_list = n_list;
  fill_frame_record(c, h, o.raw);
  o.raw->n_active_blocks = n_list;
  o.raw->n_blocks = c->adaptive.ad_n_blocks;
  o.raw->samples = (long long)h[3];
  if (o.filtered) fill_filtered_record(c, hf, o.filtered);
  if (o.temporal) {   // step T's record: over the pixels of the blocks active on entry
    mcpt_adaptive_temporal_t* t = o.temporal;
    t->n_px_t = (long long)hf[3];
    t->n_above_t = (long long)hf[0];
    t->sum_qt = hf[1];
    const unsigned mb = (unsigned)(hf[2] & 0xffffffffull);
    std::memcpy(&t->max_rt, &mb, sizeof(float));
    t->mean_rt = t->n_px_t > 0 ? (double)hf[1] / 65536.0 / (double)t->n_px_t : 0.0;
    t->n_history = (long long)hf[5];
  }
  return MCPT_OK;
}

// one select now, into d_conv (and d_conv_f), one wait for its records.  Every precondition is checked
// before the enqueue, so a refusal leaves the flags, the map and the result buffers alone.
static int select_once(mcpt_ctx* c, const SelectRule& rule, const char* who, const SelectOut& o) {
  if (!c->adaptive.ad_on) return refuse(MCPT_ERR_NO_ADAPTIVE, who, "adaptive mode is off (mcpt_adaptive_begin)");
  OK_OR_RETURN(check_select_rule(c, rule, true, who));
  HIP_OR_RETURN(hipSetDevice(c->device));
  OK_OR_RETURN(ensure_select(c, rule.f));
  const bool two = rule.f || rule.t;   // the rule runs a second reducing kernel
  if (two) HIP_OR_RETURN(c->stats.d_conv_f.ensure(mcpt::kStatsRecWords));
  const SelectDest dest = {c->stats.d_conv, two ? c->stats.d_conv_f : nullptr, nullptr};
  OK_OR_RETURN(enqueue_select(c, rule, dest, true));
  unsigned long long h[6] = {0, 0, 0, 0, 0, 0}, hf[6] = {0, 0, 0, 0, 0, 0};
  int n_list = 0;
  OK_OR_RETURN(read_stats_records(c, 6, 2, dest.rec, h, dest.rec_f, hf, c->adaptive.d_ad_list + c->adaptive.ad_n_blocks, &n_list));
  return finish_select(c, h, hf, n_list, who, o);
}

int mcpt_adaptive_select(mcpt_ctx* c, float threshold, float mu_floor, mcpt_adaptive_t* out) {
  if (!c || !out) return mcpt_err_bare(MCPT_ERR_INVALID_ARG);
  return select_once(c, {threshold, mu_floor, nullptr}, "mcpt_adaptive_select", {out, nullptr, nullptr});
}

int mcpt_adaptive_select_filtered(mcpt_ctx* c, float threshold, float raw_cap, float mu_floor, int iterations,
                                  float k_color, float sigma_plane, mcpt_adaptive_filtered_t* out) {
  if (!c || !out) return mcpt_err_bare(MCPT_ERR_INVALID_ARG);
  const RunFilter f = {raw_cap, iterations, k_color, sigma_plane};
  return select_once(c, {threshold, mu_floor, &f}, "mcpt_adaptive_select_filtered", {&out->raw, out, nullptr});
}

int mcpt_adaptive_select_temporal(mcpt_ctx* c, const float* prevPV16, int max_history, float plane_tol, float threshold,
                                  float mu_floor, mcpt_adaptive_temporal_t* out) {
  if (!c || !out) return mcpt_err_bare(MCPT_ERR_INVALID_ARG);
  const RunTemporal t = {prevPV16, max_history, plane_tol};
  return select_once(c, {threshold, mu_floor, nullptr, &t}, "mcpt_adaptive_select_temporal", {&out->raw, nullptr, out});
}

int mcpt_read_active_blocks(mcpt_ctx* c, int* ids, int capacity, int* n) {
  if (!c || !n || (capacity > 0 && !ids) || capacity < 0) return mcpt_err_bare(MCPT_ERR_INVALID_ARG);
  if (!c->adaptive.ad_on) return set_err(MCPT_ERR_NO_ADAPTIVE, "mcpt_read_active_blocks: adaptive mode is off (mcpt_adaptive_begin)");
  HIP_OR_RETURN(hipSetDevice(c->device));
  *n = c->adaptive.ad_n_list;
  const int k = std::min(capacity, c->adaptive.ad_n_list);
  if (k > 0) HIP_OR_RETURN(hipMemcpyAsync(ids, c->adaptive.d_ad_list, sizeof(int) * (size_t)k, hipMemcpyDeviceToHost, c->stream));
  HIP_OR_RETURN(hipStreamSynchronize(c->stream));
  return MCPT_OK;
}

// The listed blocks' passes first_pass .. first_pass + n_passes - 1 on the context's stream (ordered
// after the render lanes): the scene's per-lane kernel's LIST twin, one segment per item, dispatch
// order.  No part in AUTO's trials, the item-cost sort, the render lanes or the timing ring.
// (adaptive_round: the round behind mcpt_render_adaptive and, counted, one round of a queued run,
// the grids hold the list's length on the host, c->adaptive.ad_n_list, the kernels read the
// length it has by then on the device, and the statistics' batch skips once it is 0; timed false:
// the round records no events)
static int check_render_adaptive(const mcpt_ctx* c, const float* invPV, const float* invV, int n_passes, int variant,
                                 const char* who) {
  const bool args_ok = invPV && invV && n_passes >= 0 && variant >= 0 && variant <= 2;
  if (c && args_ok && !c->adaptive.ad_on) return refuse(MCPT_ERR_NO_ADAPTIVE, who, "adaptive mode is off (mcpt_adaptive_begin)");
  return check_renderable(c, args_ok, who);
}
// the round's launch parameters except its pass range; returns the most segments a sub-launch holds
static long long adaptive_round_params(const mcpt_ctx* c, const float* invPV, const float* invV, bool counted,
                                       mcpt::RenderParams& p) {
  scene_params(c, invPV, invV, p);
  p.walk_exit = plan::resolve_walk_exit(c->walk_exit, c->meshes.n_meshes, c->depth);
  p.leaf_batch = plan::resolve_leaf_batch(c->leaf_batch, c->depth);
  p.walk_min_done = 1;
  p.seg_per_item = 1;
  p.list = c->adaptive.d_ad_list;
  p.n_list = counted ? -c->adaptive.ad_n_list : c->adaptive.ad_n_list;
  p.blocks_x = c->adaptive.ad_blocks_x;
  p.n_blocks = c->adaptive.ad_n_blocks;
  p.n_tiles = plan::run_list_groups(c->adaptive.ad_n_list, p.tile_w);   // workgroup groups of the list
  plan::LimitsIn lin;   // (no spare workgroups, no pass stealing)
  lin.n_local_px = p.n_local_px; lin.n_tiles = p.n_tiles; lin.tile_w = p.tile_w; lin.n_cu = c->n_cu;
  lin.partial_budget = c->partial_budget; lin.mesh = c->meshes.n_meshes > 0; lin.steal = false; lin.spare = false;
  return plan::limits(lin).max_seg;
}
static int adaptive_round(mcpt_ctx* c, const float* invPV, const float* invV, int first_pass, int n_passes, float date,
                          int bounces, float refract_ind, int variant, bool counted, bool timed) {
  HIP_OR_RETURN(hipSetDevice(c->device));
  mcpt::RenderParams p;
  const long long max_seg = adaptive_round_params(c, invPV, invV, counted, p);
  pass_params(first_pass, n_passes, date, bounces, refract_ind, variant, p);
  const size_t seg_bytes = (size_t)p.n_local_px * 3 * sizeof(float);
  if (timed) HIP_OR_RETURN(ensure_timing_events(c->adaptive.ad_ev + 2, 2));
  mcpt_ctx::Lane& L = c->lanes[0];   // its segment-sum buffer (free: `stream` is ordered after the lanes' work)
  if (timed) HIP_OR_RETURN(hipEventRecord(c->adaptive.ad_ev[2], c->stream));
  // sub-launches at chunk boundaries, as launch() cuts them (segment-sum budget, grid size)
  plan::SubLaunch sub;
  int k = 0;
  for (long long lo = first_pass, end = (long long)first_pass + n_passes; lo < end; lo = sub.end(), ++k) {
    sub = plan::next_sub_launch(lo, end, max_seg, false);
    p.first_pass = sub.first_pass; p.n_passes = sub.n_passes; p.n_segments = sub.n_segments;
    p.n_items = (int)((long long)p.n_tiles * p.n_segments);
    if (p.n_segments > 1) OK_OR_RETURN(ensure_lane_bytes(c, L.d_partial, (size_t)p.n_segments * seg_bytes));
    p.partial = L.d_partial;
    HIP_OR_RETURN(mcpt_launch_render_list(p, c->stream));
    HIP_OR_RETURN(mcpt_launch_combine_list(p, c->stream));
    c->seq.used_in_order(0);   // (the lane's next launch waits for `stream`'s work so far)
#ifdef MCPT_CHECKED
    OK_OR_RETURN(checked_sub_launch(c, k, -1, p));
#endif
  }
  (void)k;
  if (timed) {
    HIP_OR_RETURN(hipEventRecord(c->adaptive.ad_ev[3], c->stream));
    c->adaptive.ad_render_timed = true;
  }
  if (counted)
    HIP_OR_RETURN(mcpt_launch_adaptive_add_passes_counted(adaptive_target(c), c->adaptive.d_ad_list, c->adaptive.d_ad_list + c->adaptive.ad_n_blocks,
                                                          c->adaptive.ad_n_list, n_passes, c->stream));
  else
    HIP_OR_RETURN(mcpt_launch_adaptive_add_passes(adaptive_target(c), c->adaptive.d_ad_list, c->adaptive.ad_n_list, n_passes, c->stream));
  c->pass_count += n_passes;   // the active blocks' count: the largest
  if (c->stats.stats_on) HIP_OR_RETURN(stats_batch(c, n_passes, counted ? c->adaptive.d_ad_list + c->adaptive.ad_n_blocks : nullptr, timed));
  return MCPT_OK;
}

int mcpt_render_adaptive(mcpt_ctx* c, const float* invPV, const float* invV, int first_pass, int n_passes, float date,
                         int bounces, float refract_ind, int variant) {
  OK_OR_RETURN(check_render_adaptive(c, invPV, invV, n_passes, variant, "mcpt_render_adaptive"));
  invalidate_planes(c);   // (a gathered frame's counts do not describe what is rendered into it)
  if (c->adaptive.ad_n_list == 0 || n_passes == 0) return MCPT_OK;   // every block retired: nothing to launch
  return adaptive_round(c, invPV, invV, first_pass, n_passes, date, bounces, refract_ind, variant, false, true);
}

// ---- queued adaptive runs: `rounds` rounds of {the active blocks' passes, the
// statistics' batch, on the schedule's rounds a select and the scan} on the stream, every list length
// read on the device, one wait at the end for all the records.  f: the filtered rule's arguments, t:
// the temporal rule's (both null: mcpt_adaptive_select's rule); records: mcpt_adaptive_t or, with f,
// mcpt_adaptive_filtered_t, with t, mcpt_adaptive_temporal_t.
static int adaptive_run(mcpt_ctx* c, const float* invPV, const float* invV, int first_pass, int n_passes, int rounds,
                        int check_every, float threshold, float mu_floor, float date, int bounces, float refract_ind,
                        int variant, const RunFilter* f, const RunTemporal* t, void* records, int records_capacity,
                        mcpt_adaptive_run_t* out) {
  const char* who = t ? "mcpt_adaptive_run_temporal" : f ? "mcpt_adaptive_run_filtered" : "mcpt_adaptive_run";
  const SelectRule rule = {threshold, mu_floor, f, t};
  const bool two = f || t;   // the rule runs a second reducing kernel (step C, step T): the second ring
  // mcpt_render_adaptive's checks, then the select's, then the run's own: before anything is enqueued
  OK_OR_RETURN(check_render_adaptive(c, invPV, invV, n_passes, variant, who));
  if (!out) return mcpt_err_bare(MCPT_ERR_INVALID_ARG);
  OK_OR_RETURN(check_select_rule(c, rule, false, who));
  if (n_passes <= 0 || rounds < 1 || rounds > plan::kAdaptiveRunMaxRounds || check_every <= 0)
    return refuse(MCPT_ERR_INVALID_ARG, who, "n_passes and check_every must be positive, rounds in 1..256");
  const long long last_pass = (long long)first_pass + (long long)rounds * n_passes;
  if (last_pass > 0x7fffffffLL || (long long)c->pass_count + (long long)rounds * n_passes > 0x7fffffffLL)
    return refuse(MCPT_ERR_INVALID_ARG, who, "the run's passes do not fit the pass counters");
  const int n_sel = plan::run_select_count(rounds, check_every, c->stats.stats_batches);
  if (records_capacity < n_sel || (records_capacity > 0 && !records))
    return refuse(MCPT_ERR_INVALID_ARG, who, "records holds fewer selects than the schedule can run");
  std::memset(out, 0, sizeof(*out));
  out->rounds_queued = rounds;
  if (c->adaptive.ad_n_list == 0) return MCPT_OK;   // every block retired: the host loop stops before its first round

  HIP_OR_RETURN(hipSetDevice(c->device));
  OK_OR_RETURN(ensure_select(c, f));
  HIP_OR_RETURN(ensure_timing_events(c->stats.stats_ev, 2));
  HIP_OR_RETURN(ensure_timing_events(c->stats.run_ev, 2));
  const size_t ring_words = mcpt::kStatsRecWords * (size_t)plan::kAdaptiveRunMaxRounds;
  HIP_OR_RETURN(c->stats.d_run_rec.ensure(ring_words));
  HIP_OR_RETURN(c->stats.d_run_len.ensure((size_t)plan::kAdaptiveRunMaxRounds));
  if (two) HIP_OR_RETURN(c->stats.d_run_rec_f.ensure(ring_words));
  {   // the segment-sum buffer of the run's largest sub-launch now: growing it waits for the stream
    mcpt::RenderParams p;
    const long long max_seg = adaptive_round_params(c, invPV, invV, true, p);
    int most = 1;
    for (int i = 0; i < rounds; ++i) {
      plan::SubLaunch sub;
      for (long long lo = (long long)first_pass + (long long)i * n_passes, end = lo + n_passes; lo < end; lo = sub.end()) {
        sub = plan::next_sub_launch(lo, end, max_seg, false);
        most = std::max(most, sub.n_segments);
      }
    }
    mcpt_ctx::Lane& L = c->lanes[0];
    if (most > 1)
      OK_OR_RETURN(ensure_lane_bytes(c, L.d_partial, (size_t)most * (size_t)p.n_local_px * 3 * sizeof(float)));
  }

  const int list_in = c->adaptive.ad_n_list, pass_in = c->pass_count, batches_in = c->stats.stats_batches;
  const long long window_in = c->stats.stats_passes;
  const bool emap_in = c->stats.emap_valid;
  int sel_round[plan::kAdaptiveRunMaxRounds];
  invalidate_planes(c);
  HIP_OR_RETURN(hipEventRecord(c->stats.run_ev[0], c->stream));
  int k = 0;
  for (int i = 0; i < rounds; ++i) {
    OK_OR_RETURN(adaptive_round(c, invPV, invV, first_pass + i * n_passes, n_passes, date, bounces, refract_ind, variant,
                                true, i == rounds - 1));
    if (!plan::run_round_selects(i, rounds, check_every, batches_in)) continue;
    const size_t slot = (size_t)k * mcpt::kStatsRecWords;   // the select's own slices of the rings
    const SelectDest dest = {c->stats.d_run_rec + slot, two ? c->stats.d_run_rec_f + slot : nullptr, c->stats.d_run_len + k};
    OK_OR_RETURN(enqueue_select(c, rule, dest, k == n_sel - 1));   // (events around the run's last select only)
    sel_round[k++] = i;
  }
  HIP_OR_RETURN(hipEventRecord(c->stats.run_ev[1], c->stream));
  std::vector<unsigned long long> part((size_t)k * mcpt::kStatsRecWords), part_f(two ? part.size() : 0);
  std::vector<int> len((size_t)k);
  if (k > 0) {
    HIP_OR_RETURN(hipMemcpyAsync(part.data(), c->stats.d_run_rec, part.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
    if (two)
      HIP_OR_RETURN(hipMemcpyAsync(part_f.data(), c->stats.d_run_rec_f, part_f.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
    HIP_OR_RETURN(hipMemcpyAsync(len.data(), c->stats.d_run_len, len.size() * sizeof(int), hipMemcpyDeviceToHost, c->stream));
  }
  HIP_OR_RETURN(hipStreamSynchronize(c->stream));   // the run's one wait
  HIP_OR_RETURN(hipEventElapsedTime(&out->device_ms, c->stats.run_ev[0], c->stats.run_ev[1]));

  // what the host loop would have done (mcpt_adaptive_run_plan.h): the rounds after the list emptied
  // changed nothing on the device, and the host's counters follow the rounds that ran
  const plan::RunOutcome o = plan::run_outcome(rounds, check_every, batches_in, list_in, len.data(), k);
  c->pass_count = pass_in + o.rounds_run * n_passes;
  c->stats.stats_passes = window_in + (long long)o.rounds_run * n_passes;
  c->stats.stats_batches = batches_in + o.rounds_run;
  c->stats.emap_valid = emap_in || o.selects_run > 0;
  out->rounds_run = o.rounds_run;
  out->selects_run = o.selects_run;
  out->passes_run = (long long)o.rounds_run * n_passes;
  int status = MCPT_OK;
  for (int s = 0; s < o.selects_run; ++s) {
    unsigned long long h[6] = {0, 0, 0, 0, 0, 0}, hf[6] = {0, 0, 0, 0, 0, 0};
    reduce_stats_records(part.data() + (size_t)s * mcpt::kStatsRecWords, 6, 2, h);
    if (two) reduce_stats_records(part_f.data() + (size_t)s * mcpt::kStatsRecWords, 6, 2, hf);
    mcpt_adaptive_filtered_t* filtered = f ? &static_cast<mcpt_adaptive_filtered_t*>(records)[s] : nullptr;
    mcpt_adaptive_temporal_t* temporal = t ? &static_cast<mcpt_adaptive_temporal_t*>(records)[s] : nullptr;
    mcpt_adaptive_t* raw = f ? &filtered->raw : t ? &temporal->raw : &static_cast<mcpt_adaptive_t*>(records)[s];
    status = finish_select(c, h, hf, len[(size_t)s], who, {raw, filtered, temporal});
    if (status != MCPT_OK) break;
    raw->passes = window_in + (long long)(sel_round[s] + 1) * n_passes;   // (the window as that select saw it)
    raw->batches = batches_in + sel_round[s] + 1;
  }
  return status;
}

int mcpt_adaptive_run(mcpt_ctx* c, const float* invPV, const float* invV, int first_pass, int n_passes, int rounds,
                      int check_every, float threshold, float mu_floor, float date, int bounces, float refract_ind,
                      int variant, mcpt_adaptive_t* records, int records_capacity, mcpt_adaptive_run_t* out) {
  return adaptive_run(c, invPV, invV, first_pass, n_passes, rounds, check_every, threshold, mu_floor, date, bounces,
                      refract_ind, variant, nullptr, nullptr, records, records_capacity, out);
}

int mcpt_adaptive_run_filtered(mcpt_ctx* c, const float* invPV, const float* invV, int first_pass, int n_passes,
                               int rounds, int check_every, float threshold, float raw_cap, float mu_floor,
                               int iterations, float k_color, float sigma_plane, float date, int bounces,
                               float refract_ind, int variant, mcpt_adaptive_filtered_t* records, int records_capacity,
                               mcpt_adaptive_run_t* out) {
  const RunFilter f = {raw_cap, iterations, k_color, sigma_plane};
  return adaptive_run(c, invPV, invV, first_pass, n_passes, rounds, check_every, threshold, mu_floor, date, bounces,
                      refract_ind, variant, &f, nullptr, records, records_capacity, out);
}

int mcpt_adaptive_run_temporal(mcpt_ctx* c, const float* invPV, const float* invV, int first_pass, int n_passes,
                               int rounds, int check_every, float threshold, float mu_floor, const float* prevPV16,
                               int max_history, float plane_tol, float date, int bounces, float refract_ind, int variant,
                               mcpt_adaptive_temporal_t* records, int records_capacity, mcpt_adaptive_run_t* out) {
  const RunTemporal t = {prevPV16, max_history, plane_tol};
  return adaptive_run(c, invPV, invV, first_pass, n_passes, rounds, check_every, threshold, mu_floor, date, bounces,
                      refract_ind, variant, nullptr, &t, records, records_capacity, out);
}

int mcpt_adaptive_until_next(int done, int calls, int batch, int max_passes, int check_every, int queued_rounds,
                             int* rounds, int* n_passes, int* select) {
  if (!plan::until_next(done, calls, batch, max_passes, check_every, queued_rounds, rounds, n_passes, select))
    return set_err(MCPT_ERR_INVALID_ARG, "mcpt_adaptive_until_next: bad arguments");
  return MCPT_OK;
}

// every local pixel's sample count (mcpt_read_sample_counts) or, resolved, its accum / (float)count
// (mcpt_read_resolved), through a device buffer of the call's own, on the host
static int read_counted(mcpt_ctx* c, void* out, bool resolved, const char* who) {
  if (!c || !out) return mcpt_err_bare(MCPT_ERR_INVALID_ARG);
  if (!has_pixel_counts(c)) return refuse(MCPT_ERR_NO_ADAPTIVE, who, "adaptive mode is off (mcpt_adaptive_begin)");
  HIP_OR_RETURN(hipSetDevice(c->device));
  const size_t n = (size_t)c->n_local_rows * c->W, bytes = n * (resolved ? 3 * sizeof(float) : sizeof(int));
  if (n) {
    DevBuf<char> scratch;
    HIP_OR_RETURN(scratch.alloc(bytes));
    void* d = scratch;
    hipError_t e = resolved ? mcpt_launch_resolve(count_source(c), c->target.d_accum, (float*)d, (long long)n, c->stream)
                            : mcpt_launch_counts(count_source(c), (int*)d, (long long)n, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(out, d, bytes, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) return set_err(MCPT_ERR_HIP, who, e);
  }
  return MCPT_OK;
}

int mcpt_read_sample_counts(mcpt_ctx* c, int* counts) { return read_counted(c, counts, false, "mcpt_read_sample_counts"); }

int mcpt_read_resolved(mcpt_ctx* c, float* rgb) { return read_counted(c, rgb, true, "mcpt_read_resolved"); }

// ---- checkpoint / resume of an adaptive render (the file layer: mcpt_image.cpp)
int mcpt_adaptive_checkpoint_save(mcpt_ctx* c, const char* path, int next_pass, const char* tag) {
  if (!c || !path) return mcpt_err_bare(MCPT_ERR_INVALID_ARG);
  if (!c->has_target) return mcpt_err_bare(MCPT_ERR_NO_TARGET);
  if (!c->adaptive.ad_on) return set_err(MCPT_ERR_NO_ADAPTIVE, "mcpt_adaptive_checkpoint_save: adaptive mode is off (mcpt_adaptive_begin)");
  HIP_OR_RETURN(hipSetDevice(c->device));
  const size_t n = (size_t)c->n_local_rows * c->W, nb = (size_t)c->adaptive.ad_n_blocks;
  std::vector<float> acc(n * 3), stats(n * 4), emap(n * 2);
  std::vector<int> flags(nb), passes(nb);
  if (n) {
    HIP_OR_RETURN(hipMemcpyAsync(acc.data(), c->target.d_accum, n * 3 * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    HIP_OR_RETURN(hipMemcpyAsync(stats.data(), c->stats.d_stats, n * sizeof(float4), hipMemcpyDeviceToHost, c->stream));
    HIP_OR_RETURN(hipMemcpyAsync(emap.data(), c->stats.d_emap, n * sizeof(float2), hipMemcpyDeviceToHost, c->stream));
  }
  if (nb) {
    HIP_OR_RETURN(hipMemcpyAsync(flags.data(), c->adaptive.d_ad_flags, nb * sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIP_OR_RETURN(hipMemcpyAsync(passes.data(), c->adaptive.d_ad_passes, nb * sizeof(int), hipMemcpyDeviceToHost, c->stream));
  }
  HIP_OR_RETURN(hipStreamSynchronize(c->stream));
  mcpt_adaptive_checkpoint_t h;
  std::memset(&h, 0, sizeof(h));
  h.W = c->W; h.rows = c->n_local_rows; h.pass_count = c->pass_count; h.next_pass = next_pass; h.H = c->H;
  h.rows_hash = rows_hash(c);
  h.p0 = c->adaptive.ad_p0; h.min_passes = c->adaptive.ad_min_passes;
  h.stats_passes = c->stats.stats_passes; h.stats_batches = c->stats.stats_batches; h.emap_valid = c->stats.emap_valid ? 1 : 0;
  h.n_blocks = c->adaptive.ad_n_blocks; h.blocks_x = c->adaptive.ad_blocks_x;
  if (mcpt_adaptive_checkpoint_write(path, &h, tag, flags.data(), passes.data(), acc.data(), stats.data(), emap.data()) !=
      MCPT_OK)
    return set_err(MCPT_ERR_INVALID_ARG, "mcpt_adaptive_checkpoint_save: cannot write the file");
  return MCPT_OK;
}

int mcpt_adaptive_checkpoint_load(mcpt_ctx* c, const char* path, const char* tag, int* next_pass) {
  if (!c || !path) return mcpt_err_bare(MCPT_ERR_INVALID_ARG);
  if (!c->has_target) return mcpt_err_bare(MCPT_ERR_NO_TARGET);
  const size_t n = (size_t)c->n_local_rows * c->W;
  const size_t nb = (size_t)((c->W + 7) / 8) * (size_t)((c->n_local_rows + 7) / 8);
  std::vector<float> acc(n * 3), stats(n * 4), emap(n * 2);
  std::vector<int> flags(nb), passes(nb);
  std::vector<char> t(MCPT_CHECKPOINT_TAG_MAX);
  mcpt_adaptive_checkpoint_t h;
  if (mcpt_adaptive_checkpoint_read(path, &h, t.data(), flags.data(), passes.data(), (long long)nb, acc.data(),
                                    stats.data(), emap.data(), (long long)n) != MCPT_OK)
    return set_err(MCPT_ERR_INVALID_ARG, "mcpt_checkpoint_load: missing, foreign or truncated file, or not this target's size");
  if (h.H == 0 || h.rows_hash == 0)
    return set_err(MCPT_ERR_INVALID_ARG,
                   "mcpt_checkpoint_load: the file carries no target identity (mcpt_checkpoint_write); "
                   "read it with mcpt_checkpoint_read and load it with mcpt_write_accum");
  if (h.W != c->W || h.rows != c->n_local_rows || h.H != c->H || h.rows_hash != rows_hash(c))
    return set_err(MCPT_ERR_INVALID_ARG, "mcpt_checkpoint_load: the checkpoint belongs to another target or shard");
  if (tag && std::strcmp(tag, t.data()) != 0)
    return set_err(MCPT_ERR_INVALID_ARG, "mcpt_checkpoint_load: the render parameters differ (tag)");
  OK_OR_RETURN(mcpt_write_accum(c, acc.data(), h.pass_count));   // (waits for the stream's queued work)
  HIP_OR_RETURN(hipSetDevice(c->device));
  // statistics and the adaptive mode on in the saved state: the buffers mcpt_stats_begin /
  // mcpt_adaptive_begin allocate, the list from the flags by the select's scan
  OK_OR_RETURN(ensure_stats_buffers(c));
  OK_OR_RETURN(ensure_adaptive_buffers(c));
  if (n) {
    HIP_OR_RETURN(hipMemcpyAsync(c->stats.d_stats, stats.data(), n * sizeof(float4), hipMemcpyHostToDevice, c->stream));
    HIP_OR_RETURN(hipMemcpyAsync(c->stats.d_emap, emap.data(), n * sizeof(float2), hipMemcpyHostToDevice, c->stream));
  }
  if (nb) {
    HIP_OR_RETURN(hipMemcpyAsync(c->adaptive.d_ad_flags, flags.data(), nb * sizeof(int), hipMemcpyHostToDevice, c->stream));
    HIP_OR_RETURN(hipMemcpyAsync(c->adaptive.d_ad_passes, passes.data(), nb * sizeof(int), hipMemcpyHostToDevice, c->stream));
  }
  c->stats.stats_on = true;
  c->stats.stats_passes = h.stats_passes;
  c->stats.stats_batches = h.stats_batches;
  c->stats.emap_valid = h.emap_valid != 0;
  c->adaptive.ad_p0 = h.p0;
  c->adaptive.ad_min_passes = h.min_passes;
  int* d_count = c->adaptive.d_ad_list + c->adaptive.ad_n_blocks;
  int n_list = 0;
  HIP_OR_RETURN(mcpt_launch_adaptive_compact(adaptive_target(c), c->adaptive.d_ad_list, d_count, c->stream));
  HIP_OR_RETURN(hipMemcpyAsync(&n_list, d_count, sizeof(int), hipMemcpyDeviceToHost, c->stream));
  HIP_OR_RETURN(hipStreamSynchronize(c->stream));   // (the host arrays are read until here)
  if (n_list < 0 || n_list > c->adaptive.ad_n_blocks) {
    c->adaptive = {};
    return set_err(MCPT_ERR_HIP, "mcpt_adaptive_checkpoint_load: the rebuilt active list is out of range");
  }
  c->adaptive.ad_n_list = n_list;
  c->adaptive.ad_on = true;
  if (next_pass) *next_pass = h.next_pass;
  return MCPT_OK;
}

int mcpt_last_adaptive_ms(mcpt_ctx* c, float* select_ms, float* render_ms) {
  if (!c) return mcpt_err_bare(MCPT_ERR_INVALID_ARG);
  HIP_OR_RETURN(hipSetDevice(c->device));
  OK_OR_RETURN(pair_ms(c->adaptive.ad_select_timed, c->adaptive.ad_ev[0], c->adaptive.ad_ev[1], select_ms));
  if (select_ms && c->adaptive.ad_select_timed && c->adaptive.ad_select_split) {   // a filtered select: steps A + C, not the filter between
    float tail = 0.0f;
    OK_OR_RETURN(pair_ms(true, c->adaptive.ad_ev[4], c->adaptive.ad_ev[5], &tail));
    *select_ms += tail;
  }
  return pair_ms(c->adaptive.ad_render_timed, c->adaptive.ad_ev[2], c->adaptive.ad_ev[3], render_ms);
}

// ---- the held error map's source and record (mcpt_ctx.h: held_error_map)
int mcpt_error_map_source(mcpt_ctx* c, int* source) {
  if (!c || !source) return mcpt_err_bare(MCPT_ERR_INVALID_ARG);
  *source = error_map_source(c);
  return MCPT_OK;
}

int mcpt_error_map_record(mcpt_ctx* c, float threshold, mcpt_convergence_t* out) {
  if (!c || !out) return mcpt_err_bare(MCPT_ERR_INVALID_ARG);
  if (!positive_finite({threshold}))
    return set_err(MCPT_ERR_INVALID_ARG, "mcpt_error_map_record: threshold must be positive and finite");
  const int source = error_map_source(c);
  if (source == 0) return set_err(MCPT_ERR_NO_STATS, "mcpt_error_map_record: no error map (gathered or of the current statistics)");
  HIP_OR_RETURN(hipSetDevice(c->device));
  HIP_OR_RETURN(c->planes.d_emap_rec.ensure(mcpt::kStatsRecWords));
  const long long n = (long long)c->n_local_rows * c->W;
  HIP_OR_RETURN(mcpt_launch_error_map_record(held_error_map(c), n, threshold, c->planes.d_emap_rec, c->stream));
  unsigned long long h[3] = {0, 0, 0};
  OK_OR_RETURN(read_stats_records(c, 3, 2, c->planes.d_emap_rec, h));
  fill_frame_record(c, h, out);
  if (source == 2) {   // (a gathered map belongs to no window of this context)
    out->passes = c->pass_count;
    out->batches = 0;
  }
  return MCPT_OK;
}

// ---- temporal reprojection (mcpt_temporal.hip)
// which form keeps the history's guides when MCPT_TEMPORAL_COPY is unset: 0 the ping-pong (the
// kernel writes them), 1 a device copy behind the kernel (the A/B: tools/temporal_bench.py,
// profiles/temporal_bench.json); read by mcpt_temporal_begin when it allocates
constexpr int kTemporalCopyDefault = 0;

int mcpt_temporal_begin(mcpt_ctx* c) {
  if (!c) return mcpt_err_bare(MCPT_ERR_INVALID_ARG);
  if (!c->has_target) return set_err(MCPT_ERR_NO_TARGET, "no render target");
  HIP_OR_RETURN(hipSetDevice(c->device));
  if (!c->temporal.d_tp_rec) {
    const size_t n = (size_t)c->n_local_rows * c->W;
    mcpt_ctx::Temporal g;
    g.tp_copy = env_int("MCPT_TEMPORAL_COPY", kTemporalCopyDefault) != 0;
    hipError_t e = g.d_tp_rec.alloc(mcpt::kStatsRecWords);
    for (int k = 0; k < 2 && e == hipSuccess && n; ++k) {
      e = g.d_tp_c[k].alloc(n);
      if (e == hipSuccess) e = g.d_tp_len[k].alloc(n);
      if (e == hipSuccess && (k == 0 || !g.tp_copy)) e = g.d_tp_g[k].alloc(n * 2);
    }
    if (e != hipSuccess) return set_err(MCPT_ERR_HIP, "mcpt_temporal_begin: allocation", e);
    c->temporal = std::move(g);
  }
  c->temporal.tp_on = true;
  c->temporal.tp_frames = 0;
  return MCPT_OK;
}

int mcpt_temporal_end(mcpt_ctx* c) {
  if (!c) return mcpt_err_bare(MCPT_ERR_INVALID_ARG);
  HIP_OR_RETURN(hipSetDevice(c->device));
  if (c->temporal.d_tp_rec) HIP_OR_RETURN(hipStreamSynchronize(c->stream));   // (a queued filter still reads the history)
  c->temporal = {};
  return MCPT_OK;
}

int mcpt_temporal_info(mcpt_ctx* c, int* on, int* history_valid, long long* frames) {
  if (!c) return mcpt_err_bare(MCPT_ERR_INVALID_ARG);
  if (on) *on = c->temporal.tp_on ? 1 : 0;
  if (history_valid) *history_valid = c->temporal.tp_on && c->temporal.tp_frames > 0 ? 1 : 0;
  if (frames) *frames = c->temporal.tp_on ? c->temporal.tp_frames : 0;
  return MCPT_OK;
}

// one accumulate behind mcpt_temporal_accumulate and, resolved, mcpt_temporal_accumulate_resolved
// (DESIGN.md §3.10.1): the current colour accum / (float)count with every pixel's own count, retired
// blocks allowed
static int temporal_accumulate(mcpt_ctx* c, const float* prevPV16, int max_history, float plane_tol,
                               mcpt_temporal_t* out, bool resolved, const char* who) {
  if (!c) return mcpt_err_bare(MCPT_ERR_INVALID_ARG);
  if (!c->temporal.tp_on) return refuse(MCPT_ERR_NO_TEMPORAL, who, "temporal mode is off (mcpt_temporal_begin)");
  if (resolved && !c->adaptive.ad_on) return refuse(MCPT_ERR_NO_ADAPTIVE, who, "adaptive mode is off (mcpt_adaptive_begin)");
  if (!out) return mcpt_err_bare(MCPT_ERR_INVALID_ARG);
  if (max_history < 1 || max_history > MCPT_TEMPORAL_MAX_HISTORY)
    return refuse(MCPT_ERR_INVALID_ARG, who, "max_history not in 1..65535");
  if (!positive_finite({plane_tol})) return refuse(MCPT_ERR_INVALID_ARG, who, "plane_tol must be positive and finite");
  const bool empty = c->temporal.tp_frames == 0;
  if (!empty && !prevPV16) return refuse(MCPT_ERR_INVALID_ARG, who, "the history needs the previous camera's P*V");
  if (!plan::is_full_frame(c->rows, c->H))
    return refuse(MCPT_ERR_INVALID_ARG, who, "needs a full-frame target (gather the shards first)");
  if (c->pass_count <= 0) return refuse(MCPT_ERR_INVALID_ARG, who, "the accumulator holds no passes");
  if (c->planes.plane_valid) return refuse(MCPT_ERR_INVALID_ARG, who, "the context holds a gathered frame's counts");
  if (!resolved && c->adaptive.ad_on && c->adaptive.ad_n_list < c->adaptive.ad_n_blocks)
    return refuse(MCPT_ERR_INVALID_ARG, who, "adaptive mode has retired blocks (per-pixel sample counts)");
  const float2* emap = held_error_map(c);
  if (error_map_source(c) == 0)
    return refuse(MCPT_ERR_NO_STATS, who, "no error map (mcpt_convergence) of the current statistics");
  if (!c->denoise.guides_valid) return refuse(MCPT_ERR_NO_GUIDES, who, "no guides rendered for this target and scene");
  HIP_OR_RETURN(hipSetDevice(c->device));
  HIP_OR_RETURN(ensure_timing_events(c->temporal.tp_ev, 3));
  const mcpt::TemporalParams p = temporal_params(c, emap, prevPV16, max_history, plane_tol);
  const size_t n = (size_t)c->H * c->W;
  // (the context's stream is ordered after all queued renders: their combines run on it)
  // (the record is zeroed before the timed interval: the events enclose the kernel alone)
  HIP_OR_RETURN(hipMemsetAsync(c->temporal.d_tp_rec, 0, sizeof(unsigned long long) * mcpt::kStatsRecWords, c->stream));
  HIP_OR_RETURN(hipEventRecord(c->temporal.tp_ev[0], c->stream));
  HIP_OR_RETURN(mcpt_launch_temporal(p, resolved, c->stream));
  HIP_OR_RETURN(hipEventRecord(c->temporal.tp_ev[1], c->stream));
  if (c->temporal.tp_copy) {
    if (n)
      HIP_OR_RETURN(hipMemcpyAsync(c->temporal.d_tp_g[0], c->denoise.d_guide, n * 2 * sizeof(float4), hipMemcpyDeviceToDevice, c->stream));
    HIP_OR_RETURN(hipEventRecord(c->temporal.tp_ev[2], c->stream));
  }
  c->temporal.tp_cur ^= 1;
  c->temporal.tp_frames += 1;
  c->temporal.tp_timed = true;
  unsigned long long h[6] = {0, 0, 0, 0, 0, 0};   // (word 5: the longest history, a maximum)
  OK_OR_RETURN(read_stats_records(c, 6, 5, c->temporal.d_tp_rec, h));
  out->n_px = (long long)n;
  out->n_history = (long long)h[0];
  out->n_miss = (long long)h[1];
  out->n_offscreen = (long long)h[2];
  out->n_rejected = (long long)h[3];
  out->n_new = out->n_miss + out->n_offscreen + out->n_rejected;
  out->sum_len = (long long)h[4];
  out->max_len = (int)h[5];
  out->frames = c->temporal.tp_frames;
  return MCPT_OK;
}

int mcpt_temporal_accumulate(mcpt_ctx* c, const float* prevPV16, int max_history, float plane_tol,
                             mcpt_temporal_t* out) {
  return temporal_accumulate(c, prevPV16, max_history, plane_tol, out, false, "mcpt_temporal_accumulate");
}

int mcpt_temporal_accumulate_resolved(mcpt_ctx* c, const float* prevPV16, int max_history, float plane_tol,
                                      mcpt_temporal_t* out) {
  return temporal_accumulate(c, prevPV16, max_history, plane_tol, out, true, "mcpt_temporal_accumulate_resolved");
}

int mcpt_denoise_temporal(mcpt_ctx* c, int iterations, float k_color, float sigma_plane) {
  if (!c) return mcpt_err_bare(MCPT_ERR_INVALID_ARG);
  if (!c->temporal.tp_on) return set_err(MCPT_ERR_NO_TEMPORAL, "mcpt_denoise_temporal: temporal mode is off (mcpt_temporal_begin)");
  if (iterations < 0 || iterations > 8) return set_err(MCPT_ERR_INVALID_ARG, "mcpt_denoise_temporal: iterations not in 0..8");
  if (!positive_finite({k_color, sigma_plane}))
    return set_err(MCPT_ERR_INVALID_ARG, "mcpt_denoise_temporal: k_color and sigma_plane must be positive and finite");
  if (c->temporal.tp_frames == 0)
    return set_err(MCPT_ERR_NO_STATS, "mcpt_denoise_temporal: the history is empty (mcpt_temporal_accumulate)");
  if (!c->denoise.guides_valid) return set_err(MCPT_ERR_NO_GUIDES, "mcpt_denoise_temporal: no guides rendered for this target and scene");
  HIP_OR_RETURN(hipSetDevice(c->device));
  HIP_OR_RETURN(ensure_denoise_buffers(c));
  HIP_OR_RETURN(ensure_timing_events(c->denoise.dn_ev, 10));
  const bool naive = env_int("MCPT_DENOISE_NAIVE", kAtrousNaiveDefault) != 0;
  HIP_OR_RETURN(hipEventRecord(c->denoise.dn_ev[9], c->stream));
  HIP_OR_RETURN(mcpt_launch_temporal_init(c->temporal.d_tp_c[c->temporal.tp_cur], c->denoise.d_dn[0], c->denoise.d_guide, c->W, c->H, c->stream));
  HIP_OR_RETURN(hipEventRecord(c->denoise.dn_ev[0], c->stream));
  // (the variance form's iterations on the history: guided, the variance filtered along, timed)
  return atrous_iterations(c, iterations, k_color, sigma_plane, kVariance, nullptr, naive);
}

int mcpt_read_temporal(mcpt_ctx* c, float* rgbv4, int* history_len) {
  if (!c) return mcpt_err_bare(MCPT_ERR_INVALID_ARG);
  if (!c->temporal.tp_on) return set_err(MCPT_ERR_NO_TEMPORAL, "mcpt_read_temporal: temporal mode is off (mcpt_temporal_begin)");
  if (c->temporal.tp_frames == 0) return set_err(MCPT_ERR_NO_STATS, "mcpt_read_temporal: the history is empty (mcpt_temporal_accumulate)");
  HIP_OR_RETURN(hipSetDevice(c->device));
  const size_t n = (size_t)c->n_local_rows * c->W;
  if (rgbv4 && n)
    HIP_OR_RETURN(hipMemcpyAsync(rgbv4, c->temporal.d_tp_c[c->temporal.tp_cur], n * sizeof(float4), hipMemcpyDeviceToHost, c->stream));
  if (history_len && n)
    HIP_OR_RETURN(hipMemcpyAsync(history_len, c->temporal.d_tp_len[c->temporal.tp_cur], n * sizeof(int), hipMemcpyDeviceToHost, c->stream));
  HIP_OR_RETURN(hipStreamSynchronize(c->stream));
  return MCPT_OK;
}

int mcpt_last_temporal_ms(mcpt_ctx* c, float* accumulate_ms, float* copy_ms) {
  if (!c) return mcpt_err_bare(MCPT_ERR_INVALID_ARG);
  if (!c->temporal.tp_on) return set_err(MCPT_ERR_NO_TEMPORAL, "mcpt_last_temporal_ms: temporal mode is off (mcpt_temporal_begin)");
  HIP_OR_RETURN(hipSetDevice(c->device));
  OK_OR_RETURN(pair_ms(c->temporal.tp_timed, c->temporal.tp_ev[0], c->temporal.tp_ev[1], accumulate_ms));
  return pair_ms(c->temporal.tp_timed && c->temporal.tp_copy, c->temporal.tp_ev[1], c->temporal.tp_ev[2], copy_ms);   // (ping-pong: no copy, 0)
}

// channels first .. first + n_ch - 1 of the last filter run's result d_dn[dn_result], packed
static int read_denoised_channels(mcpt_ctx* c, int first, int n_ch, float* out) {
  HIP_OR_RETURN(hipSetDevice(c->device));
  const size_t n = (size_t)c->n_local_rows * c->W;
  std::vector<float> h(n * 4);
  if (n) HIP_OR_RETURN(hipMemcpyAsync(h.data(), c->denoise.d_dn[c->denoise.dn_result], n * sizeof(float4), hipMemcpyDeviceToHost, c->stream));
  HIP_OR_RETURN(hipStreamSynchronize(c->stream));
  for (size_t i = 0; i < n; ++i)
    for (int k = 0; k < n_ch; ++k) out[(size_t)n_ch * i + k] = h[4 * i + first + k];
  return MCPT_OK;
}

int mcpt_read_denoised(mcpt_ctx* c, float* rgb_out) {
  if (!c || !rgb_out) return mcpt_err_bare(MCPT_ERR_INVALID_ARG);
  if (!c->has_target) return mcpt_err_bare(MCPT_ERR_NO_TARGET);
  if (c->denoise.dn_result < 0) return set_err(MCPT_ERR_INVALID_ARG, "mcpt_read_denoised: no mcpt_denoise on this target yet");
  return read_denoised_channels(c, 0, 3, rgb_out);
}

int mcpt_read_denoised_variance(mcpt_ctx* c, float* v_out) {
  if (!c || !v_out) return mcpt_err_bare(MCPT_ERR_INVALID_ARG);
  if (!c->has_target) return mcpt_err_bare(MCPT_ERR_NO_TARGET);
  if (c->denoise.dn_result < 0 || !c->denoise.dn_variance)
    return set_err(MCPT_ERR_NO_STATS, "mcpt_read_denoised_variance: the last filter run was no mcpt_denoise_variance");
  return read_denoised_channels(c, 3, 1, v_out);
}

int mcpt_last_denoise_ms(mcpt_ctx* c, float* guides_ms, float* filter_ms) {
  if (!c) return mcpt_err_bare(MCPT_ERR_INVALID_ARG);
  HIP_OR_RETURN(hipSetDevice(c->device));
  OK_OR_RETURN(pair_ms(c->denoise.guides_timed, c->denoise.guide_ev[0], c->denoise.guide_ev[1], guides_ms));
  // (the average and every iteration)
  return pair_ms(c->denoise.dn_iters >= 0, c->denoise.dn_ev[9], c->denoise.dn_ev[std::max(c->denoise.dn_iters, 0)], filter_ms);
}

int mcpt_last_denoise_path(mcpt_ctx* c, int* lds_mask) {
  if (!c || !lds_mask || c->denoise.dn_iters < 0) return mcpt_err_bare(MCPT_ERR_INVALID_ARG);
  *lds_mask = c->denoise.dn_lds_mask;
  return MCPT_OK;
}

int mcpt_denoise_iteration_ms(mcpt_ctx* c, int iteration, float* ms) {
  if (!c || !ms || iteration < -1 || iteration >= c->denoise.dn_iters) return mcpt_err_bare(MCPT_ERR_INVALID_ARG);
  HIP_OR_RETURN(hipSetDevice(c->device));
  hipEvent_t a = iteration < 0 ? c->denoise.dn_ev[9] : c->denoise.dn_ev[iteration], b = c->denoise.dn_ev[iteration + 1];
  HIP_OR_RETURN(hipEventSynchronize(b));
  HIP_OR_RETURN(hipEventElapsedTime(ms, a, b));
  return MCPT_OK;
}

}  // extern "C"
