// mcpt_render — headless entry point of the MI355X path tracer (the montecarlo.cpp main,
// MontecarloGPU/montecarlo.cpp:797-803, without the GL window).
//
// Builds one of the 8 reference scenes (keys Q..I = 1..8), accumulates passes with the
// reference's uniform ABI (numero_pass, date, NB_BOUNCES, refract_ind, shader variant),
// progressively in chunks like the "lock" mode (optionally writing a checkpoint after each
// chunk, and resuming from one), then writes the averaged image (fs_frag,
// montecarlo.cpp:59-70) as PFM (float) and/or PNG (8-bit framebuffer view).  Prints one JSON
// line with the timing.  Host C++ over the C ABI (include/mcpt.hpp); no CPU fallback.
//
// Several GPUs (--devices 0,1,...,7): one context and one host thread per device, each
// rendering its rows of the balanced row partition (mcpt_balanced_rows) for all
// passes; the shards' rows are then copied device to device into a full frame on the first
// device (mcpt_gather_rows: peer copies over xGMI — no collective on the data path).  The
// bits equal the one-GPU render's.  A device may be listed more than once (shards sharing a
// GPU: the 1-GPU rehearsal of the N-GPU path).
//
//   mcpt_render --scene 6 --width 1920 --height 1080 --spp 256 --bounces 8 --out s6.png
//   mcpt_render --scene 8 --width 1920 --height 1080 --spp 512 --bounces 12 --devices 0,1,2,3,4,5,6,7
//   mcpt_render --scene 6 --spp 16 --denoise --aov s6 --out s6_denoised.png   (a-trous filter + guide AOVs)
//   mcpt_render --scene 6 --spp 4096 --chunk 32 --target-error 0.02 --out s6.png   (stop at 2 % mean relative error)
//   mcpt_render --scene 6 --spp 4096 --chunk 32 --adaptive --target-error 0.05 --denoise 3 --checkpoint s6.ckpt
//   mcpt_render --scene 6 --spp 4096 --chunk 32 --adaptive --target-error 0.05 --devices 0,1,2,3 --aov s6
//   mcpt_render --scene 8 --spp 512 --chunk 32 --devices 0,1,2,3 --denoise-guided 3 --out s8.png   (the shards'
//       error maps are gathered after the rows, mcpt_gather_error_map, for the noise-guided filter)
//   mcpt_render --scene 6 --spp 16 --chunk 4 --denoise-variance --aov s6 --out s6.png   (the variance-propagating
//       filter; --aov also writes s6_variance.pfm)
//   mcpt_render --scene 6 --spp 1024 --chunk 32 --adaptive --target-error 0.05 --target-denoised --out s6.png
//       (render until the DENOISED image meets the error: mcpt_adaptive_select_filtered; one device)
//   mcpt_render --scene 6 --spp 4 --frames 100 --orbit-deg 1 --temporal --denoise-variance --out orbit.png
//       (an orbit of 100 cameras, 4 spp each, every frame reprojected into the next: orbit_000.png ...)
//   mcpt_render --scene 6 --spp 16 --chunk 2 --frames 100 --orbit-deg 1 --temporal --temporal-target 0.05
//       --denoise-variance --out orbit.png   (the same orbit, up to 16 spp where the history cannot carry a block)
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include "mcpt.hpp"

namespace {

struct Args {
  int scene = 6, width = 1280, height = 1000, spp = 16, bounces = 3, first_pass = 1, chunk = 64;
  int device = 0, subsampling = 0, variant = MCPT_MONTECARLO, traversal = MCPT_TRAVERSAL_AUTO;
  float ior = 1.0f, light = 1.2f, date = 0.0f;
  std::string png, pfm;
  std::string checkpoint, resume;   // --checkpoint FILE (after every chunk), --resume FILE
  std::vector<int> devices;   // --devices: one shard per entry
  int denoise = -1;           // --denoise [N]: a-trous iterations (-1: off; N defaults to 5)
  std::string aov;            // --aov PREFIX: PREFIX_normal.pfm, _albedo.pfm, _depth.pfm (+ _error.pfm with statistics)
  double target_error = 0.0;  // --target-error E: stop once the mean relative error <= E (--spp: the cap; 0: off)
  int denoise_guided = -1;    // --denoise-guided [N]: the noise-guided filter (-1: off; N defaults to 5)
  int denoise_variance = -1;  // --denoise-variance [N]: the variance-propagating filter (-1: off; N defaults to 5)
  // one of the filters that read the error map (statistics on, >= 2 chunks)
  bool noise_filter() const { return denoise_guided >= 0 || denoise_variance >= 0; }
  int target_denoised = -1;   // --target-denoised [N]: --adaptive selects on the variance filter's error (-1: off; N defaults to 5)
  float raw_cap = 64.0f;      // --raw-cap R: with --target-denoised a block also stays while its largest raw r > R (64: off)
  bool adaptive = false;      // --adaptive: --target-error is the per-pixel threshold; retired 8x8 blocks stop receiving passes
  int queue_rounds = 0;       // --queue-rounds K: with --adaptive, one device: the chunks go out as queued runs of up to K (0: off)
  int frames = 0;             // --frames N: N cameras, one image each (0: off; with --temporal alone: 1)
  float orbit_deg = 0.0f;     // --orbit-deg D: frame k's world is turned k * D degrees about the up axis
  int temporal = -1;          // --temporal [max_history]: every frame is reprojected into the next (-1: off)
  double temporal_target = 0.0;   // --temporal-target E: with --temporal, a frame's 8x8 blocks stop once the blend the
                              // history would give them meets E (--spp: the cap, --chunk: a round's passes; 0: off)
};

bool parse_list(const char* v, std::vector<int>& out) {
  out.clear();
  for (const char* p = v; *p;) {
    char* end = nullptr;
    const long d = std::strtol(p, &end, 10);
    if (end == p || d < 0 || d > 1024) return false;
    if (*end && *end != ',') return false;
    out.push_back((int)d);
    p = (*end == ',') ? end + 1 : end;
  }
  return !out.empty();
}

void usage() {
  std::fprintf(stderr,
               "usage: mcpt_render [--scene 1..8] [--width W] [--height H] [--subsampling k]\n"
               "                   [--spp S] [--first-pass P] [--chunk C] [--bounces B] [--ior R]\n"
               "                   [--light L] [--date T] [--variant montecarlo|mat|mat_tr]\n"
               "                   [--traversal auto|lane|wave|stream] [--device D | --devices D0,D1,...]\n"
               "                   [--out img.png] [--pfm img.pfm]\n"
               "                   [--checkpoint state.ckpt] [--resume state.ckpt]   (one device)\n"
               "                   [--denoise [N]]   (write the a-trous filtered image, N iterations, default 5)\n"
               "                   [--aov PREFIX]    (PREFIX_normal.pfm, PREFIX_albedo.pfm, PREFIX_depth.pfm;\n"
               "                                      PREFIX_error.pfm = {se, r, 0} with noise statistics)\n"
               "                   [--target-error E]   (one device: render chunks of --chunk passes until the mean\n"
               "                                         relative error <= E, at most --spp passes)\n"
               "                   [--adaptive]   (with --target-error: E is the per-pixel threshold on r; 8x8 blocks\n"
               "                                   whose largest r <= E stop receiving passes; --aov also writes\n"
               "                                   PREFIX_samples.pfm; the image is accum / each pixel's own count;\n"
               "                                   with --devices every shard selects on its own rows; --denoise,\n"
               "                                   --checkpoint and --resume use the per-pixel-count forms)\n"
               "                   [--denoise-guided [N]]   (the a-trous filter with the colour width from each\n"
               "                                             pixel's standard error; >= 2 chunks; with --devices\n"
               "                                             the shards' error maps are gathered with the rows,\n"
               "                                             not together with --adaptive)\n"
               "                   [--denoise-variance [N]]   (the variance-propagating a-trous filter: the error\n"
               "                                               map's variance prefiltered 3x3 and filtered along\n"
               "                                               with the colour; accepted and refused where\n"
               "                                               --denoise-guided is; --aov also writes\n"
               "                                               PREFIX_variance.pfm)\n"
               "                   [--target-denoised [N]] [--raw-cap R]   (with --adaptive --target-error E, one\n"
               "                                   device: E bounds the error of the variance-filtered image (N\n"
               "                                   iterations, default 5) in place of the raw one; a block also stays\n"
               "                                   while its largest raw r > R (default 64: off); writes the\n"
               "                                   filtered image as --denoise-variance N would)\n"
               "                   [--queue-rounds K]   (with --adaptive, one device: up to K chunks and their selects\n"
               "                                         are queued on the device per host wait, 1..256; the same\n"
               "                                         image; a checkpoint is written after each run)\n"
               "                   [--temporal-target E]   (with --temporal: per frame rounds of --chunk passes, --spp the\n"
               "                                   cap, for the 8x8 blocks whose blend with the history does not meet\n"
               "                                   E yet; queued on the device, --queue-rounds K rounds per wait)\n"
               "                   [--temporal [max_history]] [--frames N] [--orbit-deg D]   (N cameras, frame k with the\n"
               "                                   world turned k * D degrees about the up axis, --spp passes each in\n"
               "                                   two batches or more; every frame's result is reprojected into the\n"
               "                                   next and blended over at most max_history frames (default 8, 1..65535),\n"
               "                                   then filtered: needs --denoise-variance; writes NAME_000.png, ...\n"
               "                                   for --out NAME.png (default out.png); one device, not with\n"
               "                                   --adaptive, --target-error, --checkpoint, --resume, --aov,\n"
               "                                   --denoise or --denoise-guided)\n");
}

// a refused combination: why, then the usage (parse's false)
bool refuse(const char* why) {
  std::fprintf(stderr, "mcpt_render: %s\n", why);
  return false;
}

bool parse(int argc, char** argv, Args& a) {
  for (int i = 1; i < argc; ++i) {
    const std::string k = argv[i];
    if (k == "-h" || k == "--help") return false;
    if (k == "--denoise") {   // the iteration count is optional
      a.denoise = 5;
      if (i + 1 < argc && argv[i + 1][0] >= '0' && argv[i + 1][0] <= '9') a.denoise = std::atoi(argv[++i]);
      if (a.denoise > 8) return false;
      continue;
    }
    if (k == "--adaptive") {
      a.adaptive = true;
      continue;
    }
    if (k == "--denoise-guided") {
      a.denoise_guided = 5;
      if (i + 1 < argc && argv[i + 1][0] >= '0' && argv[i + 1][0] <= '9') a.denoise_guided = std::atoi(argv[++i]);
      if (a.denoise_guided > 8) return false;
      continue;
    }
    if (k == "--denoise-variance") {
      a.denoise_variance = 5;
      if (i + 1 < argc && argv[i + 1][0] >= '0' && argv[i + 1][0] <= '9') a.denoise_variance = std::atoi(argv[++i]);
      if (a.denoise_variance > 8) return false;
      continue;
    }
    if (k == "--temporal") {
      a.temporal = mcpt::Renderer::kTemporalMaxHistory;
      if (i + 1 < argc && argv[i + 1][0] >= '0' && argv[i + 1][0] <= '9') a.temporal = std::atoi(argv[++i]);
      if (a.temporal < 1 || a.temporal > MCPT_TEMPORAL_MAX_HISTORY) return false;
      continue;
    }
    if (k == "--target-denoised") {
      a.target_denoised = 5;
      if (i + 1 < argc && argv[i + 1][0] >= '0' && argv[i + 1][0] <= '9') a.target_denoised = std::atoi(argv[++i]);
      if (a.target_denoised > 8) return false;
      continue;
    }
    if (i + 1 >= argc) return false;
    const char* v = argv[++i];
    if (k == "--scene") a.scene = std::atoi(v);
    else if (k == "--width") a.width = std::atoi(v);
    else if (k == "--height") a.height = std::atoi(v);
    else if (k == "--subsampling") a.subsampling = std::atoi(v);
    else if (k == "--spp") a.spp = std::atoi(v);
    else if (k == "--first-pass") a.first_pass = std::atoi(v);
    else if (k == "--chunk") a.chunk = std::atoi(v);
    else if (k == "--bounces") a.bounces = std::atoi(v);
    else if (k == "--ior") a.ior = (float)std::atof(v);
    else if (k == "--light") a.light = (float)std::atof(v);
    else if (k == "--date") a.date = (float)std::atof(v);
    else if (k == "--device") a.device = std::atoi(v);
    else if (k == "--devices") {
      if (!parse_list(v, a.devices)) return false;
    }
    else if (k == "--out") a.png = v;
    else if (k == "--pfm") a.pfm = v;
    else if (k == "--checkpoint") a.checkpoint = v;
    else if (k == "--resume") a.resume = v;
    else if (k == "--aov") a.aov = v;
    else if (k == "--target-error") {
      a.target_error = std::atof(v);
      if (!(a.target_error > 0.0)) return false;
    }
    else if (k == "--temporal-target") {
      a.temporal_target = std::atof(v);
      if (!(a.temporal_target > 0.0) || !std::isfinite(a.temporal_target)) return false;
    }
    else if (k == "--queue-rounds") {
      a.queue_rounds = std::atoi(v);
      if (a.queue_rounds < 1 || a.queue_rounds > MCPT_ADAPTIVE_RUN_MAX_ROUNDS) return false;
    }
    else if (k == "--frames") {
      a.frames = std::atoi(v);
      if (a.frames < 1 || a.frames > 100000) return false;
    }
    else if (k == "--orbit-deg") a.orbit_deg = (float)std::atof(v);
    else if (k == "--raw-cap") {
      a.raw_cap = (float)std::atof(v);
      if (!(a.raw_cap > 0.0f)) return false;
    }
    else if (k == "--variant") {
      const std::string s = v;
      a.variant = s == "mat" ? MCPT_MAT : (s == "mat_tr" ? MCPT_MAT_TR : MCPT_MONTECARLO);
      if (s != "mat" && s != "mat_tr" && s != "montecarlo") return false;
    } else if (k == "--traversal") {
      const std::string s = v;
      a.traversal = s == "lane"     ? MCPT_TRAVERSAL_LANE
                    : s == "wave"   ? MCPT_TRAVERSAL_WAVE
                    : s == "stream" ? MCPT_TRAVERSAL_STREAM
                                    : MCPT_TRAVERSAL_AUTO;
    } else {
      return false;
    }
  }
  // (first: these refusals carry a message)
  if (a.temporal < 0 && (a.frames > 0 || a.orbit_deg != 0.0f))
    return refuse("--frames and --orbit-deg move the camera of a --temporal render: give --temporal");
  if (a.temporal < 0 && a.temporal_target > 0.0)
    return refuse("--temporal-target is the stopping rule of a --temporal render: give --temporal");
  if (a.temporal >= 0) {
    if (a.frames == 0) a.frames = 1;
    if (!a.devices.empty()) return refuse("--temporal keeps its history on one device: not with --devices (not built)");
    if (a.adaptive || a.target_error > 0.0)
      return refuse("--temporal blends frames of one sample count: not with --adaptive or --target-error (not built)");
    if (!a.checkpoint.empty() || !a.resume.empty())
      return refuse("--temporal: the history is not part of a checkpoint: not with --checkpoint or --resume (not built)");
    if (a.denoise >= 0 || a.denoise_guided >= 0)
      return refuse("--temporal filters with the variance filter alone: not with --denoise or --denoise-guided");
    if (!a.aov.empty()) return refuse("--temporal writes its frames only: not with --aov (not built)");
    if (a.denoise_variance < 0) return refuse("--temporal filters with the variance filter: give --denoise-variance [N]");
    if (a.spp < 2) return refuse("--temporal needs two batches per frame for its error map: --spp 2 or more");
    if (a.temporal_target > 0.0 && (a.chunk <= 0 || a.spp / a.chunk < 2))
      return refuse("--temporal-target renders rounds of --chunk passes up to --spp: two rounds or more");
  }
  if (!a.devices.empty() && (!a.checkpoint.empty() || !a.resume.empty())) return false;   // one device only
  // (stopping N host threads on a merged record is not built: a uniform --target-error is one device's)
  if (!a.devices.empty() && a.target_error > 0.0 && !a.adaptive) return false;
  // (the guided filter on a gathered frame: the uniform shards' error maps travel with
  // mcpt_gather_error_map; with --adaptive the combination stays refused here, and the library calls
  // gather_rows_counted + gather_error_map + denoise_resolved_guided serve it)
  if (!a.devices.empty() && a.adaptive && a.noise_filter()) return false;
  if ((a.denoise >= 0) + (a.denoise_guided >= 0) + (a.denoise_variance >= 0) > 1) return false;   // one filter
  if (a.adaptive && !(a.target_error > 0.0)) return false;   // adaptive sampling needs its threshold
  if (a.queue_rounds > 0 && !(a.temporal_target > 0.0)) {
    if (!a.adaptive) return refuse("--queue-rounds queues the chunks of --adaptive --target-error E: give both");
    if (!a.devices.empty()) return refuse("--queue-rounds runs on one device: not with --devices");
  }
  if (a.target_denoised >= 0) {
    if (!a.adaptive || !(a.target_error > 0.0))
      return refuse("--target-denoised is a rule of --adaptive --target-error E: give both");
    if (!a.devices.empty())   // (a shard is not a full frame: the filter has no rows beyond its own)
      return refuse("--target-denoised needs the full frame on one device: not with --devices");
    if (a.denoise >= 0 || a.noise_filter())
      return refuse("--target-denoised writes its own variance-filtered image: no other --denoise* with it");
    a.denoise_variance = a.target_denoised;   // the image, the AOVs and the JSON fields of --denoise-variance N
  }
  return a.width > 0 && a.height > 0 && a.spp >= 0 && a.chunk > 0 && a.subsampling >= 0 && a.subsampling < 16;
}

// the threshold of a convergence query that is made for its error map alone (no --target-error): the
// map does not depend on it
constexpr float kMapThreshold = 0.05f;

// NAME.ext -> NAME_007.ext
std::string frame_path(const std::string& path, int k) {
  const size_t dot = path.find_last_of('.'), slash = path.find_last_of('/');
  const bool ext = dot != std::string::npos && (slash == std::string::npos || dot > slash);
  char num[16];
  std::snprintf(num, sizeof(num), "_%03d", k);
  return ext ? path.substr(0, dot) + num + path.substr(dot) : path + num;
}

// --temporal: a.frames cameras on one device, the loop of mcpt.h's temporal section per camera.  The
// passes keep advancing across the frames (independent samples); a frame's passes go out in batches
// of at most --chunk, two at the least.
int run_temporal(const Args& a, mcpt::BVH_GPU_Scene& scene, int W, int H) {
  mcpt::Renderer r(a.device);
  r.set_traversal(a.traversal);
  r.upload(scene);
  r.set_target(W, H);
  r.temporal_begin();
  const int batch = std::min(a.chunk, (a.spp + 1) / 2);
  const std::string png = a.png.empty() && a.pfm.empty() ? "out.png" : a.png;
  double kernel_ms = 0.0, temporal_ms = 0.0, filter_ms = 0.0;
  mcpt_temporal_t rec{};
  mcpt_adaptive_temporal_t sel{};   // --temporal-target: the frame's last select
  double samples = 0.0;             // mean samples per pixel, summed over the frames
  mcpt::GLMat4 prev;
  int pass = a.first_pass;
  double mean = 0.0;
  const auto t0 = std::chrono::steady_clock::now();
  for (int k = 0; k < a.frames; ++k) {
    const mcpt::Camera cam = mcpt::Camera::orbit(a.width, a.height, (float)k * a.orbit_deg);
    r.clear_accum();
    r.stats_begin();
    if (a.temporal_target > 0.0) {
      // the adaptive form of the frame loop (mcpt.h): rounds of --chunk passes for the blocks the
      // history cannot carry, as queued runs of up to --queue-rounds rounds (none given: one run)
      r.adaptive_begin(0);
      r.render_guides(cam);
      const int rounds = std::min(a.spp / a.chunk, MCPT_ADAPTIVE_RUN_MAX_ROUNDS);
      std::vector<mcpt_adaptive_temporal_t> recs;
      const auto run = [&](int first, int q) {   // (whole chunks, a select per round: every step is a run)
        const mcpt_adaptive_run_t got =
            r.adaptive_run_temporal(cam, first, a.chunk, q, 1, (float)a.temporal_target, k ? &prev : nullptr, a.date,
                                    a.bounces, a.ior, recs, a.variant, a.temporal);
        kernel_ms += got.device_ms;
        if (!recs.empty()) sel = recs.back();   // (the frame's last select)
        return mcpt::AdaptiveRan{got.rounds_run, got.selects_run, sel.raw.n_active_blocks};
      };
      mcpt::adaptive_until(pass, a.chunk, rounds * a.chunk, 1, a.queue_rounds > 0 ? a.queue_rounds : rounds, nullptr,
                           nullptr, run);
      samples += (double)sel.raw.samples / (double)(sel.raw.n_px > 0 ? sel.raw.n_px : 1);
      pass += a.spp;   // (pass ids never repeat, whatever the frame rendered)
      rec = r.temporal_accumulate_resolved(k ? &prev : nullptr, a.temporal);
    } else {
      for (int done = 0; done < a.spp; done += batch) {
        const int n = std::min(batch, a.spp - done);
        r.render(cam, pass, n, a.date, a.bounces, a.ior, a.variant);
        kernel_ms += r.last_render_ms();
        pass += n;
      }
      samples += (double)a.spp;
      r.convergence(kMapThreshold);
      r.render_guides(cam);
      rec = r.temporal_accumulate(k ? &prev : nullptr, a.temporal);
    }
    const std::vector<float> img = r.denoise_temporal(a.denoise_variance);
    float am = 0.0f, cm = 0.0f, gm = 0.0f, fm = 0.0f;
    r.last_temporal_ms(am, cm);
    r.last_denoise_ms(gm, fm);
    temporal_ms += am + cm;
    filter_ms += fm;
    prev = cam.PV();
    if (!png.empty()) mcpt::write_png(frame_path(png, k), img, W, H);
    if (!a.pfm.empty()) mcpt::write_pfm(frame_path(a.pfm, k), img, W, H);
    mean = 0.0;
    for (float v : img) mean += v;
    mean /= (double)(img.size() ? img.size() : 1);
  }
  const double wall_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  std::printf("{\"scene\": %d, \"width\": %d, \"height\": %d, \"spp\": %d, \"bounces\": %d, \"frames\": %d, "
              "\"orbit_deg\": %g, \"temporal\": %d, \"denoise_variance\": %d, \"kernel_ms\": %.3f, \"temporal_ms\": %.3f, "
              "\"filter_ms\": %.3f, \"wall_ms\": %.3f, \"mean\": %.6f, \"n_history\": %lld, \"n_new\": %lld, "
              "\"n_miss\": %lld, \"n_offscreen\": %lld, \"n_rejected\": %lld, \"max_len\": %d, \"mean_len\": %.4f, "
              "\"passes\": %d, \"temporal_target\": %g, \"mean_spp\": %.4f, \"active_blocks\": %lld}\n",
              a.scene, W, H, a.spp, a.bounces, a.frames, a.orbit_deg, a.temporal, a.denoise_variance, kernel_ms, temporal_ms,
              filter_ms, wall_ms, mean, rec.n_history, rec.n_new, rec.n_miss, rec.n_offscreen, rec.n_rejected, rec.max_len,
              rec.n_px > 0 ? (double)rec.sum_len / (double)rec.n_px : 0.0, pass - a.first_pass, a.temporal_target,
              samples / (double)(a.frames > 0 ? a.frames : 1), (long long)sel.raw.n_active_blocks);
  return 0;
}

// the adaptive part of the JSON line from a select's record (a frame's, or the shards' combined)
std::string adaptive_json(double target_error, bool converged, const mcpt_adaptive_t& rec) {
  char buf[400];
  std::snprintf(buf, sizeof(buf),
                ", \"adaptive\": true, \"target_error\": %g, \"converged\": %s, \"window_passes\": %lld, "
                "\"batches\": %d, \"mean_r\": %.6f, \"max_r\": %.6f, \"n_above\": %lld, \"n_px\": %lld, "
                "\"sum_q\": %llu, \"samples\": %lld, \"n_active_blocks\": %lld, \"n_blocks\": %lld, "
                "\"mean_spp\": %.4f",
                target_error, converged ? "true" : "false", rec.passes, rec.batches, rec.mean_r, rec.max_r, rec.n_above,
                rec.n_px, rec.sum_q, rec.samples, rec.n_active_blocks, rec.n_blocks,
                rec.n_px > 0 ? (double)rec.samples / (double)rec.n_px : 0.0);
  return buf;
}

// one chunk for the active blocks; its render time (synchronizes)
float render_adaptive_ms(const Args& a, mcpt::Renderer& r, const mcpt::Camera& cam, int first, int n) {
  r.render_adaptive(cam, first, n, a.date, a.bounces, a.ior, a.variant);
  float sel = 0.0f, ren = 0.0f;
  r.last_adaptive_ms(sel, ren);
  return ren;
}

// --denoise / --aov on the context that holds the whole frame: the guide buffers, the AOV files,
// and the filtered image in place of the averaged one
void post_process(const Args& a, mcpt::Renderer& r, const mcpt::Camera& cam, int W, int H, std::vector<float>& img,
                  double& guides_ms, double& filter_ms) {
  r.render_guides(cam);
  if (!a.aov.empty()) {
    std::vector<float> g, al;
    r.read_guides(g, al);
    const size_t n = (size_t)W * H;
    std::vector<float> normal(n * 3), albedo(n * 3), depth(n * 3);
    for (size_t i = 0; i < n; ++i)
      for (int k = 0; k < 3; ++k) {
        normal[3 * i + k] = g[8 * i + k];
        albedo[3 * i + k] = al[4 * i + k];
        depth[3 * i + k] = g[8 * i + 7];
      }
    mcpt::write_pfm(a.aov + "_normal.pfm", normal, W, H);
    mcpt::write_pfm(a.aov + "_albedo.pfm", albedo, W, H);
    mcpt::write_pfm(a.aov + "_depth.pfm", depth, W, H);
  }
  if (a.adaptive && !a.aov.empty()) {   // every pixel's sample count
    const std::vector<int> cnt = r.read_sample_counts();
    std::vector<float> smp(cnt.size() * 3);
    for (size_t i = 0; i < cnt.size(); ++i) smp[3 * i] = smp[3 * i + 1] = smp[3 * i + 2] = (float)cnt[i];
    mcpt::write_pfm(a.aov + "_samples.pfm", smp, W, H);
  }
  // noise statistics on: the error map (of the final state) and its filter; a gathered frame
  // (--devices) holds the shards' maps, which mcpt_gather_error_map delivered
  const bool gathered_map = r.error_map_source() == 2;
  if (gathered_map || r.stats_info().batches >= 2) {
    if (!a.adaptive && !gathered_map)   // (adaptive: the last select's map)
      r.convergence(a.target_error > 0.0 ? (float)a.target_error : kMapThreshold);
    if (!a.aov.empty()) {
      const std::vector<float> m = r.read_error_map();
      const size_t n = (size_t)W * H;
      std::vector<float> err(n * 3, 0.0f);
      for (size_t i = 0; i < n; ++i) {
        err[3 * i] = m[2 * i];
        err[3 * i + 1] = m[2 * i + 1];
      }
      mcpt::write_pfm(a.aov + "_error.pfm", err, W, H);
    }
  }
  // (adaptive: every pixel divided by its own count)
  if (a.denoise >= 0) img = a.adaptive ? r.denoise_resolved(a.denoise) : r.denoise(a.denoise);
  if (a.denoise_guided >= 0)   // (fewer than two chunks: an error)
    img = a.adaptive ? r.denoise_resolved_guided(a.denoise_guided) : r.denoise_guided(a.denoise_guided);
  if (a.denoise_variance >= 0) {   // (fewer than two chunks: an error)
    img = a.adaptive ? r.denoise_resolved_variance(a.denoise_variance) : r.denoise_variance(a.denoise_variance);
    if (!a.aov.empty()) {
      const std::vector<float> v = r.read_denoised_variance();
      std::vector<float> var(v.size() * 3);
      for (size_t i = 0; i < v.size(); ++i) var[3 * i] = var[3 * i + 1] = var[3 * i + 2] = v[i];
      mcpt::write_pfm(a.aov + "_variance.pfm", var, W, H);
    }
  }
  float gm = 0.0f, fm = 0.0f;
  r.last_denoise_ms(gm, fm);
  guides_ms = gm; filter_ms = fm;
}

}  // namespace

int main(int argc, char** argv) {
  Args a;
  if (!parse(argc, argv, a)) {
    usage();
    return 2;
  }
  try {
    mcpt::BVH_GPU_Scene scene;
    scene.build_reference(a.scene, a.light);
    // sub-sampling renders the FBO at (W>>k) x (H>>k) with the window's aspect (montecarlo.cpp:616-626)
    const int W = a.width >> a.subsampling, H = a.height >> a.subsampling;
    if (W <= 0 || H <= 0) throw std::runtime_error("sub-sampled framebuffer is empty");
    if (a.temporal >= 0) return run_temporal(a, scene, W, H);
    const mcpt::Camera cam = mcpt::Camera::canonical(a.width, a.height);

    double kernel_ms = 0.0, wall_ms = 0.0, gather_ms = 0.0, guides_ms = 0.0, filter_ms = 0.0;
    const bool post = a.denoise >= 0 || a.noise_filter() || !a.aov.empty();
    const bool stats = a.target_error > 0.0 || a.noise_filter();
    std::vector<float> img;
    std::string shard_json;
    int rendered = a.spp;   // passes in the image (fewer with --target-error)
    if (a.devices.empty()) {
      mcpt::Renderer r(a.device);
      r.set_traversal(a.traversal);
      r.upload(scene);
      r.set_target(W, H);
      // checkpoint / resume: --spp counts the whole render's passes (first_pass .. first_pass +
      // spp - 1); a resumed run continues at the checkpoint's next pass with its sums loaded,
      // and the tag makes a resume with other render parameters fail
      char tag[320];
      // (the chunk too: a call that splits a 32-pass accumulation chunk adds its own partial sum,
      // so the resumed bits equal the uninterrupted run's only with the same call boundaries)
      int len = std::snprintf(tag, sizeof(tag),
                              "scene=%d W=%d H=%d bounces=%d ior=%a light=%a date=%a variant=%d first=%d chunk=%d", a.scene,
                              W, H, a.bounces, a.ior, a.light, a.date, a.variant, a.first_pass, a.chunk);
      // (adaptive: the threshold decides which blocks the later chunks reach)
      if (a.adaptive) len += std::snprintf(tag + len, sizeof(tag) - (size_t)len, " adaptive=%a", a.target_error);
      // (the rule too: it decides which blocks the later chunks reach)
      if (a.target_denoised >= 0)
        std::snprintf(tag + len, sizeof(tag) - (size_t)len, " denoised=%d cap=%a", a.target_denoised, a.raw_cap);
      const bool resumed_adaptive = a.adaptive && !a.resume.empty();
      int next = a.first_pass;
      if (resumed_adaptive) next = r.load_adaptive_checkpoint(a.resume, tag);   // (statistics and the mode on, as saved)
      else if (!a.resume.empty()) next = r.load_checkpoint(a.resume, tag);
      const auto t0 = std::chrono::steady_clock::now();
      // noise statistics: a window from here (a resumed plain render begins a new one), a batch per
      // chunk; --target-error asks every 4 chunks and after the last
      if (stats && !resumed_adaptive) r.stats_begin();
      mcpt_convergence_t rec{};
      bool have_rec = false, converged = false;
      int calls = 0;
      mcpt_adaptive_t arec{};
      mcpt_adaptive_filtered_t frec{};
      bool have_arec = false;
      if (a.target_denoised >= 0) r.render_guides(cam);   // (after a resume too: a checkpoint holds no guides)
      if (a.adaptive && !resumed_adaptive) r.adaptive_begin(0);
      if (resumed_adaptive) {   // the chunks so far were one batch each; a select has run from the second on
        calls = r.stats_info().batches;
        converged = calls >= 2 && r.adaptive_info().n_active == 0;
        rendered = next - a.first_pass;
      }
      if (a.adaptive && next - a.first_pass < a.spp && !converged) {
        // chunks for the active blocks with a select after every chunk from the second on; with
        // --queue-rounds K the whole chunks ahead go out as queued runs of up to K rounds
        const bool filtered = a.target_denoised >= 0;
        const float thr = (float)a.target_error;
        std::vector<mcpt_adaptive_t> recs;
        std::vector<mcpt_adaptive_filtered_t> frecs;
        const mcpt::AdaptiveUntil u = mcpt::adaptive_until(
            a.first_pass, a.chunk, a.spp, 1, a.queue_rounds,
            [&](int first, int n) { kernel_ms += render_adaptive_ms(a, r, cam, first, n); },
            [&] {
              if (filtered)
                frec = r.adaptive_select_filtered(thr, a.raw_cap, mcpt::Renderer::kErrorMuFloor, a.target_denoised);
              return (arec = filtered ? frec.raw : r.adaptive_select(thr)).n_active_blocks;
            },
            [&](int first, int k) {
              const mcpt_adaptive_run_t run =
                  filtered ? r.adaptive_run_filtered(cam, first, a.chunk, k, 1, thr, a.raw_cap, a.target_denoised, a.date,
                                                     a.bounces, a.ior, frecs, a.variant)
                           : r.adaptive_run(cam, first, a.chunk, k, 1, thr, a.date, a.bounces, a.ior, recs, a.variant);
              kernel_ms += run.device_ms;
              if (filtered && run.selects_run > 0) frec = frecs.back();
              if (run.selects_run > 0) arec = filtered ? frec.raw : recs.back();
              return mcpt::AdaptiveRan{run.rounds_run, run.selects_run, arec.n_active_blocks};
            },
            // (after the step's select: the resumed run continues with the next chunk's render)
            [&](int done, int) {
              if (!a.checkpoint.empty()) r.save_adaptive_checkpoint(a.checkpoint, a.first_pass + done, tag);
            },
            next - a.first_pass, calls);
        rendered = u.done;
        have_arec = u.selects > 0;
        if (have_arec) converged = arec.n_active_blocks == 0;
      }
      for (int done = next - a.first_pass; !a.adaptive && done < a.spp && !converged; done += a.chunk) {
        const int n = std::min(a.chunk, a.spp - done);
        r.render(cam, a.first_pass + done, n, a.date, a.bounces, a.ior, a.variant);
        kernel_ms += r.last_render_ms();
        if (!a.checkpoint.empty()) r.save_checkpoint(a.checkpoint, a.first_pass + done + n, tag);
        rendered = done + n;
        ++calls;
        if (a.target_error > 0.0 && (calls % 4 == 0 || rendered >= a.spp) && r.stats_info().batches >= 2) {
          rec = r.convergence((float)a.target_error);
          have_rec = true;
          converged = rec.mean_r <= a.target_error;
        }
      }
      img = a.adaptive ? r.read_resolved() : r.read_image();
      if (post) post_process(a, r, cam, W, H, img, guides_ms, filter_ms);
      if (a.adaptive) {
        char buf[400];
        if (have_arec) {
          shard_json += adaptive_json(a.target_error, converged, arec);
          if (a.target_denoised >= 0) {
            std::snprintf(buf, sizeof(buf),
                          ", \"target_denoised\": %d, \"raw_cap\": %g, \"mean_rf\": %.6f, \"max_rf\": %.6f, "
                          "\"n_above_f\": %lld, \"sum_qf\": %llu",
                          a.target_denoised, a.raw_cap, frec.mean_rf, frec.max_rf, frec.n_above_f, frec.sum_qf);
            shard_json += buf;
          }
        } else {   // no select in this run (fewer than two chunks, or a resume with nothing left to do)
          long long samples = 0;
          for (int c : r.read_sample_counts()) samples += c;
          std::snprintf(buf, sizeof(buf),
                        ", \"adaptive\": true, \"target_error\": %g, \"converged\": %s, \"mean_r\": null, "
                        "\"samples\": %lld, \"n_active_blocks\": %lld, \"mean_spp\": %.4f",
                        a.target_error, converged ? "true" : "false", samples, r.adaptive_info().n_active,
                        (double)samples / ((double)W * H));
          shard_json += buf;
        }
      } else if (a.target_error > 0.0) {
        char buf[320];
        if (have_rec)
          std::snprintf(buf, sizeof(buf),
                        ", \"target_error\": %g, \"converged\": %s, \"window_passes\": %lld, \"batches\": %d, "
                        "\"mean_r\": %.6f, \"max_r\": %.6f, \"n_above\": %lld, \"n_px\": %lld, \"sum_q\": %llu",
                        a.target_error, converged ? "true" : "false", rec.passes, rec.batches, rec.mean_r, rec.max_r,
                        rec.n_above, rec.n_px, rec.sum_q);
        else   // fewer than two chunks: no estimate
          std::snprintf(buf, sizeof(buf), ", \"target_error\": %g, \"converged\": false, \"mean_r\": null",
                        a.target_error);
        shard_json += buf;
      }
      wall_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    } else {
      // N shards: scene upload and targets first (untimed), then one host thread per shard
      const int N = (int)a.devices.size();
      std::vector<std::unique_ptr<mcpt::Renderer>> shards;
      for (int k = 0; k < N; ++k) {
        shards.emplace_back(new mcpt::Renderer(a.devices[(size_t)k]));
        shards.back()->set_traversal(a.traversal);
        shards.back()->upload(scene);
        shards.back()->set_target_rows(W, H, mcpt::Renderer::balanced_rows(H, N, k));
      }
      mcpt::Renderer frame(a.devices[0]);
      frame.set_target(W, H);
      if (post) frame.upload(scene);   // the guides are traced on the frame context
      std::vector<double> shard_ms((size_t)N, 0.0);
      std::vector<std::string> errors((size_t)N);
      // adaptive: every shard's own statistics window and select / render loop on its rows
      std::vector<mcpt_adaptive_t> shard_rec((size_t)N);
      std::vector<mcpt::AdaptiveUntil> shard_until((size_t)N, mcpt::AdaptiveUntil{0, 0, 0});   // passes, calls, selects
      const auto t0 = std::chrono::steady_clock::now();
      std::vector<std::thread> workers;
      for (int k = 0; k < N; ++k)
        workers.emplace_back([&, k]() {
          try {
            mcpt::Renderer& s = *shards[(size_t)k];
            if (a.adaptive) {
              s.stats_begin();
              s.adaptive_begin(0);
            }
            if (a.adaptive && a.spp > 0)   // until the shard's list is empty
              shard_until[(size_t)k] = mcpt::adaptive_until(
                  a.first_pass, a.chunk, a.spp, 1, 0,
                  [&](int first, int n) { shard_ms[(size_t)k] += render_adaptive_ms(a, s, cam, first, n); },
                  [&] { return (shard_rec[(size_t)k] = s.adaptive_select((float)a.target_error)).n_active_blocks; });
            // uniform shards with --denoise-guided / --denoise-variance: a statistics window over the chunks and, after the
            // last, the shard's error map (fewer than two chunks: MCPT_ERR_NO_STATS, as on one device)
            if (!a.adaptive && a.noise_filter()) s.stats_begin();
            for (int done = 0; !a.adaptive && done < a.spp; done += a.chunk) {
              const int n = std::min(a.chunk, a.spp - done);
              s.render(cam, a.first_pass + done, n, a.date, a.bounces, a.ior, a.variant);
              shard_ms[(size_t)k] += s.last_render_ms();   // (synchronizes this shard)
            }
            if (!a.adaptive && a.noise_filter()) s.convergence(kMapThreshold);
          } catch (const std::exception& e) {
            errors[(size_t)k] = e.what();
          }
        });
      for (std::thread& t : workers) t.join();
      for (const std::string& e : errors)
        if (!e.empty()) throw std::runtime_error(e);
      const auto t1 = std::chrono::steady_clock::now();
      std::vector<const mcpt::Renderer*> views;
      for (const auto& r : shards) views.push_back(r.get());
      if (a.adaptive) {   // the shards' counts travel with their rows
        frame.gather_rows_counted(views);
        img = frame.read_resolved();
      } else {
        frame.gather_rows(views);
        img = frame.read_image();
      }
      if (a.noise_filter()) frame.gather_error_map(views);   // (after the rows: a row gather invalidates it)
      if (post) post_process(a, frame, cam, W, H, img, guides_ms, filter_ms);
      const auto t2 = std::chrono::steady_clock::now();
      wall_ms = std::chrono::duration<double, std::milli>(t2 - t0).count();
      gather_ms = std::chrono::duration<double, std::milli>(t2 - t1).count();
      for (double ms : shard_ms) kernel_ms = std::max(kernel_ms, ms);   // the slowest shard bounds the frame
      shard_json = ", \"devices\": [";
      for (int k = 0; k < N; ++k) shard_json += (k ? ", " : "") + std::to_string(a.devices[(size_t)k]);
      shard_json += "], \"shard_kernel_ms\": [";
      for (int k = 0; k < N; ++k) {
        char buf[32];
        std::snprintf(buf, sizeof(buf), "%s%.3f", k ? ", " : "", shard_ms[(size_t)k]);
        shard_json += buf;
      }
      char buf[64];
      std::snprintf(buf, sizeof(buf), "], \"gather_ms\": %.3f", gather_ms);
      shard_json += buf;
      if (a.adaptive) {
        // the shards' records combined: the sums add, max_r is the largest; the window is the longest
        mcpt_adaptive_t all{};
        bool every = true;
        rendered = 0;
        for (int k = 0; k < N; ++k) {
          const mcpt_adaptive_t& q = shard_rec[(size_t)k];
          every = every && shard_until[(size_t)k].selects > 0;
          rendered = std::max(rendered, shard_until[(size_t)k].done);
          all.n_px += q.n_px; all.n_above += q.n_above; all.sum_q += q.sum_q; all.samples += q.samples;
          all.n_active_blocks += q.n_active_blocks; all.n_blocks += q.n_blocks;
          all.max_r = std::max(all.max_r, q.max_r);
          all.passes = std::max(all.passes, q.passes);
          all.batches = std::max(all.batches, q.batches);
        }
        all.mean_r = all.n_px > 0 ? (double)all.sum_q / 65536.0 / (double)all.n_px : 0.0;
        if (every) {
          shard_json += adaptive_json(a.target_error, all.n_active_blocks == 0, all);
        } else {   // fewer than two chunks: no select
          char nb[160];
          std::snprintf(nb, sizeof(nb), ", \"adaptive\": true, \"target_error\": %g, \"converged\": false, \"mean_r\": null",
                        a.target_error);
          shard_json += nb;
        }
      }
    }
    if (!a.pfm.empty()) mcpt::write_pfm(a.pfm, img, W, H);
    if (!a.png.empty()) mcpt::write_png(a.png, img, W, H);
    double mean = 0.0;
    for (float v : img) mean += v;
    mean /= (double)(img.size() ? img.size() : 1);
    const double samples = (double)W * H * rendered;
    if (post) {
      char buf[128];
      std::snprintf(buf, sizeof(buf), ", \"denoise\": %d, \"guides_ms\": %.3f, \"filter_ms\": %.3f", a.denoise, guides_ms,
                    filter_ms);
      shard_json += buf;
      if (a.denoise_guided >= 0) shard_json += ", \"denoise_guided\": " + std::to_string(a.denoise_guided);
      if (a.denoise_variance >= 0) shard_json += ", \"denoise_variance\": " + std::to_string(a.denoise_variance);
    }
    shard_json += ", \"passes\": " + std::to_string(rendered);
    std::printf("{\"scene\": %d, \"width\": %d, \"height\": %d, \"spp\": %d, \"bounces\": %d, \"ior\": %g, "
                "\"light\": %g, \"variant\": %d, \"prims\": %d, \"depth\": %d, \"kernel_ms\": %.3f, "
                "\"wall_ms\": %.3f, \"msamples_per_s\": %.2f, \"mean\": %.6f%s}\n",
                a.scene, W, H, a.spp, a.bounces, a.ior, a.light, a.variant, scene.nb_prim(), scene.depth(),
                kernel_ms, wall_ms, kernel_ms > 0 ? samples / kernel_ms / 1e3 : 0.0, mean, shard_json.c_str());
  } catch (const std::exception& e) {
    std::fprintf(stderr, "mcpt_render: %s\n", e.what());
    return 1;
  }
  return 0;
}
