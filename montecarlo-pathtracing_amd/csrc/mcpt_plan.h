// mcpt_plan.h — the launch plan of a render call: integer arithmetic only (pass geometry, grid and
// budget limits, sub-launch cutting, per-sub-launch facts, AUTO's tuner).  Plain C++17, no HIP
// header: compiled and tested on the CPU (tests/cpp/plan_test.cpp); mcpt_capi.hip reads the plan.
#pragma once
#include <stddef.h>

#include <algorithm>

namespace mcpt {

// accumulation chunk of the arithmetic contract: passes are summed from 0
// inside each chunk of kPassChunk consecutive absolute pass numbers, chunk sums added to
// the accumulator in chunk order
constexpr int kPassChunk = 32;
constexpr int kSplitPieces = 4;   // pass ranges of a split work item (RenderParams::split_n)
// work-item tile (pixels): a work item is a kTileW x kTileH pixel tile for one pass chunk, one
// lane per pixel, made of 8x8-pixel waves side by side: 32x8 = four waves in one 8-row strip, so
// in a row-band shard (8-row bands) all waves of a workgroup lie in one band of the image (16x16
// tiles: the slowest 8-GPU shard 2.4-4.1 % slower, profiles/r01_ab33_tile_shape.jsonl)
constexpr int kTileW = 32, kTileH = 8;
constexpr int kTileThreads = kTileW * kTileH;   // the widest tile (LDS-scene kernels)

namespace plan {

// default bound of the segment-sum buffer of one sub-launch (4 GiB of the 288 GB of HBM: 172
// segments = 5,504 passes per launch at 1080p, 43 = 1,376 at 4K, so a C5 step of 1,024 passes
// is one launch: +0.7 % against four launches under a 1 GiB bound, whose grid tails add up,
// profiles/r03_ab_partial_budget_c5.jsonl; mcpt_set_partial_budget / MCPT_PARTIAL_BYTES)
constexpr size_t kDefaultPartialBudget = size_t(4) << 30;
// per-pass value store of pass stealing (steal_store_bytes), per render lane: of mesh launches
constexpr size_t kStealBudget = size_t(8) << 30;
// ... and of the LDS-scene launches, per render lane: 1080p in 16-wide tiles holds
// 21 segments (C2's eight are one launch of 6.4 GB), 4K five
constexpr size_t kSceneStealBudget = size_t(16) << 30;
// work-item order (mcpt_order.hip): launches with at least this many work items run in the
// order sorted from an earlier launch of their shape; the order is re-sorted every
// kOrderRefresh launches of the shape (costs drift little: the same tiles and pass counts)
constexpr long long kOrderMinItems = 4096;
constexpr int kOrderRefresh = 16;
// split items (mesh launches): at most this many of the costliest items run in
// mcpt::kSplitPieces pass ranges each (RenderParams::split_n; 100 MB of per-pass values)
constexpr int kSplitMax = 1024;
// pass split (launch()): launches with fewer than this many work items per CU, of at most
// kPassSplitMaxPasses passes
constexpr int kPassSplitItemsPerCu = 4, kPassSplitMaxPasses = 256;

// ---- pass geometry
constexpr long long floor_div(long long a, long long b) { return (a >= 0) ? a / b : -((-a + b - 1) / b); }
// accumulation chunks (pass segments) that passes first_pass .. first_pass + n_passes - 1 touch
constexpr long long pass_segments(long long first_pass, long long n_passes) {
  return n_passes > 0 ? floor_div(first_pass + n_passes - 2, kPassChunk) - floor_div(first_pass - 1, kPassChunk) + 1 : 0;
}

// ---- limits of one sub-launch
struct LimitsIn {
  long long n_local_px = 0, n_tiles = 0;
  int tile_w = 16, seg_per_item = 1, n_cu = 256;
  size_t partial_budget = kDefaultPartialBudget;
  bool mesh = false, wave_traversal = false;
  bool lds_scene = false;   // the LDS-scene kernel (a staged scene, no meshes)
  bool steal = true;    // the MCPT_STEAL switch (adaptive launches: false)
  bool spare = true;    // reserve the grid's spare workgroups (adaptive launches add none: false)
};
struct Limits {
  long long max_items = 0;   // grid-size bound on the work items (n_tiles above it: target too large)
  long long max_seg = 1;     // most pass segments of one sub-launch
  bool may_steal = false;    // mesh launches of one segment per item; LDS-scene launches (lds_scene)
  bool too_large = false;
};
// bytes of the pass-stealing value store (RenderParams::steal_vals) of a launch of n_segments
// segments: three floats per (tile, segment, pass of the chunk, thread of the tile)
constexpr long long steal_store_bytes(long long n_tiles, int tile_w, long long n_segments) {
  return n_tiles * n_segments * kPassChunk * tile_w * kTileH * 3 * (long long)sizeof(float);
}
// The call's pass range is cut at accumulation-chunk boundaries into sub-launches of at
// most max_seg segments, so that the segment-sum buffer stays within partial_budget and
// the grid within 2^32 work-items (an 84,000-pass 4K call is ~2,600 segments: 261 GB of
// segment sums in one launch).  Chunk sums still reach the accumulator in chunk order, so
// the result is bit-identical to one launch.
inline Limits limits(const LimitsIn& in) {
  Limits r;
  const long long seg_bytes = in.n_local_px * 3 * (long long)sizeof(float);
  // (the grid's spare workgroups — split pieces of mesh launches, tail pieces: mcpt_launch_render —
  // are reserved: tail_m <= 4 x 7 workgroups per CU (tile_w >= 16 outside the mesh kernels))
  const long long kseg_max = std::max(1, in.seg_per_item);
  const long long spare = in.spare ? (long long)kSplitMax * (kSplitPieces - 1) + 28LL * in.n_cu * (kseg_max - 1) : 0;
  r.max_items = (1LL << 32) / (in.tile_w * kTileH) - 1 - spare;
  r.too_large = in.n_tiles > r.max_items;
  long long max_seg = seg_bytes > 0 ? (long long)(in.partial_budget / (size_t)seg_bytes) : (1LL << 30);
  // launches that steal passes store every pass's value (steal_store_bytes); one segment's:
  const long long val_bytes = steal_store_bytes(in.n_tiles, in.tile_w, 1);
  // mesh launches (one segment per item): at most kStealBudget per render lane, but two segments
  // at least, so that split items and stealing still apply (1080p: 10 segments per sub-launch,
  // 7.96 GB; 4K: 2, 6.4 GB)
  r.may_steal = in.mesh && !in.wave_traversal && kseg_max == 1 && in.steal;
  if (r.may_steal && val_bytes > 0) max_seg = std::min(max_seg, std::max(2LL, (long long)(kStealBudget / (size_t)val_bytes)));
  // the LDS-scene launches steal at any number of segments per item: at most
  // kSceneStealBudget per render lane, in whole items (kseg_max segments), one at least.
  // 4K in 16-wide tiles: 3.19 GB per segment, so five segments fit and a launch of four-segment
  // items holds four of them: C5's 1,024-pass step is eight sub-launches of 128 passes.
  if (in.lds_scene && !in.mesh && !in.wave_traversal && in.steal) {
    r.may_steal = true;
    // (the kernel indexes the store's 12-byte slots in 32 bits: a frame whose single item would
    // hold 2^32 of them does not steal)
    if (val_bytes * kseg_max >= (12LL << 32)) r.may_steal = false;
    else if (val_bytes > 0) {
      const long long fit = (long long)(kSceneStealBudget / (size_t)val_bytes);
      max_seg = std::min(max_seg, std::max(kseg_max, fit / kseg_max * kseg_max));
    }
  }
  r.max_seg = std::max(1LL, std::min(max_seg, in.n_tiles > 0 ? r.max_items / in.n_tiles : r.max_items));
  return r;
}

// Pass split: a launch with too few work items to fill the chip (C1: 256 tiles x 1 segment
// on 256 CUs, one wave per SIMD running every pass of its pixels in turn) runs one segment per
// pass instead, so the passes of a pixel run side by side in different work items; the split
// combine sums each chunk's passes from 0 in pass order (the bits of the unsplit launch).
// env_split (MCPT_PASS_SPLIT): 0/1 forces it off/on (tests, A/B), -1 decides by the item count.
inline bool pass_split(const Limits& lim, long long n_tiles, int n_passes, long long total_seg, int n_cu,
                       bool stream, int env_split) {
  const bool split_fits = !stream && n_passes > 1 && n_passes <= lim.max_seg && n_passes <= kPassSplitMaxPasses &&
                          n_tiles * (long long)n_passes <= lim.max_items;
  return split_fits && (env_split >= 0 ? env_split > 0 : n_tiles * total_seg < (long long)kPassSplitItemsPerCu * n_cu);
}

// ---- sub-launch cutting: the sub-launch that starts at pass lo of a call ending before `end`
struct SubLaunch {
  int first_pass = 0, n_passes = 0, n_segments = 0;
  long long end() const { return (long long)first_pass + n_passes; }
};
inline SubLaunch next_sub_launch(long long lo, long long end, long long max_seg, bool split) {
  const long long c0 = floor_div(lo - 1, kPassChunk);
  const long long hi = split ? end : std::min(end, (c0 + max_seg) * kPassChunk + 1);
  SubLaunch s;
  s.first_pass = (int)lo;
  s.n_passes = (int)(hi - lo);
  s.n_segments = split ? s.n_passes : (int)(floor_div(hi - 2, kPassChunk) - c0 + 1);
  return s;
}
inline int count_sub_launches(long long first_pass, long long n_passes, long long max_seg, bool split) {
  int n = 0;
  for (long long lo = first_pass, end = first_pass + n_passes; lo < end; ++n)
    lo = next_sub_launch(lo, end, max_seg, split).end();
  return n;
}

// ---- per-sub-launch facts
struct ItemsIn {
  long long n_tiles = 0;
  SubLaunch sub;
  int seg_per_item = 1, walk_exit = 0, bounces = 0, variant = 0, tile_w = 16, n_cu = 256;
  bool wave_traversal = false, pass_split = false, mesh = false;
  bool orderable = true;        // a timed megakernel launch (no count, no stream) with MCPT_ITEM_ORDER on
  bool split_items_on = true;   // MCPT_SPLIT_ITEMS
  bool tail_pieces_on = true;   // MCPT_TAIL_PIECES
};
struct Items {
  int kseg = 1;              // pass segments per work item
  long long items = 0;       // work items
  long long key[8] = {};     // the shape a sorted work-item order belongs to
  bool order = false;        // runs (and measures for) the work-item order
  bool split_items = false;
};
inline Items items(const ItemsIn& in) {
  Items r;
  // work-item order (mcpt_order.hip): launches of >= kOrderMinItems items run the order
  // sorted from an earlier launch of the same shape and measure their items for the next sort
  r.kseg = in.seg_per_item > 1 ? in.seg_per_item : 1;
  r.items = in.n_tiles * ((in.sub.n_segments + r.kseg - 1) / r.kseg);
  const long long key[8] = {r.items, in.sub.n_segments, r.kseg, in.wave_traversal, in.walk_exit, in.bounces,
                            in.variant, (long long)in.pass_split};
  std::copy(key, key + 8, r.key);
  r.order = in.orderable && r.items >= kOrderMinItems;
  // split items: mesh launches of whole 32-pass segments, one per item (MCPT_SPLIT_ITEMS=0: off)
  r.split_items = r.order && in.mesh && !in.wave_traversal && r.kseg == 1 && !in.pass_split && in.sub.n_segments > 1 &&
                  (in.sub.first_pass - 1) % kPassChunk == 0 && in.sub.n_passes % kPassChunk == 0 && in.split_items_on;
  return r;
}
// items of several segments: the cheapest (last) one workgroup-generation of the order
// runs one segment per workgroup, so the launch does not end on whole long items
// (order_valid: the launch runs a sorted order of its shape); 0: no tail pieces
inline int tail_m(const ItemsIn& in, const Items& it, bool order_valid) {
  if (!(it.order && order_valid && it.kseg > 1 && !in.pass_split && !in.mesh && in.tail_pieces_on))
    return 0;   // (the mesh kernels split items their own way)
  const int waves_simd = in.mesh ? 5 : 7;
  const long long per_cu = 4LL * waves_simd / (in.tile_w / 8);
  // (one generation: C4 +2.0 %, C2 +0.3 %; 0.5 / 2 / 3 generations no better on C4:
  // profiles/r05_ab_tail_pieces.jsonl)
  return (int)std::min(it.items / 2, per_cu * in.n_cu);
}

// ---- schedule candidates.  1 = per-lane walk, 2 = wave-coherent walk (BVH depth < 8), 3 = the
// stream schedule (the values of MCPT_TRAVERSAL_*), per-lane walks with 2 (4, on launches of >= 2
// pass segments) or 4 (5, >= 4 segments) pass segments per work item, and for BVH depth >= 8
// per-lane walks with the deep knobs (leaf batch 16, walk exit 40) and 4 (6) or 8 (7, >= 8
// segments) segments per item.
constexpr int kCandLane = 1, kCandWave = 2, kCandStream = 3, kCandLaneSeg2 = 4, kCandLaneSeg4 = 5;
// deep-BVH candidates (BVH depth >= 8): per-lane walks with the deep knobs at leaf batch 16 and
// walk exit 40 (instead of 8 / 16), four or eight segments per item.  Scene 8 (C4 workload):
// 539 / 544 Msamples/s at walk exit 32 against 515 for the defaults at four segments; walk exit
// 40 another +2..3 % at eight segments (552 / 540; with the node rows loaded together 574 / 558);
// scene 3 prefers the defaults (profiles/r03_ab_deep_knobs.jsonl, r03_ab_deep_walk_exit.jsonl,
// r02_deep_knobs_sweep.jsonl): timed, not guessed
constexpr int kCandDeepSeg4 = 6, kCandDeepSeg8 = 7, kCandLast = kCandDeepSeg8;
constexpr int kDeepLeafBatch = 16, kDeepWalkExit = 40;
// ... and they leave the walk loop only once at least 8 walks of the call have ended (shading
// rounds with more lanes): C4 shape 593 -> 608 Msamples/s; 4 / 12 / 16: 603 / 605 / 604
// (profiles/r04_ab_walk_min_done.jsonl)
constexpr int kDeepMinDone = 8;
// AUTO does not time the wave-coherent walk on BVHs at least this deep: the union of a wave's
// incoherent secondary rays visits nearly the whole tree, and on scene 8 (C4) one trial launch
// took 8.36 s against 1.81 s for the per-lane walk (profiles/r03_r03s_c4_kernel_stats.csv).  The
// stream schedule (candidate 3) is never timed by AUTO: it was 5 % behind the megakernel on
// scene 8 and 4-7x slower on shallow scenes; mcpt_set_traversal selects it.
constexpr int kWaveAutoMaxDepth = 7;

inline int cand_seg_per_item(int cand) {
  return cand == kCandLaneSeg2 ? 2 : (cand == kCandLaneSeg4 || cand == kCandDeepSeg4) ? 4 : cand == kCandDeepSeg8 ? 8 : 1;
}
// pass segments per work item: the candidate's; MCPT_SEG_PER_ITEM (env_seg > 0) overrides
inline int resolved_seg_per_item(int cand, int env_seg) { return env_seg > 0 ? env_seg : cand_seg_per_item(cand); }
inline bool cand_deep_knobs(int cand) { return cand == kCandDeepSeg4 || cand == kCandDeepSeg8; }
inline int cand_traversal(int cand) { return cand >= kCandLaneSeg2 ? kCandLane : cand; }

// Deep-BVH walk (walk_run's SUSPEND kernel): suspend the walk loop at <= walk_exit walking
// lanes and batch leaf visits (>= leaf_batch waiting lanes).  Both pay off when traversals
// are long (depth >= 8: scenes 3/7/8 +63-76 % over v6, profiles/r01_ab21_leaf_batch.jsonl)
// and cost extra rounds when they are short (scenes 1/2/6: -10-30 %), so they are off there.
// (`set`: the explicit setting, -1: by BVH depth)
inline int resolve_walk_exit(int set, int n_meshes, int depth) {
  if (set >= 0) return set;
  // mesh scenes: a lane's walk includes its instances' mesh DFSs (walk_run_mesh), long and
  // very unequal across lanes: leaving the loop once 24 lanes are done more than doubled
  // throughput in round 1 (1 M-triangle meshes 173 -> 381 Msamples/s, walk exit 40); with the
  // one-fetch mesh records of round 5, exit 24 (40 lanes done) measures best (24 / 32 / 40 / 48:
  // 840 / 784 / 760 / 691 Msamples/s, profiles/r05_ab_mesh_walk_exit.jsonl)
  if (n_meshes > 0) return 24;
  return depth >= 8 ? 16 : 0;
}
inline int resolve_leaf_batch(int set, int depth) {
  if (set >= 0) return set;
  return depth >= 8 ? 8 : 0;
}
// ... of a launch of candidate `cand`: the deep candidates' knobs, unless set explicitly
inline int cand_walk_exit(int cand, int set, int n_meshes, int depth) {
  return (cand_deep_knobs(cand) && set < 0) ? kDeepWalkExit : resolve_walk_exit(set, n_meshes, depth);
}
inline int cand_leaf_batch(int cand, int set, int depth) {
  return (cand_deep_knobs(cand) && set < 0) ? kDeepLeafBatch : resolve_leaf_batch(set, depth);
}

// AUTO times every applicable candidate kTuneRounds times and keeps each one's best time:
// round 1 in candidate order, round 2 in reverse, so that the clock ramp and cache warm-up of
// the first launches after an upload do not favour the candidates tried last (one trial each
// picked two- or four-segment items run to run on scene 6, 1-2.5 % apart)
constexpr int kTuneRounds = 2;
// The decision's one tie-break: the per-lane walk with two segments per item gives way to four
// when the four-segment trials are within kSegMargin of it (render lanes on).  The trials run in
// order, the settled schedule on the render lanes, where an item of four segments overlaps the
// previous launch's tail better: on the lanes four are 3.1 % (C2) and 3.4 % (C5) faster than two
// (profiles/r06_seg_ab.jsonl), while the in-order trials put the two within ~1-2 % of each other
// either way, so AUTO settled on two in some runs (the r06w bench: 14,585 against 14,814
// Msamples/s with four).
constexpr double kSegMargin = 0.02;
constexpr double kTuneMinSamples = 1 << 24;   // launches smaller than this are not timed

// AUTO schedule: the first sizeable launches after a scene upload run each candidate twice
// (kernel time per sample from the launch events), later launches use the fastest (results
// are identical either way).  (3, the stream schedule, is only run when selected explicitly.)
struct Tuner {
  // trial launches whose timing is not collected yet, oldest first: a trial's time is read when the
  // call after the next one starts, so that consecutive trials overlap on the render lanes as the
  // settled launches do (its period is then measured as the settled launches' is)
  struct Pending {
    int cand = 0;                   // its candidate
    double samples = 0.0;           // its samples
    long long shape[2] = {0, 0};    // its (local pixels, passes)
    int slot = 0;                   // its timing-ring slot
  };
  Pending pend[2];
  int n_pend = 0;
  long long meas_shape[2] = {0, 0};   // shape the measurements below were taken on
  int meas_segs = 0;                // pass segments of that shape (which candidates apply)
  double tune_ns[8] = {0.0};        // best ns per sample measured, by candidate (same shape)
  int tune_cnt[8] = {0};            // trials of each candidate so far
  int tune_choice = 0;              // resolved candidate once all are measured
  bool deep_auto = false;           // the deep-knob candidates apply (BVH depth >= 8, per-lane kernel)
  int overlap = 1;                  // render lanes on (MCPT_OVERLAP; 0: every launch in order)
  int depth = 0;                    // the scene's BVH depth

  // the candidates that apply to a launch of `segs` pass segments
  bool applies(int cand, long long segs) const {
    return cand == 1 || (cand == 2 && depth <= kWaveAutoMaxDepth) || (cand == kCandLaneSeg2 && segs >= 2) ||
           (cand == kCandLaneSeg4 && segs >= 4) || (cand == kCandDeepSeg4 && deep_auto && segs >= 4) ||
           (cand == kCandDeepSeg8 && deep_auto && segs >= 8);
  }
  int prefer_longer_items(int best, long long segs) const {   // (kSegMargin)
    if (overlap && best == kCandLaneSeg2 && applies(kCandLaneSeg4, segs) && tune_cnt[kCandLaneSeg4] > 0 &&
        tune_ns[kCandLaneSeg4] <= tune_ns[kCandLaneSeg2] * (1.0 + kSegMargin))
      return kCandLaneSeg4;
    return best;
  }
  // trials of candidate k issued so far on the measured shape (collected + pending)
  int issued(int k) const {
    int n = tune_cnt[k];
    for (int i = 0; i < n_pend; ++i) n += pend[i].cand == k ? 1 : 0;
    return n;
  }
  // schedule candidate of AUTO's next launch (`segs`: its pass segments)
  int next_candidate(long long segs) const {
    if (tune_choice) return tune_choice;
    // next trial: in the current round (the fewest issued trials of any applicable candidate), the
    // first candidate of the round's order not yet tried that often on the measured shape
    int round = kTuneRounds;
    for (int k = 1; k <= kCandLast; ++k)
      if (applies(k, segs)) round = std::min(round, issued(k));
    if (round >= kTuneRounds) {   // every trial issued, the last ones not collected yet: the best so far
      int best = kCandLane;
      for (int k = 1; k <= kCandLast; ++k)
        if (applies(k, segs) && tune_cnt[k] > 0 && (tune_cnt[best] == 0 || tune_ns[k] < tune_ns[best])) best = k;
      return prefer_longer_items(best, segs);
    }
    for (int i = 0; i < kCandLast; ++i) {
      const int k = (round % 2 == 0) ? 1 + i : kCandLast - i;
      if (applies(k, segs) && issued(k) == round) return k;
    }
    return kCandLane;
  }
  // a pending trial was launched on another shape than (px, passes)
  bool pending_other_shape(long long px, long long passes) const {
    bool other = false;
    for (int i = 0; i < n_pend; ++i) other |= pend[i].shape[0] != px || pend[i].shape[1] != passes;
    return other;
  }
  // a launch of candidate `cand` on shape (px, passes) of `segs` pass segments, its events in ring
  // slot `slot`, becomes a pending trial; false: not timed (settled, too small, two pending)
  bool issue(int cand, double samples, long long px, long long passes, long long segs, int slot) {
    if (tune_choice || !(samples >= kTuneMinSamples) || n_pend >= 2) return false;
    if (px != meas_shape[0] || passes != meas_shape[1]) meas_segs = (int)segs;
    Pending& t = pend[n_pend++];
    t.cand = cand;
    t.samples = samples;
    t.shape[0] = px;
    t.shape[1] = passes;
    t.slot = slot;
    return true;
  }
  Pending pop_oldest() {   // (n_pend > 0)
    const Pending t0 = pend[0];
    for (int i = 1; i < n_pend; ++i) pend[i - 1] = pend[i];
    n_pend--;
    return t0;
  }
  // a trial's time (ns per sample); decides once every applicable candidate is measured
  // kTuneRounds times
  void collect(int cand, const long long shape[2], double ns) {
    // per-sample times are compared only between launches of the same shape (pixels, passes):
    // a launch of another shape restarts the comparison
    if (shape[0] != meas_shape[0] || shape[1] != meas_shape[1]) {
      for (double& t : tune_ns) t = 0.0;
      for (int& n : tune_cnt) n = 0;
      meas_shape[0] = shape[0];
      meas_shape[1] = shape[1];
    }
    tune_ns[cand] = (tune_cnt[cand] == 0) ? ns : std::min(tune_ns[cand], ns);
    tune_cnt[cand]++;
    bool all = true;
    int best = kCandLane;
    for (int k = 1; k <= kCandLast; ++k) {
      if (!applies(k, meas_segs)) continue;
      if (tune_cnt[k] < kTuneRounds) all = false;
      else if (tune_ns[k] < tune_ns[best]) best = k;
    }
    if (all) {
      tune_choice = prefer_longer_items(best, meas_segs);
      n_pend = 0;   // (trials of another shape still pending are dropped with the decision)
    }
  }
  void reset() {   // a new scene / schedule setting: the trials start over
    n_pend = 0;
    meas_shape[0] = meas_shape[1] = 0;
    meas_segs = 0;
    for (double& t : tune_ns) t = 0.0;
    for (int& n : tune_cnt) n = 0;
    tune_choice = 0;
  }
};

}  // namespace plan
}  // namespace mcpt
