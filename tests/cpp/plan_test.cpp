// Known-answer tests of the render launch plan (csrc/mcpt_plan.h): pass geometry, limits, pass
// split, sub-launch cutting, per-sub-launch facts and AUTO's tuner, on the CPU.  Every expected
// value is derived next to its assertion from the constants of the plan, not from a run of it.
#include <cstdio>
#include <vector>

#include "mcpt_plan.h"

namespace plan = mcpt::plan;

static int g_fails = 0, g_case_fails = 0;
#define CHECK(cond)                                                        \
  do {                                                                     \
    if (!(cond)) {                                                         \
      std::printf("  line %d: CHECK(%s) failed\n", __LINE__, #cond);       \
      ++g_case_fails;                                                      \
    }                                                                      \
  } while (0)
static void done(const char* name) {
  std::printf("%s: %s\n", name, g_case_fails ? "FAIL" : "ok");
  g_fails += g_case_fails;
  g_case_fails = 0;
}

constexpr long long kSegBytesPerPx = 12;   // three floats per pixel and segment

// a W x H full-frame launch of tile width tile_w
static plan::LimitsIn frame(int W, int H, int tile_w, bool mesh) {
  plan::LimitsIn in;
  in.n_local_px = (long long)W * H;
  in.n_tiles = (long long)((W + tile_w - 1) / tile_w) * ((H + 7) / 8);
  in.tile_w = tile_w;
  in.mesh = mesh;
  return in;
}

static void test_pass_segments() {
  // chunk of pass p = floor((p - 1) / 32): passes 1..32 are chunk 0, 33..64 chunk 1, -31..0 chunk -1
  CHECK(plan::pass_segments(1, 32) == 1);     // 1..32: chunk 0
  CHECK(plan::pass_segments(1, 33) == 2);     // 1..33: chunks 0, 1
  CHECK(plan::pass_segments(32, 2) == 2);     // 32, 33: chunks 0, 1
  CHECK(plan::pass_segments(33, 1) == 1);     // 33: chunk 1
  CHECK(plan::pass_segments(7, 100) == 4);    // 7..106: chunks 0..3 (106 = 3 * 32 + 10)
  CHECK(plan::pass_segments(20, 150) == 6);   // 20..169: chunks 0..5 (169 = 5 * 32 + 9)
  CHECK(plan::pass_segments(1, 0) == 0);      // no passes
  CHECK(plan::pass_segments(0, 1) == 1);      // 0: chunk -1
  CHECK(plan::pass_segments(-31, 32) == 1);   // -31..0: chunk -1
  CHECK(plan::pass_segments(-31, 33) == 2);   // -31..1: chunks -1, 0
  CHECK(plan::floor_div(-1, 32) == -1 && plan::floor_div(-32, 32) == -1 && plan::floor_div(-33, 32) == -2);
  done("pass_segments");
}

static void test_max_seg() {
  // no stealing (no meshes): 4 GiB / (12 B x pixels)
  // 1080p: 12 x 2,073,600 = 24,883,200 B per segment; 4,294,967,296 / 24,883,200 = 172.6
  CHECK(plan::limits(frame(1920, 1080, 16, false)).max_seg == 172);
  // 4K: 12 x 8,294,400 = 99,532,800; 4,294,967,296 / 99,532,800 = 43.2
  CHECK(plan::limits(frame(3840, 2160, 16, false)).max_seg == 43);
  CHECK(!plan::limits(frame(1920, 1080, 16, false)).may_steal);
  // stealing (mesh launch, one segment per item): 8 GiB / (32 passes x 12 B x pixels), 2 at least
  // 1080p: 32 x 24,883,200 = 796,262,400; 8,589,934,592 / 796,262,400 = 10.8
  plan::Limits l = plan::limits(frame(1920, 1080, 8, true));
  CHECK(l.may_steal && l.max_seg == 10);
  // 4K: 32 x 99,532,800 = 3,185,049,600; 8,589,934,592 / that = 2.7 -> 2 (= the floor)
  CHECK(plan::limits(frame(3840, 2160, 8, true)).max_seg == 2);
  // 8K: 32 x 12 x 33,177,600 = 12,740,198,400 > 8 GiB: quotient 0 -> the floor 2 (the segment-sum
  // budget allows 4 GiB / 398,131,200 = 10)
  CHECK(plan::limits(frame(7680, 4320, 8, true)).max_seg == 2);
  done("max_seg");
}

// the pass-stealing value store: 12 B x 32 passes x tile threads per tile and segment, and the
// sub-launch bounds it gives (the values of before the store had one size function)
static void test_steal_store() {
  plan::LimitsIn in = frame(1920, 1080, 8, true);   // 240 x 135 = 32,400 tiles of 64 threads
  CHECK(in.n_tiles == 32400);
  CHECK(plan::steal_store_bytes(in.n_tiles, 8, 10) == 7962624000LL);   // 32,400 x 10 x 32 x 64 x 12
  CHECK(plan::steal_store_bytes(in.n_tiles, 8, 10) <= (long long)plan::kStealBudget);
  CHECK(plan::steal_store_bytes(in.n_tiles, 8, 11) > (long long)plan::kStealBudget);
  CHECK(plan::limits(in).max_seg == 10);
  in = frame(3840, 2160, 8, true);   // 480 x 270 = 129,600 tiles
  CHECK(plan::steal_store_bytes(in.n_tiles, 8, 2) == 6370099200LL);   // 129,600 x 2 x 32 x 64 x 12
  CHECK(plan::limits(in).max_seg == 2);
  // 253 x 131: 32 x 17 = 544 tiles, the partial ones whole in the store (not 33,143 px / 64 = 517.9)
  in = frame(253, 131, 8, true);
  CHECK(in.n_tiles == 544);
  CHECK(plan::steal_store_bytes(in.n_tiles, 8, 1) == 544LL * 32 * 64 * 12);   // 13,369,344
  // 8 GiB / 13,369,344 = 642.5 (the segment-sum budget allows 10,799).  Sized by pixels, 8 GiB /
  // (33,143 x 32 x 12) gave 674, whose store of 544 tiles is 9,010,937,856 B > 8 GiB: the one
  // shape here whose bound moves, and only above the 24 segments the suite renders at this size
  CHECK(plan::limits(in).max_seg == 642);
  CHECK(plan::steal_store_bytes(in.n_tiles, 8, 674) > (long long)plan::kStealBudget);
  in.partial_budget = (size_t)(253 * 131 * 12 * 8);   // (tests/test_gpu_work_items.py: eight segments)
  CHECK(plan::limits(in).max_seg == 8);
  // the LDS-scene kernels' store at 1080p in 16-wide tiles: 120 x 135 tiles of 128 threads
  in = frame(1920, 1080, 16, false);
  in.lds_scene = true;
  in.seg_per_item = 4;
  CHECK(plan::steal_store_bytes(in.n_tiles, 16, 8) == in.n_tiles * 16 * mcpt::kTileH * 12 * mcpt::kPassChunk * 8);
  CHECK(plan::steal_store_bytes(in.n_tiles, 16, 8) == 6370099200LL);
  CHECK(plan::limits(in).max_seg == 20);
  in.seg_per_item = 1;
  CHECK(plan::limits(in).max_seg == 21);
  in = frame(3840, 2160, 16, false);
  in.lds_scene = true;
  in.seg_per_item = 4;
  CHECK(plan::limits(in).max_seg == 4);
  done("steal_store");
}

static void test_may_steal() {
  plan::LimitsIn in = frame(1920, 1080, 8, true);
  CHECK(plan::limits(in).may_steal);
  in.seg_per_item = 2;
  CHECK(!plan::limits(in).may_steal && plan::limits(in).max_seg == 172);   // (the segment-sum budget alone)
  in = frame(1920, 1080, 8, true);
  in.wave_traversal = true;
  CHECK(!plan::limits(in).may_steal);
  in = frame(1920, 1080, 8, false);
  CHECK(!plan::limits(in).may_steal);
  in = frame(1920, 1080, 8, true);
  in.steal = false;
  CHECK(!plan::limits(in).may_steal && plan::limits(in).max_seg == 172);
  done("may_steal");
}

static void test_grid_bound() {
  for (int tile_w : {8, 16, 32})
    for (int K : {1, 8}) {
      // 2^32 work-items of tile_w x 8 lanes each, less one, less the spare workgroups: 1024 split
      // items x 3 further pieces, and 28 tail-piece workgroups per CU and further segment of an item
      const long long want = (1LL << 32) / (tile_w * 8) - 1 - (1024 * 3 + 28LL * 256 * (K - 1));
      plan::LimitsIn in;
      in.tile_w = tile_w; in.seg_per_item = K; in.n_cu = 256;
      in.n_tiles = want;
      CHECK(plan::limits(in).max_items == want && !plan::limits(in).too_large);
      in.n_tiles = want + 1;
      CHECK(plan::limits(in).too_large);
      // no pixels: the budget does not bind (2^30), the grid does: max_items / n_tiles
      in.n_tiles = want / 3;
      CHECK(plan::limits(in).max_seg == 3);
      in.n_tiles = want / 3 + 1;
      CHECK(plan::limits(in).max_seg == 2);
      // an adaptive launch reserves no spare workgroups
      in.spare = false;
      CHECK(plan::limits(in).max_items == (1LL << 32) / (tile_w * 8) - 1);
    }
  done("grid_bound");
}

static void test_cutting() {
  const int firsts[3] = {1, 20, 7}, counts[3] = {200, 150, 33};
  for (int b = 1; b <= 3; ++b) {
    // 24 x 16 pixels: 384 x 12 B = 4,608 B per segment, a budget of b segments
    plan::LimitsIn in = frame(24, 16, 16, false);
    in.partial_budget = (size_t)(24 * 16 * kSegBytesPerPx * b);
    const long long max_seg = plan::limits(in).max_seg;
    CHECK(max_seg == b);
    for (int i = 0; i < 3; ++i) {
      const int first = firsts[i], S = counts[i];
      const int chunks = (first + S - 2) / 32 - (first - 1) / 32 + 1;   // (positive passes: plain division)
      std::vector<plan::SubLaunch> subs;
      for (long long lo = first, end = first + S; lo < end; lo = subs.back().end())
        subs.push_back(plan::next_sub_launch(lo, end, max_seg, false));
      CHECK((int)subs.size() == (chunks + b - 1) / b);
      CHECK(plan::count_sub_launches(first, S, max_seg, false) == (int)subs.size());
      long long at = first, segs = 0;
      for (size_t k = 0; k < subs.size(); ++k) {
        CHECK(subs[k].first_pass == at && subs[k].n_passes > 0);   // the pieces tile the range
        if (k > 0) CHECK((subs[k].first_pass - 1) % 32 == 0);      // cut at a chunk boundary
        CHECK(subs[k].n_segments <= b);
        at = subs[k].end();
        segs += subs[k].n_segments;
      }
      CHECK(at == first + S && segs == chunks && segs == plan::pass_segments(first, S));
    }
  }
  // 1080p, default budget: 172 segments = 5,504 passes from a chunk's first pass
  const long long m = plan::limits(frame(1920, 1080, 16, false)).max_seg;
  CHECK(plan::count_sub_launches(1, 5504, m, false) == 1);
  CHECK(plan::count_sub_launches(1, 5505, m, false) == 2);
  const plan::SubLaunch a = plan::next_sub_launch(1, 5506, m, false), b2 = plan::next_sub_launch(a.end(), 5506, m, false);
  CHECK(a.n_passes == 5504 && a.n_segments == 172 && b2.first_pass == 5505 && b2.n_passes == 1 && b2.n_segments == 1);
  CHECK(plan::count_sub_launches(2, 5504, m, false) == 2);   // passes 2..5505 touch 173 chunks
  // pass split: the whole call, one segment per pass
  const plan::SubLaunch s = plan::next_sub_launch(5, 5 + 100, 1, true);
  CHECK(s.first_pass == 5 && s.n_passes == 100 && s.n_segments == 100 && plan::count_sub_launches(5, 100, 1, true) == 1);
  CHECK(plan::count_sub_launches(1, 0, 1, false) == 0);
  done("cutting");
}

static void test_pass_split() {
  // 256 CUs: a split below 4 x 256 = 1,024 work items (tiles x pass segments), at most 256 passes
  plan::LimitsIn in;
  in.tile_w = 16; in.n_cu = 256;
  in.n_tiles = 256; in.n_local_px = 256 * 128;
  const plan::Limits small = plan::limits(in);
  CHECK(plan::pass_split(small, 256, 4, 1, 256, false, -1));      // 256 x 1 segment < 1,024
  CHECK(!plan::pass_split(small, 256, 1, 1, 256, false, -1));     // one pass: nothing to split
  CHECK(!plan::pass_split(small, 256, 1, 1, 256, false, 1));
  in.n_tiles = 8160; in.n_local_px = 8160 * 128;
  const plan::Limits big = plan::limits(in);
  CHECK(!plan::pass_split(big, 8160, 2, 1, 256, false, -1));      // 8,160 >= 1,024
  CHECK(plan::pass_split(big, 8160, 2, 1, 256, false, 1));        // forced on: it fits
  CHECK(!plan::pass_split(small, 256, 257, 9, 256, false, -1));   // 257 > 256 passes
  CHECK(!plan::pass_split(small, 256, 257, 9, 256, false, 1));
  CHECK(plan::pass_split(small, 256, 256, 8, 256, false, 1));
  CHECK(!plan::pass_split(small, 256, 4, 1, 256, false, 0));      // forced off
  CHECK(!plan::pass_split(small, 256, 4, 1, 256, true, -1));      // the stream schedule
  CHECK(!plan::pass_split(small, 256, 4, 1, 256, true, 1));
  done("pass_split");
}

static void test_items() {
  plan::ItemsIn in;
  in.n_tiles = 4095;
  in.sub = plan::next_sub_launch(1, 33, 100, false);   // 32 passes: one segment
  CHECK(plan::items(in).items == 4095 && !plan::items(in).order);   // below kOrderMinItems = 4096
  in.n_tiles = 4096;
  CHECK(plan::items(in).order);
  in.orderable = false;
  CHECK(!plan::items(in).order);
  // the order key: items, segments, segments per item, wave walk, walk exit, bounces, variant, pass split
  in = plan::ItemsIn();
  in.n_tiles = 5000; in.seg_per_item = 4; in.walk_exit = 16; in.bounces = 8; in.variant = 2;
  in.sub = plan::next_sub_launch(1, 1 + 320, 100, false);   // 10 segments: ceil(10 / 4) = 3 items per tile
  const plan::Items it = plan::items(in);
  const long long want[8] = {15000, 10, 4, 0, 16, 8, 2, 0};
  for (int i = 0; i < 8; ++i) CHECK(it.key[i] == want[i]);
  CHECK(it.kseg == 4 && it.items == 15000);
  // split items: mesh launches of whole segments from a chunk's first pass, one segment per item
  in = plan::ItemsIn();
  in.n_tiles = 4096; in.mesh = true; in.tile_w = 8;
  in.sub = plan::next_sub_launch(1, 65, 100, false);   // passes 1..64: two whole segments
  CHECK(in.sub.n_segments == 2 && plan::items(in).split_items);
  in.sub = plan::next_sub_launch(2, 66, 100, false);   // starts inside a chunk
  CHECK(!plan::items(in).split_items);
  in.sub = plan::next_sub_launch(1, 49, 100, false);   // 48 passes: a partial last segment
  CHECK(in.sub.n_segments == 2 && !plan::items(in).split_items);
  in.sub = plan::next_sub_launch(1, 33, 100, false);   // one segment
  CHECK(!plan::items(in).split_items);
  in.sub = plan::next_sub_launch(1, 65, 100, false);
  in.seg_per_item = 2;
  CHECK(!plan::items(in).split_items);
  in.seg_per_item = 1; in.split_items_on = false;
  CHECK(!plan::items(in).split_items);
  in.split_items_on = true; in.mesh = false;
  CHECK(!plan::items(in).split_items);
  // tail pieces: tile_w 16 = two waves per workgroup, 7 waves per SIMD: 4 x 7 / 2 = 14 workgroups per
  // CU, x 256 CUs = 3,584; half the items at most
  in = plan::ItemsIn();
  in.tile_w = 16; in.seg_per_item = 4; in.n_cu = 256;
  in.n_tiles = 16200;
  in.sub = plan::next_sub_launch(1, 257, 100, false);   // 8 segments: 2 items per tile, 32,400 items
  CHECK(plan::tail_m(in, plan::items(in), true) == 14 * 256);
  CHECK(plan::tail_m(in, plan::items(in), false) == 0);   // no sorted order of the shape yet
  in.n_tiles = 1500;
  in.sub = plan::next_sub_launch(1, 513, 100, false);   // 16 segments: 4 items per tile, 6,000 items
  CHECK(plan::tail_m(in, plan::items(in), true) == 3000);
  in.mesh = true;
  CHECK(plan::tail_m(in, plan::items(in), true) == 0);
  in.mesh = false; in.pass_split = true;
  CHECK(plan::tail_m(in, plan::items(in), true) == 0);
  in.pass_split = false; in.seg_per_item = 1;
  CHECK(plan::tail_m(in, plan::items(in), true) == 0);
  in.seg_per_item = 4; in.tail_pieces_on = false;
  CHECK(plan::tail_m(in, plan::items(in), true) == 0);
  done("items");
}

// One AUTO launch as launch() drives the tuner: collect while more than one trial is pending (the
// synthetic time of candidate k's n-th trial is ns[k][n]), pick the candidate, issue the trial.
struct TunerRun {
  plan::Tuner t;
  long long px = 1 << 20, passes = 256, segs = 8;   // 2^28 samples
  double ns[8][4] = {};
  int n_collected = 0, seen[8] = {};
  void collect_one() {
    const plan::Tuner::Pending p = t.pop_oldest();
    t.collect(p.cand, p.shape, ns[p.cand][seen[p.cand]++]);
    ++n_collected;
  }
  int call() {
    while (t.n_pend > 1) collect_one();
    const int cand = t.next_candidate(segs);
    t.issue(cand, (double)px * (double)passes, px, passes, segs, 0);
    return cand;
  }
};

static void test_tuner_order() {
  {
    // depth 5, 8 segments: 1, 2 (depth < 8), 4 (>= 2 segments), 5 (>= 4); 6 and 7 need depth >= 8
    TunerRun r;
    r.t.depth = 5;
    // best of two: candidate 2 (9.5, 4.0); lowest mean and lowest first trial: candidate 4 (6, 6)
    const double ns[8][2] = {{0, 0}, {8, 8}, {9.5, 4.0}, {0, 0}, {6, 6}, {7, 7}, {0, 0}, {0, 0}};
    for (int k = 0; k < 8; ++k) for (int n = 0; n < 4; ++n) r.ns[k][n] = ns[k][n < 2 ? n : 1];
    const int want[8] = {1, 2, 4, 5, 5, 4, 2, 1};
    for (int i = 0; i < 8; ++i) CHECK(r.call() == want[i]);
    CHECK(r.n_collected == 6 && r.t.n_pend == 2 && r.t.tune_choice == 0);
    r.call();   // (collects the seventh trial; every trial is issued: runs the best so far)
    CHECK(r.n_collected == 7 && r.t.tune_choice == 0);
    r.collect_one();
    CHECK(r.n_collected == 8 && r.t.tune_choice == 2 && r.t.n_pend == 0);
    CHECK(r.t.next_candidate(8) == 2);
    r.t.reset();
    CHECK(r.t.tune_choice == 0 && r.t.n_pend == 0 && r.t.next_candidate(8) == 1 && r.t.depth == 5);
  }
  {
    // depth 8: no wave walk (2), the deep candidates 6 (>= 4 segments) and 7 (>= 8) apply
    TunerRun r;
    r.t.depth = 8; r.t.deep_auto = true;
    const int want[10] = {1, 4, 5, 6, 7, 7, 6, 5, 4, 1};
    for (int i = 0; i < 10; ++i) CHECK(r.call() == want[i]);
  }
  {
    TunerRun r;   // one segment, depth 8: the per-lane walk alone
    r.t.depth = 8; r.t.deep_auto = true; r.passes = 32; r.segs = 1;
    CHECK(r.call() == 1 && r.call() == 1);
    TunerRun q;   // one segment, depth 5: 1, 2 and back
    q.t.depth = 5; q.passes = 32; q.segs = 1;
    const int want[4] = {1, 2, 2, 1};
    for (int i = 0; i < 4; ++i) CHECK(q.call() == want[i]);
  }
  done("tuner_order");
}

// depth 5, 8 segments, every trial of candidate k at ns[k]: the decision
static int decide(const double ns[8], int overlap) {
  TunerRun r;
  r.t.depth = 5; r.t.overlap = overlap;
  for (int k = 0; k < 8; ++k) for (int n = 0; n < 4; ++n) r.ns[k][n] = ns[k];
  for (int i = 0; i < 12 && !r.t.tune_choice; ++i) r.call();
  return r.t.tune_choice;
}

static void test_tuner_decision() {
  // two segments per item (4) fastest, four (5) 1.9 % behind: within kSegMargin = 2 %
  const double near[8] = {0, 10, 10, 0, 1.0, 1.019, 0, 0}, far[8] = {0, 10, 10, 0, 1.0, 1.021, 0, 0};
  CHECK(decide(near, 1) == 5);   // render lanes on: the longer items
  CHECK(decide(far, 1) == 4);    // 2.1 % behind
  CHECK(decide(near, 0) == 4);   // render lanes off
  {
    plan::Tuner t;   // a trial of another shape restarts the comparison
    const long long A[2] = {1000, 64}, B[2] = {2000, 64};
    t.collect(1, A, 5.0);
    CHECK(t.tune_cnt[1] == 1 && t.meas_shape[0] == 1000);
    t.collect(2, B, 3.0);
    CHECK(t.tune_cnt[1] == 0 && t.tune_cnt[2] == 1 && t.tune_ns[2] == 3.0 && t.meas_shape[0] == 2000);
  }
  {
    plan::Tuner t;   // depth 8, one segment: candidate 1 twice decides; a pending trial of shape B is dropped
    t.depth = 8; t.deep_auto = true;
    const double samples = (double)(1 << 24);
    CHECK(t.issue(1, samples, 1 << 19, 32, 1, 3) && t.issue(1, samples, 1 << 19, 32, 1, 4));
    CHECK(!t.issue(1, samples, 1 << 19, 32, 1, 5) && t.n_pend == 2);   // a third pending trial
    plan::Tuner::Pending p = t.pop_oldest();
    CHECK(p.slot == 3 && p.cand == 1);
    t.collect(p.cand, p.shape, 2.0);
    CHECK(t.issue(1, samples, 1 << 18, 32, 1, 6) && t.n_pend == 2);    // shape B
    CHECK(t.pending_other_shape(1 << 19, 32) && t.tune_choice == 0);
    p = t.pop_oldest();
    t.collect(p.cand, p.shape, 3.0);
    CHECK(t.tune_choice == 1 && t.n_pend == 0 && t.tune_ns[1] == 2.0);
    CHECK(!t.issue(1, samples, 1 << 19, 32, 1, 7));                    // settled
  }
  {
    plan::Tuner t;   // launches under 2^24 samples are not timed
    CHECK(!t.issue(1, (double)((1 << 24) - 1), 1 << 12, 4095, 128, 0) && t.n_pend == 0);
    CHECK(t.issue(1, (double)(1 << 24), 1 << 12, 4096, 128, 0) && t.n_pend == 1 && t.meas_segs == 128);
  }
  done("tuner_decision");
}

static void test_candidate_knobs() {
  const int seg[8] = {1, 1, 1, 1, 2, 4, 4, 8};   // candidates 4..7: two, four, four (deep), eight (deep)
  for (int k = 1; k < 8; ++k) {
    CHECK(plan::cand_seg_per_item(k) == seg[k] && plan::resolved_seg_per_item(k, 0) == seg[k]);
    CHECK(plan::resolved_seg_per_item(k, 3) == 3);   // MCPT_SEG_PER_ITEM overrides
    CHECK(plan::cand_traversal(k) == (k <= 3 ? k : 1));
    CHECK(plan::cand_deep_knobs(k) == (k >= 6));
  }
  // walk exit: set explicitly, else 24 on mesh scenes, 16 from depth 8, 0 below; deep candidates 40
  CHECK(plan::resolve_walk_exit(5, 2, 9) == 5 && plan::resolve_walk_exit(-1, 2, 9) == 24);
  CHECK(plan::resolve_walk_exit(-1, 0, 8) == 16 && plan::resolve_walk_exit(-1, 0, 7) == 0);
  CHECK(plan::cand_walk_exit(6, -1, 0, 8) == 40 && plan::cand_walk_exit(6, 5, 0, 8) == 5 && plan::cand_walk_exit(5, -1, 0, 8) == 16);
  // leaf batch: set explicitly, else 8 from depth 8, 0 below; deep candidates 16
  CHECK(plan::resolve_leaf_batch(3, 9) == 3 && plan::resolve_leaf_batch(-1, 8) == 8 && plan::resolve_leaf_batch(-1, 7) == 0);
  CHECK(plan::cand_leaf_batch(7, -1, 8) == 16 && plan::cand_leaf_batch(7, 4, 8) == 4 && plan::cand_leaf_batch(1, -1, 8) == 8);
  done("candidate_knobs");
}

int main() {
  test_pass_segments();
  test_max_seg();
  test_may_steal();
  test_steal_store();
  test_grid_bound();
  test_cutting();
  test_pass_split();
  test_items();
  test_tuner_order();
  test_tuner_decision();
  test_candidate_knobs();
  std::printf("%d failures\n", g_fails);
  return g_fails ? 1 : 0;
}
