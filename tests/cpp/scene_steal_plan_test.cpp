// plan::limits for launches of the LDS-scene kernel with pass stealing: may_steal
// and the sub-launch bound against known answers, and the byte budgets in every case.
#include <cstdio>
#include <cstdlib>

#include "mcpt_plan.h"

using namespace mcpt;

static int failures = 0;
#define CHECK(c)                                                \
  do {                                                          \
    if (!(c)) {                                                 \
      std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c);  \
      failures++;                                               \
    }                                                           \
  } while (0)

static plan::LimitsIn frame(int W, int H, int tile_w, int seg_per_item) {
  plan::LimitsIn in;
  in.n_local_px = (long long)W * H;
  in.n_tiles = (long long)((W + tile_w - 1) / tile_w) * ((H + 7) / 8);
  in.tile_w = tile_w;
  in.seg_per_item = seg_per_item;
  return in;
}

// bytes of segment sums and of per-pass values that a sub-launch of max_seg segments holds
static long long partial_bytes(const plan::LimitsIn& in, long long segs) { return in.n_local_px * 12 * segs; }
static long long value_bytes(const plan::LimitsIn& in, long long segs) {
  return in.n_tiles * in.tile_w * kTileH * 12 * kPassChunk * segs;
}
static void check_budgets(const plan::LimitsIn& in, const plan::Limits& l) {
  CHECK(l.max_seg >= 1);
  // the segment-sum budget binds unless one segment alone exceeds it
  CHECK(partial_bytes(in, l.max_seg) <= (long long)in.partial_budget || l.max_seg == 1);
  if (l.may_steal && in.lds_scene) {
    // the value store: within its budget, or the single item that is its floor
    CHECK(value_bytes(in, l.max_seg) <= (long long)plan::kSceneStealBudget || l.max_seg == in.seg_per_item);
    CHECK(value_bytes(in, l.max_seg) / 12 < (1LL << 32));   // 32-bit slot index
  }
}

int main() {
  // C2: 1080p, 16-wide tiles, four segments per item.  796,262,400 B of values per segment:
  // 16 GiB / that = 21.5 -> 21 -> whole items: 20.  The segment-sum budget allows 172.
  {
    plan::LimitsIn in = frame(1920, 1080, 16, 4);
    in.lds_scene = true;
    const plan::Limits l = plan::limits(in);
    CHECK(l.may_steal && l.max_seg == 20);
    check_budgets(in, l);
    CHECK(plan::count_sub_launches(1, 256, l.max_seg, false) == 1);   // C2's step: one launch, 6.4 GB
    CHECK(value_bytes(in, 8) == 6370099200LL);
    CHECK(plan::steal_store_bytes(in.n_tiles, in.tile_w, 8) == value_bytes(in, 8));   // the plan's own size function
    CHECK(plan::steal_store_bytes(in.n_tiles, in.tile_w, l.max_seg) == value_bytes(in, l.max_seg));
    in.seg_per_item = 2;
    CHECK(plan::limits(in).may_steal && plan::limits(in).max_seg == 20);
    in.seg_per_item = 1;
    CHECK(plan::limits(in).may_steal && plan::limits(in).max_seg == 21);
    check_budgets(in, plan::limits(in));
  }
  // C5: 4K, 1,024 passes, four segments per item.  3,185,049,600 B per segment: five fit, a launch
  // holds one item of four: eight sub-launches of 128 passes.
  {
    plan::LimitsIn in = frame(3840, 2160, 16, 4);
    in.lds_scene = true;
    const plan::Limits l = plan::limits(in);
    CHECK(l.may_steal && l.max_seg == 4);
    check_budgets(in, l);
    CHECK(plan::count_sub_launches(1, 1024, l.max_seg, false) == 8);
    const plan::SubLaunch s = plan::next_sub_launch(1, 1025, l.max_seg, false);
    CHECK(s.n_passes == 128 && s.n_segments == 4);
    in.seg_per_item = 2;
    CHECK(plan::limits(in).max_seg == 4);
    in.seg_per_item = 8;   // one item exceeds the budget: the floor is the item, 25.5 GB
    CHECK(plan::limits(in).may_steal && plan::limits(in).max_seg == 8);
    check_budgets(in, plan::limits(in));
  }
  // 8K, eight segments per item: one item is 2^32 slots or more, the kernel's 32-bit index: no stealing
  {
    plan::LimitsIn in = frame(7680, 4320, 16, 8);
    in.lds_scene = true;
    const plan::Limits l = plan::limits(in);
    CHECK(!l.may_steal && l.max_seg == 10);   // 4 GiB / 398,131,200
    check_budgets(in, l);
  }
  // 32-wide tiles (scenes 1 and 2) at 1080p: 60 x 135 tiles of 256 threads = the same store
  {
    plan::LimitsIn in = frame(1920, 1080, 32, 4);
    in.lds_scene = true;
    CHECK(plan::limits(in).may_steal && plan::limits(in).max_seg == 20);
    check_budgets(in, plan::limits(in));
  }
  // a mesh shape: the answer of before, with or without the new flag
  for (int lds = 0; lds < 2; ++lds) {
    plan::LimitsIn in = frame(1920, 1080, 8, 1);
    in.mesh = true;
    in.lds_scene = lds != 0;
    const plan::Limits l = plan::limits(in);
    CHECK(l.may_steal && l.max_seg == 10);
    in.seg_per_item = 2;
    CHECK(!plan::limits(in).may_steal && plan::limits(in).max_seg == 172);
  }
  // no stealing: MCPT_STEAL=0 and adaptive launches (steal false), the wave walk, kernels that read
  // the scene through L1/L2 (lds_scene false); the segment-sum budget alone
  {
    plan::LimitsIn in = frame(1920, 1080, 16, 4);
    in.lds_scene = true;
    in.steal = false;
    CHECK(!plan::limits(in).may_steal && plan::limits(in).max_seg == 172);
    in.spare = false;   // an adaptive launch
    in.seg_per_item = 1;
    CHECK(!plan::limits(in).may_steal && plan::limits(in).max_seg == 172);
    in = frame(1920, 1080, 16, 4);
    in.lds_scene = true;
    in.wave_traversal = true;
    CHECK(!plan::limits(in).may_steal && plan::limits(in).max_seg == 172);
    check_budgets(in, plan::limits(in));
    in = frame(1920, 1080, 16, 4);
    CHECK(!plan::limits(in).may_steal && plan::limits(in).max_seg == 172);
  }
  // a small segment-sum budget still binds a stealing launch
  {
    plan::LimitsIn in = frame(40, 24, 16, 2);
    in.lds_scene = true;
    in.partial_budget = (size_t)(40 * 24 * 12 * 3);
    const plan::Limits l = plan::limits(in);
    CHECK(l.may_steal && l.max_seg == 3);
    check_budgets(in, l);
  }
  if (failures) return 1;
  std::printf("scene_steal_limits: ok\n");
  return 0;
}
