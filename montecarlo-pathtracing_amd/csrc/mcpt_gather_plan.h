// mcpt_gather_plan.h — the row plan of the frame gathers (mcpt_capi_gather.hip):
// which targets are full frames, which shard sets cover a frame, which runs of a shard's rows are
// one contiguous copy.  Plain host code, no HIP and no context: tests/cpp/gather_plan_test.cpp
// checks it against known answers on the CPU.
#pragma once
#include <cstddef>
#include <vector>

namespace mcpt {
namespace plan {

// the target is a full frame in row order: H rows, local row i = global row i
inline bool is_full_frame(const std::vector<int>& rows, int H) {
  if (H < 0 || rows.size() != (size_t)H) return false;
  for (int i = 0; i < H; ++i)
    if (rows[(size_t)i] != i) return false;
  return true;
}

// every frame row 0 .. H-1 is held by exactly one of the n_shards row lists; a row outside 0 .. H-1
// makes the answer false (the gathers' own loops indexed held[y] unchecked, relying on
// mcpt_set_target_rows having refused such a row)
inline bool rows_held_once(const std::vector<int>* const* shard_rows, int n_shards, int H) {
  std::vector<int> held((size_t)(H > 0 ? H : 0), 0);
  for (int k = 0; k < n_shards; ++k)
    for (int y : *shard_rows[k]) {
      if (y < 0 || y >= H) return false;
      ++held[(size_t)y];
    }
  for (int n : held)
    if (n != 1) return false;
  return true;
}

// a maximal run of consecutive global rows of a shard: local rows local_first .. local_first + n - 1
// are global rows global_first .. global_first + n - 1 (one contiguous copy)
struct RowRun { int local_first, global_first, n; };
inline std::vector<RowRun> row_runs(const std::vector<int>& rows) {
  std::vector<RowRun> runs;
  const int n_rows = (int)rows.size();
  for (int i = 0; i < n_rows;) {
    int j = i + 1;
    while (j < n_rows && rows[(size_t)j] == rows[(size_t)j - 1] + 1) ++j;
    runs.push_back({i, rows[(size_t)i], j - i});
    i = j;
  }
  return runs;
}

// every frame row's source row lies inside a packed buffer of src_rows rows
inline bool src_rows_in_range(const int* src_row, int H, long long src_rows) {
  for (int y = 0; y < H; ++y)
    if (src_row[y] < 0 || src_row[y] >= src_rows) return false;
  return true;
}

}  // namespace plan
}  // namespace mcpt
