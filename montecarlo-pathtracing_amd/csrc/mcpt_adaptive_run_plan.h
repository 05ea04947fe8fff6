// mcpt_adaptive_run_plan.h — the schedule of a queued adaptive run (mcpt_adaptive_run*,
// mcpt_capi_post.hip): which rounds select, the grid that holds the list whatever
// it shrinks to, and what the host loop over mcpt_render_adaptive / mcpt_adaptive_select would have
// done, from the list lengths the selects left on the device; and the step rule of the host loops
// that issue those calls and runs until a render is finished (until_next).  Plain host code, no HIP and no
// context: tests/cpp/adaptive_run_plan_test.cpp checks it against known answers on the CPU.
#pragma once

namespace mcpt {
namespace plan {

constexpr int kAdaptiveRunMaxRounds = 256;   // = MCPT_ADAPTIVE_RUN_MAX_ROUNDS (mcpt.h)

// round i (0-based) of a run of `rounds` ends in a select: the window then holds two batches or more
// (batches_on_entry before the run, one more per round) and the round is a multiple of check_every
// or the run's last
inline bool run_round_selects(int i, int rounds, int check_every, int batches_on_entry) {
  if (i < 0 || i >= rounds || check_every <= 0) return false;
  return (long long)batches_on_entry + i + 1 >= 2 && ((i + 1) % check_every == 0 || i == rounds - 1);
}

// the selects the schedule can run: what records[] must hold
inline int run_select_count(int rounds, int check_every, int batches_on_entry) {
  int n = 0;
  for (int i = 0; i < rounds; ++i) n += run_round_selects(i, rounds, check_every, batches_on_entry) ? 1 : 0;
  return n;
}

// Workgroup groups of a list launch over at most n_list blocks, tile_w / 8 blocks per group (tile
// widths 8, 16, 32).  The list only shrinks during a run, so the groups of its length on entry hold
// every later list; the kernels read the real length on the device.
inline int run_list_groups(int n_list, int tile_w) {
  const int per_group = tile_w / 8;
  if (n_list <= 0 || per_group <= 0) return 0;
  return (int)(((long long)n_list + per_group - 1) / per_group);
}

// What the host loop would have done, from the length the list had on entry and the lengths the
// queued selects left (lengths[k]: select k's, in order; n_lengths of them): a round runs while the
// list is not empty, and the first select that reports 0 is the last one that ran.  Every queued
// round after it changed nothing on the device.
struct RunOutcome {
  int rounds_run;    // rounds the host loop would have rendered
  int selects_run;   // ... and the selects it would have made (records[] entries that count)
  int n_list;        // the list's length afterwards
};
inline RunOutcome run_outcome(int rounds, int check_every, int batches_on_entry, int n_list_on_entry,
                              const int* lengths, int n_lengths) {
  RunOutcome o = {0, 0, n_list_on_entry};
  for (int i = 0; i < rounds && o.n_list > 0; ++i) {
    o.rounds_run = i + 1;
    if (!run_round_selects(i, rounds, check_every, batches_on_entry)) continue;
    if (o.selects_run >= n_lengths) break;   // (fewer lengths than the schedule's selects: stop at what is known)
    o.n_list = lengths[o.selects_run++];
  }
  return o;
}

// The host side of the schedule (mcpt_adaptive_until_next, mcpt.h, states the contract): the step that
// follows `done` passes in `calls` render calls.  *rounds > 0: a queued run.  Its selects fall on the
// multiples of check_every counted from ITS first round and after its last, so it starts on a multiple
// of check_every calls, holds whole batches only and is trimmed to a multiple unless it ends at the
// cap.  Else *n_passes > 0: a single call, *select: a select follows it.  Both 0: finished.  false,
// nothing written: a bad argument.
inline bool until_next(int done, int calls, int batch, int max_passes, int check_every, int queued_rounds,
                       int* rounds, int* n_passes, int* select) {
  if (batch <= 0 || max_passes <= 0 || check_every <= 0 || done < 0 || calls < 0 || queued_rounds < 0 || !rounds ||
      !n_passes || !select)
    return false;
  *rounds = *n_passes = *select = 0;
  if (done >= max_passes) return true;
  const int left = max_passes - done, full = left / batch;
  int r = queued_rounds > 0 && calls % check_every == 0 ? queued_rounds : 0;
  r = r < full ? r : full;
  r = r < kAdaptiveRunMaxRounds ? r : kAdaptiveRunMaxRounds;
  if (!(r == full && r * batch == left)) r -= r % check_every;
  if ((*rounds = r) > 0) return true;
  *n_passes = batch < left ? batch : left;
  const long long then = (long long)calls + 1;
  *select = then >= 2 && (then % check_every == 0 || *n_passes == left);
  return true;
}

}  // namespace plan
}  // namespace mcpt
