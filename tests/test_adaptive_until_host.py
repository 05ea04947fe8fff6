"""The host loop of adaptive sampling (render batches for the active blocks, select, stop at the cap or
when no block is active) asks one rule for every step: mcpt_adaptive_until_next (include/mcpt.h; the
arithmetic is csrc/mcpt_adaptive_run_plan.h, tests/cpp/adaptive_run_plan_test.cpp sweeps it against the
loops it replaced).  Here, without a GPU: the C entry through ctypes against answers worked out by hand
from the rule's statement in mcpt.h, and the Python driver over it (mcpt._adaptive_until) on recording
fakes: the exact calls it issues."""
import ctypes

import pytest

INVALID_ARG = -1   # MCPT_ERR_INVALID_ARG


def step(L, done, calls, batch, max_passes, check_every, queued_rounds):
    r, n, s = ctypes.c_int(-1), ctypes.c_int(-1), ctypes.c_int(-1)
    st = L.mcpt_adaptive_until_next(done, calls, batch, max_passes, check_every, queued_rounds, ctypes.byref(r),
                                    ctypes.byref(n), ctypes.byref(s))
    assert st == 0
    return r.value, n.value, s.value


@pytest.mark.parametrize("args, want", [
    ((0, 0, 8, 76, 1, 0), (0, 8, 0)),      # the first call: one batch in the window, no select yet
    ((8, 1, 8, 76, 1, 0), (0, 8, 1)),      # the second: a select
    ((16, 2, 8, 76, 3, 0), (0, 8, 1)),     # check_every 3: the third call selects,
    ((24, 3, 8, 76, 3, 0), (0, 8, 0)),     # the fourth does not
    ((72, 9, 8, 76, 1, 0), (0, 4, 1)),     # a short last batch
    ((72, 10, 8, 76, 3, 4), (0, 4, 1)),    # ... is a single call whatever K is; at the cap: a select
    ((76, 10, 8, 76, 1, 4), (0, 0, 0)),    # finished
    ((0, 0, 8, 76, 1, 4), (4, 0, 0)),      # a run of K rounds
    ((0, 0, 8, 76, 3, 4), (3, 0, 0)),      # trimmed to a multiple of check_every
    ((48, 6, 8, 64, 3, 4), (2, 0, 0)),     # two batches left and they end at the cap: not trimmed
    ((48, 6, 8, 76, 3, 4), (3, 0, 0)),     # three whole batches left, the cap behind them: a multiple as it is
    ((8, 1, 8, 76, 3, 4), (0, 8, 0)),      # calls no multiple of check_every: a single call
    ((0, 0, 8, 76, 5, 4), (0, 8, 0)),      # K below check_every: nothing of a run is left after the trim
    ((0, 0, 1, 1000, 1, 1000), (256, 0, 0)),   # MCPT_ADAPTIVE_RUN_MAX_ROUNDS
])
def test_until_next_known_answers(mcpt_mod, args, want):
    assert step(mcpt_mod.lib(), *args) == want


def test_until_next_refuses_bad_arguments(mcpt_mod):
    L = mcpt_mod.lib()
    out = [ctypes.c_int(7) for _ in range(3)]
    ptr = [ctypes.byref(v) for v in out]
    for bad in ((0, 0, 0, 76, 1, 0), (0, 0, 8, 76, 0, 0), (-1, 0, 8, 76, 1, 0), (0, 0, 8, 0, 1, 0), (0, -1, 8, 76, 1, 0),
                (0, 0, 8, 76, 1, -1)):
        assert L.mcpt_adaptive_until_next(*bad, *ptr) == INVALID_ARG, bad
    for k in range(3):
        assert L.mcpt_adaptive_until_next(0, 0, 8, 76, 1, 0, *[None if j == k else ptr[j] for j in range(3)]) == INVALID_ARG
    assert [v.value for v in out] == [7, 7, 7]     # a refusal writes nothing
    assert L.mcpt_adaptive_until_next(0, 0, 8, 76, 1, 0, *ptr) == 0


class Fake:
    """Recording render / select / run; active[j]: the j-th record's n_active_blocks (the last one
    repeats), short: {run index: rounds it stops after}."""

    def __init__(self, active=(3,), short=None):
        self.calls, self.active, self.short, self.n_sel, self.n_run = [], list(active), short or {}, 0, 0

    def record(self):
        rec = {"n_active_blocks": self.active[min(self.n_sel, len(self.active) - 1)], "id": self.n_sel}
        self.n_sel += 1
        return rec

    def render(self, first, n):
        self.calls.append(("render", first, n))

    def select(self):
        self.calls.append(("select",))
        return self.record()

    def run(self, first, rounds):
        self.calls.append(("run", first, rounds))
        ran = self.short.get(self.n_run, rounds)
        self.n_run += 1
        return {"rounds_run": ran, "records": [self.record()] if ran else []}


def test_driver_raw(mcpt_mod):
    f = Fake()
    rec, done, calls = mcpt_mod._adaptive_until(f.render, f.select, None, 1, 8, 20, 1)
    assert f.calls == [("render", 1, 8), ("render", 9, 8), ("select",), ("render", 17, 4), ("select",)]
    assert (rec["id"], done, calls) == (1, 20, 3)
    # check_every 2: after the second call, not the third, and at the cap; a run is never asked of None
    f = Fake()
    rec, done, calls = mcpt_mod._adaptive_until(f.render, f.select, None, 5, 4, 18, 2, queued_rounds=3)
    assert f.calls == [("render", 5, 4), ("render", 9, 4), ("select",), ("render", 13, 4), ("render", 17, 4), ("select",),
                       ("render", 21, 2), ("select",)]
    assert (rec["id"], done, calls) == (2, 18, 5)
    # the list is empty after the second select: the loop ends there
    f = Fake(active=(3, 0))
    rec, done, calls = mcpt_mod._adaptive_until(f.render, f.select, None, 1, 8, 4096, 1)
    assert f.calls == [("render", 1, 8), ("render", 9, 8), ("select",), ("render", 17, 8), ("select",)]
    assert (rec["n_active_blocks"], done, calls) == (0, 24, 3)


def test_driver_queued(mcpt_mod):
    # K = 4 at check_every 3: runs of 3 (trimmed), the short last batch as a single call with the cap's select
    f = Fake()
    rec, done, calls = mcpt_mod._adaptive_until(f.render, f.select, f.run, 1, 8, 76, 3, queued_rounds=4)
    assert f.calls == [("run", 1, 3), ("run", 25, 3), ("run", 49, 3), ("render", 73, 4), ("select",)]
    assert (rec["id"], done, calls) == (3, 76, 10)
    # a run that stops short ends the loop and its last record is the result
    f = Fake(active=(3, 0), short={1: 2})
    rec, done, calls = mcpt_mod._adaptive_until(f.render, f.select, f.run, 1, 8, 76, 1, queued_rounds=4)
    assert f.calls == [("run", 1, 4), ("run", 33, 4)]
    assert (rec["id"], rec["n_active_blocks"], done, calls) == (1, 0, 48, 6)
    # a run whose last record has no active block ends it as well, at full length
    f = Fake(active=(0,))
    rec, done, calls = mcpt_mod._adaptive_until(f.render, f.select, f.run, 1, 8, 76, 1, queued_rounds=4)
    assert f.calls == [("run", 1, 4)] and (done, calls) == (32, 4)
    # a resume enters in the middle: 16 passes in 2 calls behind it
    f = Fake()
    rec, done, calls = mcpt_mod._adaptive_until(f.render, f.select, f.run, 1, 8, 36, 1, queued_rounds=2, done=16, calls=2)
    assert f.calls == [("run", 17, 2), ("render", 33, 4), ("select",)] and (done, calls) == (36, 5)


def test_driver_selects_once_when_no_select_ran(mcpt_mod):
    # one batch only (max_passes < 2 * batch and no second call): the select the caller is owed, which
    # on a device reports MCPT_ERR_NO_STATS
    f = Fake()
    rec, done, calls = mcpt_mod._adaptive_until(f.render, f.select, f.run, 1, 8, 5, 1, queued_rounds=4)
    assert f.calls == [("render", 1, 5), ("select",)] and (rec["id"], done, calls) == (0, 5, 1)
    # a single round queued from a fresh window makes no record either
    f = Fake()
    f.run = lambda first, rounds: (f.calls.append(("run", first, rounds)), {"rounds_run": rounds, "records": []})[1]
    rec, done, calls = mcpt_mod._adaptive_until(f.render, f.select, f.run, 1, 8, 8, 1, queued_rounds=4)
    assert f.calls == [("run", 1, 1), ("select",)] and (rec["id"], done, calls) == (0, 8, 1)
