"""The status codes the four adaptive select entry points refuse with (mcpt_adaptive_select,
mcpt_adaptive_select_filtered, mcpt_adaptive_run, mcpt_adaptive_run_filtered; DESIGN.md §3.9, §3.9.2,
§3.9.3), through the raw C ABI, in states where several reasons for a refusal hold at once: the code
that comes back pins which check runs first.  After every refusal the context is what it was.  Host-side
argument checks only: nothing here reaches a kernel of the selects, and no message text is read.

(The adaptive mode needs the statistics and goes off with them, so "statistics off" is always "mode off"
too: MCPT_ERR_NO_ADAPTIVE.  What a caller can reach of the statistics' refusals is the two-batch rule.)"""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

W, H, N = 37, 21, 8                  # partial blocks on both axes; batches of 8 passes
FLOOR, BOUNCES = 0.01, 3
OK, INVALID, NO_GUIDES, NO_STATS, NO_ADAPTIVE = 0, -1, -7, -8, -9
NAN, INF = float("nan"), float("inf")


@pytest.fixture(scope="module")
def ctx(mcpt_mod):
    r = mcpt_mod.Renderer(0)
    r.upload_scene(mcpt_mod.Scene.reference(6))
    yield r
    r.close()


class Calls:
    """The four entry points with arguments every check accepts; a keyword replaces one of them."""

    def __init__(self, mcpt_mod, r):
        self.m, self.r, self.L = mcpt_mod, r, mcpt_mod.lib()
        self.cam = [np.ascontiguousarray(a, np.float32) for a in mcpt_mod.camera_canonical(W, H)]
        self.rec, self.rec_f = mcpt_mod.Adaptive(), mcpt_mod.AdaptiveFiltered()
        self.recs, self.recs_f = (mcpt_mod.Adaptive * 4)(), (mcpt_mod.AdaptiveFiltered * 4)()
        self.out = mcpt_mod.AdaptiveRun()

    def select(self, thr=0.05, floor=FLOOR, out=True):
        return self.L.mcpt_adaptive_select(self.r._h, thr, floor, ctypes.byref(self.rec) if out else None)

    def select_filtered(self, thr=0.05, cap=64.0, floor=FLOOR, it=2, k=3.0, sp=0.75, out=True):
        return self.L.mcpt_adaptive_select_filtered(self.r._h, thr, cap, floor, it, k, sp,
                                                    ctypes.byref(self.rec_f) if out else None)

    def _cam(self):
        return self.m._fp(self.cam[0]), self.m._fp(self.cam[1])

    def run(self, first=17, n=N, rounds=4, ce=1, thr=0.05, floor=FLOOR, variant=0, records=True, capacity=4, out=True):
        return self.L.mcpt_adaptive_run(self.r._h, *self._cam(), first, n, rounds, ce, thr, floor, 0.0, BOUNCES, 1.0,
                                        variant, self.recs if records else None, capacity,
                                        ctypes.byref(self.out) if out else None)

    def run_filtered(self, first=17, n=N, rounds=4, ce=1, thr=0.05, cap=64.0, floor=FLOOR, it=2, k=3.0, sp=0.75,
                     variant=0, records=True, capacity=4, out=True):
        return self.L.mcpt_adaptive_run_filtered(self.r._h, *self._cam(), first, n, rounds, ce, thr, cap, floor, it, k,
                                                 sp, 0.0, BOUNCES, 1.0, variant, self.recs_f if records else None,
                                                 capacity, ctypes.byref(self.out) if out else None)


@pytest.fixture(scope="module")
def calls(mcpt_mod, ctx):
    return Calls(mcpt_mod, ctx)


def begin(mcpt_mod, r, batches, guides=False, rows=None):
    """Target (the old state goes with it), (guides,) a statistics window, the adaptive mode and `batches`
    rounds of N passes for every block."""
    if rows is None:
        r.set_target(W, H)
    else:
        r.set_target_rows(W, H, rows)
    cam = mcpt_mod.camera_canonical(W, H)
    if guides:
        r.render_guides(*cam)
    r.stats_begin()
    r.adaptive_begin(0)
    for i in range(batches):
        r.render_adaptive(cam[0], cam[1], 1 + N * i, N, 0.0, BOUNCES, 1.0, 0)


def load_own_counts(r):
    """The count plane of a gathered frame: a counted load of the context's own packed pixels."""
    buf = torch.zeros((H, W, 4), dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    r.pack_counted_device(buf.data_ptr(), H * W * 16)
    r.synchronize()
    r.load_rows_counted(buf.data_ptr(), H, np.arange(H, dtype=np.int32), r.pass_count())
    r.synchronize()
    return buf


def snapshot(mcpt_mod, r):
    acc, n = r.read_accum()
    s = {"info": r.adaptive_info(), "stats": r.stats_info(), "source": r.error_map_source(), "pass_count": n,
         "accum": np.ascontiguousarray(acc, np.float32).view(np.uint32)}
    try:
        s["active"] = r.read_active_blocks()
    except mcpt_mod.MCPTError:
        s["active"] = None                                     # (the mode is off)
    return s


def assert_unchanged(before, after, what):
    assert before.keys() == after.keys()
    for k in before:
        if isinstance(before[k], np.ndarray):
            assert after[k] is not None and np.array_equal(before[k], after[k]), (what, k)
        else:
            assert before[k] == after[k], (what, k, before[k], after[k])


def check_table(mcpt_mod, r, calls, table):
    """Every (entry point, its replaced arguments, the status) of a state, the context unchanged after each."""
    before = snapshot(mcpt_mod, r)
    for name, kw, want in table:
        got = getattr(calls, name)(**kw)
        assert got == want, (name, kw, got, want)
        assert_unchanged(before, snapshot(mcpt_mod, r), (name, kw))
    return before


def test_mode_off_comes_before_the_arguments(mcpt_mod, ctx, calls):
    """The mode off (statistics on, two batches, guides) and a bad threshold: NO_ADAPTIVE; only a single
    select's missing record comes before it."""
    begin(mcpt_mod, ctx, 2, guides=True)
    ctx.adaptive_end()
    before = check_table(mcpt_mod, ctx, calls, [
        ("select", {"thr": 0.0}, NO_ADAPTIVE),
        ("select_filtered", {"thr": 0.0, "it": 9}, NO_ADAPTIVE),
        ("run", {"thr": 0.0, "rounds": 0}, NO_ADAPTIVE),
        ("run_filtered", {"thr": 0.0, "it": 9, "capacity": 0}, NO_ADAPTIVE),
        ("select", {"out": False}, INVALID),
        ("select_filtered", {"out": False}, INVALID),
        ("run", {"out": False}, NO_ADAPTIVE),
        ("run_filtered", {"out": False}, NO_ADAPTIVE),
        ("run", {"variant": 3}, INVALID),                      # (a render argument: before the mode)
    ])
    assert before["info"]["on"] is False and before["stats"]["on"] is True


def test_statistics_off_is_mode_off(mcpt_mod, ctx, calls):
    """Bad floats, rounds = 0 and the statistics off (the mode goes off with them): NO_ADAPTIVE."""
    begin(mcpt_mod, ctx, 2)
    ctx.stats_end()
    before = check_table(mcpt_mod, ctx, calls, [
        ("select", {"thr": NAN, "floor": 0.0}, NO_ADAPTIVE),
        ("select_filtered", {"cap": -1.0, "sp": INF}, NO_ADAPTIVE),
        ("run", {"floor": NAN}, NO_ADAPTIVE),
        ("run_filtered", {"k": 0.0}, NO_ADAPTIVE),
        ("run", {"rounds": 0}, NO_ADAPTIVE),
        ("run_filtered", {"rounds": 0}, NO_ADAPTIVE),
    ])
    assert before["info"]["on"] is False and before["stats"]["on"] is False


def test_bad_floats_come_before_the_batches_and_the_guides(mcpt_mod, ctx, calls):
    """The mode on, no batch, no passes, no guides: a bad float is INVALID everywhere; with good floats the
    single filtered select's pass count (INVALID) comes before the two-batch rule (NO_STATS), the raw select
    meets that rule, the filtered run the guides (it has no two-batch rule), the raw run its rounds."""
    begin(mcpt_mod, ctx, 0)
    check_table(mcpt_mod, ctx, calls, [
        ("select", {"floor": -1.0}, INVALID),
        ("select", {"thr": INF}, INVALID),
        ("select_filtered", {"sp": INF}, INVALID),
        ("select_filtered", {"cap": NAN}, INVALID),
        ("run", {"thr": NAN}, INVALID),
        ("run_filtered", {"cap": 0.0}, INVALID),
        ("run_filtered", {"k": -2.0}, INVALID),
        ("select", {}, NO_STATS),
        ("select_filtered", {}, INVALID),
        ("run", {"rounds": 0}, INVALID),
        ("run_filtered", {"rounds": 0}, NO_GUIDES),
    ])


def test_row_shard_comes_before_the_guides(mcpt_mod, ctx, calls):
    """A row-shard target with two batches and no guides: the filtered rule refuses the shard (INVALID),
    not the guides; the raw rule serves a shard, so only its own arguments refuse."""
    from mcpt.dist import local_rows
    rows = local_rows(H, 8, 3, 1, "balanced")
    assert 0 < len(rows) < H
    begin(mcpt_mod, ctx, 2, rows=rows)
    before = check_table(mcpt_mod, ctx, calls, [
        ("select_filtered", {}, INVALID),
        ("run_filtered", {}, INVALID),
        ("run_filtered", {"rounds": 0}, INVALID),
        ("run", {"capacity": 3}, INVALID),
    ])
    assert before["stats"]["batches"] == 2
    ctx.set_target(W, H)


def test_gathered_counts_come_before_the_batches(mcpt_mod, ctx, calls):
    """Gathered counts, one batch, current guides: the filtered rule refuses the count plane (INVALID)
    before the single call's two-batch rule (NO_STATS), which the raw select meets; the runs have no such
    rule, so rounds = 0 is their INVALID."""
    begin(mcpt_mod, ctx, 1, guides=True)
    buf = load_own_counts(ctx)
    assert (ctx.read_sample_counts() == N).all()               # the plane is valid
    check_table(mcpt_mod, ctx, calls, [
        ("select_filtered", {}, INVALID),
        ("run_filtered", {}, INVALID),
        ("select", {}, NO_STATS),
        ("run", {"rounds": 0}, INVALID),
        ("run", {"rounds": 257}, INVALID),
    ])
    del buf


def test_one_batch_comes_before_the_guides(mcpt_mod, ctx, calls):
    """One batch and no guides: the single filtered select's two-batch rule (NO_STATS) comes before its
    guides; the filtered run has no such rule and refuses the guides, before its rounds; the raw run
    refuses its rounds."""
    begin(mcpt_mod, ctx, 1)
    check_table(mcpt_mod, ctx, calls, [
        ("select", {}, NO_STATS),
        ("select_filtered", {}, NO_STATS),
        ("run_filtered", {}, NO_GUIDES),
        ("run_filtered", {"rounds": 0}, NO_GUIDES),
        ("run_filtered", {"n": 0}, NO_GUIDES),
        ("run", {"rounds": 0}, INVALID),
        ("run", {"ce": 0}, INVALID),
    ])


def test_iterations_come_before_the_guides(mcpt_mod, ctx, calls):
    """iterations = 9 with two batches and no guides: INVALID; iterations in range: NO_GUIDES."""
    begin(mcpt_mod, ctx, 2)
    check_table(mcpt_mod, ctx, calls, [
        ("select_filtered", {"it": 9}, INVALID),
        ("select_filtered", {"it": -1}, INVALID),
        ("run_filtered", {"it": 9}, INVALID),
        ("select_filtered", {}, NO_GUIDES),
        ("run_filtered", {}, NO_GUIDES),
        ("run_filtered", {"capacity": 3}, NO_GUIDES),
    ])


def test_short_records_are_refused(mcpt_mod, ctx, calls):
    """Everything valid (two batches, guides: four rounds hold four selects) but records for three, or
    none to write to: INVALID; and then the calls run."""
    begin(mcpt_mod, ctx, 2, guides=True)
    check_table(mcpt_mod, ctx, calls, [
        ("run", {"capacity": 3}, INVALID),
        ("run_filtered", {"capacity": 3}, INVALID),
        ("run", {"records": False}, INVALID),
        ("run_filtered", {"records": False}, INVALID),
        ("run", {"out": False}, INVALID),
        ("run_filtered", {"out": False}, INVALID),
        ("run", {"first": 0x7fffffff - 8}, INVALID),           # (the passes do not fit the counters)
    ])
    assert calls.run_filtered(rounds=1, capacity=1) == OK and calls.out.rounds_run == 1 and calls.out.selects_run == 1
    assert calls.run(first=25, rounds=1, capacity=1) == OK and calls.out.rounds_queued == 1
    assert calls.select() == OK and calls.select_filtered() == OK
