"""The stream contract of every entry point, made visible with stalled streams: gmg_debug_stall holds a stream back
for a bounded time, so a call that the library mis-orders -- work on stream 0 instead of the caller's stream, a side stream that is
not joined, a constructor that returns with null-stream work still queued -- demonstrably runs on the wrong side of what it depends
on and reads the OTHER job's values, which every output buffer holds beforehand (tests/stream_cases.py).  Nothing is repeated and no
host thread is started: every case is deterministic by construction.

The expected value of a case is the same call on the idle null stream (the other GPU tests pin that to the oracle); all comparisons
are bit for bit.
  B  the caller's stream S is stalled, then the call and its read-back on S: whatever the call put elsewhere runs ahead of its inputs
  C  the null stream is stalled, then the call and its read-back on S, then the wait for the null stream: whatever the call put on the
     null stream runs late.  Conclusive only when call and read-back return before the stall ends: asserted for every row but the
     three that create side streams, whose mg_one_stream twins must be conclusive
  A  the null stream is stalled, a constructor runs, its handle is used at once on S
  D  scratch that goes back to the block cache "after the stream" while a second stream asks for the same sizes"""
import contextlib
import ctypes as C
import time

import numpy as np
import pytest

import stream_cases as sc

pytestmark = pytest.mark.gpu

STALL_US = 50_000            # DESIGN.md 2.3 records the longest call + read-back measured against it
PROBE_US = 5_000


@pytest.fixture(scope="module")
def ctx(gpu):
    c = sc.Context(gpu)
    jobs = [sc.Job(c, 1), sc.Job(c, 2)]
    jobs[0].other, jobs[1].other = jobs[1], jobs[0]
    yield c, jobs
    gpu.capi.lib().gmg_synchronize(None)
    for j in jobs:
        j.close(c)


def _returns_during_stall(c, held, probe, word):
    """does a 4-byte copy on `probe` come back while `held` is stalled?  (two streams may share a hardware queue)"""
    host = np.zeros(1, np.uint32)
    t0 = time.monotonic()
    c.ck(c.lib.gmg_debug_stall(held, PROBE_US))
    c.ck(c.lib.gmg_memcpy_d2h(sc._ptr(host), word, 4, probe))
    dt = time.monotonic() - t0
    c.ck(c.lib.gmg_synchronize(held))
    return dt < PROBE_US * 1e-6


@pytest.fixture(scope="module")
def streams(ctx):
    """S: the first of up to four library streams that the stalled null stream does not hold back; S2: another one that neither the
    null stream nor S holds back (mode D), or None"""
    c, _ = ctx
    keep = sc.Keep(c)
    word = keep.dev(np.array([7], np.uint32))
    made = []
    for _ in range(4):
        s = C.c_void_p()
        c.ck(c.lib.gmg_stream_create(C.byref(s)))
        c.ck(c.lib.gmg_memcpy_d2h(sc._ptr(np.zeros(1, np.uint32)), word, 4, s))       # (the first copy on a stream sets it up)
        made.append(s)
    c.ck(c.lib.gmg_debug_stall(None, 100))                            # (loads the kernel)
    c.ck(c.lib.gmg_synchronize(None))
    free = [s for s in made if _returns_during_stall(c, None, s, word)]
    assert free, "none of four streams runs while the null stream is stalled"
    S = free[0]
    S2 = next((s for s in free[1:] if _returns_during_stall(c, S, s, word) and _returns_during_stall(c, s, S, word)), None)
    yield S, S2
    for s in made:
        c.lib.gmg_synchronize(s)
        c.lib.gmg_stream_destroy(s)
    keep.free()


@contextlib.contextmanager
def options(gpu, opts):
    with contextlib.ExitStack() as stack:
        for k, v in opts.items():
            stack.enter_context(gpu.option(k, v))
        yield


def same(a, b):
    return len(a) == len(b) and all(x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes() for x, y in zip(a, b))


def drained(c, keep, *streams):
    """every stream idle before a buffer or handle of the case is freed"""
    for s in streams:
        c.lib.gmg_synchronize(s)
    c.lib.gmg_synchronize(None)
    keep.free()


_reference = {}


def reference(ctx, row, S):
    """(result of job 0, result of job 1) on the idle null stream, once per row; the first call of the row on S, unstalled, is made
    here too (it creates the side streams and loads the code) and must already agree"""
    c, jobs = ctx
    if row.name not in _reference:
        out = []
        for j in jobs:
            keep = sc.Keep(c)
            try:
                out.append(row.run(c, j, None, None, keep, lambda: None))
            finally:
                drained(c, keep)
        assert not same(out[0], out[1]), "the two jobs give the same result: a stale read could hide"
        keep = sc.Keep(c)
        try:
            warm = row.run(c, jobs[0], S, out[1], keep, lambda: None)
        finally:
            drained(c, keep, S)
        assert same(warm, out[0]), "%s on an idle caller's stream differs from the null stream" % row.name
        _reference[row.name] = out
    return _reference[row.name]


def stalled_run(ctx, row, S, held):
    """the row on S for job 0 with stream `held` stalled in front of it -> (result, seconds from the stall's launch to the return of
    the read-back)"""
    c, jobs = ctx
    want, other = reference(ctx, row, S)
    keep, t = sc.Keep(c), {}

    def stall():
        t["t0"] = time.monotonic()
        c.ck(c.lib.gmg_debug_stall(held, STALL_US))

    try:
        got = row.run(c, jobs[0], S, other, keep, stall)
        dt = time.monotonic() - t["t0"]
    finally:
        drained(c, keep, S)
    return got, want, dt


def test_the_stall_holds_its_stream_and_nothing_else(ctx, streams):
    """gmg_debug_stall lasts at least as long as asked (the cases' clocks rely on it) and not much longer"""
    c, _ = ctx
    S, _ = streams
    for held in (None, S):
        t0 = time.monotonic()
        c.ck(c.lib.gmg_debug_stall(held, 20_000))
        launched = time.monotonic() - t0
        c.ck(c.lib.gmg_synchronize(held))
        dt = time.monotonic() - t0
        print("STREAMS stall 20 ms on %s: launch returned after %.2f ms, stream idle after %.2f ms" % ("S" if held else "null", launched * 1e3, dt * 1e3))
        assert launched < 0.020 and 0.020 <= dt < 0.100
    with pytest.raises(c.gpu.GmgError):
        c.ck(c.lib.gmg_debug_stall(S, 250_001))
    c.ck(c.lib.gmg_debug_stall(S, 0))
    c.ck(c.lib.gmg_synchronize(S))


@pytest.mark.parametrize("row", sc.ROWS, ids=repr)
def test_b_producers_stalled(ctx, streams, row):
    c, _ = ctx
    with options(c.gpu, row.options):
        got, want, dt = stalled_run(ctx, row, streams[0], streams[0])
    print("STREAMS B %s: %.1f ms" % (row.name, dt * 1e3))
    assert same(got, want), "%s behind a stalled caller's stream differs from the null-stream result" % row.name
    assert dt >= STALL_US * 1e-6, "the read-back on S came back before the stall in front of it ended"


@pytest.mark.parametrize("row", sc.ROWS, ids=repr)
def test_c_null_stream_stalled(ctx, streams, row):
    c, _ = ctx
    with options(c.gpu, row.options):
        got, want, dt = stalled_run(ctx, row, streams[0], None)
    conclusive = dt < STALL_US * 1e-6
    print("STREAMS C %s: %.1f ms%s" % (row.name, dt * 1e3, "" if conclusive else "  INCONCLUSIVE"))
    assert same(got, want), "%s with the null stream stalled differs from the null-stream result" % row.name
    if row.entry in sc.SIDE_STREAM_ENTRIES and not row.options.get("mg_one_stream"):
        return                                                        # a side stream may share the null stream's queue: its twin decides
    assert conclusive, "%s: call and read-back took %.1f ms, the stall %d ms: something waited for the null stream" % (row.name, dt * 1e3, STALL_US // 1000)


@pytest.mark.parametrize("ctor", sc.CTORS, ids=repr)
def test_a_constructor_hands_back_a_ready_handle(ctx, streams, ctor):
    """the null stream is stalled, the constructor runs, and its handle is used at once on S: the constructor has waited for whatever
    it put on the null stream"""
    c, jobs = ctx
    S, j = streams[0], jobs[0]
    results = []
    for held in (False, True):
        keep = sc.Keep(c)
        h = None
        try:
            if held:
                c.ck(c.lib.gmg_debug_stall(None, STALL_US))
            h = ctor.make(c, j, keep)
            results.append(ctor.use(c, j, h, S if held else None, keep))
        finally:
            drained(c, keep, S)
            if h is not None:
                ctor.free(c, h)
    assert sum(a.nbytes for a in results[0]) > 0
    assert same(results[1], results[0]), "%s: the handle was not ready when the constructor returned" % ctor.name


def _busy(c):
    st = (C.c_uint64 * 4)()
    c.ck(c.lib.gmg_debug_cache_stats(st))
    return st[0]


def test_d_scratch_released_after_one_stream_while_another_asks(ctx, streams):
    """gmg_entropy_regions hands its scratch back "once the stream reaches here".  Stalled S1 holds the call back (its read offsets
    come back over S1); the moment it returns, its kernel and the release behind it just queued, the same call for the other job asks
    for the same size on S2.  Whichever block S2 gets, both results are right, and the cache's busy count returns to where it started"""
    c, jobs = ctx
    S1, S2 = streams
    assert S2 is not None, "no second stream that runs while the first is stalled"
    row = next(r for r in sc.ROWS if r.name == "entropy_regions")
    want = reference(ctx, row, S1)
    c.ck(c.lib.gmg_synchronize(None))
    busy0 = _busy(c)
    n = len(jobs[0].regions)
    keep = sc.Keep(c)
    try:
        bufs = [(keep.dev(sc.like(want[1 - k], 0, np.int32, 20 * n)), keep.dev(sc.like(want[1 - k], 1, np.float64, 3 * n))) for k in (0, 1)]
        c.ck(c.lib.gmg_debug_stall(S1, STALL_US))
        for k, s in ((0, S1), (1, S2)):
            j = jobs[k]
            c.ck(c.lib.gmg_entropy_regions(j.reads.h, sc._ptr(j.regions), n, c.aa, sc._ptr(c.pos), sc._ptr(c.neg), bufs[k][0], bufs[k][1], s))
        got1 = [sc.d2h(c, bufs[1][0], np.int32, 20 * n, S2), sc.d2h(c, bufs[1][1], np.float64, 3 * n, S2)]
        got0 = [sc.d2h(c, bufs[0][0], np.int32, 20 * n, S1), sc.d2h(c, bufs[0][1], np.float64, 3 * n, S1)]
    finally:
        drained(c, keep, S1, S2)
    assert same(got0, want[0]) and same(got1, want[1])
    assert _busy(c) == busy0
