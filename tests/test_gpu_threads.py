"""The host-thread contract of every entry point: any number of host threads may call any entry point at the same
time, provided no two calls share a stream or a mutable handle.  The rows are those of tests/stream_cases.py (one self-contained
call plus its read-back on one stream); tests/thread_cases.py says which may share a job and which may overlap at all.

Four threads (the machines' four hardware queues: the streams share them), each with a gmg_stream_create stream of its own.  The
expected value of a row is the same call alone on the idle null stream, made before any thread starts (the other GPU tests pin that
to the oracle); all comparisons are bit for bit.
  A  every row, a job of its own per thread, all rows of an option group three times round, every thread from another row on
  B  the rows that read const handles only, four threads on ONE job
  C  the same entry point from four threads at once, ten rounds behind a barrier each: the calls with thread-local or cached state
  D  four trainings at once
  E  scratch handed back "after the stream" by one thread while another asks for the same sizes (mode D of 2.3 across threads)
  F  the first use of a shared host model's device mirror from four threads at once
  G  threads that end give back their side streams, events and staging
  H  after every case, its handles freed: no busy block in the cache, gmg_debug_owned_blocks where it was
A barrier or a join that does not come back within 60 s fails the test (thread_cases.run_threads): a deadlock is a failure, not a
hang.  From then on the module starts nothing on the device, waits for no stream and frees nothing there (STUCK): the cases after it
fail at once, and the fixtures' teardown leaves streams, buffers and jobs alone.  No stream is stalled for longer than the 50 ms of 2.3, and raw device inputs always hold valid data."""
import contextlib
import ctypes as C
import gc
import os
import time

import numpy as np
import pytest

import stream_cases as sc
import thread_cases as tc

pytestmark = pytest.mark.gpu

N = tc.N_THREADS
STALL_US = 50_000            # the stall of DESIGN.md 2.3; no case holds a stream back for longer
STUCK = []                   # the case whose threads did not come back: from then on nothing is started, waited for or freed on the device


def run_threads(n, body):
    try:
        tc.run_threads(n, body)
    except tc.Stuck as e:
        STUCK.append(str(e))
        raise


@pytest.fixture(autouse=True)
def nothing_after_a_stuck_case():
    if STUCK:
        pytest.fail("an earlier case of this module is stuck (%s): nothing further is started on the device" % STUCK[0])


@pytest.fixture(scope="module")
def ctx(gpu):
    c = sc.Context(gpu)
    jobs = [sc.Job(c, 1 + i) for i in range(N)]
    for i, j in enumerate(jobs):
        j.other = jobs[(i + 1) % N]
    yield c, jobs
    if STUCK:                                                         # (a wait for the device might never come back, and threads may still use the jobs)
        return
    gpu.capi.lib().gmg_synchronize(None)
    for j in jobs:
        j.close(c)


@pytest.fixture(scope="module")
def streams(ctx):
    """a stream per thread; the first copy on a stream sets it up"""
    c, _ = ctx
    keep = sc.Keep(c)
    word = keep.dev(np.array([7], np.uint32))
    made = []
    for _ in range(N):
        s = C.c_void_p()
        c.ck(c.lib.gmg_stream_create(C.byref(s)))
        c.ck(c.lib.gmg_memcpy_d2h(sc._ptr(np.zeros(1, np.uint32)), word, 4, s))
        made.append(s)
    yield made
    if STUCK:
        return
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


def counters(c):
    """(busy blocks of the cache, blocks the handles own, streams + events made for threads)"""
    st, owned, ts = (C.c_uint64 * 4)(), C.c_uint64(), C.c_uint64()
    c.ck(c.lib.gmg_debug_cache_stats(st))
    c.ck(c.lib.gmg_debug_owned_blocks(C.byref(owned)))
    c.ck(c.lib.gmg_debug_thread_streams(C.byref(ts)))
    return int(st[0]), int(owned.value), int(ts.value)


@contextlib.contextmanager
def accounted(c, streams=()):
    """H: the case's handles freed and its streams idle, the cache holds as many busy blocks as before and the handles own as many"""
    gc.collect()
    c.ck(c.lib.gmg_synchronize(None))
    busy, owned, _ = counters(c)
    yield
    gc.collect()
    for s in list(streams) + [None]:
        c.ck(c.lib.gmg_synchronize(s))
    assert counters(c)[:2] == (busy, owned), "busy cache blocks / owned blocks were %r before the case" % ((busy, owned),)


def run_row(c, row, j, S, pre):
    """the row for job j on stream S -> its result; the case's buffers go once S and the null stream (the preparations') are idle"""
    keep = sc.Keep(c)
    try:
        return row.run(c, j, S, pre, keep, lambda: None)
    finally:
        c.lib.gmg_synchronize(S)
        c.lib.gmg_synchronize(None)
        keep.free()


_expected = {}


def expected(ctx, row):
    """the row alone on the idle null stream, for every job, once (under the row's options, which the caller has set).  Each job then
    makes the call once more as the threads will make it, with the next job's result in every buffer: that must agree already, and
    the buffers the job's long-lived handles keep inside (the letters' text, the ORF batch's arrays) have their final size before a
    case counts blocks"""
    c, jobs = ctx
    if row.name not in _expected:
        out = [run_row(c, row, j, None, None) for j in jobs]
        for i in range(N):
            assert not same(out[i], out[(i + 1) % N]), "two jobs give the same result: a foreign read could hide"
        for i, j in enumerate(jobs):
            assert same(run_row(c, row, j, None, out[(i + 1) % N]), out[i]), "%s: differs over buffers that hold another job's result" % row.name
        _expected[row.name] = out
    return _expected[row.name]


def threaded(ctx, streams, plan):
    """plan(t) -> [(row, job index)] for thread t, run in that order on the thread's own stream behind one barrier; `pre` is the row's
    result for the next job.  -> the list of (thread, position, row name) whose result is not the expected one"""
    c, jobs = ctx
    want = {r.name: expected(ctx, r) for t in range(N) for r, _ in plan(t)}
    bad = []

    def body(t, barrier):
        todo = plan(t)
        barrier.wait()
        for k, (r, ji) in enumerate(todo):
            got = run_row(c, r, jobs[ji], streams[t], want[r.name][(ji + 1) % N])
            if not same(got, want[r.name][ji]):
                bad.append((t, k, r.name))

    with accounted(c, streams):
        run_threads(N, body)
    return bad


GROUPS = tc.option_groups()


def group_id(g):
    return ",".join("%s=%d" % kv for kv in sorted(g[0].items())) or "defaults"


@pytest.mark.parametrize("group", GROUPS, ids=group_id)
def test_a_every_row_own_job_per_thread(ctx, streams, group):
    c, _ = ctx
    opts, rows = group
    with options(c.gpu, opts):
        def plan(t):
            first = t * len(rows) // N                                # every thread from another row on: different kernels overlap
            return [(rows[(first + k) % len(rows)], t) for k in range(3 * len(rows))]
        bad = threaded(ctx, streams, plan)
    assert not bad, "differs from the call alone on the null stream: %s" % ", ".join("%s (thread %d, call %d)" % (n, t, k) for t, k, n in bad[:8])


SHARED_GROUPS = tc.option_groups([r for r in sc.ROWS if r.name in tc.SHARED_OK])


@pytest.mark.parametrize("group", SHARED_GROUPS, ids=group_id)
def test_b_shared_const_handles(ctx, streams, group):
    """ONE job and one context for all four threads: shared reads, segments, models, null set, scored result, ORF result"""
    c, _ = ctx
    opts, rows = group
    with options(c.gpu, opts):
        def plan(t):
            first = t * len(rows) // N
            return [(rows[(first + k) % len(rows)], 0) for k in range(len(rows))]
        bad = threaded(ctx, streams, plan)
    assert not bad, "on a shared job, differs from the call alone: %s" % ", ".join("%s (thread %d, call %d)" % (n, t, k) for t, k, n in bad[:8])


@pytest.mark.parametrize("name", tc.SAME_ENTRY)
def test_c_same_entry_point_four_threads_at_once(ctx, streams, name):
    c, jobs = ctx
    row = tc.row(name)
    with options(c.gpu, row.options):
        want = expected(ctx, row)
        bad = []

        def body(t, barrier):
            for k in range(10):
                barrier.wait()
                got = run_row(c, row, jobs[t], streams[t], want[(t + 1) % N])
                if not same(got, want[t]):
                    bad.append((t, k))

        with accounted(c, streams):
            run_threads(N, body)
    assert not bad, "%s: (thread, round) %r differ from the call alone" % (name, bad[:8])


def training_strings(seed):
    rng = np.random.default_rng(seed)
    return [bytes(rng.choice(np.frombuffer(b"acgt", np.uint8), size=int(n))) for n in rng.integers(1, 1501, size=300)]


@pytest.mark.parametrize("sort_min", [0, 2**40])
def test_d_training_in_parallel(ctx, sort_min):
    """gmg_icm_train (12 / 7 / 3) of four threads' own strings: the tables are those of the serial trainings (the cached page-locked
    buffer of the training strings, the trainer's sort scratch)"""
    c, _ = ctx
    gpu = c.gpu
    sets = [training_strings(40 + t) for t in range(N)]

    def train(t):
        m = gpu.Icm.train(sets[t], 12, 7, 3)
        try:
            return list(m.tables())
        finally:
            m.close()

    with options(gpu, {"train_sort_min": sort_min}):
        want = [train(t) for t in range(N)]
        assert not same(want[0], want[1])
        got = [None] * N

        def body(t, barrier):
            barrier.wait()
            got[t] = train(t)

        with accounted(c):
            run_threads(N, body)
    for t in range(N):
        assert same(got[t], want[t]), "thread %d's model differs from its serial training" % t


def test_e_scratch_handed_back_across_threads(ctx, streams):
    """gmg_entropy_regions hands its scratch back "after the stream".  Thread 0 stalls its stream and makes the call; thread 1 runs the
    same-sized call for another job to completion, twenty times.  What this can and cannot show: the call first waits for its stream
    (the read offsets come back over it, behind the stall) and takes its scratch only then, so during the stall thread 0 holds no
    block -- thread 1's first ten calls pin only that a call held back on one stream does not disturb the cache for another.  The
    moment thread 0's call returns, its kernel and the release behind it are just queued: thread 1's other ten calls, and ten more
    calls of thread 0, ask for the same sizes across those moments, one short kernel long each -- mode D of 2.3, from two threads,
    about thirty times.  No entry point queues a release behind a stall: each that releases "after the stream" waits for that stream
    first, inside the call"""
    c, jobs = ctx
    row = tc.row("entropy_regions")
    n = len(jobs[0].regions)
    want = expected(ctx, row)
    with accounted(c, streams):
        keep = sc.Keep(c)
        got0, got1 = [], []
        try:
            bufs = [(keep.dev(sc.like(want[1 - k], 0, np.int32, 20 * n)), keep.dev(sc.like(want[1 - k], 1, np.float64, 3 * n))) for k in (0, 1)]

            def call(k, s):
                j = jobs[k]
                c.ck(c.lib.gmg_entropy_regions(j.reads.h, sc._ptr(j.regions), n, c.aa, sc._ptr(c.pos), sc._ptr(c.neg), bufs[k][0], bufs[k][1], s))

            def fetch(k, s):
                return [sc.d2h(c, bufs[k][0], np.int32, 20 * n, s), sc.d2h(c, bufs[k][1], np.float64, 3 * n, s)]

            def body(t, barrier):
                barrier.wait()
                if t == 0:
                    c.ck(c.lib.gmg_debug_stall(streams[0], STALL_US))
                    call(0, streams[0])                               # (waits behind the stall for the read offsets, then takes its scratch)
                    barrier.wait()                                    # the kernel is queued, the release behind it
                    got0.append(fetch(0, streams[0]))
                    for _ in range(10):                               # ... and ten more such moments, beside thread 1's
                        call(0, streams[0])
                        got0.append(fetch(0, streams[0]))
                else:
                    for k in range(20):
                        if k == 10:
                            barrier.wait()                            # ten calls while thread 0's call is held back, ten from the moment it returns
                        call(1, streams[1])
                        got1.append(fetch(1, streams[1]))

            run_threads(2, body)
        finally:
            if not STUCK:
                for s in streams[:2] + [None]:
                    c.lib.gmg_synchronize(s)
                keep.free()
        assert len(got0) == 11 and all(same(g, want[0]) for g in got0), "the stalled thread's result is not its own"
        assert len(got1) == 20 and all(same(g, want[1]) for g in got1)


def fixed_training_strings(seed):
    rng = np.random.default_rng(seed)
    return [bytes(rng.choice(np.frombuffer(b"acgt", np.uint8), size=12)) for _ in range(120)]


def test_f_first_use_of_a_shared_host_model(ctx):
    """the device mirror of a host model is made at its first use by a const method: four threads make that first use at once, on a
    freshly opened gmg_icm and a freshly trained fixed-length model, eight times.  One upload each: all threads get the same pointer,
    and the handles own what ONE upload takes (measured on models mirrored serially)"""
    c, _ = ctx
    gpu = c.gpu
    path = os.path.join(sc.DATA, "NC_000915.icm")

    def fresh(k):
        return gpu.Icm.open(path), gpu.FixedIcm.train(fixed_training_strings(k), 2)

    with accounted(c):
        start = counters(c)[1]
        icm, fixed = fresh(0)
        unmirrored = counters(c)[1]
        first = (icm.device().value, fixed.device().value)
        one_upload = counters(c)[1] - unmirrored
        assert one_upload >= 2 and (icm.device().value, fixed.device().value) == first and counters(c)[1] == unmirrored + one_upload
        icm.close()
        fixed.close()
        assert counters(c)[1] == start
        print("THREADS F one upload of both mirrors owns %d blocks" % one_upload)
        for k in range(1, 9):
            icm, fixed = fresh(k)
            assert counters(c)[1] == unmirrored
            seen = [None] * N

            def body(t, barrier):
                barrier.wait()
                seen[t] = (icm.device().value, fixed.device().value)

            try:
                run_threads(N, body)
                assert seen[0][0] and seen[0][1] and all(s == seen[0] for s in seen), "model %d: the threads got different mirrors: %r" % (k, seen)
                assert counters(c)[1] == unmirrored + one_upload, "model %d: %d blocks are owned, one upload takes %d" % (k, counters(c)[1] - unmirrored, one_upload)
            finally:
                if STUCK:                                             # (threads may still be inside these models: they are left alone, for good)
                    icm.h = fixed.h = C.c_void_p()
                else:
                    icm.close()
                    fixed.close()
            assert counters(c)[1] == start


def ended(c, before, limit=2.0):
    """the counters once the joined thread is gone: join returns when the thread's Python side has ended, the thread_local
    destructors run a moment later, as the OS thread itself ends -- looked at again until they have (a cap, not a measurement)"""
    t0 = time.monotonic()
    while True:
        now = counters(c)
        if now[1:] == before[1:] or time.monotonic() - t0 > limit:
            return now
        time.sleep(0.0005)


def test_g_threads_that_end_give_everything_back(ctx):
    """eight threads one after the other, each joined before the next starts: one gmg_mg_score_reads -i call on a stream of the
    thread's own (the path that makes all three stream sets: 6 streams, 8 events) and one string through the host class (which makes
    the thread's staging).  While the thread lives the counters show both; after the last join they are where they were"""
    c, jobs = ctx
    row = tc.row("mg_score_reads_indels")
    s = jobs[0].seqs[0].encode()
    want = expected(ctx, row)
    score = C.c_double()
    c.ck(c.lib.gmg_debug_icm_score_string(c.gene.h, s, len(s), 0, C.byref(score)))            # (the main thread's staging exists from here on)
    with accounted(c):
        before = counters(c)
        for k in range(tc.MAX_THREADS):
            seen = {}

            def body(t, barrier):
                S = C.c_void_p()
                c.ck(c.lib.gmg_stream_create(C.byref(S)))
                try:
                    seen["got"] = run_row(c, row, jobs[k % N], S, want[(k + 1) % N])
                finally:
                    c.lib.gmg_synchronize(S)
                    c.lib.gmg_stream_destroy(S)
                mine = C.c_double()
                c.ck(c.lib.gmg_debug_icm_score_string(c.gene.h, s, len(s), 0, C.byref(mine)))
                seen["score"] = mine.value
                seen["counters"] = counters(c)

            run_threads(1, body)
            assert same(seen["got"], want[k % N]) and seen["score"] == score.value
            assert seen["counters"][2] == before[2] + 14, "thread %d: %d streams + events live, %d before it" % (k, seen["counters"][2], before[2])
            assert seen["counters"][1] > before[1], "thread %d: no staging block is owned while it lives" % k
            after = ended(c, before)
            assert after[2] == before[2], "thread %d has ended: %d of its streams and events are left" % (k, after[2] - before[2])
            assert after[1] == before[1], "thread %d has ended: %d of its staging blocks are left" % (k, after[1] - before[1])
