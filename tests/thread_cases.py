"""What tests/test_gpu_threads.py needs beyond the rows of tests/stream_cases.py: which handle types several host
threads may share, which rows therefore may run from several threads on ONE job, and which rows may run at the same time at all
(options are process-wide: rows with different option sets never overlap).  The rows themselves are stream_cases.ROWS, unchanged:
a row's run(c, j, S, pre, keep, stall) is one self-contained call plus its read-back on one stream.
tests/test_thread_cases_host.py checks all of this against include/gmg.h without a device."""
import re
import threading
import time

import stream_cases as sc

N_THREADS = 4                 # the machines' hardware queues: four streams share them, so a missing order is not hidden by idle hardware
MAX_THREADS = 8               # no case starts more
TIMEOUT_S = 60.0              # barriers and joins: a cap far above the work (a case is well under a second of device time), no measurement

# Handle types of include/gmg.h (typedef struct gmg_x gmg_x).  A mutable handle belongs to ONE call at a time:
MUTABLE_HANDLES = [
    "gmg_letters",            # its device text is valid until the next text call
    "gmg_tophits",
    "gmg_trainer",
    "gmg_single",             # one per host thread
    "gmg_orf_batch",          # between _begin and _fetch
    "gmg_model_set",          # until _finish
]
# ... a const handle may be read by any number of calls at once:
CONST_HANDLES = [
    "gmg_model", "gmg_null_set", "gmg_fixed_model", "gmg_reads", "gmg_segments", "gmg_mg_result", "gmg_fasta", "gmg_audit",
    "gmg_windows", "gmg_gaps", "gmg_features", "gmg_classes",
]

# Rows that use a mutable handle OF THEIR JOB, by the handle: two threads never run them on one job
OWN_JOB_ONLY = {
    "regions_text": "gmg_letters", "regions_text_device": "gmg_letters", "runs_text": "gmg_letters", "runs_text_device": "gmg_letters",
    "score_orfs_path0": "gmg_orf_batch", "score_orfs_path1": "gmg_orf_batch", "score_orfs_path2": "gmg_orf_batch",
    "score_orfs_begin": "gmg_orf_batch", "score_orfs_fetch": "gmg_orf_batch",
}
# ... every other row reads const handles of its job only (reads, segments, the scored result, the ORF result; the top-hits rows make
# a gmg_tophits of their own per call): these may run from several threads on ONE job
SHARED_OK = [r.name for r in sc.ROWS if r.name not in OWN_JOB_ONLY]

# Case C: the entry points that keep thread-local or cached state (side streams, the calls-per-base hint, the retry flag, page-locked
# buffers), each from four threads at once
SAME_ENTRY = [
    "mg_score_reads", "mg_score_reads_indels", "mg_score_reads_subs", "mg_score_reads_nulls", "mg_score_groups", "find_orfs",
    "fasta_ingest_on", "fasta_ingest_on_pieces", "score_orfs_path0", "score_orfs_path1", "score_orfs_path2", "features_count",
    "tophits_scores",
]


def handle_types(header_text):
    """the opaque handle types of a header: typedef struct gmg_x gmg_x;"""
    text = re.sub(r"/\*.*?\*/", "", header_text, flags=re.S)
    return sorted(set(m.group(1) for m in re.finditer(r"\btypedef\s+struct\s+(gmg_[a-z0-9_]+)\s+(gmg_[a-z0-9_]+)\s*;", text) if m.group(1) == m.group(2)))


def option_groups(rows=None):
    """[(options, rows)]: the rows grouped by their option dict, in table order; a group's rows may overlap, two groups never do"""
    groups = []
    for r in (sc.ROWS if rows is None else rows):
        for opts, members in groups:
            if opts == r.options:
                members.append(r)
                break
        else:
            groups.append((dict(r.options), [r]))
    return groups


def row(name):
    return next(r for r in sc.ROWS if r.name == name)


class Stuck(AssertionError):
    """a barrier or a join ran into TIMEOUT_S: the caller starts nothing further on the device"""


def run_threads(n, body, timeout=TIMEOUT_S):
    """body(t, barrier) on n daemon threads, t = 0 .. n - 1; barrier.wait() releases them together, as often as the body asks (a
    round each).  An exception in one thread breaks the barrier, so that the others do not wait for it, and is raised here once all
    have ended; a thread that has not ended after `timeout` seconds raises Stuck instead (a deadlock becomes a failure, not a hang)."""
    assert 1 <= n <= MAX_THREADS
    barrier = threading.Barrier(n, timeout=timeout)
    errors = []

    def main(t):
        try:
            body(t, barrier)
        except threading.BrokenBarrierError as e:                     # (another thread's failure, or a timeout: told below)
            errors.append((t, e))
        except BaseException as e:                                    # noqa: B036 -- carried over to the caller's thread
            errors.append((t, e))
            barrier.abort()

    threads = [threading.Thread(target=main, args=(t,), daemon=True, name="gmg-test-%d" % t) for t in range(n)]
    for th in threads:
        th.start()
    deadline = time.monotonic() + timeout
    for th in threads:
        th.join(max(deadline - time.monotonic(), 0.0))
    alive = [th.name for th in threads if th.is_alive()]
    if alive:
        barrier.abort()
        raise Stuck("still running after %.0f s: %s" % (timeout, ", ".join(alive)))
    real = [(t, e) for t, e in errors if not isinstance(e, threading.BrokenBarrierError)]
    if real:
        raise real[0][1]
    if errors:
        raise Stuck("a barrier was not reached by all %d threads within %.0f s" % (n, timeout))
