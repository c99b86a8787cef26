"""The case table of tests/test_gpu_streams.py: one row per entry point of include/gmg.h that takes a `void *stream`,
each with how to call it on a small fixed job and how to read its result back on the same stream; and the constructors, which have
no stream parameter but must hand back a handle that any stream may use at once.

A row's run(c, j, S, pre, keep, stall) makes the call for job j on stream S and returns its result as a list of numpy arrays:
  pre    None, or the result of the same row on the OTHER job (same shapes, other bases): what every buffer the library only writes
         holds before the call -- the caller's device outputs, the host result arrays, and (through a call with other arguments on
         the null stream) the buffers a handle keeps inside.  A stale read then gives a wrong answer, never the right one by luck.
  keep   device buffers and handles of the case: freed by the test after both streams are drained (hipFree waits for the device)
  stall  called once, after every preparation and directly in front of the call under test: the test starts its clock and its stall

Raw device INPUTS a caller supplies are never garbage: they hold valid data before anything is stalled.
tests/test_stream_cases_host.py checks the table against the header without a device."""
import ctypes as C
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DATA = os.path.join(ROOT, "tests", "golden", "data")

# entry points with a `void *stream` that get no row, and why
EXCLUDED = {
    "gmg_synchronize": "the wait itself: every case ends with it",
    "gmg_memcpy_h2d": "the copies the cases are read back with",
    "gmg_memcpy_d2h": "the copies the cases are read back with",
    "gmg_stream_destroy": "takes the stream to end it, queues nothing",
    "gmg_model_set_load": "tests/test_gpu_model_set.py loads on a second stream",
}
# rows whose call forks into side streams the library creates: a side stream may share the null stream's hardware queue, so mode C
# (null stream stalled) need not be conclusive for them -- it must be for the same row under mg_one_stream = 1
SIDE_STREAM_ENTRIES = ("gmg_mg_score_reads", "gmg_mg_score_groups", "gmg_find_orfs")


def stream_prototypes(header_text):
    """names of the functions of include/gmg.h with a `void *stream` parameter"""
    text = re.sub(r"/\*.*?\*/", "", header_text, flags=re.S)
    return sorted(set(m.group(1) for m in re.finditer(r"\b(gmg_[a-z0-9_]+)\s*\(([^;{}]*?)\)\s*;", text) if re.search(r"\bvoid\s*\*\s*stream\b", m.group(2))))


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def like(pre, i, dtype, count):
    """a host array of `count` items that holds the other job's result i, repeated or cut to fit (zeros without one)"""
    a = np.zeros(int(count), dtype)
    if pre is not None and a.nbytes and pre[i].nbytes:
        a.view(np.uint8)[:] = np.resize(np.frombuffer(pre[i].tobytes(), np.uint8), a.nbytes)
    return a


class Keep:
    """what a case holds on the device until its streams are drained"""

    def __init__(self, c):
        self.c, self.ptrs, self.later = c, [], []

    def dev(self, host):
        """a device buffer that holds `host` (copied on the null stream, waited for)"""
        host = np.ascontiguousarray(host)
        p = C.c_void_p()
        self.c.ck(self.c.lib.gmg_device_malloc(C.byref(p), max(host.nbytes, 1)))
        self.ptrs.append(p)
        if host.nbytes:
            self.c.ck(self.c.lib.gmg_memcpy_h2d(p, _ptr(host), host.nbytes, None))
        return p

    def defer(self, fn, *args):
        self.later.append((fn, args))

    def free(self):
        for fn, args in reversed(self.later):
            fn(*args)
        for p in self.ptrs:
            self.c.lib.gmg_device_free(p)
        self.ptrs, self.later = [], []


def d2h(c, ptr, dtype, count, S):
    out = np.zeros(int(count), dtype)
    if out.nbytes:
        c.ck(c.lib.gmg_memcpy_d2h(_ptr(out), ptr, out.nbytes, S))
    return out


# ------------------------------------------------------------------------------------------------------------------------------
# the job
# ------------------------------------------------------------------------------------------------------------------------------
N_READS, N_SEGS, N_REGIONS = 200, 64, 300
STOPS = ("taa", "tag", "tga")


def lengths():
    """about 200 ragged reads of 0 .. 700 bases, one empty, one of 961 bases (beyond the 960 bases the error branch's wave kernel takes:
    the batch falls back); the same for both jobs"""
    rng = np.random.default_rng(2024)
    n = rng.integers(1, 701, size=N_READS)
    n[:64] = np.maximum(n[:64], 60)                                   # the segments' reads
    n[70], n[71] = 0, 961
    return n


class Context:
    """models and parameters both jobs share"""

    def __init__(self, gpu):
        self.gpu, self.api, self.lib = gpu, gpu.api, gpu.capi.lib()
        self.capi = gpu.capi
        self.gene = gpu.Icm.open(os.path.join(DATA, "NC_000915.icm"))            # 12 / 7 / 3
        self.gene2 = gpu.Icm.open(os.path.join(DATA, "seqs.cluster-4.run1.filt.gicm"))
        self.null = gpu.Icm.indep(0.5)                                            # (3, 2, 3)
        self.gcs = [0.35, 0.5, 0.61]
        self.nulls = gpu.NullSet.build(self.gcs)
        self.p1 = gpu.Icm.open(os.path.join(DATA, "cluster-1.icm"))               # periodicity 1: the strings' batched path
        self.string_models = [self.p1, self.gene]                                 # ... and the exact segment path
        genome = b"".join(line.strip() for line in open(os.path.join(DATA, "NC_000915.fna"), "rb") if not line.startswith(b">")).lower()
        rng = np.random.default_rng(5)
        self.fixed = gpu.FixedIcm.train([genome[s:s + 12] for s in rng.integers(0, len(genome) - 12, 300)], 3)
        self.aa = gpu.xlate_table(11)
        self.pos, self.neg = gpu.entropy_default_profiles()
        self.tparams = gpu.text_params(60)
        self.rparams = gpu.runs_text_params(gpu.api.RUNS_TEXT_DNA, 0, 60)
        self.audit = gpu.api.audit_params()
        self.fparams = gpu.capi.FeaturesParams(75, 50, 0, 0)

    def ck(self, rc):
        self.api._ck(rc)

    def mg_params(self, flags=0, nulls=None, read_null=None):
        p = self.capi.MgParams(75, 1, 2**31 - 1, 3, 3, flags, -6.0)
        for i, s in enumerate(("atg", "gtg", "ttg")):
            p.start_codon[i].value = s.encode()
        for i, s in enumerate(STOPS):
            p.stop_codon[i].value = s.encode()
        p.min_indel_orf_len, p.indel_quality_threshold, p.indel_max, p.indel_suffix_score_threshold = 15, 18, 2, -12.0
        if nulls is not None:
            p.nulls, p.read_null = nulls.h, read_null.ctypes.data
        return p

    def orf_params(self, alt=False):
        p = self.capi.OrfParams(75, 0, int(alt), 2**31 - 1, -6.0 if not alt else -2.0, 3)
        for i, s in enumerate(("atg", "gtg", "ttg")):
            p.start_codon[i].value = s.encode()
        return p


class Job:
    """one of the two jobs: the same read lengths, segments, regions, runs and intervals over other bases"""

    def __init__(self, c, seed):
        gpu = c.gpu
        rng = np.random.default_rng(seed)
        self.len = lengths()
        self.seqs = ["".join("acgt"[b] for b in rng.integers(0, 4, size=int(n))) for n in self.len]
        for r in range(0, N_READS, 3):                               # genes to find: an open frame between a start and a stop codon
            if self.len[r] >= 200:
                s = list(self.seqs[r])
                body = "".join(("gct", "gaa", "aaa", "ctg", "ggc")[b] for b in rng.integers(0, 5, size=40))
                s[30:30 + 126] = "atg" + body + "taa"
                self.seqs[r] = "".join(s)
        self.reads = gpu.Reads.from_strings(self.seqs)
        self.off = self.reads.offsets
        self.total = self.reads.total_bases
        r2 = np.random.default_rng(99)                               # the same coordinates for both jobs
        rows = []
        for i in range(N_SEGS):
            L = int(self.len[i])
            ln = int(r2.integers(40, L + 1))
            rows.append((i, int(r2.integers(0, L - ln + 1)), ln, i % 4))
        self.segs = gpu.Segments(self.reads, rows)
        self.prefix = np.maximum(np.array([r[2] for r in rows]) - np.arange(N_SEGS) % 5, 0).astype(np.uint32)
        self.frames = np.array([(1, 2, 3, -1, -2, -3)[i % 6] for i in range(N_SEGS)], np.int32)
        live = [r for r in range(N_READS) if self.len[r] > 0]
        regions, alt, runs, intervals = [], [], [], []
        for k in range(N_REGIONS):
            r = live[int(r2.integers(0, len(live)))]
            L = int(self.len[r])
            first, ln, strand = int(r2.integers(0, L)), int(r2.integers(0, L + 1)), 1 if k % 3 else -1
            regions.append((r, first, ln, strand))
            alt.append((r, (first + 1) % L, ln, -strand))
            a, b = sorted(int(x) for x in rng.integers(0, L + 1, size=2))       # (the job's own: the gaps depend on nothing else)
            intervals.append((r, a, b))
            up = k % 2 == 0
            n = int(r2.integers(0, L + 1))
            f = int(r2.integers(0, L - n + 1)) if up else int(r2.integers(max(n - 1, 0), L))
            runs.append((r, f, n, 0 if up else 1))
        self.regions, self.regions_alt = np.array(regions, np.int32), np.array(alt, np.int32)
        self.runs = np.array(runs, np.uint32)
        self.runs_alt = self.runs.copy()
        self.runs_alt[:, 3] += 2                                     # the substituting kinds: other bytes, the same lengths
        self.sro = np.arange(0, N_REGIONS + 1, 3, dtype=np.uint64)
        self.intervals = np.array(intervals, np.int64)
        self.heads = [b">r%d\n" % k for k in range(N_REGIONS)]
        self.run_heads = self.heads[:len(self.sro) - 1]
        letters = "".join(self.seqs).upper().encode()
        self.letters = gpu.Letters(letters, self.off)
        self.fasta = b"".join(b">read%d some text\n%s\n" % (r, s.encode()) for r, s in enumerate(self.seqs))
        self.read_null = (np.arange(N_READS) % 3).astype(np.uint32)
        # windows of the 12-base model and their sub-models
        self.windows = rng.integers(0, 4, size=(N_REGIONS, 12)).astype(np.uint8)
        self.wframes = (np.arange(N_REGIONS) % 3).astype(np.int32)
        # ORFs (gmg_find_orfs on the null stream): a list for gmg_score_orfs, the result itself for gmg_entropy_orfs
        self.orf_res = gpu.OrfResult(self.reads, min_gene_len=75)
        found, _ = self.orf_res.fetch()
        found = found[found["orf_len"] > 0]
        # linear ORFs that lie inside their read (gmg_orfs_upload refuses the rest)
        ok = []
        for o in found:
            L = int(self.len[o["read"]])
            lo = o["stop_position"] - 1 - o["orf_len"] if o["frame"] > 0 else o["stop_position"] + 2
            if lo >= 0 and lo + o["orf_len"] <= L:
                ok.append((int(o["read"]), int(o["frame"]), int(o["stop_position"]), int(o["orf_len"])))
        self.orfs = np.zeros(min(len(ok), N_REGIONS), gpu.api.ORF_DTYPE)
        for k in range(len(self.orfs)):
            self.orfs[k] = ok[k]
        self.batch, ms = C.c_void_p(), C.c_uint64()
        c.ck(c.lib.gmg_orfs_upload(self.reads.h, _ptr(self.orfs), len(self.orfs), C.byref(ms), C.byref(self.batch)))
        self.max_starts = int(ms.value)
        # a scored result for gmg_mg_result_fetch_on
        self.mg_res = C.c_void_p()
        prm = c.mg_params()
        c.ck(c.lib.gmg_mg_score_reads(c.gene.device(), c.null.device(), self.reads.h, C.byref(prm), None, C.byref(self.mg_res), None))
        # genes for gmg_features_count: the planted ones, as a predict file would list them
        self.genes = [(r, 1, 30, 156, 1) for r in range(0, N_READS, 3) if self.len[r] >= 200]
        self.sums = gpu.score_reads_strings(c.string_models, self.reads)          # [2, n_reads, 2]
        self.other = None

    def close(self, c):
        c.lib.gmg_mg_result_free(self.mg_res)
        c.lib.gmg_orf_batch_free(self.batch)
        self.orf_res.close()
        self.letters.close()
        self.segs.close()
        self.reads.close()


# ------------------------------------------------------------------------------------------------------------------------------
# the rows
# ------------------------------------------------------------------------------------------------------------------------------
class Row:
    def __init__(self, name, entry, run, options=None):
        self.name, self.entry, self.run, self.options = name, entry, run, dict(options or {})

    def __repr__(self):
        return self.name


def _frame6(which):
    def run(c, j, S, pre, keep, stall):
        stride = j.total + (3 if which != "plain" else 0)
        out = keep.dev(like(pre, 0, np.float64, 6 * stride))
        stall()
        if which == "plain":
            c.ck(c.lib.gmg_frame_score6(c.gene.device(), c.null.device(), j.reads.h, out, S))
        elif which == "strided":
            c.ck(c.lib.gmg_frame_score6_strided(c.gene.device(), c.null.device(), j.reads.h, out, stride, S))
        else:
            c.ck(c.lib.gmg_frame_score6_nulls(c.gene.device(), c.nulls.h, _ptr(j.read_null), j.reads.h, out, stride, S))
        return [d2h(c, out, np.float64, 6 * stride, S).reshape(6, stride)[:, :j.total].copy()]
    return run


def _segment(fn, per_base, frame=1):
    def run(c, j, S, pre, keep, stall):
        n = j.segs.total_len if per_base else j.segs.n
        out = keep.dev(like(pre, 0, np.float64, n))
        stall()
        c.ck(getattr(c.lib, fn)(c.gene.device(), j.reads.h, j.segs.h, frame, out, S))
        return [d2h(c, out, np.float64, n, S)]
    return run


def _all_frame(c, j, S, pre, keep, stall):
    d_pre, d_fr = keep.dev(j.prefix), keep.dev(j.frames)
    out = keep.dev(like(pre, 0, np.float64, 6 * j.segs.n))
    stall()
    c.ck(c.lib.gmg_all_frame_score(c.gene.device(), j.reads.h, j.segs.h, d_pre, d_fr, out, S))
    return [d2h(c, out, np.float64, 6 * j.segs.n, S)]


def _window_distrib(c, j, S, pre, keep, stall):
    n = len(j.windows)
    d_w, d_f = keep.dev(j.windows), keep.dev(j.wframes)
    d_dist, d_prob = keep.dev(like(pre, 0, np.float32, 4 * n)), keep.dev(like(pre, 1, np.float64, n))
    stall()
    c.ck(c.lib.gmg_window_distrib(c.gene.device(), d_w, d_f, n, d_dist, d_prob, S))
    return [d2h(c, d_dist, np.float32, 4 * n, S), d2h(c, d_prob, np.float64, n, S)]


def _fixed_score(c, j, S, pre, keep, stall):
    out = keep.dev(like(pre, 0, np.float64, j.segs.n))
    stall()
    c.ck(c.lib.gmg_fixed_score(c.fixed.device(), j.reads.h, j.segs.h, 0, 12, out, S))
    return [d2h(c, out, np.float64, j.segs.n, S)]


def _strings(c, j, S, pre, keep, stall):
    n = len(c.string_models) * N_READS * 2
    arr = (C.c_void_p * len(c.string_models))(*[m.device() for m in c.string_models])
    out = keep.dev(like(pre, 0, np.float64, n))
    stall()
    c.ck(c.lib.gmg_score_reads_strings(arr, len(c.string_models), j.reads.h, out, S))
    return [d2h(c, out, np.float64, n, S)]


def _tophits(c, j, keep):
    h = C.c_void_p()
    c.ck(c.lib.gmg_tophits_create(j.reads.h, 2, C.byref(h)))
    keep.defer(c.lib.gmg_tophits_free, h)
    return h


def _tophits_fetch(c, h, pre):
    keys, models = like(pre, 0, np.int64, N_READS * 2), like(pre, 1, np.int32, N_READS * 2)
    c.ck(c.lib.gmg_tophits_fetch(h, _ptr(keys), _ptr(models)))
    return [keys, models]


def _tophits_update(c, j, S, pre, keep, stall):
    """the caller's raw device input d_sums is produced on S behind the stall (gmg_score_reads_strings); before that it holds the other
    job's sums, valid values that a mis-ordered update would take"""
    B = len(c.string_models)
    arr = (C.c_void_p * B)(*[m.device() for m in c.string_models])
    h = _tophits(c, j, keep)
    d_sums = keep.dev(j.other.sums)
    stall()
    c.ck(c.lib.gmg_score_reads_strings(arr, B, j.reads.h, d_sums, S))
    c.ck(c.lib.gmg_tophits_update_sums(h, d_sums, B, 0, None, 0, S))
    return _tophits_fetch(c, h, pre)


def _tophits_scores(c, j, S, pre, keep, stall):
    B = len(c.string_models)
    arr = (C.c_void_p * B)(*[m.device() for m in c.string_models])
    h = _tophits(c, j, keep)
    d = C.c_void_p()
    if pre is not None:                                               # the handle's scratch holds other sums; no slot changes (nothing informative)
        rev = (C.c_void_p * B)(*[m.device() for m in reversed(c.string_models)])
        none = np.zeros(B, np.uint8)
        c.ck(c.lib.gmg_tophits_scores(h, rev, B, 0, _ptr(none), 0, None, C.byref(d)))
    stall()
    c.ck(c.lib.gmg_tophits_scores(h, arr, B, 0, None, 0, S, C.byref(d)))
    return _tophits_fetch(c, h, pre) + [d2h(c, d, np.float64, B * N_READS * 2, S)]


def _tophits_format(c, j, S, pre, keep, stall):
    B = len(c.string_models)
    arr = (C.c_void_p * B)(*[m.device() for m in c.string_models])
    h = _tophits(c, j, keep)
    cap = B * N_READS * c.capi.TOPHITS_MAX_FIELD
    d_sums = keep.dev(j.other.sums)
    if pre is not None:
        # the handle's text buffer holds other lines, and longer ones (three more digits a field): the call under test does not
        # replace the buffer, which would hipFree the old one and wait for the whole device
        tmp, size = np.zeros(cap, np.uint8), C.c_size_t(cap)
        c.ck(c.lib.gmg_tophits_format_rows(h, keep.dev(j.other.sums * 1000.0), B, 0, _ptr(tmp), C.byref(size), None))
    out, size = like(pre, 0, np.uint8, cap), C.c_size_t(cap)
    stall()
    c.ck(c.lib.gmg_score_reads_strings(arr, B, j.reads.h, d_sums, S))
    c.ck(c.lib.gmg_tophits_format_rows(h, d_sums, B, 0, _ptr(out), C.byref(size), S))
    return [out[:size.value].copy()]


def _regions_text(device):
    def run(c, j, S, pre, keep, stall):
        L = c.api.Letters
        regs, n, blob, off = L._args(j.regions, j.heads)
        size = C.c_size_t(0)
        c.ck(c.lib.gmg_regions_text(j.letters.h, regs, n, blob, _ptr(off), C.byref(c.tparams), None, C.byref(size), None))
        if pre is not None:                                           # the handle's text buffer holds another text of the same length
            j.letters.regions_text_device(j.regions_alt, j.heads, c.tparams)
        if device:
            ptr, got = C.c_void_p(), C.c_size_t(0)
            stall()
            c.ck(c.lib.gmg_regions_text_device(j.letters.h, regs, n, blob, _ptr(off), C.byref(c.tparams), C.byref(ptr), C.byref(got), S))
            return [d2h(c, ptr, np.uint8, got.value, S)]
        out, cap = like(pre, 0, np.uint8, size.value), C.c_size_t(size.value)
        stall()
        c.ck(c.lib.gmg_regions_text(j.letters.h, regs, n, blob, _ptr(off), C.byref(c.tparams), _ptr(out), C.byref(cap), S))
        return [out[:cap.value].copy()]
    return run


def _runs_text(device):
    def run(c, j, S, pre, keep, stall):
        L = c.api.Letters
        kept, args = L._run_args(j.runs, j.sro, j.run_heads, None, None)
        size = C.c_size_t(0)
        c.ck(c.lib.gmg_runs_text(j.letters.h, *args, C.byref(c.rparams), None, C.byref(size), None))
        if pre is not None:
            j.letters.runs_text_device(j.runs_alt, j.sro, j.run_heads, c.rparams)
        if device:
            ptr, got = C.c_void_p(), C.c_size_t(0)
            stall()
            c.ck(c.lib.gmg_runs_text_device(j.letters.h, *args, C.byref(c.rparams), C.byref(ptr), C.byref(got), S))
            return [d2h(c, ptr, np.uint8, got.value, S)]
        out, cap = like(pre, 0, np.uint8, size.value), C.c_size_t(size.value)
        stall()
        c.ck(c.lib.gmg_runs_text(j.letters.h, *args, C.byref(c.rparams), _ptr(out), C.byref(cap), S))
        return [out[:cap.value].copy()]
    return run


def _orf_arrays(c, j, pre):
    res = like(pre, 0, c.api.ORF_RESULT_DTYPE, max(len(j.orfs), 1))
    starts = like(pre, 1, c.api.START_DTYPE, max(j.max_starts, 1))
    return res, starts


def _orf_result(j, res, starts):
    n = int(res["n_starts"][:len(j.orfs)].sum())
    return [res[:len(j.orfs)].copy(), starts[:n].copy()]


def _score_orfs(c, j, S, pre, keep, stall):
    prm, alt, n = c.orf_params(), c.orf_params(True), C.c_uint64()
    res, starts = _orf_arrays(c, j, pre)
    if pre is not None:                                               # the batch's result arrays hold the scores under other parameters
        c.ck(c.lib.gmg_score_orfs_begin(c.gene.device(), c.null.device(), j.reads.h, j.batch, C.byref(alt), C.byref(n), None))
    stall()
    c.ck(c.lib.gmg_score_orfs(c.gene.device(), c.null.device(), j.reads.h, j.batch, C.byref(prm), _ptr(res), _ptr(starts), S))
    return _orf_result(j, res, starts)


def _score_orfs_begin(c, j, S, pre, keep, stall):
    prm, alt, n = c.orf_params(), c.orf_params(True), C.c_uint64()
    res, starts = _orf_arrays(c, j, pre)
    if pre is not None:
        c.ck(c.lib.gmg_score_orfs_begin(c.gene.device(), c.null.device(), j.reads.h, j.batch, C.byref(alt), C.byref(n), None))
    stall()
    c.ck(c.lib.gmg_score_orfs_begin(c.gene.device(), c.null.device(), j.reads.h, j.batch, C.byref(prm), C.byref(n), S))
    c.ck(c.lib.gmg_score_orfs_fetch(j.batch, _ptr(res), _ptr(starts), S))
    return _orf_result(j, res, starts) + [np.array([n.value], np.uint64)]


def _score_orfs_fetch(c, j, S, pre, keep, stall):
    prm, n = c.orf_params(), C.c_uint64()
    res, starts = _orf_arrays(c, j, pre)
    c.ck(c.lib.gmg_score_orfs_begin(c.gene.device(), c.null.device(), j.reads.h, j.batch, C.byref(prm), C.byref(n), None))
    stall()
    c.ck(c.lib.gmg_score_orfs_fetch(j.batch, _ptr(res), _ptr(starts), S))
    return _orf_result(j, res, starts)


def _mg_fetch(c, j, res, S, pre, errs):
    no, ns = C.c_uint64(), C.c_uint64()
    c.ck(c.lib.gmg_mg_result_info(res, C.byref(no), C.byref(ns)))
    orfs = like(pre, 0, c.api.MG_ORF_DTYPE, max(no.value, 1))
    starts = like(pre, 1, c.api.START_DTYPE, max(ns.value, 1))
    off = like(pre, 2, np.uint64, N_READS + 1)
    c.ck(c.lib.gmg_mg_result_fetch_on(res, _ptr(orfs), _ptr(starts), _ptr(off), S))
    out = [orfs[:no.value].copy(), starts[:ns.value].copy(), off]
    if errs:
        e = like(pre, 3, c.api.START_ERRORS_DTYPE, max(ns.value, 1))
        c.ck(c.lib.gmg_mg_result_fetch_errors(res, _ptr(e)))
        out.append(e[:ns.value].copy())
    return out


def _mg_reads(flags=0, per_read_nulls=False):
    def run(c, j, S, pre, keep, stall):
        prm = c.mg_params(flags, c.nulls if per_read_nulls else None, j.read_null)
        # the default mode also hands the caller its Frame_Scores table
        table = None if flags or per_read_nulls else keep.dev(like(pre, 3, np.float64, 6 * j.total))
        res = C.c_void_p()
        stall()
        c.ck(c.lib.gmg_mg_score_reads(c.gene.device(), c.null.device(), j.reads.h, C.byref(prm), table, C.byref(res), S))
        keep.defer(c.lib.gmg_mg_result_free, res)
        out = _mg_fetch(c, j, res, S, pre, bool(flags))
        return out if table is None else out + [d2h(c, table, np.float64, 6 * j.total, S)]
    return run


def _mg_groups(c, j, S, pre, keep, stall):
    prm = c.mg_params(0, c.nulls, j.read_null)
    groups = (c.capi.MgGroup * 2)(c.capi.MgGroup(c.gene.device(), 0, 120), c.capi.MgGroup(c.gene2.device(), 120, N_READS))
    res = C.c_void_p()
    stall()
    c.ck(c.lib.gmg_mg_score_groups(groups, 2, c.null.device(), j.reads.h, C.byref(prm), C.byref(res), S))
    keep.defer(c.lib.gmg_mg_result_free, res)
    return _mg_fetch(c, j, res, S, pre, False)


def _find_orfs(c, j, S, pre, keep, stall):
    prm = c.mg_params()
    res = C.c_void_p()
    stall()
    c.ck(c.lib.gmg_find_orfs(j.reads.h, C.byref(prm), C.byref(res), S))
    keep.defer(c.lib.gmg_mg_result_free, res)
    return _mg_fetch(c, j, res, S, pre, False)


def _mg_result_fetch_on(c, j, S, pre, keep, stall):
    stall()
    return _mg_fetch(c, j, j.mg_res, S, pre, False)


def _ingest(piece_min):
    def run(c, j, S, pre, keep, stall):
        reads, index = C.c_void_p(), C.c_void_p()
        table = keep.dev(like(pre, 3, np.float64, 6 * j.total))
        stall()
        c.ck(c.lib.gmg_fasta_ingest_on(j.fasta, len(j.fasta), C.byref(reads), C.byref(index), S))
        keep.defer(c.lib.gmg_reads_free, reads)
        keep.defer(c.lib.gmg_fasta_free, index)
        n, total, gc = C.c_uint64(), C.c_uint64(), C.c_uint64()
        c.ck(c.lib.gmg_fasta_info(index, C.byref(n), C.byref(total), C.byref(gc)))
        assert (n.value, total.value) == (N_READS, j.total)
        hb, he = like(pre, 1, np.uint64, N_READS), like(pre, 2, np.uint64, N_READS)
        c.ck(c.lib.gmg_fasta_headers(index, _ptr(hb), _ptr(he)))
        # the packed batch, read through a scoring call on the same stream
        c.ck(c.lib.gmg_frame_score6(c.gene.device(), c.null.device(), reads, table, S))
        return [np.array([n.value, total.value, gc.value], np.uint64), hb, he, d2h(c, table, np.float64, 6 * j.total, S)]
    return run


def _entropy_regions(c, j, S, pre, keep, stall):
    n = len(j.regions)
    d_counts, d_dist = keep.dev(like(pre, 0, np.int32, 20 * n)), keep.dev(like(pre, 1, np.float64, 3 * n))
    stall()
    c.ck(c.lib.gmg_entropy_regions(j.reads.h, _ptr(j.regions), n, c.aa, _ptr(c.pos), _ptr(c.neg), d_counts, d_dist, S))
    return [d2h(c, d_counts, np.int32, 20 * n, S), d2h(c, d_dist, np.float64, 3 * n, S)]


def _entropy_orfs(c, j, S, pre, keep, stall):
    n = j.orf_res.n_orfs
    d_counts, d_dist = keep.dev(like(pre, 0, np.int32, 20 * n)), keep.dev(like(pre, 1, np.float64, 3 * n))
    stall()
    c.ck(c.lib.gmg_entropy_orfs(j.reads.h, j.orf_res.h, c.aa, _ptr(c.pos), _ptr(c.neg), d_counts, d_dist, S))
    return [d2h(c, d_counts, np.int32, 20 * n, S), d2h(c, d_dist, np.float64, 3 * n, S)]


def _genes_audit(c, j, S, pre, keep, stall):
    h, nr, ni = C.c_void_p(), C.c_uint64(), C.c_uint64()
    stall()
    c.ck(c.lib.gmg_genes_audit(j.reads.h, _ptr(j.regions), len(j.regions), C.byref(c.audit), None, 0, C.byref(h), S))
    keep.defer(c.lib.gmg_audit_free, h)
    c.ck(c.lib.gmg_audit_info(h, C.byref(nr), C.byref(ni)))
    rec, inner, hist = like(pre, 0, c.api.GENE_AUDIT_DTYPE, max(nr.value, 1)), like(pre, 1, np.int32, max(ni.value, 1)), like(pre, 2, np.int64, 65)
    c.ck(c.lib.gmg_audit_fetch(h, _ptr(rec), _ptr(inner), _ptr(hist)))
    return [rec[:nr.value].copy(), inner[:ni.value].copy(), hist]


def _window_counts(c, j, S, pre, keep, stall):
    h, nr, nw = C.c_void_p(), C.c_uint64(), C.c_uint64()
    stall()
    c.ck(c.lib.gmg_window_counts(j.reads.h, 100, 37, None, 0, C.byref(h), S))
    keep.defer(c.lib.gmg_windows_free, h)
    c.ck(c.lib.gmg_windows_info(h, C.byref(nr), C.byref(nw)))
    off, counts = like(pre, 0, np.uint64, nr.value + 1), like(pre, 1, np.int32, 5 * max(nw.value, 1))
    c.ck(c.lib.gmg_windows_fetch(h, _ptr(off), _ptr(counts)))
    return [off, counts[:5 * nw.value].copy()]


def _regions_uncovered(c, j, S, pre, keep, stall):
    iv = np.ascontiguousarray(j.intervals.astype(np.uint32).view(np.int32))
    h, ng = C.c_void_p(), C.c_uint64()
    stall()
    c.ck(c.lib.gmg_regions_uncovered(j.reads.h, _ptr(iv), len(iv), 5, C.byref(h), S))
    keep.defer(c.lib.gmg_gaps_free, h)
    c.ck(c.lib.gmg_gaps_info(h, C.byref(ng)))
    gaps, off = like(pre, 0, np.int32, 4 * max(ng.value, 1)), like(pre, 1, np.uint64, N_READS + 1)
    c.ck(c.lib.gmg_gaps_fetch(h, _ptr(gaps), _ptr(off)))
    return [gaps[:4 * ng.value].copy(), off]


def _features_count(c, j, S, pre, keep, stall):
    arr = (c.capi.FeatureGene * len(j.genes))(*[c.capi.FeatureGene(*g) for g in j.genes])
    h = C.c_void_p()
    stall()
    c.ck(c.lib.gmg_features_count(j.reads.h, arr, len(j.genes), None, 0, C.byref(c.fparams), C.byref(h), S))
    keep.defer(c.lib.gmg_features_free, h)
    out = []
    for which in (0, 1):                                              # (the result lives on the host)
        t = c.capi.FeaturesTable()
        c.ck(c.lib.gmg_features_fetch(h, which, C.byref(t)))
        out += [np.array(t.lengths[:t.n_lengths], np.int64), np.array(list(t.starts), np.int64), np.array(list(t.orient) + list(t.orient_raw))]
        out += [np.array(t.dist[k][:t.n_dist[k]], np.float64) for k in range(3)]
    return out


ERR_I, ERR_S = 2, 4                                                   # GMG_MG_ALLOW_INDELS, GMG_MG_ALLOW_SUBS
ROWS = [
    Row("regions_text", "gmg_regions_text", _regions_text(False)),
    Row("regions_text_device", "gmg_regions_text_device", _regions_text(True)),
    Row("runs_text", "gmg_runs_text", _runs_text(False)),
    Row("runs_text_device", "gmg_runs_text_device", _runs_text(True)),
    Row("frame_score6", "gmg_frame_score6", _frame6("plain")),
    Row("frame_score6_strided", "gmg_frame_score6_strided", _frame6("strided")),
    Row("frame_score6_nulls", "gmg_frame_score6_nulls", _frame6("nulls")),
    Row("segment_frame_score", "gmg_segment_frame_score", _segment("gmg_segment_frame_score", True)),
    Row("segment_cumscore", "gmg_segment_cumscore", _segment("gmg_segment_cumscore", True)),
    Row("score_string", "gmg_score_string", _segment("gmg_score_string", False)),
    Row("segment_partial_prob", "gmg_segment_partial_prob", _segment("gmg_segment_partial_prob", False)),
    Row("all_frame_score", "gmg_all_frame_score", _all_frame),
    Row("window_distrib", "gmg_window_distrib", _window_distrib),
    Row("fixed_score", "gmg_fixed_score", _fixed_score),
    Row("score_reads_strings_fused", "gmg_score_reads_strings", _strings, {"strings_fused": 1}),
    Row("score_reads_strings_two_pass", "gmg_score_reads_strings", _strings, {"strings_fused": 0}),
    Row("score_orfs_path0", "gmg_score_orfs", _score_orfs, {"orfs_exact_path": 0}),
    Row("score_orfs_path1", "gmg_score_orfs", _score_orfs, {"orfs_exact_path": 1}),
    Row("score_orfs_path2", "gmg_score_orfs", _score_orfs, {"orfs_exact_path": 2}),
    Row("score_orfs_begin", "gmg_score_orfs_begin", _score_orfs_begin),
    Row("score_orfs_fetch", "gmg_score_orfs_fetch", _score_orfs_fetch),
    Row("mg_score_reads", "gmg_mg_score_reads", _mg_reads()),
    Row("mg_score_reads_indels", "gmg_mg_score_reads", _mg_reads(ERR_I)),
    Row("mg_score_reads_subs", "gmg_mg_score_reads", _mg_reads(ERR_S)),
    Row("mg_score_reads_nulls", "gmg_mg_score_reads", _mg_reads(0, True)),
    Row("mg_score_groups", "gmg_mg_score_groups", _mg_groups),
    Row("find_orfs", "gmg_find_orfs", _find_orfs),
    Row("mg_result_fetch_on", "gmg_mg_result_fetch_on", _mg_result_fetch_on),
    Row("fasta_ingest_on", "gmg_fasta_ingest_on", _ingest(None)),
    Row("fasta_ingest_on_pieces", "gmg_fasta_ingest_on", _ingest(0), {"ingest_piece_min": 0}),
    Row("entropy_regions", "gmg_entropy_regions", _entropy_regions),
    Row("entropy_orfs", "gmg_entropy_orfs", _entropy_orfs),
    Row("genes_audit", "gmg_genes_audit", _genes_audit),
    Row("window_counts", "gmg_window_counts", _window_counts),
    Row("regions_uncovered", "gmg_regions_uncovered", _regions_uncovered),
    Row("tophits_update_sums", "gmg_tophits_update_sums", _tophits_update),
    Row("tophits_scores", "gmg_tophits_scores", _tophits_scores),
    Row("tophits_format_rows", "gmg_tophits_format_rows", _tophits_format),
    Row("features_count", "gmg_features_count", _features_count),
]
# the side-stream rows once more on the caller's stream alone: these must be conclusive with the null stream stalled
ROWS += [Row(r.name + "_one_stream", r.entry, r.run, dict(r.options, mg_one_stream=1)) for r in list(ROWS) if r.entry in SIDE_STREAM_ENTRIES]


# ------------------------------------------------------------------------------------------------------------------------------
# constructors: make(c, j) -> handle on the null stream; use(c, j, handle, S, keep) -> result of a call on S that reads all of it
# ------------------------------------------------------------------------------------------------------------------------------
class Ctor:
    def __init__(self, name, entries, make, use, free):
        self.name, self.entries, self.make, self.use, self.free = name, entries, make, use, free

    def __repr__(self):
        return self.name


class _Reads:
    """a bare gmg_reads handle with what the scoring helpers need of a Reads object"""

    def __init__(self, c, h):
        self.h = h
        n, total = C.c_uint64(), C.c_uint64()
        c.ck(c.lib.gmg_reads_info(h, C.byref(n), C.byref(total)))
        self.n_reads, self.total = n.value, total.value


def _use_reads(c, j, reads, S, keep):
    """six-frame scores of the whole batch: every base and every offset of the new handle is read"""
    out = keep.dev(np.zeros(6 * max(reads.total, 1)))
    c.ck(c.lib.gmg_frame_score6(c.gene.device(), c.null.device(), reads.h, out, S))
    return [d2h(c, out, np.float64, 6 * reads.total, S)]


def _free_reads(c, reads):
    c.lib.gmg_reads_free(reads.h)


def _make_reads_upload(c, j, keep):
    packed, off = c.api.pack_strings(j.seqs)
    h = C.c_void_p()
    c.ck(c.lib.gmg_reads_upload(_ptr(packed), _ptr(off), N_READS, C.byref(h)))
    return _Reads(c, h)


def _make_reads_wrap(c, j, keep):
    packed, off = c.api.pack_strings(j.seqs)
    d_packed, d_off = keep.dev(packed), keep.dev(off)                 # (valid and complete before the stall)
    h = C.c_void_p()
    c.ck(c.lib.gmg_reads_wrap_device(d_packed, d_off, N_READS, j.total, C.byref(h)))
    return _Reads(c, h)


def _make_reads_select(c, j, keep):
    idx = np.arange(N_READS - 1, -1, -1, dtype=np.uint64)
    h = C.c_void_p()
    c.ck(c.lib.gmg_reads_select(j.reads.h, _ptr(idx), len(idx), C.byref(h)))
    return _Reads(c, h)


def _make_reads_extract(c, j, keep):
    h = C.c_void_p()
    c.ck(c.lib.gmg_reads_extract(j.reads.h, _ptr(j.regions), len(j.regions), 0, None, None, 0, C.byref(h)))
    return _Reads(c, h)


def _make_reads_splice(c, j, keep):
    h = C.c_void_p()
    c.ck(c.lib.gmg_reads_splice(j.reads.h, _ptr(j.runs), len(j.runs), _ptr(j.sro), len(j.sro) - 1, 0, C.byref(h)))
    return _Reads(c, h)


def _make_tophits(c, j, keep):
    h = C.c_void_p()
    c.ck(c.lib.gmg_tophits_create(j.reads.h, 2, C.byref(h)))
    return h


def _use_tophits(c, j, h, S, keep):
    d_sums = keep.dev(j.sums)
    c.ck(c.lib.gmg_tophits_update_sums(h, d_sums, len(c.string_models), 0, None, 0, S))
    return _tophits_fetch(c, h, None)


def _null_tables(c):
    tabs = [c.gpu.Icm.indep(g).tables() for g in c.gcs]
    return np.ascontiguousarray(np.stack([t[0] for t in tabs])), np.ascontiguousarray(np.stack([t[1] for t in tabs]))


def _make_null_upload(c, j, keep):
    keep.icms = [c.gpu.Icm.indep(g) for g in c.gcs]
    arr = (C.c_void_p * 3)(*[m.device() for m in keep.icms])
    h = C.c_void_p()
    c.ck(c.lib.gmg_null_set_upload(arr, 3, C.byref(h)))
    return h


def _make_null_tables(c, j, keep):
    mip, prob = _null_tables(c)
    h = C.c_void_p()
    c.ck(c.lib.gmg_null_set_from_tables(_ptr(mip), _ptr(prob), 3, C.byref(h)))
    return h


def _make_null_build(c, j, keep):
    gcs = np.array(c.gcs)
    buf = ((C.c_char * 4) * 8)()
    for i, s in enumerate(STOPS):
        buf[i].value = s.encode()
    h = C.c_void_p()
    c.ck(c.lib.gmg_null_set_build(_ptr(gcs), 3, buf, 3, C.byref(h)))
    return h


def _use_nulls(c, j, h, S, keep):
    out = keep.dev(np.zeros(6 * j.total))
    c.ck(c.lib.gmg_frame_score6_nulls(c.gene.device(), h, _ptr(j.read_null), j.reads.h, out, j.total, S))
    return [d2h(c, out, np.float64, 6 * j.total, S)]


def _make_model(c, j, keep):
    w, d, p, n = c.gene.params
    mip, prob = c.gene.tables()
    h = C.c_void_p()
    c.ck(c.lib.gmg_model_upload(_ptr(mip), _ptr(prob), w, d, p, n, C.byref(h)))
    return h


def _use_model(c, j, h, S, keep):
    out = keep.dev(np.zeros(j.segs.total_len))
    c.ck(c.lib.gmg_segment_cumscore(h, j.reads.h, j.segs.h, 1, out, S))
    return [d2h(c, out, np.float64, j.segs.total_len, S)]


def _make_fixed(c, j, keep):
    """six sub-models of depth 0: one node each, its row the four log-probabilities"""
    rng = np.random.default_rng(17)
    probs = [np.log(rng.dirichlet(np.ones(4))).astype(np.float32).reshape(1, 4) for _ in range(6)]
    keep.fixed = c.gpu.FixedModel([2, 0, 1, 5, 4, 3], [(np.array([-1], np.int16), p, 0) for p in probs])
    return keep.fixed


def _use_fixed(c, j, m, S, keep):
    out = keep.dev(np.zeros(j.segs.n))
    c.ck(c.lib.gmg_fixed_score(m.device(), j.reads.h, j.segs.h, 0, 6, out, S))
    return [d2h(c, out, np.float64, j.segs.n, S)]


def _make_orfs(c, j, keep):
    h, ms = C.c_void_p(), C.c_uint64()
    c.ck(c.lib.gmg_orfs_upload(j.reads.h, _ptr(j.orfs), len(j.orfs), C.byref(ms), C.byref(h)))
    return h


def _use_orfs(c, j, h, S, keep):
    prm = c.orf_params()
    res, starts = _orf_arrays(c, j, None)
    c.ck(c.lib.gmg_score_orfs(c.gene.device(), c.null.device(), j.reads.h, h, C.byref(prm), _ptr(res), _ptr(starts), S))
    return _orf_result(j, res, starts)


def _make_segments(c, j, keep):
    h, total = C.c_void_p(), C.c_uint64()
    c.ck(c.lib.gmg_segments_upload(j.reads.h, _ptr(j.segs.rows), j.segs.n, None, C.byref(total), C.byref(h)))
    return h


def _use_segments(c, j, h, S, keep):
    out = keep.dev(np.zeros(j.segs.total_len))
    c.ck(c.lib.gmg_segment_cumscore(c.gene.device(), j.reads.h, h, 1, out, S))
    return [d2h(c, out, np.float64, j.segs.total_len, S)]


def _make_letters(c, j, keep):
    return c.gpu.Letters("".join(j.seqs).upper().encode(), j.off)


def _use_letters(c, j, l, S, keep):
    regs, n, blob, off = c.api.Letters._args(j.regions, j.heads)
    size = C.c_size_t(0)
    c.ck(c.lib.gmg_regions_text(l.h, regs, n, blob, _ptr(off), C.byref(c.tparams), None, C.byref(size), None))
    out, cap = np.zeros(size.value, np.uint8), C.c_size_t(size.value)
    c.ck(c.lib.gmg_regions_text(l.h, regs, n, blob, _ptr(off), C.byref(c.tparams), _ptr(out), C.byref(cap), S))
    return [out]


def _make_trainer(c, j, keep):
    return c.gpu.Trainer(j.reads, 12, 2, 3)


def _use_trainer(c, j, t, S, keep):
    return [t.level_counts(0)]                                        # (the trainer has no stream parameter: the null stream)


CTORS = [
    Ctor("tophits_create", ["gmg_tophits_create"], _make_tophits, _use_tophits, lambda c, h: c.lib.gmg_tophits_free(h)),
    Ctor("null_set_upload", ["gmg_null_set_upload"], _make_null_upload, _use_nulls, lambda c, h: c.lib.gmg_null_set_free(h)),
    Ctor("null_set_from_tables", ["gmg_null_set_from_tables"], _make_null_tables, _use_nulls, lambda c, h: c.lib.gmg_null_set_free(h)),
    Ctor("null_set_build", ["gmg_null_set_build"], _make_null_build, _use_nulls, lambda c, h: c.lib.gmg_null_set_free(h)),
    Ctor("model_upload", ["gmg_model_upload"], _make_model, _use_model, lambda c, h: c.lib.gmg_model_free(h)),
    Ctor("fixed_model_upload", ["gmg_fixed_model_upload"], _make_fixed, _use_fixed, lambda c, m: m.close()),
    Ctor("orfs_upload", ["gmg_orfs_upload"], _make_orfs, _use_orfs, lambda c, h: c.lib.gmg_orf_batch_free(h)),
    Ctor("segments_upload", ["gmg_segments_upload"], _make_segments, _use_segments, lambda c, h: c.lib.gmg_segments_free(h)),
    Ctor("letters_upload", ["gmg_letters_upload"], _make_letters, _use_letters, lambda c, l: l.close()),
    Ctor("reads_upload", ["gmg_reads_upload"], _make_reads_upload, _use_reads, _free_reads),
    Ctor("reads_wrap_device", ["gmg_reads_wrap_device"], _make_reads_wrap, _use_reads, _free_reads),
    Ctor("reads_select", ["gmg_reads_select"], _make_reads_select, _use_reads, _free_reads),
    Ctor("reads_extract", ["gmg_reads_extract"], _make_reads_extract, _use_reads, _free_reads),
    Ctor("reads_splice", ["gmg_reads_splice"], _make_reads_splice, _use_reads, _free_reads),
    Ctor("trainer_create", ["gmg_trainer_create"], _make_trainer, _use_trainer, lambda c, t: t.close()),
]
