#!/usr/bin/env python3
"""gmg_window_counts and gmg_regions_uncovered on batches resident on the device.
  reads   1 M synthetic reads of 500 bp: (W, S) = (100, 50), nine windows a read, and (500, 500), one window a read
  genome  tests/golden/data/NC_000915.fna (1.67 Mbases, one record): (1000, 1000) and (1000, 1) -- the design constraint of the
          kernel: 1000 times the rows from the same bases must cost what the rows cost, not 1000 passes over the bases
  gaps    gmg_regions_uncovered on the ORFs gmg_mg_score_reads accepts on the 1 M reads, as intervals
Per leg one JSON block: ms per call (3 warm-ups, median of 10, host clock around the call and gmg_synchronize, nothing copied back),
the bytes the call has to move at least (the packed bases once, the rows, both offset arrays; for the gaps the intervals in and the
gaps out) and what fraction of the HBM roof (6.3 TB/s, the measured copy rate of the card; its data sheet says 8.0) that is, and in
the same process gmg_reads_select of the whole batch: a plain copy of the same packed bases, what reading them once costs.  The
Python restatement (tests/windows_oracle.py, one core) runs on the first 2,000 reads (the whole genome), is compared with the device
row by row -- a mismatch fails the benchmark -- and is scaled by bases.

usage: python3 tests/bench/bench_windows.py [n_reads]"""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _gmg_pkg  # noqa: E402
import windows_oracle as wo  # noqa: E402

gmg = _gmg_pkg.load()
n, L = (int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000), 500
ROOF = 6.3e12
gmg.init(0)
lib = gmg.capi.lib()
ck = gmg.api._ck


def timed(fn):
    for _ in range(3):
        fn()
    t = []
    for _ in range(10):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(t)), float(min(t)), float(max(t))


def select_ms(reads, n_reads):
    idx = np.arange(n_reads, dtype=np.uint64)

    def call():
        h = C.c_void_p()
        ck(lib.gmg_reads_select(reads.h, gmg.api._ptr(idx), n_reads, C.byref(h)))
        ck(lib.gmg_synchronize(None))
        lib.gmg_reads_free(h)
    return timed(call)


def window_leg(reads, n_reads, total_bases, W, S, amb, sample_seqs, sample_reads, sample_amb, sel):
    ab = np.ascontiguousarray(amb, np.uint64) if amb is not None and len(amb) else None

    def call():
        h = C.c_void_p()
        ck(lib.gmg_window_counts(reads.h, W, S, gmg.api._ptr(ab) if ab is not None else None, 0 if ab is None else len(ab), C.byref(h), None))
        ck(lib.gmg_synchronize(None))
        nw = C.c_uint64()
        ck(lib.gmg_windows_info(h, None, C.byref(nw)))
        lib.gmg_windows_free(h)
        return nw.value
    rows = call()
    ms, lo, hi = timed(call)
    t0 = time.perf_counter()
    want_off, want = wo.batch_window_counts(sample_seqs, W, S)
    oracle_s = time.perf_counter() - t0
    off, counts = gmg.window_counts(sample_reads, W, S, amb=sample_amb)
    assert [int(x) for x in off] == want_off and counts.tolist() == want, "the sample differs from the restatement at (%d, %d)" % (W, S)
    sample_bases = sum(len(s) for s in sample_seqs)
    must = total_bases // 4 + 20 * rows + 16 * (n_reads + 1)
    return {"window_len": W, "window_skip": S, "rows": int(rows), "window_counts_ms": ms, "window_counts_ms_min_max": [lo, hi],
            "bytes_at_least": int(must), "fraction_of_hbm_roof": must / (ms * 1e-3) / ROOF, "rows_per_s": rows / (ms * 1e-3),
            "reads_select_whole_batch_ms": sel[0], "ratio_to_reads_select": ms / sel[0],
            "restatement_python3_one_core": {"sample_bases": int(sample_bases), "sample_s": oracle_s,
                                             "scaled_to_batch_s": oracle_s * total_bases / max(sample_bases, 1), "sample_equals_device": True}}


out = {"reads": n, "read_len": L, "hbm_roof_bytes_per_s": ROOF,
       "timing": "3 warm-ups, median of 10 calls; host clock around the call and gmg_synchronize; nothing copied back"}

# ---- the reads ----
packed, off = gmg.synth.packed_reads(n, L, 1)
reads = gmg.Reads(packed, off)
m = min(2000, n)
sample = [gmg.synth.unpack_ascii(packed, k * L, L).decode() for k in range(m)]
sample_reads = gmg.Reads.from_strings(sample)
sel = select_ms(reads, n)
out["reads_legs"] = [window_leg(reads, n, n * L, W, S, None, sample, sample_reads, None, sel) for W, S in ((100, 50), (500, 500))]

# ---- the gaps: the accepted ORFs of the batch as intervals ----
gene_icm = gmg.Icm.open(os.path.join(ROOT, "tests", "golden", "data", "NC_000915.icm"))
orfs, _, _ = gmg.mg_score_reads(gene_icm, gmg.Icm.indep(0.5), reads, accepted_only=True)
lib.gmg_trim_cache()
fwd = orfs["frame"] > 0
glen = np.maximum(orfs["gene_len"].astype(np.int64), 0) + 3                       # the gene with its stop codon
s1 = np.where(fwd, orfs["stop_position"].astype(np.int64) - orfs["gene_len"], orfs["stop_position"].astype(np.int64) + orfs["gene_len"] + 2)
lo = np.where(fwd, s1 - 1, s1 - glen)
hi = np.clip(lo + glen, 0, L)                                                     # (ORFs truncated by the read's end: clipped to the read)
lo = np.clip(lo, 0, L)
iv = np.ascontiguousarray(np.stack([orfs["read"].astype(np.int64), lo, np.maximum(lo, hi)], 1).astype(np.int32))


def gaps_call():
    h = C.c_void_p()
    ck(lib.gmg_regions_uncovered(reads.h, gmg.api._ptr(iv), len(iv), 0, C.byref(h), None))
    ck(lib.gmg_synchronize(None))
    ng = C.c_uint64()
    ck(lib.gmg_gaps_info(h, C.byref(ng)))
    lib.gmg_gaps_free(h)
    return ng.value


n_gaps = gaps_call()
g_ms, g_lo, g_hi = timed(gaps_call)
sub = iv[iv[:, 0] < m]
t0 = time.perf_counter()
want, want_off = wo.batch_uncovered([L] * m, [tuple(int(x) for x in row) for row in sub])
oracle_s = time.perf_counter() - t0
gaps, goff = gmg.regions_uncovered(sample_reads, sub)
assert [tuple(int(x) for x in g) for g in gaps] == want and [int(x) for x in goff] == want_off, "the sample's gaps differ from the restatement"
must = 12 * len(iv) + 16 * n_gaps + 16 * (n + 1)
out["gaps_of_accepted_orfs"] = {"intervals": int(len(iv)), "gaps": int(n_gaps), "regions_uncovered_ms": g_ms, "regions_uncovered_ms_min_max": [g_lo, g_hi],
                                "bytes_at_least": int(must), "fraction_of_hbm_roof": must / (g_ms * 1e-3) / ROOF,
                                "reads_select_whole_batch_ms": sel[0], "ratio_to_reads_select": g_ms / sel[0],
                                "restatement_python3_one_core": {"sample_intervals": int(len(sub)), "sample_s": oracle_s,
                                                                 "scaled_to_batch_s": oracle_s * len(iv) / max(len(sub), 1),
                                                                 "sample_equals_device": True}}
reads.close()
lib.gmg_trim_cache()

# ---- the genome ----
data = open(os.path.join(ROOT, "tests", "golden", "data", "NC_000915.fna"), "rb").read()
genome, _, _ = gmg.Reads.from_fasta_bytes(data)
amb, _ = gmg.fasta_ambiguous(data)
letters = [b"".join(data[data.index(b"\n"):].split()).decode()]
gsel = select_ms(genome, 1)
legs = [window_leg(genome, 1, genome.total_bases, W, S, amb, letters, genome, amb, gsel) for W, S in ((1000, 1000), (1000, 1))]
out["genome_bases"] = genome.total_bases
out["genome_legs"] = legs
out["genome_1000_1_over_1000_1000"] = {"ms_ratio": legs[1]["window_counts_ms"] / legs[0]["window_counts_ms"],
                                       "rows_ratio": legs[1]["rows"] / legs[0]["rows"], "window_len_over_skip": 1000.0}
print(json.dumps(out))
