#!/usr/bin/env python3
"""Phymm's classification step (integration/phymm_gpu's workload): n reads of 500 bp against 64 distinct period-1 ICMs
(tests/models64.py).  Prints one JSON line:
  * ms per model for the scores alone (gmg_score_reads_strings) and for scores + top hits (gmg_tophits_scores: the same scoring,
    the slot update and its flag check), so the update's share shows as the difference,
  * the device formatter (gmg_tophits_format_rows: two passes, the scan and the copy to page-locked host memory) in GB/s of text,
  * the host baseline: CPython's "%.4f" (one core) on a sample of 2 M values, in MB/s of text.
Every timed call is checked first: the slots against the numpy oracle on a read sample, the text against "%.4f".

usage: python3 tests/bench/bench_phymm.py [n_reads]"""
import ctypes as C
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _gmg_pkg  # noqa: E402
import models64  # noqa: E402
import phymm_oracle as po  # noqa: E402

gmg = _gmg_pkg.load()
lib = gmg.capi.lib()
n = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000
L, B, T, REPS = 500, 64, 3, 3
gmg.init(0)
packed, off = gmg.synth.packed_reads(n, L, 23)
reads = gmg.Reads(packed, off)
with tempfile.TemporaryDirectory() as tmp:
    models = [m for m, _ in models64.period1_models(gmg, tmp, B)]
arr = (C.c_void_p * B)(*[m.device() for m in models])
sums = gmg.api._DeviceBuffer(B * n * 2 * 8)
res = {"reads": n, "read_len": L, "models": B, "top_hits": T}


def timed(f):
    ts = []
    for _ in range(REPS):
        t0 = time.perf_counter()
        f()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts)) * 1e3


# scores alone (the call synchronises)
gmg.api._ck(lib.gmg_score_reads_strings(arr, B, reads.h, sums.ptr, None))
res["ms_per_model_scores"] = timed(lambda: gmg.api._ck(lib.gmg_score_reads_strings(arr, B, reads.h, sums.ptr, None))) / B

# scores + top hits, checked on a sample of reads
h = gmg.TopHits(reads, T)
d = C.c_void_p()
gmg.api._ck(lib.gmg_tophits_scores(h.h, arr, B, 0, None, 0, None, C.byref(d)))
keys, slots = h.fetch()
host = np.empty(B * n * 2, np.float64)
gmg.api._ck(lib.gmg_memcpy_d2h(host.ctypes.data_as(C.c_void_p), d, host.nbytes, None))
gmg.api._ck(lib.gmg_synchronize(None))
host = host.reshape(B, n, 2)
sample = np.random.default_rng(1).integers(0, n, 2000)
wk, wm = po.tophits_numpy(po.merged_keys(host[:, sample]), T)
assert np.array_equal(slots[sample], wm) and np.array_equal(keys[sample], wk)


def one_pass():
    hh = gmg.TopHits(reads, T)
    gmg.api._ck(lib.gmg_tophits_scores(hh.h, arr, B, 0, None, 0, None, None))
    hh.close()


res["ms_per_model_scores_tophits"] = timed(one_pass) / B
res["tophits_overhead_pct"] = 100.0 * (res["ms_per_model_scores_tophits"] / res["ms_per_model_scores"] - 1.0)

# the device formatter: into page-locked host memory
cap = B * n * gmg.capi.TOPHITS_MAX_FIELD
text = np.empty(cap, np.uint8)
gmg.api._ck(lib.gmg_host_register(text.ctypes.data_as(C.c_void_p), cap))
size = C.c_size_t(cap)


def fmt():
    size.value = cap
    gmg.api._ck(lib.gmg_tophits_format_rows(h.h, d, B, 0, text.ctypes.data_as(C.c_void_p), C.byref(size), None))


fmt()
nbytes = size.value
lines = text[:nbytes].tobytes().split(b"\n")
for b in (0, B - 1):
    row = lines[b].split(b"\t")
    for r in (0, 1, n - 1):
        assert row[r].decode() == po.merged_text(host[b, r, 0], host[b, r, 1])
ms = timed(fmt)
res["format_bytes"] = nbytes
res["format_ms"] = ms
res["format_GBps"] = nbytes / ms / 1e6
gmg.api._ck(lib.gmg_host_unregister(text.ctypes.data_as(C.c_void_p)))

# the host baseline: "%.4f" in CPython on 2 M values, one core
vals = host[:, :, 0].ravel()[:2_000_000]
t0 = time.perf_counter()
s = "\t".join(map("%.4f".__mod__, vals.tolist()))
dt = time.perf_counter() - t0
res["host_fmt_MBps_one_core"] = len(s) / dt / 1e6
res["host_fmt_s_for_the_matrix_one_core"] = nbytes / (len(s) / dt)
print(json.dumps(res))
