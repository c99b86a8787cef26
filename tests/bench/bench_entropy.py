#!/usr/bin/env python3
"""The entropy distance ratio of every ORF of a batch of reads: 1 M synthetic reads of 500 bp -> gmg_find_orfs (minimum gene length
90, truncated ORFs allowed) -> gmg_entropy_orfs on the result as it sits in HBM.  Prints one JSON line: ms per call (HIP events, 3
warm-ups, median of 10 calls) with both outputs, with the counts alone and with the distances alone, codons per second, and the
share of a call that the finish (log, the in-order sums, sqrt) adds to the counting steps.  A sample of the ORFs is checked against
the Python restatement first (tests/entropy_oracle.py: counts exact, distances within 1e-13); the largest distance difference over
the sample is reported.

usage: python3 tests/bench/bench_entropy.py [n_reads]"""
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _gmg_pkg  # noqa: E402
import entropy_oracle as eo  # noqa: E402
import torch  # noqa: E402

gmg = _gmg_pkg.load()
n, L = (int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000), 500
gmg.init(0)
lib = gmg.capi.lib()
packed, off = gmg.synth.packed_reads(n, L, 1)
reads = gmg.Reads(packed, off)
res = gmg.OrfResult(reads, min_gene_len=90, allow_truncated=True)
orfs, _ = res.fetch()
n_orfs = res.n_orfs
codons = int(np.sum(np.maximum(orfs["gene_len"], 0) // 3))
aa = gmg.xlate_table(11)
pos, neg = gmg.entropy_default_profiles()
d_counts, d_dist = gmg.api._DeviceBuffer(n_orfs * 80), gmg.api._DeviceBuffer(n_orfs * 24)


def call(counts, dist):
    gmg.api._ck(lib.gmg_entropy_orfs(reads.h, res.h, aa, gmg.api._ptr(pos), gmg.api._ptr(neg), d_counts.ptr if counts else None,
                                     d_dist.ptr if dist else None, None))


# a sample against the restatement
call(True, True)
torch.cuda.synchronize()
sample = np.random.default_rng(3).choice(n_orfs, size=min(2000, n_orfs), replace=False)
got_c, got_d = d_counts.to_host(np.int32, n_orfs * 20).reshape(-1, 20)[sample], d_dist.to_host(np.float64, n_orfs * 3).reshape(-1, 3)[sample]
table = aa.decode()
want_c = []
for o in orfs[sample]:
    seq = gmg.synth.unpack_ascii(packed, int(o["read"]) * L, L)
    seq = seq.decode() if isinstance(seq, bytes) else seq
    want_c.append(eo.counts(seq, *eo.orf_region(int(o["stop_position"]), int(o["gene_len"]), int(o["frame"]), L), table))
want_c = np.array(want_c, np.int32)
assert np.array_equal(got_c, want_c), "counts differ from the restatement"
host = eo.finish_rows(want_c)
assert np.array_equal(np.isnan(got_d), np.isnan(host))
ok = ~np.isnan(host[:, 0])
worst = float(np.max(np.abs(got_d[ok, :2] - host[ok, :2])))
assert worst <= 1e-13, worst

out = {"reads": n, "read_len": L, "orfs": n_orfs, "codons": codons, "sample_checked": int(len(sample)),
       "sample_max_abs_distance_diff": worst}
for name, (c, d) in {"both": (True, True), "counts_only": (True, False), "dist_only": (False, True)}.items():
    for _ in range(3):
        call(c, d)
    torch.cuda.synchronize()
    ms = []
    for _ in range(10):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        call(c, d)
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    out["%s_ms" % name] = float(np.median(ms))
out["codons_per_s"] = codons / (out["both_ms"] * 1e-3)
out["orfs_per_s"] = n_orfs / (out["both_ms"] * 1e-3)
out["finish_share_of_call"] = max(0.0, 1.0 - out["counts_only_ms"] / out["both_ms"])
print(json.dumps(out))
