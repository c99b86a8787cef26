#!/usr/bin/env python3
"""gmg_genes_audit on 1 M synthetic reads of 500 bp, resident on the device.
  A  one 300-base region per read (first = 7 * read mod 200, strands alternating)
  B  the ORFs gmg_mg_score_reads accepts on that batch as regions (Entropy_Filter's rule, as bench_features.py takes them as genes)
Per workload one JSON block: ms per call (3 warm-ups, median of 10, wall clock around the call up to the end of the device work,
nothing copied back), regions/s, codons/s (len / 3 per region: what the count pass visits at least; most of B's genes end in a stop
codon, so no next-stop walk; A's mostly do not, and the codons of their walks are not counted), the inner stops found, and in the same
process gmg_entropy_regions (counts only) on the same regions: the existing call with the same access pattern.  Both calls upload the
region list (16 bytes per region from pageable memory) inside the timed window.  The Python restatement (tests/audit_oracle.py,
one core) runs on the regions of the first 2,000 reads, is compared with the device record by record, and is scaled by regions.

usage: python3 tests/bench/bench_audit.py [n_reads]"""
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
import audit_oracle as ao  # noqa: E402

gmg = _gmg_pkg.load()
n, L = (int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000), 500
gmg.init(0)
lib = gmg.capi.lib()
packed, off = gmg.synth.packed_reads(n, L, 1)
reads = gmg.Reads(packed, off)

r = np.arange(n, dtype=np.int64)
reg_a = np.stack([r, (7 * r) % 200 + np.where(r & 1, 299, 0), np.full(n, 300), np.where(r & 1, -1, 1)], 1).astype(np.int32)

gene_icm = gmg.Icm.open(os.path.join(ROOT, "tests", "golden", "data", "NC_000915.icm"))
orfs, _, _ = gmg.mg_score_reads(gene_icm, gmg.Icm.indep(0.5), reads, accepted_only=True)
lib.gmg_trim_cache()
fwd = orfs["frame"] > 0
glen = np.maximum(orfs["gene_len"].astype(np.int64), 0) + 3                       # the gene with its stop codon
s1 = np.where(fwd, orfs["stop_position"].astype(np.int64) - orfs["gene_len"], orfs["stop_position"].astype(np.int64) + orfs["gene_len"] + 2)
keep = (glen <= L) & (s1 >= 1) & (s1 <= L)                                        # (ORFs truncated by the read's end stay out)
reg_b = np.stack([orfs["read"].astype(np.int64), s1 - 1, glen, np.where(fwd, 1, -1)], 1)[keep].astype(np.int32)

aa = gmg.xlate_table(11)
pos, neg = gmg.entropy_default_profiles()
prm = gmg.audit_params()


def audit_call(arr):
    h = C.c_void_p()
    gmg.api._ck(lib.gmg_genes_audit(reads.h, gmg.api._ptr(arr), len(arr), C.byref(prm), None, 0, C.byref(h), None))
    gmg.api._ck(lib.gmg_synchronize(None))
    ni = C.c_uint64()
    gmg.api._ck(lib.gmg_audit_info(h, None, C.byref(ni)))
    lib.gmg_audit_free(h)
    return ni.value


def timed(fn):
    for _ in range(3):
        fn()
    t = []
    for _ in range(10):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(t)), float(min(t)), float(max(t))


def workload(name, arr):
    arr = np.ascontiguousarray(arr)
    counts = gmg.api._DeviceBuffer(len(arr) * 80)

    def entropy_call():
        gmg.api._ck(lib.gmg_entropy_regions(reads.h, gmg.api._ptr(arr), len(arr), aa, gmg.api._ptr(pos), gmg.api._ptr(neg), counts.ptr, None, None))
        gmg.api._ck(lib.gmg_synchronize(None))

    n_inner = audit_call(arr)
    a_ms, a_min, a_max = timed(lambda: audit_call(arr))
    e_ms, e_min, e_max = timed(entropy_call)
    counts.free()
    codons = int((arr[:, 2] // 3).sum())
    # the restatement on the regions of the first 2,000 reads, and the device on the same ones
    m = min(2000, n)
    sub = arr[arr[:, 0] < m]
    letters = [gmg.synth.unpack_ascii(packed, k * L, L).decode() for k in range(m)]
    t0 = time.perf_counter()
    want, want_inner, want_hist = ao.audit_records(letters, [tuple(int(x) for x in row) for row in sub])
    oracle_s = time.perf_counter() - t0
    rec, inner, hist = gmg.genes_audit(reads, sub)
    same = all([int(x) for x in rec[f]] == [w[f] for w in want] for f in rec.dtype.names) and \
        [int(x) for x in inner] == want_inner and [int(x) for x in hist] == want_hist
    assert same, "the sample differs from the restatement"
    return {"workload": name, "regions": int(len(arr)), "codons": codons, "inner_stops": int(n_inner),
            "sample_fraction_ending_in_a_stop_codon": float((rec["stop_which"] >= 0).mean()) if len(rec) else 0.0,
            "genes_audit_ms": a_ms, "genes_audit_ms_min_max": [a_min, a_max], "regions_per_s": len(arr) / (a_ms * 1e-3),
            "codons_per_s": codons / (a_ms * 1e-3), "entropy_regions_counts_ms": e_ms, "entropy_regions_ms_min_max": [e_min, e_max],
            "ratio_to_entropy_regions": a_ms / e_ms,
            "restatement_python3_one_core": {"sample_regions": int(len(sub)), "sample_s": oracle_s,
                                             "scaled_to_batch_s": oracle_s * len(arr) / max(len(sub), 1), "sample_equals_device": True}}


out = {"reads": n, "read_len": L, "timing": "3 warm-ups, median of 10 calls; host clock around the call and gmg_synchronize; region upload included",
       "A_one_300_base_region_per_read": workload("A", reg_a), "B_accepted_orfs_of_mg_score_reads": workload("B", reg_b)}
print(json.dumps(out))
