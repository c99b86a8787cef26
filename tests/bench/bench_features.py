#!/usr/bin/env python3
"""gmg_features_count (the counting of scripts/train_features.py) on 1 M synthetic reads of 500 bp.  The genes are the ORFs that
gmg_mg_score_reads accepts on that batch (each ORF with its gene_len as one gene line, clipped to its read as parse_predict does).
Prints one JSON line: ms per call (3 warm-ups, median of 10 calls, wall clock around the synchronous call), the device time of
its stages (gmg_features_info: HIP events inside the call and the host's clock around them, median over the same calls), gmg_find_orfs on the same batch as the
nearest existing comparison, and the Python 3 restatement (tests/features_oracle.py, one core -- NOT the reference's Python 2
script) on a 2,000-read sample, scaled to the batch by bases.  The sample is also checked against the device, bit for bit.

usage: python3 tests/bench/bench_features.py [n_reads]"""
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
import features_cases as fc  # noqa: E402
import features_oracle as fo  # noqa: E402

gmg = _gmg_pkg.load()
n, L = (int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000), 500
gmg.init(0)
lib = gmg.capi.lib()
packed, off = gmg.synth.packed_reads(n, L, 1)
reads = gmg.Reads(packed, off)

# ---- the genes: the accepted ORFs, in read order
gene_icm = gmg.Icm.open(os.path.join(ROOT, "tests", "golden", "data", "NC_000915.icm"))
orfs, _, _ = gmg.mg_score_reads(gene_icm, gmg.Icm.indep(0.5), reads, accepted_only=True)
lib.gmg_trim_cache()
fwd = orfs["frame"] > 0
start = np.where(fwd, orfs["stop_position"] - 1 - orfs["gene_len"], orfs["stop_position"] - 1).astype(np.int64)
end = np.where(fwd, orfs["stop_position"] + 2, orfs["stop_position"] + orfs["gene_len"] + 2).astype(np.int64)
GENE = np.dtype([("read", np.uint32), ("strand", np.int32), ("start", np.int32), ("end", np.int32), ("start_codon", np.int32)])
genes = np.zeros(len(orfs), GENE)
genes["read"] = orfs["read"]
genes["strand"] = np.where(fwd, 1, -1)
genes["start"] = np.clip(start, 0, L)
genes["end"] = np.clip(end, 0, L)
genes["start_codon"] = np.where(fwd, start >= 0, end <= L)
assert np.all(np.diff(genes["read"].astype(np.int64)) >= 0)
prm = gmg.capi.FeaturesParams(75, 50, 0, 0)


def call():
    h = C.c_void_p()
    gmg.api._ck(lib.gmg_features_count(reads.h, gmg.api._ptr(genes), len(genes), None, 0, C.byref(prm), C.byref(h), None))
    units, recs = C.c_uint64(), C.c_uint64()
    ms = np.zeros(8, np.float32)
    gmg.api._ck(lib.gmg_features_info(h, C.byref(units), C.byref(recs), gmg.api._ptr(ms)))
    lib.gmg_features_free(h)
    return units.value, recs.value, ms.copy()


for _ in range(3):
    units, recs, _ = call()
wall, stages = [], []
for _ in range(10):
    t0 = time.perf_counter()
    _, _, ms = call()
    wall.append((time.perf_counter() - t0) * 1e3)
    stages.append(ms)
stages = np.median(np.array(stages), axis=0)

# ---- gmg_find_orfs on the same batch
find = []
for k in range(13):
    t0 = time.perf_counter()
    res = gmg.OrfResult(reads, min_gene_len=75, allow_truncated=True)
    lib.gmg_synchronize(None)
    if k >= 3:
        find.append((time.perf_counter() - t0) * 1e3)
    res.close()

# ---- the restatement on a sample: reads [0, 2000) and their genes
m = min(2000, n)
letters = [gmg.synth.unpack_ascii(packed, r * L, L).decode().upper() for r in range(m)]
sub = genes[genes["read"] < m]
seqs = {"r%d" % r: s for r, s in enumerate(letters)}
og = {}
for g in sub:
    gene = fo.Gene(int(g["start"]), int(g["end"]), 0, 0, int(g["strand"]), bool(g["start_codon"]), True)
    og.setdefault("r%d" % g["read"], []).append(gene)
t0 = time.perf_counter()
gs, ns = fo.count(og, seqs)
oracle_s = time.perf_counter() - t0
sample = gmg.Reads.from_strings(letters)
got_g, got_n, _ = gmg.features_count(sample, [tuple(int(x) for x in g) for g in sub], None)
assert fc.same_table(got_g, fc.table_of(gs, 50)) == [] and fc.same_table(got_n, fc.table_of(ns, 50)) == [], "the sample differs from the restatement"

out = {"reads": n, "read_len": L, "genes": int(len(genes)), "genes_are": "ORFs accepted by gmg_mg_score_reads (NC_000915.icm), gene_len as the gene",
       "units_of_32_positions": units, "fraction_records": recs, "features_count_ms": float(np.median(wall)),
       "stage_ms": {"opaque_and_codon_classes": float(stages[0]), "count_pass": float(stages[1]), "scan": float(stages[2]),
                    "write_pass": float(stages[3]), "sorts_and_in_order_sums": float(stages[4])},
       "host_clock_ms": {"extents_read_back_and_gene_list": float(stages[5]), "first_to_last_device_event": float(stages[6]),
                         "histograms_read_back_and_destranding": float(stages[7])},
       "find_orfs_ms": float(np.median(find)), "bases_per_s": n * L / (float(np.median(wall)) * 1e-3),
       "restatement_python3_one_core": {"sample_reads": m, "sample_s": oracle_s, "scaled_to_batch_s": oracle_s * n / m,
                                        "sample_equals_device": True}}
print(json.dumps(out))
