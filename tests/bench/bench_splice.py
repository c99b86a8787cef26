#!/usr/bin/env python3
"""gmg_reads_splice against gmg_reads_extract.  Prints one JSON line (kept as profiles/splice_bench.json).

1 M synthetic reads of 500 bp resident in HBM, one gene string of 300 bases per read at a random first base, both strands mixed:
  no edits    one run per string -- the same strings as gmg_reads_extract of the same regions, which is the floor: both calls are
              timed in the same process on the same build, and the two batches must be identical word for word
  two edits   two substitutions inside every gene: five runs per string (copy, substitute, copy, substitute, copy)
Both calls are synchronous: wall time around the call, 3 warm-ups, median of 10; the result batches are freed outside the timed
part.  The copies the calls start with -- 16 bytes per region against 16 bytes per run and 8 per string -- are part of the calls.
A sample of the edited strings is checked against the Python restatement (tests/splice_oracle.py) first.

usage: python3 tests/bench/bench_splice.py [n_reads]"""
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
import extract_oracle as xo  # noqa: E402
import splice_oracle as so  # noqa: E402

gmg = _gmg_pkg.load()
n, L, RL = (int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000), 500, 300
gmg.init(0)
lib = gmg.capi.lib()
packed, off = gmg.synth.packed_reads(n, L, 1)
reads = gmg.Reads(packed, off)
rng = np.random.default_rng(9)
REGION = np.dtype([("read", "<u4"), ("first", "<i4"), ("len", "<i4"), ("strand", "<i4")])

forward = rng.integers(0, 2, size=n) == 1
lo = rng.integers(0, L - RL + 1, size=n)                # the gene covers positions lo .. lo + RL - 1
regions = np.zeros(n, REGION)
regions["read"], regions["len"] = np.arange(n), RL
regions["strand"] = np.where(forward, 1, -1)
regions["first"] = np.where(forward, lo, lo + RL - 1)

# no edits: the region as one run
plain = np.zeros((n, 4), np.uint32)
plain[:, 0], plain[:, 1], plain[:, 2], plain[:, 3] = regions["read"], regions["first"], RL, np.where(forward, so.UP, so.DOWN)
plain_off = np.arange(n + 1, dtype=np.uint64)

# two substitutions at offsets a < b of the string: copy a, substitute 1, copy b - a - 1, substitute 1, copy the rest
a = rng.integers(1, RL // 2 - 1, size=n)
b = rng.integers(RL // 2 + 1, RL - 1, size=n)
cut = np.stack([np.zeros(n, np.int64), a, a + 1, b, b + 1, np.full(n, RL)], 1)      # run q covers offsets cut[q] .. cut[q + 1] - 1
edited = np.zeros((n, 5, 4), np.uint32)
for q in range(5):
    edited[:, q, 0] = regions["read"]
    edited[:, q, 1] = np.where(forward, lo + cut[:, q], lo + RL - 1 - cut[:, q])
    edited[:, q, 2] = cut[:, q + 1] - cut[:, q]
    edited[:, q, 3] = np.where(forward, so.UP, so.DOWN) + (2 if q % 2 else 0)
edited = np.ascontiguousarray(edited.reshape(-1, 4))
edited_off = 5 * np.arange(n + 1, dtype=np.uint64)


def timed(call):
    ms = []
    for k in range(13):
        h = C.c_void_p()
        lib.gmg_synchronize(None)
        t0 = time.perf_counter()
        gmg.api._ck(call(C.byref(h)))
        t1 = time.perf_counter()
        lib.gmg_reads_free(h)
        if k >= 3:
            ms.append(1e3 * (t1 - t0))
    return float(np.median(ms))


def extract(ph):
    return lib.gmg_reads_extract(reads.h, gmg.api._ptr(regions), n, 0, None, None, 0, ph)


def splice(runs, sro):
    return lambda ph: lib.gmg_reads_splice(reads.h, gmg.api._ptr(runs), len(runs), gmg.api._ptr(sro), n, 0, ph)


# the two ways to the unedited strings agree; a sample of the edited ones against the restatement
mine, theirs = reads.splice(plain, plain_off), gmg.Reads.__new__(gmg.Reads)
theirs.h = C.c_void_p()
gmg.api._ck(extract(C.byref(theirs.h)))
got_p, got_o = mine.download()
want_p, want_o = theirs.download()
assert np.array_equal(got_p, want_p) and np.array_equal(got_o, want_o)
mine.close()
theirs.close()
sub = reads.splice(edited, edited_off)
got_p, got_o = sub.download()
sub.close()
for k in rng.choice(n, size=200, replace=False):
    seq = gmg.synth.unpack_ascii(packed, int(k) * L, L)
    seq = seq.decode() if isinstance(seq, bytes) else seq
    codes = {int(k): [xo.code(ch) for ch in seq]}
    want = so.spliced(codes, edited[5 * k:5 * k + 5], [0, 5])[0]
    idx = np.arange(int(got_o[k]), int(got_o[k]) + RL)
    assert ((got_p[idx >> 4] >> (2 * (idx & 15)).astype(np.uint32)) & 3).tolist() == want, int(k)

out = {"reads": n, "read_len": L, "string_len": RL, "output_bases": n * RL}
out["extract_ms"] = timed(extract)
out["splice_no_edits_ms"] = timed(splice(plain, plain_off))
out["splice_no_edits_runs"] = int(len(plain))
out["splice_two_edits_ms"] = timed(splice(edited, edited_off))
out["splice_two_edits_runs"] = int(len(edited))
out["ratio_no_edits"] = out["splice_no_edits_ms"] / out["extract_ms"]
out["ratio_two_edits"] = out["splice_two_edits_ms"] / out["extract_ms"]
reads.close()
print(json.dumps(out))
