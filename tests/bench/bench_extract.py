#!/usr/bin/env python3
"""gmg_reads_extract and the extract | build-icm chain.  Prints one JSON line.

Gather: 1 M synthetic reads of 500 bp resident in HBM, one region of 300 bases per read at a random first base -- forward only,
reverse only, and both strands mixed with a third of the regions wrapping around their read -- against gmg_reads_select of whole
reads that total the same number of output bases (600,000 reads), in the same process.  Both calls are synchronous: wall time
around the call, 3 warm-ups, median of 10; the result batches are freed outside the timed part; the copies of
the region list and of the index list, which both calls start with, are also timed on their own.  A sample of strings is checked
against the Python restatement (tests/extract_oracle.py) first.

Chain: build-icm_gpu -r --list over 16 slices of NC_000915.fna with the NC_000915.longorfs lines that fall into each (extract -t)
against 16 runs of build-icm_dropin -r fed by the training text of the same regions, the way without gmg_reads_extract; the 16
pairs of model files must be identical.  Wall time of both, median of 5 after one warm-up, and the driver's own per-job split
(--timing, GMG_TRAIN_TIMING).

usage: python3 tests/bench/bench_extract.py [n_reads]"""
import ctypes as C
import json
import os
import re
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _gmg_pkg  # noqa: E402
import extract_oracle as xo  # noqa: E402

gmg = _gmg_pkg.load()
n, L, RL = (int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000), 500, 300
gmg.init(0)
lib = gmg.capi.lib()
packed, off = gmg.synth.packed_reads(n, L, 1)
reads = gmg.Reads(packed, off)
rng = np.random.default_rng(8)
REGION = np.dtype([("read", "<u4"), ("first", "<i4"), ("len", "<i4"), ("strand", "<i4")])


def regions(kind):
    r = np.zeros(n, REGION)
    r["read"], r["len"] = np.arange(n), RL
    if kind == "mixed_wrap":
        r["first"] = np.where(np.arange(n) % 3 == 0, rng.integers(L - RL + 1, L, size=n), rng.integers(0, L - RL + 1, size=n))
        r["strand"] = np.where(rng.integers(0, 2, size=n) == 1, 1, -1)
        r["first"] = np.where(r["strand"] < 0, (r["first"] + RL - 1) % L, r["first"])
    elif kind == "forward":
        r["first"], r["strand"] = rng.integers(0, L - RL + 1, size=n), 1
    else:
        r["first"], r["strand"] = rng.integers(RL - 1, L, size=n), -1
    return r


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


out = {"reads": n, "read_len": L, "region_len": RL, "output_bases": n * RL}
for kind in ("forward", "reverse", "mixed_wrap"):
    r = regions(kind)
    sub = gmg.Reads.__new__(gmg.Reads)
    sub.h = C.c_void_p()
    gmg.api._ck(lib.gmg_reads_extract(reads.h, gmg.api._ptr(r), n, 0, None, None, 0, C.byref(sub.h)))
    got_p, got_o = sub.download()
    sub.close()
    for k in rng.choice(n, size=200, replace=False):
        seq = gmg.synth.unpack_ascii(packed, int(k) * L, L)
        seq = seq.decode() if isinstance(seq, bytes) else seq
        want = xo.region_codes([xo.code(ch) for ch in seq], int(r["first"][k]), RL, int(r["strand"][k]))
        b = int(got_o[k])
        idx = np.arange(b, b + RL)
        assert ((got_p[idx >> 4] >> (2 * (idx & 15)).astype(np.uint32)) & 3).tolist() == want, (kind, int(k))
    out["extract_%s_ms" % kind] = timed(lambda ph, r=r: lib.gmg_reads_extract(reads.h, gmg.api._ptr(r), n, 0, None, None, 0, ph))
n_sel = n * RL // L
idx = rng.permutation(n)[:n_sel].astype(np.uint64)
out["select_reads"] = n_sel
out["select_ms"] = timed(lambda ph: lib.gmg_reads_select(reads.h, gmg.api._ptr(idx), n_sel, ph))
# what the two calls send to the device first: 16 bytes per region against 8 bytes per selected read, from pageable memory
for name, nbytes in (("upload_regions_ms", n * 16), ("upload_index_ms", n_sel * 8)):
    host, dev, ms = np.ones(nbytes, np.uint8), gmg.api._DeviceBuffer(nbytes), []
    for k in range(13):
        lib.gmg_synchronize(None)
        t0 = time.perf_counter()
        gmg.api._ck(lib.gmg_memcpy_h2d(dev.ptr, gmg.api._ptr(host), nbytes, None))
        lib.gmg_synchronize(None)
        if k >= 3:
            ms.append(1e3 * (time.perf_counter() - t0))
    out[name] = float(np.median(ms))
    dev.free()
for kind in ("forward", "reverse", "mixed_wrap"):
    out["ratio_%s" % kind] = out["extract_%s_ms" % kind] / out["select_ms"]
out["extract_gbases_per_s"] = n * RL / (out["extract_mixed_wrap_ms"] * 1e6)
reads.close()

# ---- the chain --------------------------------------------------------------------------------------------------------------
gpu_exe = os.path.join(ROOT, "integration", "_build", "build-icm_gpu")
dropin = os.path.join(ROOT, "integration", "_build", "build-icm_dropin")
if os.access(gpu_exe, os.X_OK) and os.access(dropin, os.X_OK):
    data = open(os.path.join(ROOT, "tests", "golden", "data", "NC_000915.fna"), "rb").read()
    genome = xo.records(data)[0][1]
    lines = [ln.split() for ln in open(os.path.join(ROOT, "tests", "golden", "data", "NC_000915.longorfs"))]
    tmp = tempfile.mkdtemp(prefix="bench_extract_")
    S = len(genome) // 16
    jobs = []
    for j in range(16):
        lo = j * S
        sl = genome[lo:lo + S]
        mine = [(f[0], int(f[1]) - lo, int(f[2]) - lo) for f in lines if lo < min(int(f[1]), int(f[2])) and max(int(f[1]), int(f[2])) <= lo + S]
        fa, co, tr = (os.path.join(tmp, "%s%02d" % (p, j)) for p in ("slice", "coords", "train"))
        with open(fa, "w") as fp:
            fp.write(">slice%d\n" % j + "\n".join(sl[i:i + 70] for i in range(0, S, 70)) + "\n")
        with open(co, "w") as fp:
            fp.write("".join("%s %d %d\n" % m for m in mine))
        with open(tr, "w") as fp:                        # what extract -t prints for these lines (all of them shorter than half a slice)
            for tag, s, e in mine:
                n_b = abs(e - s) + 1 - 3
                fp.write(">%s\n%s\n" % (tag, xo.region_chars(sl, s - 1, n_b, 1 if s < e else -1)))
        jobs.append((fa, co, tr, len(mine)))
    with open(os.path.join(tmp, "jobs"), "w") as fp:
        fp.write("".join("-t %s %s %s\n" % (fa, co, os.path.join(tmp, "gpu%02d.icm" % j)) for j, (fa, co, _, _) in enumerate(jobs)))

    def run_list(extra=(), env=None):
        t0 = time.perf_counter()
        res = subprocess.run([gpu_exe, "-r", *extra, "--list", os.path.join(tmp, "jobs")], stderr=subprocess.PIPE, check=True, env=env)
        return 1e3 * (time.perf_counter() - t0), res.stderr.decode()

    def run_dropins():
        t0 = time.perf_counter()
        for j, (_, _, tr, _) in enumerate(jobs):
            with open(tr, "rb") as fp:
                subprocess.run([dropin, "-r", os.path.join(tmp, "dropin%02d.icm" % j)], stdin=fp, check=True)
        return 1e3 * (time.perf_counter() - t0)

    a = [run_list()[0] for _ in range(6)][1:]
    b = [run_dropins() for _ in range(6)][1:]
    for j in range(16):
        assert open(os.path.join(tmp, "gpu%02d.icm" % j), "rb").read() == open(os.path.join(tmp, "dropin%02d.icm" % j), "rb").read(), j
    _, err = run_list(["--timing"], dict(os.environ, GMG_TRAIN_TIMING="1"))
    split = {k: 0.0 for k in ("ingest", "plan", "extract", "train", "write")}
    for k in split:
        split[k] = sum(float(x) for x in re.findall(r"%s ([0-9.]+) ms" % k, err)) / 16
    counts = sum(float(x) for x in re.findall(r"\[gmg_train\] counts +level +\d+ +([0-9.]+) ms", err)) / 16
    nodes = sum(float(x) for x in re.findall(r"\[gmg_train\] (?:nodes|logs) +level +-?\d+ +([0-9.]+) ms", err)) / 16
    out.update({"chain_jobs": 16, "chain_regions": sum(j[3] for j in jobs), "chain_list_ms": float(np.median(a)),
                "chain_dropin_runs_ms": float(np.median(b)), "chain_speedup": float(np.median(b) / np.median(a)),
                "chain_models_identical": True,
                "chain_per_job_ms": dict(split, train_counts=counts, train_host_nodes=nodes)})
print(json.dumps(out))
