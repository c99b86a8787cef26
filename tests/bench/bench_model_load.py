#!/usr/bin/env python3
"""What it costs to get a database of ICMs into HBM: the 64 period-1 models of tests/models64.py (12 / 7 / 1, the shape of a Phymm
database), loaded
  (a) on the host, one model at a time: gmg_icm_open + gmg_icm_device_model (Try_Input, gmg_model_upload) + gmg_icm_free,
  (b) on the device, all at once: the files' bytes through gmg_model_set_load + gmg_model_set_finish (+ gmg_model_set_free),
      timed with the files already in memory and with reading them included ((a) always reads its files: they are in the page cache),
  (c) inside integration/phymm_gpu: wall time of the whole program on synthetic 500 bp reads against those 64 models with the device
      loader (default) and with --host-load, with and without the raw matrix.
Every figure is the median of REPS runs, the variants of one comparison interleaved run by run.  Before anything is timed, every
member of the set is compared with the host path's blob, and the program's two loaders must write the same bytes.
Prints one JSON line; --out FILE also writes it there.

usage: python3 tests/bench/bench_model_load.py [--reads 200000,1000000] [--reps 5] [--out FILE] [--no-cli]"""
import argparse
import json
import os
import subprocess
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

ap = argparse.ArgumentParser()
ap.add_argument("--reads", default="200000,1000000")
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--out")
ap.add_argument("--no-cli", action="store_true")
args = ap.parse_args()
REPS, B, L = args.reps, 64, 500

gmg = _gmg_pkg.load()
gmg.init(0)
res = {"models": B, "shape": [12, 7, 1], "reps": REPS}


def interleaved(variants):
    """{name: f} -> {name: median seconds}; run r takes every variant once, in turn"""
    ts = {k: [] for k in variants}
    for _ in range(REPS):
        for k, f in variants.items():
            t0 = time.perf_counter()
            f()
            ts[k].append(time.perf_counter() - t0)
    return {k: float(np.median(v)) for k, v in ts.items()}, {k: [round(x * 1e3, 3) for x in v] for k, v in ts.items()}


with tempfile.TemporaryDirectory() as tmp:
    made = models64.period1_models(gmg, tmp, B)
    paths = [p for _, p in made]
    data = [open(p, "rb").read() for p in paths]
    res["file_bytes"] = sum(len(d) for d in data)

    # ---- the two paths give the same tables ----
    with gmg.ModelSet.load(data) as ms:
        ms.finish()
        for icm, _ in made:                             # (a model trained here holds more than its file does: what the training left in
            icm.close()                                 # the slots of cut nodes; the reference of the check is the FILE read on the host)
        res["blob_bytes"] = 0
        for k, p in enumerate(paths):
            icm = gmg.Icm.open(p)
            blob = gmg.model_blob(ms.model(k))
            assert blob == gmg.model_blob(icm), p
            assert gmg.model_value_stats(ms.model(k)) == gmg.model_value_stats(icm), p
            res["blob_bytes"] += len(blob)
            icm.close()

    # ---- (a) against (b) ----
    def host_path():
        for p in paths:
            icm = gmg.Icm.open(p)
            icm.device()
            icm.close()

    def device_path(blobs):
        ms = gmg.ModelSet.load(blobs)
        ms.finish()
        ms.close()

    for f in (host_path, lambda: device_path(data)):    # (first calls: allocations the later ones reuse)
        f()
    med, runs = interleaved({"host": host_path, "device": lambda: device_path(data),
                             "device_with_read": lambda: device_path([open(p, "rb").read() for p in paths])})
    res["ms_per_model_host"] = med["host"] * 1e3 / B
    res["ms_per_model_device"] = med["device"] * 1e3 / B
    res["ms_per_model_device_with_file_read"] = med["device_with_read"] * 1e3 / B
    res["load_runs_ms_all_models"] = runs

    # ---- (c) the program ----
    if not args.no_cli:
        exe = po.phymm_binary(os.path.join(tmp, "bin"))
        env = dict(os.environ, LD_LIBRARY_PATH=os.path.join(ROOT, "glimmer-mg_amd", "lib"))
        os.makedirs(os.path.join(tmp, ".genomeData", "db"))
        for k, p in enumerate(paths):
            os.symlink(p, os.path.join(tmp, ".genomeData", "db", "NC_%06d.icm" % k))
        res["phymm_gpu"] = {}
        for n in [int(x) for x in args.reads.split(",") if x]:
            packed, _ = gmg.synth.packed_reads(n, L, 23)
            with open(os.path.join(tmp, "reads.fa"), "wb") as f:        # ">r0000017\n" + 500 bases + "\n" per read, a piece at a time
                for r0 in range(0, n, 20000):
                    cnt = min(20000, n - r0)
                    rec = np.empty((cnt, 10 + L + 1), np.uint8)
                    rec[:, :10] = np.frombuffer(b"".join(b">r%07d\n" % r for r in range(r0, r0 + cnt)), np.uint8).reshape(cnt, 10)
                    rec[:, 10:10 + L] = np.frombuffer(gmg.synth.unpack_ascii(packed, r0 * L, cnt * L), np.uint8).reshape(cnt, L)
                    rec[:, -1] = 10
                    f.write(rec.tobytes())
            del packed

            def run(*opts):
                r = subprocess.run([exe, *opts, "reads.fa"], cwd=tmp, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=900)
                assert r.returncode == 0, r.stderr.decode()[-400:]

            def outputs():
                return open(os.path.join(tmp, "rawPhymmOutput_reads_fa.txt"), "rb").read(), open(os.path.join(tmp, "reads.class.txt"), "rb").read()

            run()                                       # the two loaders write the same bytes (and the page cache is warm)
            want = outputs()
            run("--host-load")
            assert outputs() == want
            del want
            entry = {}
            for label, opts in (("no_matrix", ["--no-matrix"]), ("matrix", [])):
                med, runs = interleaved({"device_load": lambda: run(*opts), "host_load": lambda: run(*opts, "--host-load")})
                entry[label] = {"wall_s_device_load": med["device_load"], "wall_s_host_load": med["host_load"], "runs_ms": runs}
            res["phymm_gpu"][str(n)] = entry

line = json.dumps(res)
print(line)
if args.out:
    with open(args.out, "w") as f:
        f.write(line + "\n")
