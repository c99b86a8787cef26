#!/usr/bin/env python3
"""Fixed-length ICMs (score-fixed's workload): gmg_fixed_score on 1 M windows of 24 bases under a depth-5 and a depth-7 model of
length 24 (no permutation / a random one), trained with build-fixed's defaults on 20,000 windows of NC_000915.  Windows are
FORWARD segments of one resident read (16 B each).  Prints one JSON line: windows per second, timed with HIP events over warmed
calls (median of 20), and the CPU oracle's rate
(tests/fixed_oracle.py, numpy over a sample of 20,000 windows, one core).  Every timed result is checked against the oracle first.

usage: python3 tests/bench/bench_fixed.py [n_windows]"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _gmg_pkg  # noqa: E402
import fixed_oracle as fo  # noqa: E402
import oracle_py  # noqa: E402
import torch  # noqa: E402

gmg = _gmg_pkg.load()
n = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000
L = 24
gmg.init(0)
orc = oracle_py.load()
fna = os.path.join(ROOT, "tests", "golden", "data", "NC_000915.fna")
genome = b"".join(line.strip() for line in open(fna, "rb") if not line.startswith(b">"))
rng = np.random.default_rng(24)
train = [genome[s:s + L] for s in rng.integers(0, len(genome) - L, 20_000)]
models = {"d5": (5, None), "d7": (7, [int(x) for x in rng.permutation(L)])}

starts = rng.integers(0, len(genome) - L, n)
text = np.frombuffer(genome, np.uint8)[starts[:, None] + np.arange(L)]        # n windows back to back
reads = gmg.Reads.from_strings([text.tobytes()])
rows = np.zeros((n, 4), np.uint32)
rows[:, 1] = np.arange(n, dtype=np.uint32) * L
rows[:, 2] = L
segs = gmg.Segments(reads, rows)
out = gmg.api._DeviceBuffer(n * 8)
res = {"windows": n, "length": L}
check = fo.codes(text[:20_000])

for name, (depth, perm) in models.items():
    m = gmg.FixedIcm.train(train, depth, -1, perm)
    subs = fo.train(orc, train, L, depth, perm)
    p = perm if perm is not None else list(range(L))
    want = fo.score(subs, p, check)
    tb = gmg.api.C.c_uint64()
    gmg.api._ck(gmg.capi.lib().gmg_fixed_model_info(m.device(), None, None, gmg.api.C.byref(tb)))
    res["%s_table_bytes" % name] = tb.value
    gmg.fixed_score(m, reads, segs, d_out=out.ptr.value)
    got = out.to_host(np.float64, n)[:20_000]
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64)), name
    for _ in range(3):
        gmg.fixed_score(m, reads, segs, d_out=out.ptr.value)
    torch.cuda.synchronize()
    ms = []
    for _ in range(20):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        gmg.fixed_score(m, reads, segs, d_out=out.ptr.value)
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    t = float(np.median(ms))
    res["%s_ms" % name] = t
    res["%s_windows_per_s" % name] = n / (t * 1e-3)
    # the CPU oracle (numpy, vectorised over a sample of windows; one core)
    sample = 20_000
    t0 = time.perf_counter()
    fo.score(subs, p, check[:sample])
    res["%s_cpu_oracle_numpy_windows_per_s" % name] = sample / (time.perf_counter() - t0)
print(json.dumps(res))
