#!/usr/bin/env python3
"""gmg_regions_text: regions of reads as FASTA text, written on the device.  Prints one JSON line and writes it to
profiles/text_bench.json.

Input: 1 M synthetic reads of 500 bp resident in HBM (the packed batch and its letters), one region of 300 bases per read with a
head ">r<k>  <first> <end>  len=300\n", width 60: about 330 MB of text.  Three legs, each on its own: forward only, reverse only,
and both strands mixed with a third of the regions wrapping around their read.  Per leg:
  kernel_ms   k_regions_text alone: gmg_regions_text_device, the time between the two events the library records around the
              kernel (gmg_letters_kernel_ms), 3 warm-ups, median of 10 calls
  device_ms   the whole gmg_regions_text_device call (wall time: the host's offsets, the uploads of the records and heads, the kernel)
  full_ms     the whole gmg_regions_text call into page-locked host memory (wall time)
Yardsticks, in the same process and on the same regions:
  extract_ms  gmg_reads_extract (the same gather at 2 bits per base; wall time, as tests/bench/bench_extract.py takes it)
  parent_ms   the way to the same text without this call: gmg_reads_extract + gmg_reads_download + a host loop that turns the
              codes into letters and lines (as integration/extract-aa_gpu.cc does; here numpy, vectorised over all records --
              the reads are all a c g t, so no letter needs patching back in).  Median of 3.
A sample of records of every leg is compared with the Python restatement (tests/text_oracle.py) byte for byte, and the parent's
text with the device's text as a whole.

usage: python3 tests/bench/bench_text.py [n_reads]"""
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
import torch  # noqa: E402
import extract_oracle as xo  # noqa: E402
import text_oracle as to  # noqa: E402

gmg = _gmg_pkg.load()
n, L, RL, W = (int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000), 500, 300, 60
gmg.init(0)
lib = gmg.capi.lib()
packed, off = gmg.synth.packed_reads(n, L, 1)
reads = gmg.Reads(packed, off)
rng = np.random.default_rng(8)
REGION = np.dtype([("read", "<u4"), ("first", "<i4"), ("len", "<i4"), ("strand", "<i4")])
SHIFTS = (2 * np.arange(16)).astype(np.uint32)
ACGT = np.frombuffer(b"acgt", np.uint8)


def codes_of(words, n_bases):
    """2-bit codes of a packed batch as uint8, a million words at a time"""
    out = np.empty(len(words) * 16, np.uint8)
    for lo in range(0, len(words), 1 << 20):
        w = words[lo:lo + (1 << 20)]
        out[lo * 16:(lo + len(w)) * 16] = ((w[:, None] >> SHIFTS[None, :]) & 3).astype(np.uint8).reshape(-1)
    return out[:n_bases]


all_letters = ACGT[codes_of(np.asarray(packed, np.uint32), n * L)]
letters = gmg.Letters(all_letters.tobytes(), off)
prm = gmg.text_params(W)


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


def heads_of(r):
    hs = [b">r%d  %d %d  len=%d\n" % (k, f + 1, (f + s * (RL - 1)) % L + 1, RL) for k, (f, s) in enumerate(zip(r["first"].tolist(), r["strand"].tolist()))]
    ho = np.zeros(n + 1, np.uint64)
    ho[1:] = np.cumsum([len(h) for h in hs], dtype=np.uint64)
    return b"".join(hs), ho


def median_of(call, repeats=13, warm=3, after=lambda x: x):
    """(median wall time in ms of the calls behind the warm-ups, what after() made of their results, outside the timed part)"""
    ms = []
    for k in range(repeats):
        lib.gmg_synchronize(None)
        t0 = time.perf_counter()
        extra = call()
        t1 = time.perf_counter()
        extra = after(extra)
        if k >= warm:
            ms.append((1e3 * (t1 - t0), extra))
    return float(np.median([m[0] for m in ms])), [m[1] for m in ms]


def parent_text(r, blob, ho):
    """gmg_reads_extract + gmg_reads_download + the host's loop over codes"""
    h = C.c_void_p()
    gmg.api._ck(lib.gmg_reads_extract(reads.h, gmg.api._ptr(r), n, 0, None, None, 0, C.byref(h)))
    words = np.zeros(int(lib.gmg_packed_words(n * RL)), np.uint32)
    new_off = np.zeros(n + 1, np.uint64)
    gmg.api._ck(lib.gmg_reads_download(h, gmg.api._ptr(words), gmg.api._ptr(new_off)))
    lib.gmg_reads_free(h)
    body = np.full((n, RL // W, W + 1), 10, np.uint8)                    # every line with its newline
    body[:, :, :W] = ACGT[codes_of(words, n * RL)].reshape(n, RL // W, W)
    body = body.reshape(n, -1)
    hlen = np.diff(ho).astype(np.int64)
    text_off = np.concatenate([[0], np.cumsum(hlen + body.shape[1])])
    out = np.empty(int(text_off[-1]), np.uint8)
    heads = np.frombuffer(blob, np.uint8)
    head_dst = np.repeat(text_off[:-1] - ho[:-1].astype(np.int64), hlen) + np.arange(len(heads))
    out[head_dst] = heads
    body_dst = (text_off[:-1] + hlen)[:, None] + np.arange(body.shape[1])[None, :]
    out[body_dst.reshape(-1)] = body.reshape(-1)
    return out


result = {"reads": n, "read_len": L, "region_len": RL, "width": W}
for kind in ("forward", "reverse", "mixed_wrap"):
    r = regions(kind)
    blob, ho = heads_of(r)
    creg = (gmg.capi.GeneRegion * n).from_buffer(r)
    size = letters.text_size(creg, (blob, ho), prm)
    pinned = torch.empty(size, dtype=torch.uint8, pin_memory=True)
    host = pinned.numpy()
    assert letters.regions_text(creg, (blob, ho), prm, out=host) == size
    for k in rng.choice(n, size=200, replace=False):
        k = int(k)
        seq = all_letters[k * L:(k + 1) * L].tobytes().decode()
        want = to.region_record(seq, (0, int(r["first"][k]), RL, int(r["strand"][k])), blob[int(ho[k]):int(ho[k + 1])].decode(), W)
        b = int(ho[k]) + k * (RL + RL // W)
        assert host[b:b + len(want)].tobytes() == want.encode(), (kind, k)
    dev_ms, kern = median_of(lambda: (letters.regions_text_device(creg, (blob, ho), prm), letters.kernel_ms())[1])
    full_ms, _ = median_of(lambda: letters.regions_text(creg, (blob, ho), prm, out=host))

    def extract_only():
        h = C.c_void_p()
        gmg.api._ck(lib.gmg_reads_extract(reads.h, gmg.api._ptr(r), n, 0, None, None, 0, C.byref(h)))
        return h

    ext_ms, _ = median_of(extract_only, after=lib.gmg_reads_free)       # (freed outside the timed part, as bench_extract.py does)
    par_ms, same = median_of(lambda: parent_text(r, blob, ho), repeats=4, warm=1, after=lambda t: bool(np.array_equal(t, host)))
    assert all(same), kind
    kernel_ms = float(np.median(kern))
    result[kind] = {"text_bytes": size, "kernel_ms": kernel_ms, "device_ms": dev_ms, "full_ms": full_ms, "extract_ms": ext_ms,
                    "parent_ms": par_ms, "kernel_gb_per_s": size / (kernel_ms * 1e6), "kernel_over_extract": kernel_ms / ext_ms,
                    "device_over_extract": dev_ms / ext_ms, "parent_over_full": par_ms / full_ms}
letters.close()
reads.close()
line = json.dumps(result)
os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
with open(os.path.join(ROOT, "profiles", "text_bench.json"), "w") as fp:
    fp.write(line + "\n")
print(line)
