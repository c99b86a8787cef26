#!/usr/bin/env python3
"""gmg_runs_text: the strings of a plan of runs, or their translations, as text written on the device.  Prints one JSON line and
writes it to profiles/runs_text_bench.json.

Input: tests/bench/bench_splice.py's two workloads on 1 M synthetic reads of 500 bp (upper-case A C G T, resident in HBM as letters
and as a packed batch): one gene string of 300 bases per read, both strands mixed,
  no_edits    one run per string (1 M runs)
  two_edits   two substitutions inside every gene: five runs per string (5 M runs)
each as DNA (301 bytes per record behind its head) and as protein (101 bytes), heads ">r<k>_<first>,<end>_<strand>\n", width 0 as
extract-aa_gpu writes its files.  Per leg, 3 warm-ups and 10 calls; every figure is the median with (min, max) beside it:
  kernel_ms   k_runs_text alone: the time between the two events the library records around the kernel (gmg_letters_kernel_ms)
  device_ms   the whole gmg_runs_text_device call (wall time: the host's pass over the runs, the uploads, the kernel)
  full_ms     the whole gmg_runs_text call into page-locked host memory (wall time)
Yardsticks, in the same process:
  parent_ms   (a) the way to the same text without this call, as extract-aa_gpu went: gmg_reads_splice + gmg_reads_download + a
              host expansion of the codes into letters and records (numpy, vectorised over all records; the reads are all upper-case
              A C G T, so no letter needs patching back in), plus the translation on the host in protein mode.  Median of 3.
  regions     (b) gmg_regions_text of the same regions with the same heads and width, for the no_edits DNA leg: the two texts must
              be equal, and the ratio of the two kernels is reported.
A sample of 200 records of every leg is compared with the Python restatement (tests/runs_text_oracle.py) byte for byte, and the
parent's text with the device's text as a whole.

usage: python3 tests/bench/bench_runs_text.py [n_reads]"""
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
import runs_text_oracle as ro  # noqa: E402
import splice_oracle as so  # noqa: E402

gmg = _gmg_pkg.load()
n, L, RL = (int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000), 500, 300
gmg.init(0)
lib = gmg.capi.lib()
packed, off = gmg.synth.packed_reads(n, L, 1)
reads = gmg.Reads(packed, off)
rng = np.random.default_rng(9)
REGION = np.dtype([("read", "<u4"), ("first", "<i4"), ("len", "<i4"), ("strand", "<i4")])
SHIFTS = (2 * np.arange(16)).astype(np.uint32)
ACGT = np.frombuffer(b"ACGT", np.uint8)


def codes_of(words, n_bases):
    """2-bit codes of a packed batch as uint8, a million words at a time"""
    out = np.empty(len(words) * 16, np.uint8)
    for lo in range(0, len(words), 1 << 20):
        w = words[lo:lo + (1 << 20)]
        out[lo * 16:(lo + len(w)) * 16] = ((w[:, None] >> SHIFTS[None, :]) & 3).astype(np.uint8).reshape(-1)
    return out[:n_bases]


all_letters = ACGT[codes_of(np.asarray(packed, np.uint32), n * L)]
letters = gmg.Letters(all_letters.tobytes(), off)

# ---- bench_splice.py's workloads
forward = rng.integers(0, 2, size=n) == 1
lo = rng.integers(0, L - RL + 1, size=n)                # the gene covers positions lo .. lo + RL - 1
regions = np.zeros(n, REGION)
regions["read"], regions["len"] = np.arange(n), RL
regions["strand"] = np.where(forward, 1, -1)
regions["first"] = np.where(forward, lo, lo + RL - 1)
plain = np.zeros((n, 4), np.uint32)
plain[:, 0], plain[:, 1], plain[:, 2], plain[:, 3] = regions["read"], regions["first"], RL, np.where(forward, so.UP, so.DOWN)
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
WORKLOADS = {"no_edits": (plain, np.arange(n + 1, dtype=np.uint64)), "two_edits": (edited, 5 * np.arange(n + 1, dtype=np.uint64))}

head_list = [b">r%d_%d,%d_%s\n" % (k, p, p + RL, b"+" if f else b"-") for k, (p, f) in enumerate(zip(lo.tolist(), forward.tolist()))]
ho = np.zeros(n + 1, np.uint64)
ho[1:] = np.cumsum([len(h) for h in head_list], dtype=np.uint64)
blob = b"".join(head_list)
del head_list


def spread(ms):
    return {"median": float(np.median(ms)), "min": float(np.min(ms)), "max": float(np.max(ms))}


def timed(call, repeats=13, warm=3, after=lambda x: x):
    """(wall times in ms of the calls behind the warm-ups, what after() made of their results outside the timed part)"""
    ms, extra = [], []
    for k in range(repeats):
        lib.gmg_synchronize(None)
        t0 = time.perf_counter()
        x = call()
        t1 = time.perf_counter()
        x = after(x)
        if k >= warm:
            ms.append(1e3 * (t1 - t0))
            extra.append(x)
    return ms, extra


def records_text(body):
    """the text of n records: head k, then row k of body (with its newline)"""
    hlen = np.diff(ho).astype(np.int64)
    text_off = np.concatenate([[0], np.cumsum(hlen + body.shape[1])])
    out = np.empty(int(text_off[-1]), np.uint8)
    heads = np.frombuffer(blob, np.uint8)
    out[np.repeat(text_off[:-1] - ho[:-1].astype(np.int64), hlen) + np.arange(len(heads))] = heads
    out[((text_off[:-1] + hlen)[:, None] + np.arange(body.shape[1])[None, :]).reshape(-1)] = body.reshape(-1)
    return out


def parent_text(runs, sro, mode, aa):
    """gmg_reads_splice + gmg_reads_download + the host's pass over the codes (and its translation)"""
    h = C.c_void_p()
    gmg.api._ck(lib.gmg_reads_splice(reads.h, gmg.api._ptr(runs), len(runs), gmg.api._ptr(sro), n, 0, C.byref(h)))
    words = np.zeros(int(lib.gmg_packed_words(n * RL)), np.uint32)
    new_off = np.zeros(n + 1, np.uint64)
    gmg.api._ck(lib.gmg_reads_download(h, gmg.api._ptr(words), gmg.api._ptr(new_off)))
    lib.gmg_reads_free(h)
    codes = codes_of(words, n * RL).reshape(n, RL)
    if mode == ro.PROTEIN:
        c = codes.reshape(n, RL // 3, 3).astype(np.int64)
        chars = aa[16 * c[:, :, 0] + 4 * c[:, :, 1] + c[:, :, 2]]
    else:
        chars = ACGT[codes]
    body = np.full((n, chars.shape[1] + 1), 10, np.uint8)
    body[:, :-1] = chars
    return records_text(body)


result = {"reads": n, "read_len": L, "string_len": RL, "width": 0, "calls": 10, "warm_ups": 3}
for work, (runs, sro) in WORKLOADS.items():
    for mode, mode_name in ((ro.DNA, "dna"), (ro.PROTEIN, "protein")):
        prm = gmg.runs_text_params(mode, 0)
        size = letters.runs_text_size(runs, sro, (blob, ho), prm)
        nchar = RL // 3 if mode == ro.PROTEIN else RL
        assert size == len(blob) + n * (nchar + 1)
        pinned = torch.empty(size, dtype=torch.uint8, pin_memory=True)
        host = pinned.numpy()
        assert letters.runs_text(runs, sro, (blob, ho), prm, out=host) == size
        per = len(runs) // n
        want_prm = ro.Params(mode)
        for k in rng.choice(n, size=min(200, n), replace=False):
            k = int(k)
            head = blob[int(ho[k]):int(ho[k + 1])]
            seqs = {k: all_letters[k * L:(k + 1) * L].tobytes()}
            want = ro.text(seqs, runs[per * k:per * k + per], [0, per], [head], want_prm)
            at = int(ho[k]) + k * (nchar + 1)
            assert host[at:at + len(want)].tobytes() == want, (work, mode_name, k)
        dev_ms, kern = timed(lambda: (letters.runs_text_device(runs, sro, (blob, ho), prm), letters.kernel_ms())[1])
        full_ms, _ = timed(lambda: letters.runs_text(runs, sro, (blob, ho), prm, out=host))
        aa = np.frombuffer(prm.aa, np.uint8)
        par_ms, same = timed(lambda: parent_text(runs, sro, mode, aa), repeats=4, warm=1, after=lambda t: bool(np.array_equal(t, host)))
        assert all(same), (work, mode_name)
        leg = {"runs": int(len(runs)), "text_bytes": size, "kernel_ms": spread(kern), "device_ms": spread(dev_ms), "full_ms": spread(full_ms),
               "parent_ms": spread(par_ms)}
        leg["kernel_gb_per_s"] = size / (leg["kernel_ms"]["median"] * 1e6)
        leg["parent_over_full"] = leg["parent_ms"]["median"] / leg["full_ms"]["median"]
        leg["parent_over_device"] = leg["parent_ms"]["median"] / leg["device_ms"]["median"]
        if work == "no_edits" and mode == ro.DNA:
            # (b) the same text from gmg_regions_text: upper-case A C G T, so the reference's Complement is the script's rc()
            tprm = gmg.text_params(0)
            creg = (gmg.capi.GeneRegion * n).from_buffer(regions)
            theirs = np.empty(size, np.uint8)
            assert letters.regions_text(creg, (blob, ho), tprm, out=theirs) == size and np.array_equal(theirs, host)
            del theirs
            # alternating, so that both kernels meet the same state of the machine
            kr, kt = [], []
            for k in range(13):
                letters.regions_text_device(creg, (blob, ho), tprm)
                x = letters.kernel_ms()
                letters.runs_text_device(runs, sro, (blob, ho), prm)
                y = letters.kernel_ms()
                if k >= 3:
                    kr.append(x)
                    kt.append(y)
            rdev_ms, _ = timed(lambda: letters.regions_text_device(creg, (blob, ho), tprm))
            leg["regions"] = {"kernel_ms": spread(kr), "runs_kernel_ms_alternating": spread(kt), "device_ms": spread(rdev_ms),
                              "kernel_ratio": float(np.median(kt) / np.median(kr)),
                              "device_ratio": leg["device_ms"]["median"] / float(np.median(rdev_ms))}
        result[work + "_" + mode_name] = leg
        del pinned, host
letters.close()
reads.close()
line = json.dumps(result)
os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
with open(os.path.join(ROOT, "profiles", "runs_text_bench.json"), "w") as fp:
    fp.write(line + "\n")
print(line)
