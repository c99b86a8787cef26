#!/usr/bin/env python3
"""Generate tests/golden/shapes_<name>.npz and the shape entries of tests/golden/train/cases.json from the REAL reference
(oracle/_ref/build-icm and oracle/_ref/ref_dump, built by oracle/Makefile).  Runs only in the build container; the tests use
the committed fixtures.  Test infrastructure only.

Why: the oracle's scorer was pinned to the reference on 12 / 7 models and the (3,2,3) tables only.  Here the reference's
build-icm -w W -d D -p P trains a model of every shape of SHAPES, and the reference's ICM_t scores a fixed read set with it:
Frame_Score in all six frames, Score_String, Partial_Window_Prob, Cumulative_Score_String, Full_Window_Prob / _Distrib.

  periodicity 3: trained (-r, as a gene model is) on the sample run's long-ORF training set NC_000915.train, which the tests
                 rebuild (tests/test_oracle_train.py: long_orf_training_set; "train": null in cases.json)
  periodicity 1: trained on the first eighth of NC_000915.fna cut into strings of 1,000 bases (tests/models64.py: _slices),
                 written here as tests/golden/data/genome_p1_train.fa
  the committed small models of tests/golden/train/ (SMALL) are scored as they are.

The model files are NOT kept (a depth-7 file exceeds 1 MB): cases.json records bytes and sha256, "whole": false.
Read set: tests/golden/data/seqs.fa (999 x 500 bases) and tests/golden/data/short_reads.fa (written here: two reads of
every length 1 .. 40 = 2 x the longest window), so that reads shorter than, equal to and just beyond W - 1 are pinned too.
Values are stored for the first reads of seqs.fa and for every short read, plus a SHA-256 over all reads.

w 4 / d 7 (and w 3 / d 7): the reference's build-icm trains them (the tree simply stops where no context position is left);
w 4 / d 7 is in SHAPES.
"""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
REF = os.environ.get("GMG_REFERENCE", "/root/reference")
RB = os.path.join(HERE, "_ref")
GOLD = os.path.join(ROOT, "tests", "golden")
DATA = os.path.join(GOLD, "data")
TRAIN = os.path.join(GOLD, "train")
WORK = os.path.join(RB, "shapes")

P1_TRAIN = "genome_p1_train.fa"
SHORT = "short_reads.fa"
# name, (W, D, P)
SHAPES = [("s3_w8_d7", (8, 7, 3)), ("s3_w13_d7", (13, 7, 3)), ("s3_w15_d7", (15, 7, 3)), ("s3_w4_d7", (4, 7, 3)),      # the fast class
          ("s3_w16_d7", (16, 7, 3)), ("s3_w12_d8", (12, 8, 3)), ("s3_w12_d9", (12, 9, 3)), ("s3_w20_d5", (20, 5, 3)),
          ("s3_w12_d1", (12, 1, 3)),                                                                                   # the any-shape class
          ("s1_w8_d7", (8, 7, 1)), ("s1_w15_d7", (15, 7, 1)), ("s1_w16_d7", (16, 7, 1))]
SMALL = ["c3_p1_d5_w9", "c3_p2_d3_w6_r", "c4_p4_d2_w3", "c4_d1_w2", "syn_d4"]
N_FRAMES, N_SSTRING, N_PARTIAL, N_PARTIAL_ALL, N_CUMSTR, N_CUMSTR_ALL, N_WINDOWS, SEED = 2, 64, 8, 64, 1, 16, 256, 20260104


def dump(*args):
    return subprocess.run([os.path.join(RB, "ref_dump"), *map(str, args)], check=True, stdout=subprocess.PIPE).stdout


def sha(buf):
    return hashlib.sha256(buf).hexdigest()


def save_npz(path, **arrays):
    """np.savez_compressed with fixed member dates: the same inputs give the same bytes"""
    import io
    import zipfile
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for key, val in arrays.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(val), allow_pickle=False)
            info = zipfile.ZipInfo(key + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue())


def genome():
    g = "".join(line.strip() for line in open(os.path.join(DATA, "NC_000915.fna")) if not line.startswith(">")).lower()
    return "".join(c if c in "acgt" else "c" for c in g)


def write_inputs():
    g = genome()
    span = len(g) // 8
    with open(os.path.join(DATA, P1_TRAIN), "w") as fp:
        for k, i in enumerate(range(0, span - 1000 + 1, 1000)):
            fp.write(">p%d\n%s\n" % (k, g[i:i + 1000]))
    rng = np.random.default_rng(20260104)
    with open(os.path.join(DATA, SHORT), "w") as fp:
        for n in range(1, 41):
            for k in range(2):
                fp.write(">short%d_%d\n%s\n" % (n, k, "".join("acgt"[c] for c in rng.integers(0, 4, size=n))))


def fasta_lengths(path):
    return [len(line.strip()) for line in open(path) if not line.startswith(">")]


def score(icm, W, P):
    """every vector of one model -> dict for np.savez"""
    fa, short = os.path.join(DATA, "seqs.fa"), os.path.join(DATA, SHORT)
    L, n_all = 500, 999
    s_len = fasta_lengths(short)
    out = {"W": W, "P": P, "gc": 0.5, "seed": SEED}
    if P >= 3:                                           # (Frame_Score asserts frame < periodicity; rows 0 .. 5 use frames 0, 1, 2)
        raw = dump("frames", icm, fa, 0, n_all, 0.5)
        out["frames_seqs"] = np.frombuffer(raw[:N_FRAMES * 6 * L * 8], "<f8").reshape(N_FRAMES, 6, L)
        out["frames_seqs_sha256"] = sha(raw)
        out["frames_short"] = np.frombuffer(dump("frames", icm, short, 0, len(s_len), 0.5), "<f8")      # read by read: 6 x len
    raw = dump("sstring", icm, fa)
    out["sstring_seqs"] = np.frombuffer(raw[:N_SSTRING * 24], "<f8").reshape(N_SSTRING, 3)
    out["sstring_seqs_sha256"] = sha(raw)
    out["sstring_short"] = np.frombuffer(dump("sstring", icm, short), "<f8").reshape(len(s_len), 3)
    raw = dump("partial", icm, fa, N_PARTIAL_ALL)
    out["partial_seqs"] = np.frombuffer(raw[:N_PARTIAL * P * (W - 1) * 8], "<f8").reshape(N_PARTIAL, P, W - 1)
    out["partial_seqs_sha256"] = sha(raw)
    out["partial_short"] = np.frombuffer(dump("partial", icm, short, len(s_len)), "<f8")              # read x frame x min (W - 1, len)
    raw = dump("cumstr", icm, fa, N_CUMSTR_ALL)
    out["cumstr_seqs"] = np.frombuffer(raw[:N_CUMSTR * P * (L + 1) * 8], "<f8").reshape(N_CUMSTR, P, L + 1)
    out["cumstr_seqs_sha256"] = sha(raw)
    out["cumstr_short"] = np.frombuffer(dump("cumstr", icm, short, len(s_len)), "<f8")                # reads of >= W - 1 bases: frame x (len + 1)
    rec = W + P * 24
    wins = np.frombuffer(dump("windows", icm, SEED, N_WINDOWS), np.uint8).reshape(N_WINDOWS, rec)
    tail = wins[:, W:].copy().reshape(N_WINDOWS, P, 24)
    out["windows"] = wins[:, :W].copy()
    out["window_prob"] = tail[:, :, :8].copy().view("<f8").reshape(N_WINDOWS, P)
    out["window_dist"] = tail[:, :, 8:].copy().view("<f4").reshape(N_WINDOWS, P, 4)
    return out


def main():
    if not os.path.exists(os.path.join(RB, "ref_dump")) or not os.path.exists(os.path.join(RB, "build-icm")):
        sys.exit("build oracle/_ref first:  make -C oracle ref")
    os.makedirs(WORK, exist_ok=True)
    write_inputs()
    cases = json.load(open(os.path.join(TRAIN, "cases.json")))
    big = os.path.join(REF, "sample-run", "glimmer3", "results", "NC_000915.train")
    for name, (W, D, P) in SHAPES:
        icm = os.path.join(WORK, name + ".icm")
        opts = (["-r"] if P == 3 else []) + ["-w", str(W), "-d", str(D), "-p", str(P)]
        with open(big if P == 3 else os.path.join(DATA, P1_TRAIN), "rb") as fp:
            subprocess.run([os.path.join(RB, "build-icm"), *opts, icm], stdin=fp, check=True)
        data = open(icm, "rb").read()
        entry = {"name": name, "train": None if P == 3 else P1_TRAIN, "opts": opts, "model_len": W, "model_depth": D, "periodicity": P,
                 "reversed": P == 3, "whole": False, "text": False, "bytes": len(data), "sha256": sha(data)}
        if P == 3:
            entry["note"] = "trained on sample-run/glimmer3/results/NC_000915.train, rebuilt by the tests from tests/golden/data/NC_000915.longorfs"
        cases = [c for c in cases if c["name"] != name] + [entry]
        print(name, len(data), entry["sha256"][:16])
    with open(os.path.join(TRAIN, "cases.json"), "w") as fp:
        json.dump(cases, fp, indent=1)
    by_name = {c["name"]: c for c in cases}
    for name in [n for n, _ in SHAPES] + SMALL:
        c = by_name[name]
        icm = os.path.join(TRAIN, name + ".icm") if c["whole"] else os.path.join(WORK, name + ".icm")
        path = os.path.join(GOLD, "shapes_%s.npz" % name)
        save_npz(path, D=c["model_depth"], model_sha256=c["sha256"], **score(icm, c["model_len"], c["periodicity"]))
        assert os.path.getsize(path) < 200_000, (path, os.path.getsize(path))
        print(os.path.basename(path), os.path.getsize(path))


if __name__ == "__main__":
    main()
