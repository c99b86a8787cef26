#!/usr/bin/env python3
"""Generate tests/golden/fixed/* from the REAL reference's build-fixed and score-fixed (src/ICM/build-fixed.cc, score-fixed.cc,
icm.cc).  Runs only in the build container, where the reference's sources are; the tests use the committed fixtures.

The reference objects come from oracle/Makefile's pattern rules (make -C oracle <path of the object>); the two programs are
linked in a temporary directory outside the tree.  The FASTA inputs are rebuilt from tests/golden/data/NC_000915.fna by
tests/fixed_oracle.make_inputs (the tests rebuild them the same way and check their sha256).  What is written under
tests/golden/fixed/ is data only:
  <model>.fix             build-fixed's binary output when under 64 KB (every model's sha256 is in cases.json)
  cases.json              the inputs' sha256; every model (options, shape, bytes, sha256); every score-fixed run (argv, sha256 and
                          line count of stdout, stderr, exit status); build-fixed's error runs (stderr, exit status)

usage: python3 tools/gen_golden_fixed.py        (needs the reference at $GMG_REFERENCE, default /root/reference)
"""
import hashlib
import json
import os
import shutil
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import fixed_oracle  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
REF = os.environ.get("GMG_REFERENCE", "/root/reference")
OBJ = os.path.join(ROOT, "oracle", "_ref", "obj")
GOLD = os.path.join(ROOT, "tests", "golden")
OUT = os.path.join(GOLD, "fixed")
FNA = os.path.join(GOLD, "data", "NC_000915.fna")
NC_ICM = os.path.join(GOLD, "data", "NC_000915.icm")
WHOLE_MAX = 64 << 10

# name, window length, build-fixed options (besides the input), permutation kind
MODELS = [
    ("L1_d3", 1, ["-d", "3"], "none"),
    ("L2_d3_rev", 2, ["-d", "3"], "reversed"),
    ("L12_d3_rand", 12, ["-d", "3"], "random"),
    ("L12_d5_s6", 12, ["-d", "5", "-s", "6"], "none"),
    ("L12_d3_rand_text", 12, ["-d", "3", "-t"], "random"),
    ("L24_d5", 24, ["-d", "5"], "none"),
    ("L24_d7_rand", 24, ["-d", "7"], "random"),
    ("L24_d3_rev", 24, ["-d", "3"], "reversed"),
    ("L32_d7_rev", 32, ["-d", "7"], "reversed"),
    ("L32_d5_rand", 32, ["-d", "5", "-s", "16"], "random"),
]


def perm_of(kind, L, seed):
    if kind == "none":
        return None
    if kind == "reversed":
        return list(range(L - 1, -1, -1))
    return fixed_oracle.Rng(seed).permutation(L)


def build_programs(tmp):
    objs = {n: os.path.join(OBJ, n + ".o") for n in ("build-fixed", "score-fixed", "icm", "delcher", "fasta", "gene", "kelley")}
    subprocess.run(["make", "-C", os.path.join(ROOT, "oracle"), *objs.values()], check=True)
    common = [objs[n] for n in ("icm", "delcher", "fasta", "gene", "kelley")]
    for prog in ("build-fixed", "score-fixed"):
        subprocess.run(["g++", "-o", os.path.join(tmp, prog), objs[prog], *common, "-lm"], check=True)
    return os.path.join(tmp, "build-fixed"), os.path.join(tmp, "score-fixed")


def run(argv, stdin_path):
    with open(stdin_path, "rb") as fp:
        r = subprocess.run(argv, stdin=fp, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    return r.returncode, r.stdout, r.stderr


def main():
    os.makedirs(OUT, exist_ok=True)
    for f in os.listdir(OUT):
        os.remove(os.path.join(OUT, f))
    tmp_in = tempfile.mkdtemp()
    inputs = fixed_oracle.make_inputs(FNA, tmp_in)
    inp_sha = {n: hashlib.sha256(open(p, "rb").read()).hexdigest() for n, p in sorted(inputs.items())}

    with tempfile.TemporaryDirectory() as tmp:
        build_fixed, score_fixed = build_programs(tmp)
        models = []
        for idx, (name, L, opts, kind) in enumerate(MODELS):
            perm = perm_of(kind, L, 1000 + idx)
            argv = [build_fixed, *opts] + (["-p", ",".join(map(str, perm))] if perm else [])
            rc, out, err = run(argv, inputs["train_%d.fa" % L])
            assert rc == 0, (name, err)
            whole = len(out) <= WHOLE_MAX and "-t" not in opts
            path = os.path.join(OUT, name + ".fix")
            if whole:
                open(path, "wb").write(out)
            else:
                open(os.path.join(tmp, name + ".fix"), "wb").write(out)
            depth = int(opts[opts.index("-d") + 1])
            special = int(opts[opts.index("-s") + 1]) if "-s" in opts else -1
            models.append({"name": name, "length": L, "depth": depth, "special": special, "perm": perm, "perm_kind": kind,
                           "opts": opts, "text": "-t" in opts, "train": "train_%d.fa" % L, "whole": whole, "bytes": len(out),
                           "sha256": hashlib.sha256(out).hexdigest()})
            print(name, len(out), "whole" if whole else "sha256")

        def fix(name):
            p = os.path.join(OUT, name + ".fix")
            return p if os.path.exists(p) else os.path.join(tmp, name + ".fix")

        # score-fixed runs: model arguments are names of models (or the NC_000915 ICM for -I)
        RUNS = [
            ("default", [], "L24_d5", "L24_d7_rand", "score.fa"),
            ("simple", ["-s"], "L24_d5", "L24_d7_rand", "score.fa"),
            ("icm_neg", ["-I"], "L24_d5", "NC_000915.icm", "score.fa"),
            ("null_neg", ["-N"], "L24_d3_rev", None, "score.fa"),
            ("L12_pair", [], "L12_d3_rand", "L12_d5_s6", "score.fa"),
            ("L32_pair", [], "L32_d7_rev", "L32_d5_rand", "train_32.fa"),
            ("L32_short", [], "L32_d7_rev", "L32_d5_rand", "score.fa"),
            ("L1_L2", [], "L1_d3", "L2_d3_rev", "score.fa"),
            ("short", [], "L24_d5", "L24_d7_rand", "short.fa"),
            ("short_neg", ["-N"], "L32_d5_rand", None, "short.fa"),
        ]
        runs = []
        for name, opts, pos, neg, inp in RUNS:
            args = opts + [fix(pos)] + ([NC_ICM if neg == "NC_000915.icm" else fix(neg)] if neg else [])
            rc, out, err = run([score_fixed, *args], inputs[inp])
            runs.append({"name": name, "opts": opts, "pos": pos, "neg": neg, "input": inp, "status": rc,
                         "stdout_sha256": hashlib.sha256(out).hexdigest(), "stdout_lines": out.count(b"\n"),
                         "stderr": err.decode()})
            print(name, rc, len(out))
        # build-fixed's own errors: strings of two lengths, depth 0 (refused by its option parser), a duplicate in -p
        errs = []
        for name, opts, inp in [("bad_len", ["-d", "3"], "bad_len.fa"), ("depth0", ["-d", "0"], "train_12.fa"),
                                ("dup_perm", ["-p", "0,1,2,3,4,5,6,7,8,9,10,10"], "train_12.fa")]:
            rc, out, err = run([build_fixed, *opts], inputs[inp])
            errs.append({"name": name, "opts": opts, "input": inp, "status": rc, "stdout_bytes": len(out),
                         "stderr": err.decode().replace(build_fixed, "build-fixed")})
            print(name, rc, err[:60])
    with open(os.path.join(OUT, "cases.json"), "w") as fp:
        # one record per line
        parts = ['"inputs": ' + json.dumps(inp_sha)]
        for key, rows in (("models", models), ("score_runs", runs), ("build_errors", errs)):
            parts.append('"%s": [\n  %s]' % (key, ",\n  ".join(json.dumps(r) for r in rows)))
        fp.write("{" + ",\n".join(parts) + "}\n")
    shutil.rmtree(tmp_in)


if __name__ == "__main__":
    sys.exit(main())
