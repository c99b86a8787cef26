"""Models doctored to sit AT the bounds of the three exactness predicates the reordered sums rest on (tests/test_exact_bounds.py,
tests/test_gpu_exact_bounds.py):
  mg_plan (gmg_mg_run.h) and gmg_score_orfs' events path (gmg_orfs.hip):  !odd && clog (R + 2) + max_exp - min_exp <= 28
  gmg_score_reads_strings' fused form (gmg_strings.hip):  min_exp >= 109 && max_exp - min_exp <= 23, and per read
                                                          ilogb |sum| + 2 - (min_exp - 150) <= 53
doctor() rewrites ALL probability floats of a model file: negative, 23 random mantissa bits with the lowest set (so that a value
uses every bit down to 2^(exponent - 150)), the exponent field uniform in [lo, hi] with both ends present."""
import os

import numpy as np

import model_zoo

DATA = os.path.join(model_zoo.GOLD, "data")
GCS = [0.3, 0.36, 0.42, 0.5, 0.55, 0.61, 0.7]            # the null models of the front-half calls, one per read
MG_LONGEST = {"edge": 1000, "past": 1023, "wide": 1000}   # clog (R + 2): 10, 11, 10
STRINGS = {"s109_23": (109, 132), "s108_23": (108, 131), "s109_24": (109, 133), "s108_24": (108, 132)}


def doctor(src, dst, lo, hi, seed):
    raw = bytearray(open(src, "rb").read())
    at = model_zoo.records(raw)
    rng = np.random.default_rng(seed)
    n = 4 * len(at)
    ex = rng.integers(lo, hi + 1, size=n).astype(np.uint32)
    ex[0], ex[1] = lo, hi
    bits = (np.uint32(1) << 31) | (ex << 23) | (rng.integers(0, 1 << 23, size=n).astype(np.uint32) | 1)
    vals = bits.astype("<u4").view("<f4").reshape(-1, 4)
    for o, v in zip(at, vals):
        raw[int(o):int(o) + 16] = v.tobytes()
    open(dst, "wb").write(bytes(raw))


def null_range(oracle, gcs=GCS, stops=("taa", "tag", "tga")):
    """(min_exp, max_exp) over the null models' tables as gmg_null_set_build uploads them"""
    r = [model_zoo.exponent_range(*oracle.tables(oracle.indep(gc, stops))) for gc in gcs]
    assert not any(x[2] for x in r)
    return min(x[0] for x in r), max(x[1] for x in r)


def mg_bounds(oracle, which):
    """exponent fields [lo, hi] of the doctored gene model: with the null models' range and the batch's longest read R,
    clog (R + 2) + max_exp - min_exp is exactly 28 (edge), 29 through clog (past), 29 through the spread (wide)"""
    n_lo, n_hi = null_range(oracle)
    hi = n_hi                                            # the null models' largest exponent occurs in the gene model too
    lo = hi - (28 - model_zoo.clog(MG_LONGEST["edge"])) - (1 if which == "wide" else 0)
    assert lo < n_lo
    return lo, hi


def mg_model(oracle, which, tmp_dir):
    lo, hi = mg_bounds(oracle, which)
    path = os.path.join(str(tmp_dir), "mg_%s.icm" % which)
    doctor(os.path.join(DATA, "NC_000915.icm"), path, lo, hi, 11)
    return path


def mg_reads(which):
    rng = np.random.default_rng(21)
    lens = [int(x) for x in rng.integers(30, 700, size=100)] + [MG_LONGEST[which]]
    return ["".join("acgt"[c] for c in rng.integers(0, 4, size=n)) for n in lens]


def strings_model(name, tmp_dir):
    lo, hi = STRINGS[name]
    path = os.path.join(str(tmp_dir), name + ".icm")
    doctor(os.path.join(DATA, "cluster-2.icm"), path, lo, hi, 12)
    return path


def strings_reads():
    """every read of at least 86 bases (the fused form's condition), lengths on both sides of where |sum| passes the per-read test"""
    rng = np.random.default_rng(22)
    lens = [86, 87, 128, 129] + [int(x) for x in rng.integers(86, 1400, size=300)]
    return ["".join("acgt"[c] for c in rng.integers(0, 4, size=n)) for n in lens]
