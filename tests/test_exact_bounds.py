"""CPU companion of tests/test_gpu_exact_bounds.py: the doctored models (tests/exact_models.py) sit where they are meant to sit,
and on `edge` the reference's own arithmetic is exact -- every running sum, recomputed in Python integers in units of 2^-149,
equals the oracle's double.  So a device path that adds in another order must give the same bits on `edge`; on `past` and `wide`
the predicate no longer holds and the device must take the reference's order."""
from fractions import Fraction

import numpy as np
import pytest

import exact_models
import model_zoo

UNIT = 2 ** 149


def as_int(x):
    f = Fraction(float(x)) * UNIT
    assert f.denominator == 1
    return int(f.numerator)


def check_running_sums(values, sums):
    """sums[i] = values[0] + .. + values[i] added one by one in doubles; the same in integers"""
    acc = 0
    for v, s in zip(values, sums):
        acc += as_int(v)
        assert Fraction(acc, UNIT) == Fraction(float(s)), "a running sum was rounded"
    return acc


@pytest.mark.parametrize("which,total", [("edge", 28), ("past", 29), ("wide", 29)])
def test_mg_models_sit_at_the_bound(oracle, tmp_path, which, total):
    m = oracle.read(exact_models.mg_model(oracle, which, tmp_path))
    lo, hi, odd = model_zoo.exponent_range(*oracle.tables(m))
    assert (lo, hi) == exact_models.mg_bounds(oracle, which) and not odd          # both ends occur
    n_lo, n_hi = exact_models.null_range(oracle)
    longest = max(len(s) for s in exact_models.mg_reads(which))
    assert model_zoo.clog(longest) + max(hi, n_hi) - min(lo, n_lo) == total
    _, prob = oracle.tables(m)
    assert np.all((prob[prob != 0].view(np.uint32) & 1) == 1)                      # the lowest mantissa bit of every value


def test_edge_sums_are_exact_on_the_reference_alone(oracle, tmp_path):
    """Score_All_Frames' table (gene - null per base), its running sums along every row in both directions (what Score_Orf_Starts
    and the error branch add up, glimmer-mg.cc:561-604), Cumulative_Score of gene and null model in every frame (Score_Orfs) and
    the sum of |values| (every sum of every subset in every order is then exact too)"""
    m = oracle.read(exact_models.mg_model(oracle, "edge", tmp_path))
    lo = exact_models.mg_bounds(oracle, "edge")[0]
    seqs = exact_models.mg_reads("edge")
    worst = 0
    for r, s in enumerate(seqs):
        null = oracle.indep(exact_models.GCS[r % len(exact_models.GCS)])
        fs = oracle.score_all_frames(m, null, s)
        for row in fs:
            check_running_sums(row, np.cumsum(row))
            check_running_sums(row[::-1], np.cumsum(row[::-1]))
            worst = max(worst, sum(abs(as_int(v)) for v in row))
        if r % 10 == 0 or r == len(seqs) - 1:
            for model in (m, null):
                for orient in (1, 2):
                    buf = oracle.buffer(s, 0, len(s), orient)
                    per = [oracle.frame_score(model, buf, f) for f in range(3)]             # Frame_Score keeps its frame, Cumulative_Score cycles
                    for f in range(3):
                        vals = [per[(f + i) % 3][i] for i in range(len(buf))]
                        check_running_sums(vals, oracle.cumulative_score(model, buf, f))
    assert worst % (1 << (lo - 150 + 149)) == 0 and worst >> (lo - 1) < 1 << 53  # multiples of 2^(lo - 150), fewer than 53 bits of them


@pytest.mark.parametrize("name", sorted(exact_models.STRINGS))
def test_strings_models_and_reads_straddle_the_per_read_test(oracle, tmp_path, name):
    lo, hi = exact_models.STRINGS[name]
    m = oracle.read(exact_models.strings_model(name, tmp_path))
    assert model_zoo.exponent_range(*oracle.tables(m)) == (lo, hi, False)
    seqs = exact_models.strings_reads()
    assert min(len(s) for s in seqs) >= 86
    sums = np.array([oracle.score_string(m, s, 0) for s in seqs])
    limit = 2.0 ** (lo - 150 + 51)                      # ilogb |sum| + 2 - (min_exp - 150) <= 53  <=>  |sum| < 2 * limit
    assert (np.abs(sums) < limit).sum() >= 10 and (np.abs(sums) >= 2 * limit).sum() >= 10
    if name == "s109_23":                               # the model the fused form takes: short reads' sums are exact integers of 2^-41
        n = 0
        for s, total in zip(seqs, sums):
            if abs(total) < 2 * limit:                  # (a read that passes the per-read test)
                check_running_sums(oracle.frame_score(m, s, 0), oracle.cumulative_score(m, s, 0))
                n += 1
        assert n >= 10
