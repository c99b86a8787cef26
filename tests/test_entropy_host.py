"""The host side of the entropy distance ratio (include/gmg.h, gmg_entropy_*; no GPU needed): the translation tables against the
reference's Codon_Translation, the host finish bit for bit against the Python restatement (tests/entropy_oracle.py), and that
restatement against the reference's own long-orfs output for a whole genome."""
import os

import numpy as np
import pytest

import entropy_oracle as eo
from conftest import DATA


def test_xlate_tables_match_codon_translation(gmg):
    """gmg_xlate_table for the 17 GenBank codes Codon_Translation knows (and 0) against tests/golden/codon_translation.txt, the
    reference's answers for the 64 codons; any other code is GMG_EINVAL"""
    tabs = eo.tables()
    assert sorted(tabs) == sorted(eo.CODES)
    for code in eo.CODES:
        assert gmg.xlate_table(code) == tabs[code].encode(), code
    assert tabs[0] == tabs[1] == tabs[11]
    assert tabs[5] == tabs[21]                           # (the reference's table 21 keeps aaa = K, which leaves it equal to table 5)
    assert len({tabs[c] for c in eo.CODES}) == 15
    for code in (7, 8, 24, -1):
        with pytest.raises(gmg.GmgError) as e:
            gmg.xlate_table(code)
        assert e.value.code == -1


def test_default_profiles(gmg):
    pos, neg = gmg.entropy_default_profiles()
    assert np.array_equal(pos, np.array(eo.POS)) and np.array_equal(neg, np.array(eo.NEG))


def _bits(a):
    """the bit patterns of doubles; every NaN as one pattern (0 / 0 carries a sign bit in C that Python's nan does not)"""
    a = np.ascontiguousarray(a, np.float64)
    return np.where(np.isnan(a), np.uint64(0x7ff8000000000000), a.view(np.uint64))


def test_from_counts_is_bit_identical_to_the_oracle(gmg):
    """gmg_entropy_from_counts against the restatement, compared as bit patterns: random count vectors (sparse, dense, large), all
    zero (ep = 0), one non-zero entry (S = 0: NaN throughout), pos == neg (ratio 1.0), zero profiles with zero counts (0 / 0: 1.0)
    and a zero negative profile with a non-zero positive one (x / 0: 1e3)"""
    rng = np.random.default_rng(20)
    pos, neg = np.array(eo.POS), np.array(eo.NEG)
    rows = [rng.integers(0, 40, 20) for _ in range(300)]
    rows += [rng.integers(0, 3, 20) * rng.integers(0, 2, 20) for _ in range(200)]
    rows += [rng.integers(0, 100000, 20) for _ in range(100)]
    rows = np.array(rows, np.int32)
    assert np.array_equal(_bits(gmg.entropy_from_counts(rows, pos, neg)), _bits(eo.finish_rows(rows)))
    rpos, rneg = rng.random(20) / 10, rng.random(20) / 10
    assert np.array_equal(_bits(gmg.entropy_from_counts(rows, rpos, rneg)), _bits(eo.finish_rows(rows, rpos, rneg)))

    zero = np.zeros(20, np.int32)
    got = gmg.entropy_from_counts(zero, pos, neg)
    assert np.array_equal(_bits(got), _bits(eo.finish(zero)))
    assert abs(got[0] - np.sqrt(np.sum(pos * pos))) < 1e-15             # ep = 0: the profile's norm
    one = zero.copy()
    one[7] = 12
    got = gmg.entropy_from_counts(one, pos, neg)
    assert np.all(np.isnan(got)) and np.all(np.isnan(eo.finish(one)))
    got = gmg.entropy_from_counts(rows[0], pos, pos)
    assert got[2] == 1.0 and got[0] == got[1] and np.array_equal(_bits(got), _bits(eo.finish(rows[0], eo.POS, eo.POS)))
    got = gmg.entropy_from_counts(zero, np.zeros(20), np.zeros(20))
    assert tuple(got) == (0.0, 0.0, 1.0) == eo.finish(zero, [0.0] * 20, [0.0] * 20)
    got = gmg.entropy_from_counts(zero, pos, np.zeros(20))
    assert got[1] == 0.0 and got[0] > 0.0 and got[2] == 1e3 and tuple(got) == eo.finish(zero, eo.POS, [0.0] * 20)


def test_oracle_reproduces_the_reference_long_orfs_output(gmg):
    """the restatement over NC_000915.fna gives the ratio column of the reference's sample-run output NC_000915.longorfs
    (long-orfs -n -t 1.15) for all 1,161 rows, as printed (%6.3f) -- and so does the library's host finish"""
    hdrs, seqs = gmg.read_fasta(os.path.join(DATA, "NC_000915.fna"))
    seq = eo.filter_seq(seqs[0])
    rows = eo.longorfs_rows(os.path.join(DATA, "NC_000915.longorfs"))
    assert len(rows) == 1161
    aa = eo.tables()[0]
    cnt = np.array([eo.counts(seq, *eo.row_region(start, stop, frame, len(seq)), aa) for start, stop, frame, _ in rows], np.int32)
    ratios = eo.finish_rows(cnt)[:, 2]
    assert ["%6.3f" % r for r in ratios] == ["%6s" % text for _, _, _, text in rows]
    assert np.array_equal(_bits(gmg.entropy_from_counts(cnt, eo.POS, eo.NEG)[:, 2]), _bits(ratios))
    assert all(r < 1.15 for r in ratios)


def test_every_symbol_resolves(gmg):
    lib = gmg.capi.lib()
    for name in ("gmg_xlate_table", "gmg_entropy_regions", "gmg_entropy_orfs", "gmg_entropy_from_counts", "gmg_entropy_default_profiles"):
        assert name in gmg.capi.PROTOTYPES and getattr(lib, name) is not None
