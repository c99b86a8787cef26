"""Phymm's classification step on the host side (tests/phymm_oracle.py, integration/phymm_gpu.cc): the oracle's matrix against
the committed forward scores, its integer keys against "%.4f", score_insert's quirks, and the program's refusals that come before
any device work."""
import os
import subprocess

import numpy as np
import pytest

import phymm_oracle as po
from conftest import DATA, ROOT


def scores_tmp(i):
    ids, vals = [], []
    for line in open(os.path.join(DATA, "icm-%d.scores.tmp" % i)):
        f = line.split()
        ids.append(f[0])
        vals.append(f[1])
    return ids, vals


def test_oracle_rebuilds_the_forward_only_matrix_of_the_committed_scores():
    """the script prints simple-score's value text as it reads it: its forward-only matrix is the scores.tmp columns joined by
    tabs.  The oracle, from the parsed numbers, must give the same bytes."""
    cols = [scores_tmp(i) for i in range(6)]
    ids = cols[0][0]
    assert len(ids) == 999 and all(c[0] == ids for c in cols)
    icms = [".genomeData/s/cluster-%d.icm" % i for i in range(6)]
    want = "BEGIN_ICM_LIST\n" + "".join(p + "\n" for p in icms) + "END_ICM_LIST\nBEGIN_READID_LIST\n"
    want += "".join(r + "\n" for r in ids) + "END_READID_LIST\nBEGIN_DATA_MATRIX\n"
    want += "".join("\t".join(c[1]) + "\n" for c in cols) + "END_DATA_MATRIX\n"
    got = po.raw_file(icms, ids, [[float(v) for v in c[1]] for c in cols])
    assert got == want
    icms2, reads2, rows = po.parse_raw(got)
    assert icms2 == icms and reads2 == ids and rows == [c[1] for c in cols]


def test_keys_equal_the_printed_text():
    """keys_exact against "%.4f" on halfway values q/32 (exact ties, which go to the even digit), their neighbours, signed zeros,
    values that round to -0.0000, and random scores"""
    rng = np.random.default_rng(3)
    q = rng.integers(-2_000_000, 2_000_000, 4000)
    half = q / 32.0
    x = np.concatenate([half, np.nextafter(half, np.inf), np.nextafter(half, -np.inf), [0.0, -0.0, -4e-5, 4e-5, -5e-5, 5e-5, -1.5e-4],
                        rng.normal(-700, 200, 4000), rng.uniform(-1e-3, 1e-3, 500), rng.uniform(-4e11, 4e11, 500)])
    keys = po.keys_exact(x)
    for v, k in zip(x, keys):
        t = po.fmt(v)
        assert int(t.replace(".", "")) == k, (v, t, k)
    assert (np.abs(half * 1e4 - np.trunc(half * 1e4)) == 0.5).sum() > 1000         # (really ties)


def test_score_insert_fills_unsorted_then_inserts_at_the_first_strictly_beaten_slot():
    s = [None, None, None]
    for sc, g in ((-5.0, 0), (-1.0, 1), (-3.0, 2)):
        po.score_insert(s, sc, g)
    assert s == [(-5.0, 0), (-1.0, 1), (-3.0, 2)]                   # arrival order, not sorted
    po.score_insert(s, -4.0, 3)                                     # beats slot 0 first: goes in front of everything
    assert s == [(-4.0, 3), (-5.0, 0), (-1.0, 1)]
    po.score_insert(s, -4.0, 4)                                     # a tie beats nothing strictly: slot 1 (-5) is the first
    assert s == [(-4.0, 3), (-4.0, 4), (-5.0, 0)]
    po.score_insert(s, -6.0, 5)                                     # beats nothing: dropped
    assert s == [(-4.0, 3), (-4.0, 4), (-5.0, 0)]
    po.score_insert(s, -0.0, 6)
    assert s == [(-0.0, 6), (-4.0, 3), (-4.0, 4)]
    po.score_insert(s, 0.0, 7)                                      # 0.0 == -0.0: not strictly greater than slot 0
    assert s == [(-0.0, 6), (0.0, 7), (-4.0, 3)]


def test_numpy_insertion_equals_the_list_form():
    rng = np.random.default_rng(8)
    keys = rng.integers(-30, 30, size=(40, 300)).astype(np.int64)      # many exact ties
    inf = rng.integers(0, 2, 40).astype(bool)
    for T in (1, 2, 3, 5, 8):
        sk, sm = po.tophits_numpy(keys[:17], T, inf[:17])
        sk, sm = po.tophits_numpy(keys[17:], T, inf[17:], state=(sk, sm), first=17)
        for r in range(300):
            s = [None] * T
            for b in range(40):
                if inf[b]:
                    po.score_insert(s, int(keys[b, r]), b)
            assert [(int(a), int(c)) for a, c in zip(sk[r], sm[r])] == s


def test_strand_rule_takes_the_reverse_text_only_when_it_is_a_greater_number():
    assert po.merged_text(-1.00004, -1.00001) == "-1.0000"           # equal numbers: the forward text
    assert po.merged_text(-0.00001, 0.00001) == "-0.0000"             # -0.0000 == 0.0000: forward kept
    assert po.merged_text(-2.0, -1.99994) == "-1.9999"
    sums = np.array([[[-1.00004, -1.00001], [-0.00001, 0.00001], [-2.0, -1.99994]]])
    assert list(po.merged_keys(sums)[0]) == [-10000, 0, -19999]


@pytest.fixture(scope="module")
def phymm_exe(gmg, tmp_path_factory):
    return po.phymm_binary(str(tmp_path_factory.mktemp("phymm_bin")))


def run(exe, cwd, *args):
    env = dict(os.environ, LD_LIBRARY_PATH=os.path.join(ROOT, "glimmer-mg_amd", "lib"))
    return subprocess.run([exe, *args], cwd=cwd, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)


def test_program_refuses_fewer_informative_models_than_top_hits(phymm_exe, tmp_path):
    """parse_phymm would then read an empty slot and fail: the program refuses before it scores anything"""
    for d in ("a", "b"):
        os.makedirs(tmp_path / ".genomeData" / d)
    os.symlink(os.path.join(DATA, "cluster-0.icm"), tmp_path / ".genomeData" / "a" / "x.icm")
    os.symlink(os.path.join(DATA, "cluster-1.icm"), tmp_path / ".genomeData" / "b" / "y.icm")
    (tmp_path / "r.fa").write_text(">r1\nacgt\n")
    (tmp_path / "inf.txt").write_text("a|x\n")
    res = run(phymm_exe, tmp_path, "-t", "3", "r.fa")
    assert res.returncode != 0 and "fewer than top_hits" in res.stderr
    res = run(phymm_exe, tmp_path, "-t", "2", "--informative", "inf.txt", "r.fa")
    assert res.returncode != 0 and "1 informative ICMs, fewer than top_hits" in res.stderr
    assert not os.path.exists(tmp_path / "rawPhymmOutput_r_fa.txt") and not os.path.exists(tmp_path / "r.class.txt")
    # ... where the script itself fails
    text = po.raw_file([".genomeData/a/x.icm", ".genomeData/b/y.icm"], ["r1"], [[-1.0], [-2.0]])
    with pytest.raises((TypeError, IndexError)):
        po.classify(text, 2, informative={"a|x"})


def test_program_refuses_bad_options(phymm_exe, tmp_path):
    os.makedirs(tmp_path / ".genomeData" / "a")
    (tmp_path / "r.fa").write_text(">r1\nacgt\n")
    for args, msg in ((["-t", "17", "r.fa"], "top_hits must be 1..16"), (["-s", "ic*m", "r.fa"], "the suffix may hold"),
                      (["--batch-models", "0", "r.fa"], "at least 1")):
        res = run(phymm_exe, tmp_path, *args)
        assert res.returncode != 0 and msg in res.stderr, (args, res.stderr)
