"""The three things every launcher of the six-frame kernels (gmg_frame6.hip) decides from the batch's total -- whether there is a
main pass (total / 2048 > 0), whether there is a tail (total % 2048 != 0), which store form runs (the row stride's parity) --
through every launcher, on batches of 2,047 .. 6,145 bases: ragged reads of 86 .. 400 bases, and one read.  Against the CPU
oracle bit for bit where it has the value, otherwise against the library's own exact path.  Run with -m gpu."""
import os

import numpy as np
import pytest

import model_zoo
from conftest import DATA
from test_gpu_dense_batches import plain_frame_score6

pytestmark = pytest.mark.gpu

NC = os.path.join(DATA, "NC_000915.icm")
GICM = os.path.join(DATA, "seqs.cluster-4.run1.filt.gicm")
P1 = os.path.join(DATA, "cluster-0.icm")                # periodicity 1: the strings main pass
TOTALS = (2047, 2048, 2049, 4096, 6145)                 # no whole chunk; whole chunks only; a tail; odd and even totals
GC, GCS = 0.47, [0.38, 0.61]

_cache = {}


def batch(total, kind):
    """(strings, their offsets): computed once, never changed"""
    if (total, kind) not in _cache:
        rng = np.random.default_rng(total)
        lens, left = [], total
        while kind == "ragged" and left > 400:
            n = int(rng.integers(86, min(400, left - 86) + 1))
            lens.append(n)
            left -= n
        lens.append(left)
        assert sum(lens) == total and (kind == "one_read" or (min(lens) >= 86 and max(lens) <= 400 and len(lens) > 5))
        seqs = ["".join("acgt"[c] for c in rng.integers(0, 4, size=n)) for n in lens]
        _cache[total, kind] = seqs, np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    return _cache[total, kind]


def revcomp(s):
    return s[::-1].translate(str.maketrans("acgt", "tgca"))


CASES = pytest.mark.parametrize("total,kind", [(t, k) for t in TOTALS for k in ("ragged", "one_read")])


@CASES
def test_frame_table_plain_and_strided(gpu, oracle, total, kind):
    """gmg_frame_score6 (stride = total) and the strided entry at total + 1 and total + 2: one of every parity, both store forms"""
    seqs, _ = batch(total, kind)
    reads = gpu.Reads.from_strings(seqs)
    icm, indep = gpu.Icm.open(NC), gpu.Icm.indep(GC)
    om, o_indep = oracle.read(NC), oracle.indep(GC)
    want = np.concatenate([oracle.score_all_frames(om, o_indep, s) for s in seqs], axis=1)
    assert want.shape == (6, total) == (6, reads.total_bases)
    for tag, got in (("plain", plain_frame_score6(gpu, icm, indep, reads)),
                     ("total+1", gpu.frame_score6(icm, indep, reads, row_stride=total + 1)),
                     ("total+2", gpu.frame_score6(icm, indep, reads, row_stride=total + 2))):
        bad = np.flatnonzero((got != want).any(axis=0))
        assert len(bad) == 0, (tag, "first base that differs", int(bad[0]), "of", len(bad))


@CASES
def test_frame_table_with_a_null_model_per_read(gpu, oracle, total, kind):
    """gmg_frame_score6_nulls: the gene rows complete (gmg_launch_gene6_full), two GC values in turn"""
    seqs, _ = batch(total, kind)
    reads = gpu.Reads.from_strings(seqs)
    om, o_nulls = oracle.read(NC), [oracle.indep(gc) for gc in GCS]
    read_null = ((np.arange(len(seqs)) + 1) % 2).astype(np.uint32)
    want = np.concatenate([oracle.score_all_frames(om, o_nulls[k], s) for k, s in zip(read_null, seqs)], axis=1)
    got = gpu.frame_score6(gpu.Icm.open(NC), gpu.NullSet.build(GCS), reads, read_null=read_null)
    bad = np.flatnonzero((got != want).any(axis=0))
    assert got.shape == want.shape and len(bad) == 0, ("first base that differs", int(bad[0]), "of", len(bad))


@CASES
def test_string_sums_fused_and_two_pass(gpu, oracle, total, kind):
    """gmg_score_reads_strings under a periodicity-1 model the fused form takes: strings_fused 1 (gmg_launch_strings_sum) and 0
    (gmg_launch_strings; rows `total` floats apart: both parities), every read and its reverse complement"""
    seqs, _ = batch(total, kind)
    reads = gpu.Reads.from_strings(seqs)
    om = oracle.read(P1)
    lo, hi, odd = model_zoo.exponent_range(*oracle.tables(om))
    assert om.contents.periodicity == 1 and not odd and lo >= 109 and hi - lo <= 23 and min(map(len, seqs)) >= 86
    want = np.array([(oracle.score_string(om, s, 0), oracle.score_string(om, revcomp(s), 0)) for s in seqs])
    icm = gpu.Icm.open(P1)
    for fused in (1, 0):
        with gpu.option("strings_fused", fused):
            got = gpu.score_reads_strings([icm], reads)[0]
        bad = np.flatnonzero((got != want).any(axis=1))
        assert got.shape == want.shape and len(bad) == 0, ("strings_fused", fused, "first read that differs", int(bad[0]), "of", len(bad))


@CASES
def test_score_orfs_default_path_equals_the_exact_path(gpu, total, kind):
    """gmg_score_orfs on the ORFs gmg_find_orfs reports: the default path (gene rows from gmg_launch_gene6, `total` floats apart,
    the tail on the any-shape kernel) against orfs_exact_path = 1, every byte of every result and start"""
    seqs, _ = batch(total, kind)
    reads = gpu.Reads.from_strings(seqs)
    found, _ = gpu.find_orfs(reads, min_gene_len=30, allow_truncated=True)
    rows = np.stack([found["read"].astype(np.int64), found["frame"], found["stop_position"], found["orf_len"]], 1)
    assert len(rows) > 10
    icm, indep = gpu.Icm.open(NC), gpu.Icm.indep(GC)
    kw = dict(min_gene_len=30, allow_truncated=True)
    assert gpu.get_option("orfs_exact_path") == 0
    res, starts = gpu.score_orfs(icm, indep, reads, rows, **kw)
    with gpu.option("orfs_exact_path", 1):
        res_x, starts_x = gpu.score_orfs(icm, indep, reads, rows, **kw)
    assert int(res["n_starts"].sum()) > 10
    assert res.tobytes() == res_x.tobytes() and starts.tobytes() == starts_x.tobytes()


@pytest.mark.parametrize("total", TOTALS)
def test_two_groups_with_their_boundary_inside_a_chunk(gpu, total):
    """gmg_mg_score_groups (gmg_launch_gene6_groups) with two groups under two models: every record and start as with the two groups
    scored alone.  With 6,145 bases a round on either side of the chunk that holds the boundary; with 2,047 and 2,048 no round at all."""
    seqs, off = batch(total, "ragged")
    cut = len(seqs) // 2
    assert 0 < cut < len(seqs) and off[cut] % 2048 != 0
    reads = gpu.Reads.from_strings(seqs)
    models = [gpu.Icm.open(NC), gpu.Icm.open(GICM)]
    groups = [(models[0], 0, cut), (models[1], cut, len(seqs))]
    nulls = gpu.NullSet.build(GCS)
    read_null = (np.arange(len(seqs)) % 2).astype(np.uint32)
    kw = dict(min_gene_len=60)
    whole = gpu.mg_score_reads(None, nulls, reads, read_null=read_null, groups=groups, **kw)
    n_orfs = n_starts = 0
    for m, b, e in groups:
        part = gpu.mg_score_reads(m, nulls, reads.select(np.arange(b, e, dtype=np.uint64)), read_null=read_null[b:e], **kw)
        mine = whole[0][int(whole[2][b]):int(whole[2][e])].copy()
        assert len(mine) == len(part[0]) > 0
        s0 = int(mine["start_begin"][0])
        s1 = int(mine["start_begin"][-1]) + int(mine["n_starts"][-1])
        mine["read"] -= b                               # the two fields that count from the batch's start
        mine["start_begin"] -= s0
        assert mine.tobytes() == part[0].tobytes(), (b, e)
        assert whole[1][s0:s1].tobytes() == part[1].tobytes(), (b, e)
        n_orfs += len(mine)
        n_starts += s1 - s0
    assert n_orfs == len(whole[0]) and n_starts == len(whole[1]) > 0


def test_reads_without_bases(gpu):
    """two empty reads through every call that takes such a batch: an empty table, zero sums, no ORFs (gmg_launch_frame6_strided still
    launches the heads pass for its two reads)"""
    reads = gpu.Reads.from_strings(["", ""])
    assert (reads.n_reads, reads.total_bases) == (2, 0)
    icm, indep, nulls = gpu.Icm.open(NC), gpu.Icm.indep(GC), gpu.NullSet.build(GCS)
    read_null = np.array([0, 1], np.uint32)
    assert plain_frame_score6(gpu, icm, indep, reads).shape == (6, 0)
    for stride in (0, 1, 2):
        assert gpu.frame_score6(icm, indep, reads, row_stride=stride).shape == (6, 0)
    assert gpu.frame_score6(icm, nulls, reads, read_null=read_null).shape == (6, 0)
    for fused in (1, 0):
        with gpu.option("strings_fused", fused):
            sums = gpu.score_reads_strings([gpu.Icm.open(P1), icm], reads)
        assert sums.shape == (2, 2, 2) and not sums.any() and not np.signbit(sums).any()
    for got in (gpu.mg_score_reads(icm, indep, reads),
                gpu.mg_score_reads(None, nulls, reads, read_null=read_null, groups=[(icm, 0, 1), (gpu.Icm.open(GICM), 1, 2)])):
        assert len(got[0]) == 0 and len(got[1]) == 0 and got[2].tolist() == [0, 0, 0]
