"""The inputs of tests/test_gpu_dense_batches.py reach the kernels' per-tile, per-wave and per-round caps -- shown here without a
GPU, from the read offsets (numpy) and the CPU oracle alone (tests/dense_batches.py holds the builders and the preconditions, and
its docstring the table of caps).  Also: the builders are deterministic, and the two repeat units of `orf_dense` have the ORF and
start counts they were chosen for."""
import os

import numpy as np
import pytest

import dense_batches as db
from conftest import DATA


@pytest.fixture(scope="module")
def o_nc(oracle):
    return oracle.read(os.path.join(DATA, "NC_000915.icm"))


def test_builders_are_deterministic():
    for build in (db.short_ragged, db.short_ragged_long, db.orf_dense, db.strings_86, db.strings_85, db.training_strings):
        assert build() == build()
    assert np.array_equal(db.selection(3000), db.selection(3000))
    for L in db.UNIFORM_LENGTHS:
        seqs = db.short_uniform(L)
        assert seqs == db.short_uniform(L) and len(seqs) == 2000 and {len(s) for s in seqs} == {L}


def test_short_ragged_is_1500_reads_of_0_to_8_bases_then_1500_of_9_to_40():
    lens = np.array([len(s) for s in db.short_ragged()])
    assert len(lens) == 3000 and lens[:1500].max() == 8 and lens[1500:].max() == 40
    assert set(lens[:1500]) == set(range(9)) and set(lens[1500:]) == set(range(9, 41)) | {0}
    assert set("".join(db.short_ragged())) == set("acgt")


def test_short_ragged_is_dense_in_reads_everywhere():
    got = db.require_short_ragged(db.short_ragged())
    assert got["stretch400"] > 64 and got["chunk2048"] > 150 and got["tile1024"] > 32
    db.require_orfbits_window(db.short_ragged())


def test_short_ragged_long_keeps_them_and_moves_the_plan():
    seqs = db.short_ragged_long()
    got = db.require_short_ragged_long(seqs)
    assert len(seqs) == 3040 and got["n_over_512"] > 0
    short = db.short_ragged()
    assert [s for s in seqs if len(s) <= 40] == short                 # the same reads in the same order, the long ones between them
    db.require_orfbits_window(seqs)


@pytest.mark.parametrize("err", [False, True], ids=["default", "min_indel_orf_len"])
def test_short_ragged_has_more_than_192_orfs_in_64_consecutive_reads(oracle, err):
    got = db.require_orfs_per_64_reads(oracle, db.short_ragged(), err, **db.MG_KW)
    assert got["n_orfs"] > 3000 and got["per_read"] > 1
    db.require_orfs_per_64_reads(oracle, db.short_ragged_long(), err, **db.MG_KW)


def test_short_ragged_has_accepted_orfs_and_start_lists(oracle, o_nc):
    """(what the comparison of the front half is about: thousands of ORFs with starts, most of them accepted)"""
    prm, o_indep = oracle.mg_params(**db.MG_KW), oracle.indep(0.5)
    n_orfs = n_acc = n_starts = 0
    for s in db.short_ragged():
        _, scored = oracle.mg_read(o_nc, o_indep, s.encode(), prm)
        n_orfs += len(scored)
        n_acc += sum(1 for out, _ in scored if out.accepted)
        n_starts += sum(len(st) for _, st in scored)
    assert n_orfs > 5000 and n_acc > 3000 and n_starts > 5000, (n_orfs, n_acc, n_starts)


def test_uniform_batches_below_the_window_are_all_heads():
    for L in (1, 2, 3):
        db.require_all_heads(db.short_uniform(L), 12)
    db.require_all_heads(db.short_ragged()[:1500], 12)
    for L in (11, 12, 13, 40):                                           # ... and the others are not: W - 1, W, W + 1 and beyond
        with pytest.raises(AssertionError):
            db.require_all_heads(db.short_uniform(L), 12)


@pytest.mark.parametrize("unit", [db.REPEAT_A, db.REPEAT_B])
def test_repeat_units_have_the_counts_they_were_chosen_for(oracle, o_nc, unit):
    fwd, rev, n_indel, n_sub = db.require_repeat_unit(oracle, unit, o_nc, oracle.indep(0.5))
    assert max(fwd, rev) > 64 and min(fwd, rev) <= 64 and n_indel < 64 and n_sub < 128


def test_orf_dense_has_reads_beyond_64_orfs_per_strand_and_reads_below(oracle):
    seqs = db.orf_dense()
    got = db.require_orf_dense(oracle, seqs, **db.MG_KW)
    assert len(seqs) == 38 and got["over"] >= 4 and got["under"] >= 1 and got["most"] == 106
    counts = [db.strand_counts(o) for o in db.orfs_per_read(oracle, seqs, True, **db.MG_KW)]
    rich = [c for s, c in zip(seqs, counts) if len(s) == 960]
    assert len(rich) == 4 and all(55 <= x <= 70 for c in rich for x in c), rich


def test_strings_batches_open_the_fused_form_and_miss_it_by_one_base():
    a, b = db.strings_86(), db.strings_85()
    assert db.require_strings_round(a, True) < 30                        # one chunk per work-group: rounds of about 25 reads
    db.require_strings_round(b, False)
    assert len(a) == 900 and 77_000 < sum(map(len, a)) < 79_000
    assert [x == y for x, y in zip(a, b)].count(False) == 1
    with pytest.raises(AssertionError):
        db.require_strings_round(b, True)
    with pytest.raises(AssertionError):
        db.require_strings_full_rounds(a)


def test_large_strings_batch_runs_full_rounds_of_the_fused_sums():
    """14 chunks of 2,048 bases per round, 334 or 335 reads in the fullest: the most that reads of 86 bases allow, below NR_MAX = 384"""
    seqs = db.strings_86_rounds()
    assert seqs == db.strings_86_rounds() and len(seqs) == 92000
    assert db.require_strings_full_rounds(seqs) in (334, 335)
    rounds = db.string_sum_rounds(seqs)
    assert sum(k for k, _ in rounds) == sum(map(len, seqs)) // 2048 and max(k for k, _ in rounds) == 14


def test_front_half_tiles_receive_more_reads_and_orfs_than_they_take(oracle):
    """mg_plan's windows restated: 464 bases for short_ragged, 284 for short_ragged_long (its longest read widens the tile to nine
    elements per lane and takes half of it)"""
    for seqs, window, cap in ((db.short_ragged(), 464, 504), (db.short_ragged_long(), 284, 567)):
        assert db.front_half_plan(seqs)[:2] == (window, cap)
        got = db.require_front_half_tiles(oracle, seqs, False, **db.MG_KW)
        assert got["reads_max"] == 64 and got["full_tiles"] >= 10 and got["most_orfs"] > 64 and got["most_reads_in_a_window"] > 64
        got = db.require_front_half_tiles(oracle, seqs, True, **db.MG_KW)
        assert got["reads_max"] == 6 and got["full_tiles"] * 2 > got["tiles"]
    sparse = db.random_reads(np.random.default_rng(2), np.random.default_rng(3).integers(200, 400, 60))
    with pytest.raises(AssertionError):
        db.require_front_half_tiles(oracle, sparse, False, **db.MG_KW)


def test_error_branch_tiles_close_at_64_reads_and_hold_more_than_192_orfs(oracle):
    got = db.require_error_tiles(oracle, db.short_ragged(), **db.MG_KW)
    assert got["closed_by_64_reads"] >= 20 and got["most_orfs"] > 192
    with pytest.raises(AssertionError):
        db.require_error_tiles(oracle, db.orf_dense(), **db.MG_KW)


def test_selection_passes_sel_r_and_ends_in_a_partial_tile():
    seqs = db.short_ragged()
    got = db.require_selection(seqs, db.selection(len(seqs)))
    assert got["most_per_tile"] > 32


def test_one_group_per_read_puts_more_than_50_groups_into_a_chunk():
    assert db.require_groups(db.short_ragged()[1500:]) > 50


def test_training_strings_are_mostly_shorter_than_the_window():
    db.require_training_strings(db.training_strings(), 12)


def test_a_precondition_that_does_not_hold_fails():
    """(no skip: a batch that misses its cap is an AssertionError in either test file)"""
    sparse = db.random_reads(np.random.default_rng(1), [300] * 50)
    with pytest.raises(AssertionError):
        db.require_short_ragged(sparse)
    with pytest.raises(AssertionError):
        db.require_orfbits_window(sparse)
    with pytest.raises(AssertionError):
        db.require_selection(db.short_ragged(), np.arange(5000) % 3000)
