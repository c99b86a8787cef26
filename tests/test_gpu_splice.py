"""gmg_reads_splice on the device (include/gmg.h): strings spliced from runs of a batch's reads -- upwards, downwards with the code
complement, with the substitution on codes, literal codes -- as a NEW batch: every packed word against the same expansion in
Python (tests/splice_oracle.py), on shapes chosen for where the gather can go wrong (word and tile boundaries, empty strings, more
runs in a tile than the kernel stages), both ways round, the errors, and the recorded predictions end to end."""
import gc

import numpy as np
import pytest

import extract_oracle as xo
import splice_oracle as so
from splice_oracle import UP, DOWN, SUB_UP, SUB_DOWN, LITERAL, LITERAL_AS_IS

pytestmark = pytest.mark.gpu

EINVAL, ERANGE = -1, -6
LENGTHS = (1, 15, 16, 17, 31, 33, 64, 1025, 2100, 4)
STAGED = 64                                             # SPL_R: the runs of a tile the kernel stages in LDS


@pytest.fixture(scope="module")
def source(gpu):
    """reads that begin at many bit offsets (read 0: the guard words in front); the last read holds each code once"""
    rng = np.random.default_rng(51)
    reads = [rng.integers(0, 4, size=n).tolist() for n in LENGTHS[:-1]] + [[0, 1, 2, 3]]
    batch = gpu.Reads(*xo.pack(reads))
    yield reads, batch
    batch.close()


def _check(batch, want):
    """offsets, every packed word, the zero bits behind the last base and the zero guard word"""
    packed, off = batch.download()
    words, woff = xo.pack(want)
    assert np.array_equal(off, woff)
    assert len(packed) == len(words) and packed[-1] == 0
    bad = np.nonzero(packed != words)[0]
    assert len(bad) == 0, "first differing word %d: %08x, expected %08x" % (bad[0], packed[bad[0]], words[bad[0]])


def _both_ways(batch, reads, strings):
    """strings: [[run, ...], ...] -> spliced as they are and reversed, checked against the expansion"""
    runs = [r for s in strings for r in s]
    sro = np.concatenate([[0], np.cumsum([len(s) for s in strings])]).astype(np.uint64)
    arr = np.array(runs, np.uint32).reshape(-1, 4)
    for reversed in (False, True):
        sub = batch.splice(arr, sro, reversed=reversed)
        assert sub.n_reads == len(strings)
        _check(sub, so.spliced(reads, arr, sro, reversed))
        sub.close()


def test_run_ends_at_word_and_tile_boundaries(gpu, source):
    """a first run that ends on base 15, 16, 17 of a word and on base 1,023, 1,024, 1,025 of a tile, every kind of run behind it"""
    reads, batch = source
    strings = []
    for n in (15, 16, 17, 1023, 1024, 1025):
        for kind in (UP, DOWN, SUB_UP, SUB_DOWN):
            down = kind in (DOWN, SUB_DOWN)
            head = (8, 2099 if down else 3, n, kind)
            for tail in [(7, 1000, 40, DOWN), (7, 5, 40, UP), (0, 0, 21, LITERAL + 2), (3, 16, 17, SUB_DOWN), (5, 0, 33, SUB_UP)]:
                strings.append([head, tail])
    _both_ways(batch, reads, strings)


def test_runs_of_length_one_and_empty_strings(gpu, source):
    """an empty string first, last and between two others; empty runs inside a string; runs of one base of every kind"""
    reads, batch = source
    rng = np.random.default_rng(52)
    ones = [(6, int(rng.integers(0, 64)), 1, int(rng.integers(0, 4))) for _ in range(40)]
    strings = [[], ones[:7], [], [], ones[7:8], [(6, 64, 0, UP), (6, 0, 0, DOWN), ones[8], (6, 3, 0, SUB_UP)], ones[9:], [(2, 0, 0, UP)], []]
    _both_ways(batch, reads, strings)
    _both_ways(batch, reads, [[], []])


def test_long_string_many_strings_many_runs(gpu, source):
    """a string of 2,100 bases made of three runs; 1,100 one-base strings in a row (more strings than a tile has bases); one
    string of 600 one-base runs"""
    reads, batch = source
    rng = np.random.default_rng(53)
    long3 = [(8, 0, 700, UP), (8, 2099, 900, DOWN), (7, 100, 500, SUB_UP)]
    tiny = [[(7, int(rng.integers(0, 1025)), 1, int(rng.integers(0, 4)))] for _ in range(1100)]
    many = [(8, int(rng.integers(0, 2100)), 1, int(rng.integers(0, 4))) for _ in range(600)]
    _both_ways(batch, reads, [long3] + tiny + [many, long3])


@pytest.mark.parametrize("n_runs", [STAGED - 1, STAGED, STAGED + 1, 2 * STAGED + 1])
def test_the_runs_a_tile_stages(gpu, source, n_runs):
    """tiles that exactly as many runs overlap as the kernel stages, one less, one more, twice as many: runs of 14 to 18 bases, so that
    the runs behind the staged ones fill whole words, then a long run that takes the rest of the tile and the next one"""
    reads, batch = source
    head = [(8, 16 * k + 3, 14 + k % 5, (UP, DOWN, SUB_UP, SUB_DOWN)[k % 4]) for k in range(n_runs - 1)]
    for lead in (0, 1, 700):                            # the string begins at the tile's base 0, at base 1, in its middle
        strings = ([[(7, 0, lead, UP)]] if lead else []) + [head + [(8, 50, 1500, UP)], head]
        _both_ways(batch, reads, strings)


def test_downward_runs_across_source_words(gpu, source):
    """downward runs that begin and end at every offset of a source word, from reads at several bit offsets and from the read at
    word 0 (its windows reach into the guard words)"""
    reads, batch = source
    strings = []
    for r in (0, 1, 3, 5, 6):
        L = LENGTHS[r]
        strings += [[(r, f, n, kind)] for f in range(L) for n in range(1, f + 2) for kind in (DOWN, SUB_DOWN)][:600]
    strings += [[(8, f, 40, DOWN), (8, f + 1, 40, UP)] for f in range(39, 72)]
    _both_ways(batch, reads, strings)


def test_substitution_and_literals(gpu, source):
    """a substitute run on each of the four codes in both directions: c -> g, a g t -> c, complemented downwards; a literal of every
    code next to a copy inside one word"""
    reads, batch = source
    sub = batch.splice(np.array([(9, 0, 4, SUB_UP), (9, 3, 4, SUB_DOWN)], np.uint32), np.array([0, 1, 2], np.uint64))
    assert xo.unpack(*sub.download()) == [[1, 2, 1, 1], [2, 2, 1, 2]]
    sub.close()
    strings = [[(9, k, 1, SUB_UP)] for k in range(4)] + [[(9, k, 1, SUB_DOWN)] for k in range(4)]
    strings += [[(6, 10, 5, UP), (0, 0, 1, LITERAL + c), (6, 20, 5, DOWN), (99, 7, 2, LITERAL_AS_IS + c), (6, 16, 3, UP)] for c in range(4)]
    _both_ways(batch, reads, strings)


def test_errors_leave_nothing_behind(gpu, source):
    reads, batch = source
    out = (gpu.capi.C.c_uint64 * 4)()

    def busy():
        assert gpu.capi.lib().gmg_debug_cache_stats(out) == 0
        return int(out[0])

    gc.collect()
    gpu.capi.lib().gmg_synchronize(None)
    before = busy()
    good = (5, 3, 20, UP)
    for bad in [(10, 0, 1, UP), (5, 14, 20, UP), (5, 33, 1, DOWN), (5, 18, 20, DOWN), (5, 0, 2, SUB_DOWN), (5, 30, 4, SUB_UP), (5, 0, 1, 12),
                (5, 34, 0, UP)]:
        with pytest.raises(gpu.GmgError, match="run 1 ") as e:
            batch.splice(np.array([good, bad, (77, 0, 9, UP)], np.uint32), np.array([0, 2, 3], np.uint64))
        assert e.value.code == ERANGE
        assert busy() == before
    for sro in ([1, 2], [0, 2, 1, 1], [0, 0]):
        with pytest.raises(gpu.GmgError) as e:
            batch.splice(np.array([good], np.uint32), np.array(sro, np.uint64))
        assert e.value.code == EINVAL
    sub = batch.splice(np.array([good], np.uint32), np.array([0, 1], np.uint64))
    assert busy() == before + 3                          # packed words, offsets, tile table
    sub.close()
    empty = batch.splice(np.zeros((0, 4), np.uint32), np.array([0], np.uint64))
    assert empty.n_reads == 0 and empty.total_bases == 0
    packed, off = empty.download()
    assert list(off) == [0] and not packed.any()
    empty.close()
    assert busy() == before


@pytest.mark.parametrize("name", ["glimmer-mg.indel", "edges"])
def test_planned_strings_are_the_codes_of_the_recorded_text(gpu, name):
    """gmg_edits_plan + gmg_reads_splice on the sequence file as gmg_fasta_ingest packs it: Subscript of every letter of the .ffn
    file scripts/extract_aa.py wrote, blanks aside; reversed: back to front"""
    data = open(so.CASES[name][0], "rb").read()
    fasta = so.read_fasta(so.CASES[name][0])
    headers, seqs = [h for h, _ in fasta], [s for _, s in fasta]
    runs, sro, rows = gpu.edits_plan(so.offsets(seqs), so.parse_predict(so.CASES[name][1], headers), so.odd_letters(seqs))
    batch, _, _ = gpu.Reads.from_fasta_bytes(data)
    want = [[xo.code(ch) for ch in text if ch != " "] for text in so.script_ffn(gpu, name).decode().split("\n")[1::2]]
    for reversed in (False, True):
        sub = batch.splice(runs, sro, reversed=reversed)
        _check(sub, [w[::-1] for w in want] if reversed else want)
        sub.close()
    batch.close()
