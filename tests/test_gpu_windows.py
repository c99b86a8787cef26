"""gmg_window_counts and gmg_regions_uncovered on the device (glimmer-mg_amd/csrc/gmg_windows.hip; include/gmg.h) against the Python
restatement of window-acgt's ring buffer and uncovered's sort-and-merge (tests/windows_oracle.py).  Every output is an integer: all
comparisons are exact.  Shapes are the smallest at which the kernels can go wrong: reads of 0 .. 70 bases back to back, so that
reads begin at every position of a 16-base word and of a 64-base block of running counts, window lengths on both sides of one and
two words and of a block, more rows than one work-group of 256, one long read that crosses many blocks."""
import ctypes as C

import numpy as np
import pytest

import windows_oracle as wo

pytestmark = pytest.mark.gpu

WIDTHS = (1, 2, 15, 16, 17, 31, 32, 33, 64, 65, 70, 71)


def skips_of(W):
    return sorted({s for s in (1, 2, W - 1, W, W + 1, 16, 17, 100) if s >= 1})


def _rand_seq(rng, n, alphabet="acgt"):
    return "".join(alphabet[c] for c in rng.integers(0, len(alphabet), size=int(n)))


def _check(gpu, reads, seqs, W, S, amb="auto"):
    if amb == "auto":
        amb = wo.ambiguous_bases(seqs)
    off, counts = gpu.window_counts(reads, W, S, amb=amb)
    want_off, want = wo.batch_window_counts(seqs, W, S)
    assert [int(x) for x in off] == want_off, (W, S)
    got = counts.tolist()
    if got != want:
        k = next(i for i in range(len(want)) if got[i] != want[i])
        r = max(i for i in range(len(seqs)) if want_off[i] <= k)
        raise AssertionError("W %d S %d: row %d (read %d of %d bases, window %d): device %r, restatement %r"
                             % (W, S, k, r, len(seqs[r]), k - want_off[r], got[k], want[k]))
    return off, counts


@pytest.fixture(scope="module")
def ladder():
    """reads of 0 .. 70 bases back to back, then an empty read between two full ones once more"""
    rng = np.random.default_rng(21)
    seqs = [_rand_seq(rng, n) for n in range(0, 71)] + [_rand_seq(rng, 40), "", _rand_seq(rng, 33)]
    return seqs


@pytest.fixture(scope="module")
def ladder_reads(gpu, ladder):
    return gpu.Reads.from_strings(ladder)


@pytest.mark.parametrize("W", WIDTHS)
def test_every_read_length_against_the_ring_buffer(gpu, ladder, ladder_reads, W):
    for S in skips_of(W):
        _check(gpu, ladder_reads, ladder, W, S)


def test_no_ambiguous_list_with_null_pointers(gpu, ladder, ladder_reads):
    off, counts = _check(gpu, ladder_reads, ladder, 16, 5, amb=None)
    assert (counts[:, 4] == 0).all() and counts.sum() > 0


def _with_letters(seqs, places, letter):
    out = [list(s) for s in seqs]
    for r, p in places:
        out[r][p] = letter
    return ["".join(s) for s in out]


@pytest.mark.parametrize("letter", ["n", "r", "w", "N"])
def test_ambiguous_letters_at_the_edges(gpu, ladder, letter):
    """n packs as c, r as g, w as t: each code is taken off once.  Places: the first and last base of a read, the last of read r with
    the first of read r + 1, both sides of a word boundary, the first and last base of a full and of the trailing partial window
    (W 10, S 4 on the 37-base read: full windows at 0, 4, .. , 24, the partial one from 28), every base of one read."""
    W, S = 10, 4
    assert wo.closed_form_windows(37, W, S)[-2:] == [(25, 10), (29, 9)]
    base = [0]
    for s in ladder:
        base.append(base[-1] + len(s))
    r16 = next(r for r in range(20, 70) if base[r] % 16 not in (0, 15) and len(ladder[r]) > 20)       # a word boundary inside read r16
    cut = 16 - base[r16] % 16
    places = [(30, 0), (30, 29), (40, 39), (41, 0), (r16, cut - 1), (r16, cut), (37, 24), (37, 33), (37, 28), (37, 36), (50, 8), (50, 17)]
    places += [(12, p) for p in range(12)]
    seqs = _with_letters(ladder, places, letter)
    reads = gpu.Reads.from_strings(seqs)
    off, counts = _check(gpu, reads, seqs, W, S)
    assert counts[:, 4].sum() > 0
    row = int(off[12])
    assert counts[row].tolist() == [0, 0, 0, 0, 10]      # the window that is all letters
    for W2, S2 in ((1, 1), (16, 16), (17, 5), (64, 1), (70, 100)):
        _check(gpu, reads, seqs, W2, S2)


def test_one_read_whose_last_window_ends_on_the_last_base(gpu):
    rng = np.random.default_rng(22)
    for L, W, S in ((64, 16, 16), (100, 10, 9), (129, 65, 64), (16, 16, 1)):
        s = _rand_seq(rng, L)
        assert sum(wo.closed_form_windows(L, W, S)[-1]) - 1 == L
        _check(gpu, gpu.Reads.from_strings([s]), [s], W, S)


def test_two_thousand_reads(gpu):
    """more rows than one work-group's 256, reads of about 500 bases; (600, 1): every read is shorter than the window, one row each"""
    rng = np.random.default_rng(23)
    seqs = [_rand_seq(rng, n, "acgtn" if i % 97 == 0 else "acgt") for i, n in enumerate(rng.integers(440, 560, size=2000))]
    reads = gpu.Reads.from_strings(seqs)
    off, counts = _check(gpu, reads, seqs, 100, 50)
    assert len(counts) > 2000 * 8
    off, counts = _check(gpu, reads, seqs, 600, 1)
    assert len(counts) == 2000 and [int(x) for x in counts.sum(axis=1)] == [len(s) for s in seqs]


def test_one_long_read(gpu):
    rng = np.random.default_rng(24)
    s = list(_rand_seq(rng, 100000))
    for p in (0, 999, 1000, 50000, 50001, 99999):
        s[p] = "n"
    s = "".join(s)
    reads = gpu.Reads.from_strings([s])
    off, counts = _check(gpu, reads, [s], 1000, 1)
    assert len(counts) == 99001
    _check(gpu, reads, [s], 1000, 1000)


def test_device_rows_equal_the_fetched_rows(gpu, ladder, ladder_reads):
    off, counts, off2, counts2 = gpu.window_counts(ladder_reads, 17, 5, amb=None, device=True)
    assert (off == off2).all() and (counts == counts2).all() and len(counts) == int(off[-1])


def test_window_error_codes(gpu, ladder, ladder_reads, request_finalizers):
    total = sum(len(s) for s in ladder)
    for W, S in ((0, 1), (1, 0), (-5, 3), (3, -1)):
        with pytest.raises(gpu.GmgError) as e:
            gpu.window_counts(ladder_reads, W, S)
        assert e.value.code == -1                        # GMG_EINVAL
    for amb in ([5, 5], [7, 3], [total], [0, total + 3]):
        with pytest.raises(gpu.GmgError) as e:
            gpu.window_counts(ladder_reads, 10, 2, amb=amb)
        assert e.value.code == -1
    lib, h = gpu.capi.lib(), C.c_void_p()
    assert lib.gmg_window_counts(ladder_reads.h, 10, 2, None, 3, C.byref(h), None) == -1  # GMG_EINVAL: no list for three bases
    assert lib.gmg_window_counts(ladder_reads.h, 10, 2, None, 0, None, None) == -1
    want_off, want = wo.batch_window_counts(ladder, 10, 2)
    old = gpu.get_option("mg_max_entries")
    request_finalizers.append(lambda: gpu.set_option("mg_max_entries", old))
    gpu.set_option("mg_max_entries", len(want) - 1)
    with pytest.raises(gpu.GmgError) as e:
        gpu.window_counts(ladder_reads, 10, 2)
    assert e.value.code == -7                            # GMG_ETOOBIG
    gpu.set_option("mg_max_entries", len(want))
    _check(gpu, ladder_reads, ladder, 10, 2)
    gpu.set_option("mg_max_entries", old)
    assert gpu.get_option("mg_max_entries") == old


# ---- uncovered -----------------------------------------------------------------------------------------------------------------

def _check_gaps(gpu, reads, lengths, intervals, min_len=0, seed=0):
    order = np.random.default_rng(seed).permutation(len(intervals))
    shuffled = [intervals[i] for i in order]
    gaps, off = gpu.regions_uncovered(reads, shuffled, min_len)
    want, want_off = wo.batch_uncovered(lengths, intervals, min_len)
    assert [tuple(int(x) for x in g) for g in gaps] == want, min_len
    assert [int(x) for x in off] == want_off
    return gaps, off


def _many(k, L, rng):
    """k intervals in a read of L bases, some of them nested, touching or identical"""
    out = []
    for _ in range(k):
        lo = int(rng.integers(0, L + 1))
        out.append((lo, min(L, lo + int(rng.integers(0, 12)))))
    return out


@pytest.fixture(scope="module")
def gap_cases():
    rng = np.random.default_rng(31)
    L = 400
    per_read = [
        [],                                              # none
        [(0, L)],                                        # one that covers everything
        [(0, 0)], [(L, L)], [(100, 200), (250, 250), (300, 310)],      # an empty interval at 0, at L, in the middle of a gap
        [(10, 20), (20, 30), (40, 90), (50, 60), (100, 120), (100, 120), (110, 150), (130, 140)],    # touching, nested, identical, overlapping
        _many(1, L, rng), _many(63, L, rng), _many(64, L, rng), _many(65, L, rng), _many(129, L, rng),
        [], [(5, 395)], [],                              # a read with intervals between two without
        [(0, 10), (10, L)],                              # nothing left
    ]
    lengths = [L] * len(per_read) + [0, 7]               # an empty read (no gap), a short one without intervals
    seqs = [_rand_seq(rng, n) for n in lengths]
    intervals = [(r, lo, hi) for r, lst in enumerate(per_read) for lo, hi in lst]
    return seqs, lengths, intervals


def test_uncovered_cases_per_read(gpu, gap_cases):
    seqs, lengths, intervals = gap_cases
    reads = gpu.Reads.from_strings(seqs)
    gaps, off = _check_gaps(gpu, reads, lengths, intervals)
    # read 4: the empty interval splits the gap 200 .. 300 at 250
    assert [tuple(int(x) for x in g[1:3]) for g in gaps[int(off[4]):int(off[5])]] == [(0, 100), (200, 50), (250, 50), (310, 90)]
    for min_len in (1, 50, 51, 90, 91, 400, 401):        # 50, 90 and 400 are exact lengths of gaps
        _check_gaps(gpu, reads, lengths, intervals, min_len, seed=min_len)


def test_uncovered_without_intervals_and_of_an_empty_read(gpu, gap_cases):
    seqs, lengths, _ = gap_cases
    reads = gpu.Reads.from_strings(seqs)
    gaps, off = _check_gaps(gpu, reads, lengths, [])
    assert len(gaps) == sum(1 for n in lengths if n)
    gaps, off = gpu.regions_uncovered(gpu.Reads.from_strings([""]), [])
    assert len(gaps) == 0 and [int(x) for x in off] == [0, 0]


@pytest.fixture(scope="module")
def random_gaps():
    rng = np.random.default_rng(32)
    lengths = [int(n) for n in rng.integers(0, 300, size=2000)]
    seqs = [_rand_seq(rng, n, "acgtn" if i % 50 == 0 else "acgt") for i, n in enumerate(lengths)]
    intervals = []
    for r, L in enumerate(lengths):
        for _ in range(int(rng.integers(0, 7))):
            lo = int(rng.integers(0, L + 1))
            intervals.append((r, lo, int(rng.integers(lo, min(L, lo + 80) + 1))))
    return seqs, lengths, intervals


def test_uncovered_two_thousand_reads(gpu, random_gaps):
    seqs, lengths, intervals = random_gaps
    reads = gpu.Reads.from_strings(seqs)
    for min_len in (0, 30):
        _check_gaps(gpu, reads, lengths, intervals, min_len, seed=5)


def test_uncovered_result_goes_straight_into_extract(gpu, random_gaps):
    seqs, lengths, intervals = random_gaps
    reads = gpu.Reads.from_strings(seqs)
    gaps, _ = gpu.regions_uncovered(reads, intervals, 10)
    sub = reads.extract([tuple(int(x) for x in g) for g in gaps])
    packed, off = sub.download()
    want = [seqs[r][a:a + ln] for r, a, ln, _ in gaps.tolist()]
    want_packed, want_off = gpu.api.pack_strings(want)
    assert (off == want_off).all() and (packed == want_packed[:len(packed)]).all() and len(want) > 2000


def test_uncovered_error_codes(gpu, gap_cases, request_finalizers):
    seqs, lengths, intervals = gap_cases
    reads = gpu.Reads.from_strings(seqs)
    n_reads = len(seqs)
    for bad in ((n_reads, 0, 0), (0, -1, 5), (0, 6, 5), (0, 5, 401), (n_reads - 2, 0, 1), (n_reads - 1, 3, 8)):
        with pytest.raises(gpu.GmgError) as e:
            gpu.regions_uncovered(reads, intervals[:40] + [bad] + intervals[40:])
        assert e.value.code == -6 and "interval 40 " in str(e.value)        # GMG_ERANGE naming the first bad one
    lib, h = gpu.capi.lib(), C.c_void_p()
    assert lib.gmg_regions_uncovered(reads.h, None, 5, 0, C.byref(h), None) == -1        # GMG_EINVAL: no array for five intervals
    assert lib.gmg_regions_uncovered(reads.h, None, 0, 0, None, None) == -1
    want, _ = wo.batch_uncovered(lengths, intervals)
    old = gpu.get_option("mg_max_entries")
    request_finalizers.append(lambda: gpu.set_option("mg_max_entries", old))
    gpu.set_option("mg_max_entries", len(want) - 1)
    with pytest.raises(gpu.GmgError) as e:
        gpu.regions_uncovered(reads, intervals)
    assert e.value.code == -7                            # GMG_ETOOBIG
    gpu.set_option("mg_max_entries", len(want))
    _check_gaps(gpu, reads, lengths, intervals)
    gpu.set_option("mg_max_entries", old)
    assert gpu.get_option("mg_max_entries") == old
