"""gmg_genes_audit on the device (glimmer-mg_amd/csrc/gmg_audit.hip; include/gmg.h) against the Python restatement of what
anomaly and start-codon-distrib read off a gene (tests/audit_oracle.py).  Every output is an integer: all comparisons are exact.
Shapes are the smallest at which the kernel can go wrong: the 64-codon ballot step's edges, reads shorter than a step packed back to
back, regions on the last base, codons across the 16-base words of the packing."""
import ctypes as C

import numpy as np
import pytest

import audit_oracle as ao

pytestmark = pytest.mark.gpu

FIELDS = ("first_codon", "last_codon", "start_which", "stop_which", "n_inner_stops", "inner_begin", "last_back_stop", "next_stop")
STARTS, STOPS = ("atg", "gtg", "ttg"), ("taa", "tag", "tga")


def _rand_seq(rng, n, alphabet="acgt"):
    return "".join(alphabet[c] for c in rng.integers(0, len(alphabet), size=int(n)))


def _revcomp(s):
    return "".join(ao.COMP[c] for c in reversed(s))


def _check(gpu, seqs, regions, starts=STARTS, stops=STOPS, flags=1, reads=None, stream=None):
    reads = reads or gpu.Reads.from_strings(seqs)
    amb = ao.ambiguous_bases(seqs)
    rec, inner, hist = gpu.genes_audit(reads, regions, starts, stops, flags, amb=amb, stream=stream)
    want, want_inner, want_hist = ao.audit_records(seqs, regions, starts, stops, bool(flags & 1))
    assert len(rec) == len(want)
    for f in FIELDS:
        got = [int(x) for x in rec[f]]
        exp = [w[f] for w in want]
        if got != exp:
            k = next(i for i in range(len(got)) if got[i] != exp[i])
            raise AssertionError("%s of region %d %r: device %d, restatement %d" % (f, k, tuple(regions[k]), got[k], exp[k]))
    assert [int(x) for x in inner] == want_inner
    assert [int(x) for x in hist] == want_hist
    return rec, inner, hist


@pytest.fixture(scope="module")
def short_reads():
    """reads of 3 .. 70 bases back to back (no padding between them), a stop codon planted straight across every boundary: a read
    that is not taken modulo itself sees it"""
    rng = np.random.default_rng(11)
    seqs = [list(_rand_seq(rng, n)) for n in range(3, 71)]
    for a, b in zip(seqs, seqs[1:]):
        a[-2:] = "ta"
        b[0] = "ag"[len(a) & 1]
    seqs = ["".join(s) for s in seqs]
    regions = []
    for r, s in enumerate(seqs):
        L = len(s)
        for ln in sorted({3, 4, 5, 6, 7, L - 1, L}):
            if ln > L:
                continue
            for first in sorted({0, L // 2, L - 1}):
                regions += [(r, first, ln, 1), (r, first, ln, -1)]
    return seqs, regions


def test_short_reads_back_to_back(gpu, short_reads):
    """len in {3, 4, 5, 6, 7, L - 1, L} on reads of every length 3 .. 70 (L = 3 included), both strands, starting on base 0, in the
    middle and on the last base"""
    seqs, regions = short_reads
    rec, _, _ = _check(gpu, seqs, regions)
    assert (rec["next_stop"] >= 0).any() and (rec["n_inner_stops"] > 0).any() and (rec["last_back_stop"] >= 0).any()


def test_unsorted_and_repeated_regions(gpu, short_reads):
    seqs, regions = short_reads
    rng = np.random.default_rng(12)
    pick = [regions[i] for i in rng.integers(0, len(regions), size=700)]
    _check(gpu, seqs, pick + pick[:50])


def test_codons_across_the_packed_words(gpu):
    rng = np.random.default_rng(13)
    seqs = [_rand_seq(rng, 7), _rand_seq(rng, 200, "atg")]            # (read 1 starts at job-wide base 7: no word is aligned with it)
    regions = [(1, f, ln, s) for f in list(range(5, 28)) + list(range(40, 60)) for ln in (9, 10, 36) for s in (1, -1)]
    _check(gpu, seqs, regions)


def test_ambiguous_letters_in_every_codon_position(gpu):
    """an n / R / y in each position of the first, an inner and the last codon, on both strands: such a codon is no start, no stop and
    has the code -1, as the reference's comparison of raw letters gives"""
    gene = "atg" + "ccc" + "taa" + "ggg" + "tga"
    seqs, regions = [], []
    for codon in (0, 2, 4):
        for pos in range(3):
            for letter in "nRy":
                s = list(gene)
                s[3 * codon + pos] = letter
                for strand in (1, -1):
                    seqs.append("".join(s) if strand > 0 else "cc" + _revcomp("".join(c if c in "acgt" else "a" for c in s)) + "c")
                    if strand < 0:                                   # the same letter at the same region offset on the reverse strand
                        t = list(seqs[-1])
                        t[2 + len(gene) - 1 - (3 * codon + pos)] = letter
                        seqs[-1] = "".join(t)
                    r = len(seqs) - 1
                    regions.append((r, 0, len(gene), 1) if strand > 0 else (r, 2 + len(gene) - 1, len(gene), -1))
                    regions.append((r, 0, len(gene) - 1, 1) if strand > 0 else (r, 2 + len(gene) - 1, len(gene) - 1, -1))
    seqs.append(gene)
    regions.append((len(seqs) - 1, 0, len(gene), 1))
    rec, inner, hist = _check(gpu, seqs, regions)
    assert hist[64] == 2 * 2 * 3 * 3                                 # the first codon's 3 positions x 3 letters x 2 strands x 2 lengths
    assert rec[-1]["n_inner_stops"] == 1 and rec[-1]["first_codon"] == 14 and rec[-1]["stop_which"] == 2


def test_only_in_frame_stops_count(gpu):
    body = list("atg" + "cgc" * 40 + "tga")
    for off in (9, 30, 63):                                          # frame 0
        body[off:off + 3] = "taa"
    for off in (13, 46, 100):                                        # frame 1
        body[off:off + 3] = "tag"
    for off in (20, 77):                                             # frame 2
        body[off:off + 3] = "tga"
    s = "".join(body)
    seqs = [s, "g" + _revcomp(s) + "gg"]
    L = len(s)
    regions = []
    for cut in range(0, 7):
        for start in (0, 1, 2):
            regions += [(0, start, L - start - cut, 1), (1, L - start, L - start - cut, -1)]
    rec, inner, _ = _check(gpu, seqs, regions)
    assert [int(x) for x in inner[:3]] == [9, 30, 63] and rec[0]["n_inner_stops"] == 3


@pytest.mark.parametrize("m", [0, 1, 63, 64, 65, 129])
def test_inner_stop_counts_at_the_ballot_steps_edges(gpu, m):
    """exactly m inner stops, with the hits ending on lane 62 / 63 of a step, lane 0 of the next, and in a third step"""
    s = "atg" + "taa" * m + "ccc" + "tga"
    seqs = ["ac", s, "g" + _revcomp(s)]
    L = len(s)
    regions = [(1, 0, L, 1), (2, L, L, -1), (1, 0, L - 1, 1), (1, 0, L - 2, 1), (1, 0, L - 3, 1), (2, L, L - 3, -1), (1, 3, L - 3, 1)]
    rec, inner, _ = _check(gpu, seqs, regions)
    assert rec["n_inner_stops"][0] == m and rec["n_inner_stops"][1] == m
    assert rec["last_back_stop"][0] == (3 * m if m else -1)
    assert rec["n_inner_stops"][4] == m and rec["stop_which"][4] == -1     # cut before tga: ccc is the last codon


def test_stops_at_len_minus_6_and_len_minus_3(gpu):
    s = "atgccctaatga"
    seqs = [s, _revcomp(s), "atg" + "c" * 10 + "tga" + "ccc"]
    regions = [(0, 0, 12, 1), (1, 11, 12, -1), (0, 0, 9, 1), (2, 0, 19, 1), (2, 0, 18, 1), (2, 0, 17, 1)]
    rec, inner, _ = _check(gpu, seqs, regions)
    assert rec["n_inner_stops"][0] == 1 and inner[0] == 6 and rec["last_back_stop"][0] == 6 and rec["stop_which"][0] == 2
    assert rec["stop_which"][2] == 0 and rec["n_inner_stops"][2] == 0
    assert rec["last_back_stop"][3] == 13 and rec["n_inner_stops"][3] == 0             # 19 - 6: the other frame's stop (tga)


def test_next_stop_positions(gpu):
    """at j = len, at the last admissible j (reached only through the wrap: its codon ends on the read's first base), absent, and
    after several steps of 64 codons; both strands"""
    at_len = "atgccc" + "taa" + "c" * 11
    last_j = "a" + "c" * 17 + "ta"                                   # L = 20, len = 6: j = 18 reads t a + base 0
    none = "c" * 40
    far = "atgccc" + "c" * 2988 + "taa" + "ccc"                       # L = 3000: j = 2994 in the 16th step
    mid = "c" + "taa" + "ccccc" + "atgccc" + "cc"                      # first = 9: the walk wraps before it finds the stop at base 1
    seqs = [at_len, last_j, none, far, mid]
    regions = [(0, 0, 6, 1), (1, 0, 6, 1), (2, 0, 6, 1), (2, 5, 7, -1), (3, 0, 6, 1), (4, 9, 6, 1), (3, 3, 6, 1), (3, 4, 5, 1)]
    for r in (0, 1, 3, 4):
        seqs.append("gg" + _revcomp(seqs[r]))
        L = len(seqs[r])
        regions.append((len(seqs) - 1, (2 + L - 1 - (9 if r == 4 else 0)), 6, -1))
    rec, _, _ = _check(gpu, seqs, regions)
    assert [int(x) for x in rec["next_stop"][:6]] == [6, 18, -1, -1, 2994, 9]
    flagless, _, _ = _check(gpu, seqs, regions, flags=0)
    assert (flagless["next_stop"] == -1).all()


def test_custom_codon_lists(gpu, short_reads):
    seqs, regions = short_reads
    _check(gpu, seqs, regions[::3], starts=("atg",), stops=("tag", "tga"))
    _check(gpu, seqs, regions[::5], starts=("ctg", "atg", "ctg"), stops=("taa", "taa", "tcc", "aaa", "ttt", "acg", "gca", "cat"))
    _check(gpu, seqs, regions[::7], starts=(), stops=())


def test_no_regions(gpu, short_reads):
    rec, inner, hist = _check(gpu, short_reads[0], [])
    assert len(rec) == 0 and len(inner) == 0 and not hist.any()


def test_many_regions_of_one_read_and_many_reads_of_one_region(gpu):
    rng = np.random.default_rng(14)
    one = [_rand_seq(rng, 331)]
    regions = [(0, int(f), int(ln), 1 if s else -1) for f, ln, s in
               zip(rng.integers(0, 331, 5000), rng.integers(0, 120, 5000), rng.integers(0, 2, 5000))]
    _check(gpu, one, regions, flags=0)
    many = [_rand_seq(rng, n) for n in rng.integers(20, 45, 5000)]
    regions = [(r, int(rng.integers(0, len(s))), int(rng.integers(3, len(s) + 1)), 1 if r & 1 else -1) for r, s in enumerate(many)]
    _check(gpu, many, regions)


def test_histogram_with_every_region_on_one_codon(gpu):
    rng = np.random.default_rng(15)
    seqs = ["atg" + _rand_seq(rng, 30) for _ in range(40)]
    regions = [(r % 40, 0, 3 + r % 28, 1) for r in range(1500)]
    _, _, hist = _check(gpu, seqs, regions, flags=0)
    assert hist[14] == 1500 and hist.sum() == 1500


def test_too_many_inner_stops_is_refused_not_truncated(gpu):
    seqs = ["atg" + "taa" * 5 + "ccctga"]
    reads = gpu.Reads.from_strings(seqs)
    regions = [(0, 0, len(seqs[0]), 1)] * 2                           # 10 inner stops
    with gpu.option("mg_max_entries", 9):
        with pytest.raises(gpu.GmgError) as e:
            gpu.genes_audit(reads, regions)
        assert e.value.code == -7 and "10 inner stop codons" in str(e.value)
    with gpu.option("mg_max_entries", 10):
        rec, inner, _ = gpu.genes_audit(reads, regions)
        assert len(inner) == 10 and list(rec["inner_begin"]) == [0, 5]


def test_regions_that_do_not_fit_name_the_first_one(gpu):
    reads = gpu.Reads.from_strings(["acgtacgtac", "acg"])
    good = (0, 9, 10, -1)
    for bad in ((0, 10, 3, 1), (0, -1, 3, 1), (1, 0, 4, 1), (0, 0, -1, 1), (0, 0, 3, 0), (2, 0, 1, 1)):
        with pytest.raises(gpu.GmgError) as e:
            gpu.genes_audit(reads, [good, good, bad, bad])
        assert e.value.code == -6 and "region 2 " in str(e.value)
    for prm in (dict(start_codons=("ATG",)), dict(stop_codons=("ta",)), dict(stop_codons=("tan",)), dict(start_codons=("atgc",)),
                dict(flags=2), dict(stop_codons=("taa",) * 9)):
        with pytest.raises(gpu.GmgError) as e:
            gpu.genes_audit(reads, [good], **prm)
        assert e.value.code == -1
    for amb in ([3, 3], [5, 2], [13]):
        with pytest.raises(gpu.GmgError) as e:
            gpu.genes_audit(reads, [good], amb=amb)
        assert e.value.code == -1


def test_on_a_caller_stream(gpu, short_reads):
    seqs, regions = short_reads
    lib = gpu.capi.lib()
    stream = C.c_void_p()
    gpu.api._ck(lib.gmg_stream_create(C.byref(stream)))
    try:
        _check(gpu, seqs, regions[:600], stream=stream)
    finally:
        gpu.api._ck(lib.gmg_synchronize(stream))
        gpu.api._ck(lib.gmg_stream_destroy(stream))


def test_two_calls_back_to_back_do_not_depend_on_the_block_cache(gpu, short_reads):
    """a call with long lists first, so that the cache holds blocks full of its offsets; then the same small call with those blocks
    around and with an emptied cache"""
    seqs, regions = short_reads
    big = ["atg" + "taa" * 300 + "ccctga"]
    _check(gpu, big, [(0, 0, len(big[0]), 1)] * 64)
    reads = gpu.Reads.from_strings(seqs)
    first = _check(gpu, seqs, regions[:500], reads=reads)
    second = _check(gpu, seqs, regions[:500], reads=reads)
    assert gpu.capi.lib().gmg_trim_cache() == 0
    third = _check(gpu, seqs, regions[:500], reads=reads)
    for a, b in ((first, second), (first, third)):
        assert all(np.array_equal(x, y) for x, y in zip(a, b))
