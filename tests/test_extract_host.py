"""The host side of gmg_reads_extract (include/gmg.h; no GPU needed): gmg_extract_plan against recorded outputs of the reference's
extract / multi-extract (tests/golden/extract: the text, or the digest of every record where no test needs the text; made from the coordinate files beside them), gmg_fasta_ambiguous against a
Python restatement, and the rule for ambiguity letters on the reverse strand closed in pure Python against the recorded text."""
import collections
import os

import numpy as np
import pytest

import extract_oracle as xo
from conftest import DATA

EX = xo.EX
ERANGE, EINVAL = -6, -1


@pytest.fixture(scope="module")
def genome():
    data = open(os.path.join(DATA, "NC_000915.fna"), "rb").read()
    recs = xo.records(data)
    assert len(recs) == 1
    return data, recs[0][1]


@pytest.fixture(scope="module")
def slice2000():
    data = open(os.path.join(EX, "slice2000.fna"), "rb").read()
    return data, xo.records(data)[0][1]


def _plan_vs_recorded(gmg, seq, coords_file, out_file, flags, min_len=0):
    coords = xo.parse_coords(os.path.join(EX, coords_file))
    rows = [(0,) + c[1:] for c in coords]
    regions, line = gmg.extract_plan([0, len(seq)], rows, flags, min_len)
    want = xo.recorded(out_file)
    assert len(regions) == len(want)
    assert list(line) == sorted(line) and len(set(line.tolist())) == len(line)
    for (read, first, n, strand), k, (hdr, length, digest) in zip(regions, line, want):
        assert read == 0 and hdr[0] == coords[int(k)][0]
        assert length == n, hdr
        assert xo.sha(xo.region_chars(seq, first, n, strand)) == digest, hdr
    return regions


@pytest.mark.parametrize("out_file,flag_names,min_len", [
    ("nc_subset.sha256", (), 0), ("nc_subset.t.out", ("COORD_SKIP_STOP",), 0),
    ("nc_subset.s_t_l300.sha256", ("COORD_SKIP_START", "COORD_SKIP_STOP"), 300), ("nc_subset.w.sha256", ("COORD_NOWRAP",), 0),
    ("nc_subset.d.sha256", ("COORD_USE_DIR",), 0)])
def test_plan_matches_extract_on_the_genome(gmg, genome, out_file, flag_names, min_len):
    """15 lines of NC_000915.longorfs (every 250th and all that touch an IUPAC letter; the frame column serves as -d's direction)"""
    flags = sum(getattr(gmg, f) for f in flag_names)
    regions = _plan_vs_recorded(gmg, genome[1], "nc_subset.coords", out_file, flags, min_len)
    assert len(regions) == 15 and {r[3] for r in regions} == {1, -1}


@pytest.mark.parametrize("coords,out_file,flag_names,min_len,n", [
    ("slice_wrap.coords", "slice_wrap.out", (), 0, 14), ("slice_wrap.coords", "slice_wrap.t.sha256", ("COORD_SKIP_STOP",), 0, 11),
    ("slice_wrap.coords", "slice_wrap.s.sha256", ("COORD_SKIP_START",), 0, 11),
    ("slice_wrap.coords", "slice_wrap.w_l3.sha256", ("COORD_NOWRAP",), 3, 13),
    ("slice_dir.coords", "slice_dir.d.sha256", ("COORD_USE_DIR",), 0, 8),
    ("slice_dir.coords", "slice_dir.d_s_t.sha256", ("COORD_USE_DIR", "COORD_SKIP_START", "COORD_SKIP_STOP"), 0, 8)])
def test_plan_matches_extract_on_wraparound_coordinates(gmg, slice2000, coords, out_file, flag_names, min_len, n):
    """hand-made coordinates on a 2,000-base slice: both directions across the origin, the two halves of the direction rule, one
    base, lines that -s / -t / -l drop, -s on the reverse strand (the start moves down), -d against the coordinates' own order"""
    flags = sum(getattr(gmg, f) for f in flag_names)
    regions = _plan_vs_recorded(gmg, slice2000[1], coords, out_file, flags, min_len)
    assert len(regions) == n
    if "COORD_NOWRAP" not in flag_names:                 # (under -w no line of this file crosses the origin)
        assert any(f + ln > 2000 for _, f, ln, s in regions if s > 0) and any(f - ln + 1 < 0 for _, f, ln, s in regions if s < 0)


@pytest.mark.parametrize("out_file,flag_names,min_len", [
    ("seqs_multi.t.out", ("COORD_SKIP_STOP",), 0), ("seqs_multi.s_l60.sha256", ("COORD_SKIP_START",), 60)])
def test_plan_matches_multi_extract(gmg, out_file, flag_names, min_len):
    """multi-extract on seqs.fa: every record whose first header token equals the tag takes part, a tag without a record is skipped;
    compared as multisets per tag (std::sort leaves the order within a tag open)"""
    data = open(os.path.join(DATA, "seqs.fa"), "rb").read()
    recs = xo.records(data)
    off = np.concatenate([[0], np.cumsum([len(s) for _, s in recs])]).astype(np.uint64)
    by_tag = collections.defaultdict(list)
    for k, (h, _) in enumerate(recs):
        by_tag[h.split()[0].decode()].append(k)
    coords = xo.parse_coords(os.path.join(EX, "seqs_multi.coords"), multi=True)
    rows, ids = [], []
    for c in coords:
        for k in by_tag.get(c[1], ()):
            rows.append((k,) + c[2:])
            ids.append(c)
    assert any(c[1] not in by_tag for c in coords)
    flags = gmg.COORD_MULTI + sum(getattr(gmg, f) for f in flag_names)
    regions, line = gmg.extract_plan(off, rows, flags, min_len)
    got = collections.defaultdict(collections.Counter)
    for (read, first, n, strand), k in zip(regions, line):
        got[ids[int(k)][1]][(ids[int(k)][0], n, xo.sha(xo.region_chars(recs[read][1], first, n, strand)))] += 1
    want = collections.defaultdict(collections.Counter)
    for hdr, length, digest in xo.recorded(out_file):
        want[hdr[1]][(hdr[0], length, digest)] += 1
    assert got == want and sum(sum(c.values()) for c in want.values()) == len(regions) > 10


def test_multi_order_of_the_length_tests(gmg):
    """extract tests the length before and after the cuts of -s / -t, multi-extract only after them.  The cuts only shorten, so a
    line the first test drops is dropped by the second as well: the two orders keep the same lines.  Pinned here on lines of 8
    and 4 bases, both strands, with min_len around the full and the cut length (a cut length below 0 gives an empty region)"""
    off = [0, 100]
    for min_len in (-5, -2, 0, 2, 3, 8, 9):
        for rows in ([(0, 10, 17)], [(0, 17, 10)], [(0, 10, 13)]):
            flags = gmg.COORD_SKIP_START + gmg.COORD_SKIP_STOP
            a = gmg.extract_plan(off, rows, flags, min_len)[0]
            b = gmg.extract_plan(off, rows, flags + gmg.COORD_MULTI, min_len)[0]
            assert a == b
            full = 1 + abs(rows[0][2] - rows[0][1])
            assert len(a) == (1 if full - 6 >= min_len else 0)
            if a:
                assert a[0][2] == max(full - 6, 0)


def test_plan_refusals(gmg):
    """GMG_ERANGE naming the line: a read beyond the batch, an empty sequence, a start that one wrap does not bring onto the
    sequence (either side), a length above the sequence's (the reference walks round the circle again)"""
    off = [0, 250, 250, 600]
    good = (0, 10, 60)
    for bad, flags in [((3, 10, 60), 0), ((1, 1, 1), 0), ((0, 2 * 250 + 5, 2 * 250 + 40), 0), ((0, -250 - 5, -250 + 20), 0),
                       ((0, 1, 255, 1), "COORD_USE_DIR"), ((0, 300, 10, -1), "COORD_USE_DIR")]:
        fl = getattr(gmg, flags) if flags else 0
        with pytest.raises(gmg.GmgError) as e:
            gmg.extract_plan(off, [good, good, bad], fl)
        assert e.value.code == ERANGE and "line 2" in str(e.value), (bad, str(e.value))
    # the neighbours of every refusal are fine: one wrap on either side, the full circle
    regions, _ = gmg.extract_plan(off, [(0, 251, 255, 1), (0, 0, 3, 1), (0, 1, 250, 1), (2, 100, 200, -1)], gmg.COORD_USE_DIR)
    assert regions == [(0, 0, 5, 1), (0, 249, 4, 1), (0, 0, 250, 1), (2, 99, 251, -1)]
    with pytest.raises(gmg.GmgError) as e:
        gmg.extract_plan(off, [good], 32)
    assert e.value.code == EINVAL


def test_ambiguous_on_nasty_and_handmade_files(gmg):
    """gmg_fasta_ambiguous against the restatement: bytes before the first '>', a record that begins inside a line, '>' inside a
    header, both cases, digits and punctuation; d h r y come with the code complement, every other listed letter does not"""
    hand = (b"nnnn junk\n>r1 x\nacgtNACGTn\nRYKM>r2>y\nryswkmbdhvn\r\nRYSWKMBDHVN*-.0\n>e\n>last\nuUxX acgt")
    for data in (open(os.path.join(DATA, "nasty.fa"), "rb").read(), hand, b"", b"no record at all", b">only a header"):
        base, rev = gmg.fasta_ambiguous(data)
        wb, wr = xo.ambiguous(data)
        assert np.array_equal(base, wb) and np.array_equal(rev, wr)
    base, rev = gmg.fasta_ambiguous(hand)
    seq = "".join(s for _, s in xo.records(hand))
    assert [seq[int(b)] for b in base[:6]] == list("NnRYKM") and base[0] == 4
    for b, r in zip(base, rev):
        ch = seq[int(b)].lower()
        assert (int(r) == 3 - xo.code(ch)) == (ch in "dhry"), ch
    assert {seq[int(b)].lower() for b in base} >= set("dhryswkmbvnux*-.0")
    n = gmg.capi.C.c_uint64()
    one_b, one_r = np.zeros(1, np.uint64), np.zeros(1, np.uint8)                # cap below the count: counted, not written
    assert gmg.capi.lib().gmg_fasta_ambiguous(hand, len(hand), one_b.ctypes.data, one_r.ctypes.data, 1, gmg.capi.C.byref(n)) == 0
    assert n.value == len(base) and one_b[0] == base[0] and one_r[0] == rev[0]


def test_ambiguous_on_the_genome(gmg, genome):
    base, rev = gmg.fasta_ambiguous(genome[0])
    assert len(base) == 42 and np.all(np.diff(base.astype(np.int64)) > 0)
    assert np.array_equal(rev, [xo.code(xo.complement(genome[1][int(b)])) for b in base])


def test_rule_closes_against_recorded_extract(gmg, genome):
    """pure Python: code-space extraction plus the list reproduces Subscript of the recorded `extract -t` letters for every region
    of the subset; without the list exactly the reverse-strand regions with an effective patch differ (the four of
    NC_000915.longorfs are all in the subset)"""
    seq = genome[1]
    codes = [xo.code(ch) for ch in seq]
    base, rev = xo.ambiguous(genome[0])
    patches = {int(b): int(r) for b, r in zip(base, rev)}
    coords = xo.parse_coords(os.path.join(EX, "nc_subset.coords"))
    regions, _ = gmg.extract_plan([0, len(seq)], [(0,) + c[1:3] for c in coords], gmg.COORD_SKIP_STOP)
    want = xo.parse_out(os.path.join(EX, "nc_subset.t.out"))
    differ, touched = [], 0
    for k, ((_, first, n, strand), (_, text)) in enumerate(zip(regions, want)):
        sub = [xo.code(ch) for ch in text]
        assert xo.region_codes(codes, first, n, strand, patches) == sub, k
        plain = xo.region_codes(codes, first, n, strand)
        touched += any(ch not in "acgtACGT" for ch in text)
        if plain != sub:
            assert strand < 0
            differ.append((k, sum(a != b for a, b in zip(plain, sub))))
    assert touched == 10 and len(differ) == 4 and sum(d for _, d in differ) == 5
