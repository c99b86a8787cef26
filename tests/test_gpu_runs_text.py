"""gmg_runs_text on the device against the Python restatement (tests/runs_text_oracle.py), byte for byte.  The inputs are hand-made
with the kernel's shape in mind: a work-group owns 16 KiB of the text, a lane 16 bytes at a time; a lane finds the run of its first
byte by binary search and walks on run by run; a codon takes three bytes from up to three runs and either pad."""
import ctypes as C
import gc

import numpy as np
import pytest

import runs_text_oracle as ro
import splice_oracle as so

pytestmark = pytest.mark.gpu

EINVAL, ERANGE = -1, -6
UP, DOWN, SUB_UP, SUB_DOWN, LIT, AS_IS = so.UP, so.DOWN, so.SUB_UP, so.SUB_DOWN, so.LITERAL, so.LITERAL_AS_IS
ALPHABET = b"acgtACGTacgtnNrykmRYKMbdhvswBDHVSW*-"
# the last read is written by hand: upper, lower, a lower-case stop, an upper-case stop, mixed case, foreign letters
CODONS = b"ATGatgtgaTGAAcGANG*--taaTAAtagcccGGG"
LENGTHS = [1, 2, 3, 59, 61, 20000, len(CODONS)]
BIG, HAND = 5, 6
HEADS = [b"", b">", b">" + b"h" * 298 + b"\n"]
MODES = [ro.DNA, ro.PROTEIN]


@pytest.fixture(scope="module")
def batch(gpu):
    rng = np.random.default_rng(21)
    seqs = [bytes(ALPHABET[i] for i in rng.integers(0, len(ALPHABET), L)) for L in LENGTHS[:-1]] + [CODONS]
    letters = gpu.Letters(b"".join(seqs), np.cumsum([0] + LENGTHS))
    yield letters, seqs
    letters.close()


def strings_to_arrays(strings):
    """[(runs of the string, pad in front, pad behind)] -> (runs, string_run_off, pad_front, pad_behind, heads)"""
    runs = [r for s, _, _ in strings for r in s]
    sro = np.cumsum([0] + [len(s) for s, _, _ in strings]).astype(np.uint64)
    return runs, sro, [f for _, f, _ in strings], [b for _, _, b in strings], [HEADS[k % 3] for k in range(len(strings))]


def whole(r, kind):
    """the whole of read r as one run: upwards it ends at L, downwards at position 0"""
    return (r, 0 if kind in (UP, SUB_UP) else LENGTHS[r] - 1, LENGTHS[r], kind)


@pytest.fixture(scope="module")
def cases():
    s = []
    # every read whole, in every direction, and a part from its middle
    for r, L in enumerate(LENGTHS):
        for kind in (UP, DOWN, SUB_UP, SUB_DOWN):
            s.append(([whole(r, kind)], 0, 0))
            s.append(([(r, L // 2, (L + 1) // 2 if kind in (UP, SUB_UP) else L // 2 + 1, kind)], 3, 3))
    # literals and letters printed as they are, also more than once; runs of no byte of every kind, also at first = L
    for c in range(4):
        s.append(([(99, 99, c, LIT + c), (HAND, 16 + c, c + 1, AS_IS + c), (3, 58, 3, AS_IS + c)], c, 4 - c))
    s.append(([(3, 59, 0, UP), (3, 59, 0, DOWN), (3, 0, 0, SUB_DOWN), (99, 99, 0, LIT + 1), (99, 99, 0, AS_IS + 2), (3, 4, 5, UP), (3, 0, 0, SUB_UP)], 1, 1))
    s.append(([(3, 7, 0, UP)], 0, 0))
    # no runs: pads only, and nothing at all
    s += [([], 0, 0), ([], 2, 1), ([], 0, 4), ([], 3, 0), ([], 0, 0)]
    # every pad count 0 .. 4 on either side of five letters: |P| = 5 .. 13, every residue modulo 3
    for front in range(5):
        for behind in range(5):
            s.append(([(4, 10 + front, 5, UP if behind & 1 else DOWN)], front, behind))
    # codons across two and three runs (runs of one byte), pad -> run and run -> pad
    ones = [(HAND, p, 1, UP) for p in range(len(CODONS))]
    s.append((ones, 0, 0))
    s.append((ones, 1, 1))
    s.append((ones[:8], 2, 2))
    s.append(([(HAND, 0, 2, UP), (HAND, 2, 1, UP), (HAND, 5, 1, DOWN), (HAND, 4, 2, DOWN), (99, 0, 1, LIT + 0), (HAND, 1, 2, UP)], 0, 1))
    s.append(([(3, p, 1, (UP, DOWN, SUB_UP, SUB_DOWN)[p & 3]) for p in range(59)], 1, 0))
    # the hand-written codons whole: all-upper, all-lower, a lower-case stop, mixed case, foreign letters
    s.append(([whole(HAND, UP)], 0, 0))
    s.append(([whole(HAND, UP)], 3, 3))
    # records longer than a tile: three 20,000-base runs are 60,000 letters and 20,000 amino letters
    s.append(([whole(BIG, UP), whole(BIG, DOWN), whole(BIG, SUB_UP)], 0, 0))
    s.append(([whole(BIG, SUB_DOWN), (BIG, 7, 19993, UP)], 2, 0))
    return strings_to_arrays(s)


@pytest.fixture(scope="module")
def tiny():
    """5,000 records of 0 - 2 characters in either mode (0 - 8 bytes of P) with heads of 0 or 1 byte: hundreds of records in a
    tile, several in one 16-byte store"""
    rng = np.random.default_rng(22)
    out = {}
    for mode in MODES:
        s = []
        for k in range(5000):
            n = int(rng.integers(0, 3)) * (3 if mode == ro.PROTEIN else 1) + (int(rng.integers(0, 3)) if mode == ro.PROTEIN else 0)
            front = int(rng.integers(0, n + 1)) if rng.integers(0, 3) == 0 else 0
            runs, left = [], n - front
            while left and rng.integers(0, 4):
                m = int(rng.integers(0, min(left, 2) + 1))
                kind = int(rng.integers(0, 4))
                r = int(rng.integers(3, len(LENGTHS)))
                first = int(rng.integers(m, LENGTHS[r] - m))
                runs.append((r, first, m, kind))
                left -= m
            s.append((runs, front, left))
        runs, sro, front, behind, _ = strings_to_arrays(s)
        out[mode] = runs, sro, front, behind, [b">" if rng.integers(0, 2) else b"" for _ in s]
    return out


def params(gpu, mode, width, **fields):
    return gpu.runs_text_params(mode, 0, width=width, **fields), ro.Params(mode, width, **fields)


def test_the_cases_hold_what_they_are_for(batch, cases):
    _, seqs = batch
    runs, sro, front, behind, heads = cases
    prm = ro.Params(ro.DNA)
    p = [ro.printed(seqs, runs, sro, k, front[k], behind[k], prm) for k in range(len(heads))]
    assert {(f, b, len(x) % 3) for f, b, x in zip(front, behind, p)} >= {(f, b, (f + b + 5) % 3) for f in range(5) for b in range(5)}
    pads_only = [x for k, x in enumerate(p) if sro[k] == sro[k + 1]]
    assert {len(x) % 3 for x in p} == {0, 1, 2} and b"" in pads_only and b"   " in pads_only
    assert any(r[2] == 0 for r in runs) and any(r[3] >= AS_IS and r[2] > 1 for r in runs) and {r[3] for r in runs} == set(range(12))
    assert any(r[3] == UP and r[1] + r[2] == LENGTHS[r[0]] for r in runs) and any(r[3] == DOWN and r[2] == r[1] + 1 for r in runs)
    assert not any(ro.bad_run(LENGTHS, r) for r in runs)
    faa = b"".join(ro.translate(x, ro.Params(ro.PROTEIN)) for x in p)
    assert b"M" in faa and b"m" in faa and b"X" in faa and b"*" in faa
    whole_hand = ro.translate(CODONS, ro.Params(ro.PROTEIN))
    assert whole_hand == b"Mm**XXX***pG" and CODONS[6:9] == b"tga" and CODONS[21:24] == b"taa"
    assert max(len(x) for x in p) == 60000 > 3 * 16384 and max(len(x) // 3 for x in p) == 20000 > 16384


@pytest.mark.parametrize("width", [0, 1, 7, 60])
@pytest.mark.parametrize("mode", MODES)
def test_text_equals_the_restatement(gpu, batch, cases, mode, width):
    letters, seqs = batch
    runs, sro, front, behind, heads = cases
    prm, want_prm = params(gpu, mode, width)
    want = ro.text(seqs, runs, sro, heads, want_prm, front, behind)
    got = letters.runs_text(runs, sro, heads, prm, front, behind)
    assert len(got) == len(want) > 2 * 16384
    if got != want:
        at = next(i for i in range(len(want)) if got[i] != want[i])
        raise AssertionError("first difference at byte %d: got %r, want %r" % (at, got[at - 20:at + 20], want[at - 20:at + 20]))


@pytest.mark.parametrize("width", [0, 1, 60])
@pytest.mark.parametrize("mode", MODES)
def test_many_tiny_records(gpu, batch, tiny, mode, width):
    letters, seqs = batch
    runs, sro, front, behind, heads = tiny[mode]
    prm, want_prm = params(gpu, mode, width)
    want = ro.text(seqs, runs, sro, heads, want_prm, front, behind)
    assert want.count(b"\n") >= 5000 and len(want) < 5000 * 6
    assert letters.runs_text(runs, sro, heads, prm, front, behind) == want


@pytest.mark.parametrize("mode", MODES)
def test_every_total_length_modulo_16(gpu, batch, mode):
    """the buffer's last, partial 16 bytes go byte by byte: one record whose head grows by a byte at a time"""
    letters, seqs = batch
    runs, sro = [(4, 0, 61, UP), (4, 60, 61, DOWN)], [0, 1, 2]
    prm, want_prm = params(gpu, mode, 7)
    seen = set()
    for extra in range(16):
        heads = [b">a\n", b">" + b"b" * extra]
        want = ro.text(seqs, runs, sro, heads, want_prm, [1, 0], [0, 2])
        seen.add(len(want) % 16)
        assert letters.runs_text(runs, sro, heads, prm, [1, 0], [0, 2]) == want
    assert seen == set(range(16))


def test_tables_are_the_callers(gpu, batch, cases):
    """every table and byte of the parameters is applied as given: a marker for every letter read downwards, shifted tables for
    the substitutions, other literals, another pad, an amino table of its own and another letter for an unknown codon"""
    letters, seqs = batch
    runs, sro, front, behind, heads = cases
    fields = dict(up=bytes(ord(chr(c).upper()) if c < 128 else c for c in range(256)), down=b"x" * 256,
                  sub_up=bytes((c + 1) & 255 for c in range(256)), sub_down=bytes((c + 2) & 255 for c in range(256)), literal=b"TGCA", pad=ord("."),
                  unknown=ord("?"))
    for mode in MODES:
        prm, want_prm = params(gpu, mode, 60, aa=bytes(range(64, 128)), **fields)
        want = ro.text(seqs, runs, sro, heads, want_prm, front, behind)
        assert b"?" in want if mode == ro.PROTEIN else (b"x" * 60 in want and b"..." in want)
        assert letters.runs_text(runs, sro, heads, prm, front, behind) == want


def test_device_resident_text_equals_the_host_text(gpu, batch, cases):
    letters, seqs = batch
    runs, sro, front, behind, heads = cases
    for mode in MODES:
        prm, want_prm = params(gpu, mode, 60)
        ptr, size = letters.runs_text_device(runs, sro, heads, prm, front, behind)
        on_device = gpu.memcpy_d2h(ptr, size)
        assert letters.kernel_ms() > 0.0
        assert on_device == ro.text(seqs, runs, sro, heads, want_prm, front, behind) == letters.runs_text(runs, sro, heads, prm, front, behind)


def with_string(runs, sro, k, extra):
    """the arrays with one more string, made of the runs `extra`, in front of string k"""
    at = int(sro[k])
    sro = [int(x) for x in sro]
    return list(runs[:at]) + list(extra) + list(runs[at:]), sro[:k + 1] + [x + len(extra) for x in sro[k:]]


def test_api_edges(gpu, batch, cases):
    letters, seqs = batch
    runs, sro, front, behind, heads = cases
    prm, want_prm = params(gpu, ro.PROTEIN, 60)
    want = ro.text(seqs, runs, sro, heads, want_prm, front, behind)
    # no string: no byte, on either variant
    assert letters.runs_text([], [0], [], prm) == b"" and letters.runs_text_size([], [0], [], prm) == 0
    assert letters.runs_text_device([], [0], [], prm)[1] == 0
    # NULL pad arrays mean 0
    assert letters.runs_text(runs, sro, heads, prm) == ro.text(seqs, runs, sro, heads, want_prm)
    # host_out NULL: the length only
    assert letters.runs_text_size(runs, sro, heads, prm, front, behind) == len(want)
    # one byte short: GMG_ERANGE, the length reported in the message, the buffer untouched
    buf = np.full(len(want) - 1, 0xAA, np.uint8)
    with pytest.raises(gpu.GmgError) as e:
        letters.runs_text(runs, sro, heads, prm, front, behind, out=buf)
    assert e.value.code == ERANGE and str(len(want)) in str(e.value) and np.all(buf == 0xAA)
    # exactly enough is enough
    buf = np.full(len(want), 0xAA, np.uint8)
    assert letters.runs_text(runs, sro, heads, prm, front, behind, out=buf) == len(want) and buf.tobytes() == want
    # every kind of bad run in the middle of the list is named, nothing is written
    mid = len(heads) // 2
    n_reads = len(LENGTHS)
    bad_runs = [(n_reads, 0, 1, UP), (n_reads, 0, 0, DOWN), (3, 59, 1, UP), (3, 1, 59, SUB_UP), (3, 60, 0, UP), (3, 0, 2, DOWN), (3, 59, 1, DOWN),
                (3, 60, 0, SUB_DOWN), (3, 58, 60, SUB_DOWN), (3, 0, 1, 12), (3, 0, 0, 0xffffffff), (3, 59, 1, AS_IS), (n_reads, 0, 2, AS_IS + 3),
                (0, 0xffffffff, 2, UP), (3, 0xffffffff, 0xffffffff, DOWN)]
    for bad in bad_runs:
        assert ro.bad_run(LENGTHS, bad), bad
        r2, sro2 = with_string(runs, sro, mid, [(3, 0, 1, UP), bad])
        buf = np.full(len(want) + 400, 0xAA, np.uint8)
        with pytest.raises(gpu.GmgError) as e:
            letters.runs_text(r2, sro2, heads[:mid] + [b""] + heads[mid:], prm, front[:mid] + [0] + front[mid:], behind[:mid] + [0] + behind[mid:], out=buf)
        assert e.value.code == ERANGE and "run %d " % (int(sro[mid]) + 1) in str(e.value), str(e.value)
        assert np.all(buf == 0xAA)
    # a string of 2^32 characters, pads included
    for extra, pad in (([(0, 0, 0x80000000, LIT), (0, 0, 0x80000000, LIT + 1)], 0), ([(0, 0, 0xfffffffe, LIT)], 2)):
        r2, sro2 = with_string(runs, sro, mid, extra)
        with pytest.raises(gpu.GmgError) as e:
            letters.runs_text_size(r2, sro2, heads[:mid] + [b""] + heads[mid:], prm, front[:mid] + [pad] + front[mid:], behind[:mid] + [0] + behind[mid:])
        assert e.value.code == ERANGE and "string %d " % mid in str(e.value), str(e.value)
    # string_run_off that descends or does not end at n_runs; a mode that is none; a reserved byte
    for bad_sro in ([0, 2, 1, len(runs)], [0, len(runs) - 1], [1, len(runs)], [0, len(runs) + 1]):
        with pytest.raises(gpu.GmgError) as e:
            letters.runs_text(runs, bad_sro, [b""] * (len(bad_sro) - 1), prm)
        assert e.value.code == EINVAL
    for field, value in (("mode", 2), ("reserved", (C.c_uint8 * 2)(0, 1))):
        p2, _ = params(gpu, ro.DNA, 60)
        setattr(p2, field, value)
        with pytest.raises(gpu.GmgError) as e:
            letters.runs_text(runs, sro, heads, p2, front, behind)
        assert e.value.code == EINVAL


def test_the_recorded_cases_on_the_device(gpu):
    """the four recorded runs of extract_aa.py through the API: the .ffn and the .faa file the script wrote"""
    for name in sorted(so.CASES):
        seqs, runs, sro, heads, front, behind = ro.case_inputs(gpu, name)
        letters = gpu.Letters(b"".join(seqs), so.offsets(seqs))
        so.assert_recorded(name, ".ffn", letters.runs_text(runs, sro, heads, gpu.runs_text_params(ro.DNA), front, behind))
        so.assert_recorded(name, ".faa", letters.runs_text(runs, sro, heads, gpu.runs_text_params(ro.PROTEIN), front, behind))
        letters.close()


def test_nothing_stays_behind(gpu, batch):
    """a handle that wrote texts of growing size and met refusals, freed: the cache's busy blocks and the handles' own blocks are
    back where they started"""
    _, seqs = batch

    def counts():
        gc.collect()
        assert gpu.capi.lib().gmg_synchronize(None) == 0
        stats, owned = (C.c_uint64 * 4)(), C.c_uint64()
        assert gpu.capi.lib().gmg_debug_cache_stats(stats) == 0 and gpu.capi.lib().gmg_debug_owned_blocks(C.byref(owned)) == 0
        return int(stats[0]), int(owned.value)

    before = counts()
    letters = gpu.Letters(b"".join(seqs), np.cumsum([0] + LENGTHS))
    assert counts() != before                            # (the counters see the handle's blocks)
    for runs in ([whole(3, UP)], [whole(BIG, UP), whole(BIG, DOWN)]):
        for mode in MODES:
            prm = gpu.runs_text_params(mode)
            text = letters.runs_text(runs, [0, len(runs)], [b">g\n"], prm, [1], [2])
            ptr, size = letters.runs_text_device(runs, [0, len(runs)], [b">g\n"], prm, [1], [2])
            assert size == len(text) and gpu.memcpy_d2h(ptr, size) == text
    with pytest.raises(gpu.GmgError):
        letters.runs_text([(3, 59, 1, UP)], [0, 1], [b""], prm)
    with pytest.raises(gpu.GmgError):
        letters.runs_text([whole(BIG, UP)], [0, 1], [b""], prm, capacity=10)
    letters.close()
    assert counts() == before
