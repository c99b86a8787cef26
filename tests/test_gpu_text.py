"""gmg_regions_text on the device against the Python restatement of the record rule (tests/text_oracle.py), byte for byte.
The inputs are hand-made with the kernel's shape in mind: a work-group owns 16 KiB of the text, a lane 16 bytes at a time."""
import numpy as np
import pytest

import extract_oracle as xo
import text_oracle as to

pytestmark = pytest.mark.gpu

ERANGE = -6
LENGTHS = [1, 2, 59, 60, 61, 121, 20000]
ALPHABET = "acgtACGTacgtnNrykmRYKMbdhvswBDHVSW*-"
HEADS = ["", ">", ">" + "h" * 298 + "\n"]


@pytest.fixture(scope="module")
def batch(gpu):
    rng = np.random.default_rng(11)
    seqs = ["".join(ALPHABET[i] for i in rng.integers(0, len(ALPHABET), L)) for L in LENGTHS]
    off = np.cumsum([0] + LENGTHS)
    letters = gpu.Letters("".join(seqs).encode(), off)
    yield letters, seqs
    letters.close()


@pytest.fixture(scope="module")
def cases(batch):
    """(regions, heads, the letters of every region): every length around the line width on every read that holds it, from the
    read's first, a middle and its LAST position, both strands -- so most of them wrap across the read's end --, the whole read,
    and the 20,000-letter region, longer than any tile"""
    _, seqs = batch
    regions = []
    for r, L in enumerate(LENGTHS):
        for n in sorted({0, 1, 59, 60, 61, 120, 121, L}):
            if n > L:
                continue
            for first in sorted({0, L // 2, L - 1}):
                for strand in (1, -1):
                    regions.append((r, first, n, strand))
    regions += [(6, 7, 20000, 1), (6, 7, 20000, -1)]
    heads = [HEADS[k % 3] for k in range(len(regions))]
    chars = [xo.region_chars(seqs[r], f, n, s) if n else "" for r, f, n, s in regions]
    assert any(f + n > LENGTHS[r] for r, f, n, s in regions if s > 0) and any(f - n + 1 < 0 for r, f, n, s in regions if s < 0)
    return regions, heads, chars


@pytest.fixture(scope="module")
def small(batch):
    """5,000 records of 0 - 2 letters with heads of 0 or 1 byte: hundreds of records in a tile, several in one 16-byte store"""
    _, seqs = batch
    rng = np.random.default_rng(12)
    regions = []
    for k in range(5000):
        r = int(rng.integers(0, len(LENGTHS)))
        n = min(int(rng.integers(0, 3)), LENGTHS[r])
        regions.append((r, int(rng.integers(0, LENGTHS[r])), n, 1 if rng.integers(0, 2) else -1))
    heads = [">" if rng.integers(0, 2) else "" for _ in regions]
    chars = [xo.region_chars(seqs[r], f, n, s) if n else "" for r, f, n, s in regions]
    return regions, heads, chars


def expected(heads, chars, width):
    return "".join(to.record(h, c, width) for h, c in zip(heads, chars)).encode()


@pytest.mark.parametrize("width", [60, 1, 7, 0])
def test_text_equals_the_restatement(gpu, batch, cases, width):
    letters, _ = batch
    regions, heads, chars = cases
    want = expected(heads, chars, width)
    got = letters.regions_text(regions, [h.encode() for h in heads], gpu.text_params(width))
    assert len(got) == len(want) > 2 * 16384 and got == want


@pytest.mark.parametrize("width", [60, 1, 0])
def test_many_tiny_records(gpu, batch, small, width):
    letters, _ = batch
    regions, heads, chars = small
    want = expected(heads, chars, width)
    assert want.count(b"\n") >= 5000 and len(want) < 5000 * 6
    assert letters.regions_text(regions, [h.encode() for h in heads], gpu.text_params(width)) == want


def test_tables_are_the_callers(gpu, batch, cases):
    """fwd and rev are applied as given: upper case forward, a marker for every letter on the reverse strand"""
    letters, seqs = batch
    fwd = bytes(ord(chr(c).upper()) if c < 128 else c for c in range(256))
    prm = gpu.text_params(7, fwd=fwd, rev=b"x" * 256)
    regions = [(5, 100, 50, 1), (5, 100, 50, -1)]
    want = to.record("a ", xo.region_chars(seqs[5], 100, 50, 1).upper(), 7) + to.record("b ", "x" * 50, 7)
    assert letters.regions_text(regions, [b"a ", b"b "], prm) == want.encode()


def test_device_resident_text_equals_the_host_text(gpu, batch, cases):
    letters, _ = batch
    regions, heads, chars = cases
    prm, hb = gpu.text_params(60), [h.encode() for h in heads]
    ptr, size = letters.regions_text_device(regions, hb, prm)
    on_device = gpu.memcpy_d2h(ptr, size)
    assert letters.kernel_ms() > 0.0
    assert on_device == expected(heads, chars, 60) == letters.regions_text(regions, hb, prm)


def test_api_edges(gpu, batch, cases):
    letters, _ = batch
    regions, heads, chars = cases
    prm, hb = gpu.text_params(60), [h.encode() for h in heads]
    want = expected(heads, chars, 60)
    # no region: no byte, on either variant
    assert letters.regions_text([], [], prm) == b"" and letters.text_size([], [], prm) == 0
    assert letters.regions_text_device([], [], prm)[1] == 0
    # host_out NULL: the length only
    assert letters.text_size(regions, hb, prm) == len(want)
    # one byte short: GMG_ERANGE, the length reported in the message, the buffer untouched
    buf = np.full(len(want) - 1, 0xAA, np.uint8)
    with pytest.raises(gpu.GmgError) as e:
        letters.regions_text(regions, hb, prm, out=buf)
    assert e.value.code == ERANGE and str(len(want)) in str(e.value) and np.all(buf == 0xAA)
    # exactly enough is enough
    buf = np.full(len(want), 0xAA, np.uint8)
    assert letters.regions_text(regions, hb, prm, out=buf) == len(want) and buf.tobytes() == want
    # a bad region in the middle is named, nothing is written
    mid = len(regions) // 2
    for bad in [(7, 0, 1, 1), (2, 59, 1, 1), (2, 0, 60, -1), (2, 0, 1, 0), (2, -1, 1, 1), (2, 0, -1, 1)]:
        buf = np.full(len(want) + 400, 0xAA, np.uint8)
        with pytest.raises(gpu.GmgError) as e:
            letters.regions_text(regions[:mid] + [bad] + regions[mid:], hb[:mid] + [b""] + hb[mid:], prm, out=buf)
        assert e.value.code == ERANGE and "region %d " % mid in str(e.value), str(e.value)
        assert np.all(buf == 0xAA)
