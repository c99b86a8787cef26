"""gmg_regions_text and gmg_runs_text beyond 2^32, on either side (tests/big_batch.py).

(a) The source side: a gmg_letters handle of 2^32 + 2^21 + 21,332 letters (4 GiB; the layout of tests/test_gpu_big_batch.py in
    letters, the filler the text ttaa, the probes over the alphabet of tests/test_gpu_text.py).  Regions and runs in the probe groups --
    across 2^31 and 2^32 upwards and downwards, round their read's end -- in DNA and protein mode at widths 0 and 60, byte for byte
    against text_oracle / runs_text_oracle on the probe letters, and equal to the same call on the 45 probe reads alone.
(b) The output side: 215,000 records of 20,000 letters each from a batch of two reads: a text of 4.37e9 bytes that stays on the
    device.  Three slices are fetched -- 128 KiB around byte 2^31, 128 KiB around byte 2^32, the last 64 KiB -- and each equals the
    restatement of the records that overlap it.

A file of its own so that its 4 GiB allocations (one at a time: the letters of (a) are freed before (b) makes its text) can be
judged on their own.  tests/test_big_batch_host.py holds the sensitivity condition for every case here."""
import numpy as np
import pytest

import big_batch as bb
import runs_text_oracle as rto

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def layout():
    return bb.LetterLayout()


@pytest.fixture(scope="module")
def handles(gpu, layout):
    """(the 4 GiB handle, the handle of the probe reads alone)"""
    big = gpu.Letters(layout.letters(), layout.offsets)
    small = gpu.Letters(b"".join(p.tobytes() for p in bb.probe_letters()), bb.small_offsets())
    yield big, small
    big.close()
    small.close()


@pytest.mark.parametrize("width", [0, 60])
def test_regions_text_reads_its_letters_in_64_bits(gpu, layout, handles, width):
    big, small = handles
    regions, heads = bb.text_regions()
    want = bb.expect_regions_text(layout.letter_strings(), width)
    prm = gpu.text_params(width)
    assert big.regions_text(layout.big(regions).astype(np.int32), heads, prm) == want
    assert small.regions_text(regions, heads, prm) == want


@pytest.mark.parametrize("mode", [rto.DNA, rto.PROTEIN], ids=["dna", "protein"])
@pytest.mark.parametrize("width", [0, 60])
def test_runs_text_reads_its_letters_in_64_bits(gpu, layout, handles, mode, width):
    big, small = handles
    runs, sro, heads, front, behind = bb.text_runs()
    want = bb.expect_runs_text(layout.letter_strings(), mode, width)
    prm = gpu.runs_text_params(mode, 0, width=width)
    assert big.runs_text(bb.text_runs_big(layout), sro, heads, prm, front, behind) == want
    assert small.runs_text(runs.astype(np.uint32), sro, heads, prm, front, behind) == want


@pytest.fixture(scope="module")
def out_batch(gpu, handles):
    big, small = handles
    big.close()                                         # (a)'s 4 GiB go back before (b)'s text is made
    seqs = bb.out_letters()
    letters = gpu.Letters(b"".join(seqs), np.cumsum([0] + [len(s) for s in seqs]))
    heads = b"".join(bb.out_head(k) for k in range(bb.OUT_RECORDS))
    head_off = np.concatenate([[0], np.cumsum(bb.out_head_lens())]).astype(np.uint64)
    assert len(heads) == int(head_off[-1])
    yield letters, (heads, head_off), bb.out_record_offsets(bb.REGION_BODY)
    letters.close()


def _check_slices(gpu, ptr, size, off, record_of):
    assert size == int(off[-1]) > bb.M32
    for a, n in bb.out_slices(size):
        got = gpu.memcpy_d2h(gpu.capi.C.c_void_p(ptr.value + a), n)
        want = bb.expect_out_slice(off, record_of, a, n)
        assert len(want) == n
        if got != want:
            bad = np.nonzero(np.frombuffer(got, np.uint8) != np.frombuffer(want, np.uint8))[0]
            raise AssertionError("text byte %d (%d of the slice's %d bytes differ): %r, expected %r" % (a + bad[0], len(bad), n, got[bad[0]:bad[0] + 20], want[bad[0]:bad[0] + 20]))


def test_regions_text_writes_a_text_beyond_2_32_bytes(gpu, out_batch):
    letters, heads, off = out_batch
    ptr, size = letters.regions_text_device(bb.out_regions(), heads, gpu.text_params(bb.OUT_WIDTH))
    _check_slices(gpu, ptr, size, off, bb.out_region_record)


def test_runs_text_writes_a_text_beyond_2_32_bytes(gpu, out_batch):
    letters, heads, off = out_batch
    runs, sro = bb.out_runs()
    ptr, size = letters.runs_text_device(runs, sro, heads, gpu.runs_text_params(rto.DNA, 0, width=bb.OUT_WIDTH))
    _check_slices(gpu, ptr, size, off, bb.out_runs_record)
