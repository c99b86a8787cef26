"""The three front ends of the shared batch builder (csrc/gmg_gather.h) on ONE job: gmg_reads_select of an index list,
gmg_reads_extract of the forward whole-read regions of the same reads and gmg_reads_splice with one upward run per string describe
the same strings, so the three new batches are equal word for word -- and equal to the strings packed in Python
(tests/extract_oracle.py).  The job has reads that end on either side of a word and of a tile, and tiles that more items overlap
than any of the three gathers stages in LDS."""
import numpy as np
import pytest

import extract_oracle as xo

pytestmark = pytest.mark.gpu

SPECIAL = (15, 16, 17, 1023, 1024, 1025, 2049)
TINY = 80                                               # consecutive reads of 0 .. 3 bases
STAGED = 64                                             # the most items of a tile a gather stages (select, extract: 32)
TILE = 1024


@pytest.fixture(scope="module")
def job(gpu):
    rng = np.random.default_rng(61)
    lens = rng.integers(0, 41, size=3000).tolist()
    for k, n in enumerate(SPECIAL):                     # mixed in, with ordinary reads on both sides
        lens[200 + 350 * k] = n
    tiny0 = 1500
    lens[tiny0:tiny0 + TINY] = rng.integers(0, 4, size=TINY).tolist()
    lens[tiny0 + 5] = lens[tiny0 + 6] = 0               # (two empty reads in a row, whatever the draw)
    reads = [rng.integers(0, 4, size=n).tolist() for n in lens]
    tiny = list(range(tiny0, tiny0 + TINY))
    special = [200 + 350 * k for k in range(len(SPECIAL))]
    # repeats, out of order; the run of tiny reads at the head of a tile and once more further on
    idx = tiny + rng.integers(0, len(reads), size=2500).tolist() + special[::-1] + tiny + special + rng.integers(0, len(reads), size=300).tolist()
    want = [xo.region_codes(reads[r], 0, len(reads[r]), 1) for r in idx]
    batch = gpu.Reads(*xo.pack(reads))
    yield reads, batch, idx, want
    batch.close()


def _regions(reads, idx):
    """the forward whole-read region of every read of idx; an empty read as a region of no bases of the nearest read that has any"""
    full = [r for r in range(len(reads)) if len(reads[r])]
    near = np.array(full)[np.clip(np.searchsorted(full, np.arange(len(reads))), 0, len(full) - 1)]
    return [(r, 0, len(reads[r]), 1) if len(reads[r]) else (int(near[r]), 0, 0, 1) for r in idx]


def _splice(batch, reads, idx, reversed):
    runs = np.array([(r, 0, len(reads[r]), 0) for r in idx], np.uint32)         # kind 0: GMG_RUN_UP
    return batch.splice(runs, np.arange(len(idx) + 1, dtype=np.uint64), reversed=reversed)


def test_the_job_reaches_every_fallback(job):
    """(of the job itself) some tile of the new batch is overlapped by more strings than the widest staging holds"""
    _, _, _, want = job
    off = np.concatenate([[0], np.cumsum([len(w) for w in want])])
    first = np.searchsorted(off, np.arange(0, off[-1], TILE), side="right") - 1       # the string that holds a tile's first base
    last = np.searchsorted(off, np.minimum(np.arange(0, off[-1], TILE) + TILE, off[-1]) - 1, side="right") - 1
    assert (last - first + 1).max() > STAGED + 6
    assert {len(w) for w in want} >= set(SPECIAL) | {0, 1, 2, 3}


@pytest.mark.parametrize("reversed", [False, True])
def test_select_extract_and_splice_build_the_same_batch(gpu, job, reversed):
    reads, batch, idx, want = job
    words, woff = xo.pack([w[::-1] for w in want] if reversed else want)
    built = {"extract": batch.extract(_regions(reads, idx), reversed=reversed), "splice": _splice(batch, reads, idx, reversed)}
    if not reversed:
        built["select"] = batch.select(idx)
    got = {}
    for name, sub in built.items():
        assert sub.n_reads == len(idx) and sub.total_bases == int(woff[-1]), name
        got[name] = sub.download()
        sub.close()
    for name, (packed, off) in got.items():
        assert np.array_equal(off, woff), name
        assert len(packed) == len(words) and np.array_equal(packed, words), "%s: first differing word %d" % (
            name, np.nonzero(packed != words)[0][0])
    for name in got:                                    # (what the two asserts above imply, stated on the batches themselves)
        assert np.array_equal(got[name][0], got["extract"][0]) and np.array_equal(got[name][1], got["extract"][1]), name
