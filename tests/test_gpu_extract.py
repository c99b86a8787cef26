"""gmg_reads_extract on the device (include/gmg.h): regions of a batch's reads, any strand, modulo the read, as a NEW batch --
every packed word against strings built in Python (tests/extract_oracle.py), the batch as an input of the scoring calls, the
exceptions for ambiguity letters, the errors, and training from the batch (gmg_icm_train_reads) against the host path and the
reference's build-icm on recorded `extract` output."""
import ctypes as C
import gc
import os
import subprocess

import numpy as np
import pytest

import extract_oracle as xo
from conftest import built_binary, DATA

pytestmark = pytest.mark.gpu

EINVAL, ERANGE = -1, -6
LENGTHS = (1, 15, 16, 17, 31, 33, 64, 1025, 2100)


def _codes(rng, n):
    return rng.integers(0, 4, size=n).tolist()


@pytest.fixture(scope="module")
def source(gpu):
    """reads that begin at many bit offsets, every one with foreign bases on both sides (read 0: the guard words in front)"""
    rng = np.random.default_rng(41)
    reads = [_codes(rng, n) for n in LENGTHS]
    batch = gpu.Reads(*xo.pack(reads))
    yield reads, batch
    batch.close()


@pytest.fixture(scope="module")
def edge_regions():
    regions = []
    for r, L in enumerate(LENGTHS):
        if L <= 33:
            regions += [(r, f, n, s) for f in range(L) for n in range(L + 1) for s in (1, -1)]
    for r in (7, 8):
        L = LENGTHS[r]
        for s in (1, -1):
            regions += [(r, 5, L, s), (r, L - 1, L, s), (r, L // 2, L, s),             # the whole circle from a non-zero first
                        (r, L - 7, 30, s), (r, 3, 30, s), (r, L - 1, 2, s), (r, 0, 2, s),   # the wrap inside an output word
                        (r, 100, 900, s), (r, 17, 1000, s), (r, L - 500, 1000, s)]     # across tiles of the new batch
    return regions


def _want(reads, regions, reversed=False, patches=None, offsets=None):
    out = []
    for r, f, n, s in regions:
        w = xo.region_codes(reads[r], f, n, s, patches, int(offsets[r]) if offsets is not None else 0)
        out.append(w[::-1] if reversed else w)
    return out


def _check(batch, want):
    """offsets, every packed word, the zero bits behind the last base and the zero guard word"""
    packed, off = batch.download()
    words, woff = xo.pack(want)
    assert np.array_equal(off, woff)
    assert len(packed) == len(words) and packed[-1] == 0
    bad = np.nonzero(packed != words)[0]
    assert len(bad) == 0, "first differing word %d: %08x, expected %08x" % (bad[0], packed[bad[0]], words[bad[0]])


def test_word_and_offset_edge_cases(gpu, source, edge_regions):
    reads, batch = source
    sub = batch.extract(edge_regions)
    assert sub.n_reads == len(edge_regions) and sub.total_bases > 8 * 1024
    _check(sub, _want(reads, edge_regions))
    sub.close()


def test_reversed_is_the_reversal_of_every_string(gpu, source, edge_regions):
    reads, batch = source
    sub = batch.extract(edge_regions, reversed=True)
    _check(sub, _want(reads, edge_regions, reversed=True))
    sub.close()


@pytest.mark.parametrize("reversed", [False, True])
def test_more_regions_in_a_tile_than_the_kernel_stages(gpu, reversed):
    """150 regions of length 1 and 0 in turn, then 40 of length 17, all inside the first tile, from the read at word 0 of the
    source: downward windows there end in the guard words"""
    rng = np.random.default_rng(42)
    reads = [_codes(rng, 40), _codes(rng, 7), _codes(rng, 1025)]
    batch = gpu.Reads(*xo.pack(reads))
    regions = [(0, int(rng.integers(0, 40)), 1 - k % 2, 1 if k % 3 else -1) for k in range(150)]
    regions += [(0, (3 * k) % 40, 17, -1 if k % 2 else 1) for k in range(40)]
    regions += [(2, 1000, 600, -1), (1, 2, 7, -1)]
    sub = batch.extract(regions, reversed=reversed)
    _check(sub, _want(reads, regions, reversed=reversed))
    sub.close()
    batch.close()


def test_exceptions_on_the_reverse_strand(gpu, source):
    """listed bases take their listed code under strand < 0 regions only: at a region's first and last base, across the wrap, with
    and without REVERSED; forward regions over the same bases and an entry nothing covers change nothing; no list: 3 - code"""
    reads, batch = source
    off = np.concatenate([[0], np.cumsum(LENGTHS)])
    amb = {}
    for r, p in [(5, 0), (5, 32), (5, 10), (6, 63), (7, 0), (7, 1024), (7, 500), (8, 2099), (8, 1000), (3, 4), (2, 9), (4, 7)]:
        amb[int(off[r]) + p] = (3 - reads[r][p] + 1 + p % 3) % 4              # never the code complement
    base = np.array(sorted(amb), np.uint64)
    code = np.array([amb[int(b)] for b in base], np.uint8)
    regions = []
    for s in (-1, 1):
        regions += [(5, 10, 11, s), (5, 20, 11, s), (5, 3, 33, s), (5, 32, 1, s), (5, 0, 1, s), (5, 5, 12, s),      # read 5: first, last, wrap
                    (6, 63, 64, s), (6, 10, 30, s), (7, 3, 20, s), (7, 1024, 1025, s), (7, 500, 1, s), (7, 499, 600, s),
                    (8, 1000, 2100, s), (8, 50, 100, s), (8, 2099, 40, s), (3, 16, 17, s)]
    # (read 2's entry is covered by a forward region only, read 4's by nothing)
    regions += [(2, 0, 16, 1)]
    assert any(xo.region_codes(reads[r], f, n, s, amb, int(off[r])) != xo.region_codes(reads[r], f, n, s) for r, f, n, s in regions)
    for reversed in (False, True):
        sub = batch.extract(regions, reversed=reversed, amb=(base, code))
        _check(sub, _want(reads, regions, reversed, amb, off))
        sub.close()
        plain = batch.extract(regions, reversed=reversed)
        _check(plain, _want(reads, regions, reversed))
        plain.close()
    fwd = [g for g in regions if g[3] > 0]
    sub = batch.extract(fwd, amb=(base, code))
    _check(sub, _want(reads, fwd))
    sub.close()


def _models(gpu):
    gene, indep = gpu.Icm.open(os.path.join(DATA, "NC_000915.icm")), gpu.Icm.indep(0.5)
    return gene, indep


@pytest.mark.parametrize("shape", ["uniform", "ragged"])
def test_the_batch_is_a_full_citizen(gpu, shape):
    """scoring and ORF finding on the extracted batch and on an uploaded batch of the same strings: bit for bit.  300 regions of
    90 bases (uniform_len), and ragged lengths with 0, 1 and several above 512"""
    rng = np.random.default_rng(43)
    reads = [_codes(rng, 3000), _codes(rng, 777), _codes(rng, 2500)]
    batch = gpu.Reads(*xo.pack(reads))
    if shape == "uniform":
        regions = [(k % 3, int(rng.integers(0, len(reads[k % 3]))), 90, 1 if k % 2 else -1) for k in range(300)]
    else:
        lens = [0, 1, 600, 2500, 513, 512, 0, 90, 13, 777, 1500] + rng.integers(0, 400, size=40).tolist()
        regions = []
        for k, n in enumerate(lens):
            r = 2 if n > 777 else k % 3
            regions.append((r, int(rng.integers(0, len(reads[r]))), int(n), 1 if k % 2 else -1))
    want = _want(reads, regions)
    mine, theirs = batch.extract(regions), gpu.Reads(*xo.pack(want))
    _check(mine, want)
    gene, indep = _models(gpu)
    rows = [(k, 0, len(w), gpu.FORWARD) for k, w in enumerate(want) if len(w)]
    got = []
    for b in (mine, theirs):
        segs = gpu.Segments(b, rows)
        orfs, first = gpu.find_orfs(b, min_gene_len=30, allow_truncated=True)
        got.append((gpu.score_string(gene, b, segs, 1), gpu.frame_score6(gene, indep, b), orfs, first))
        segs.close()
    assert np.array_equal(got[0][0].view(np.uint64), got[1][0].view(np.uint64))
    assert np.array_equal(got[0][1].view(np.uint64), got[1][1].view(np.uint64))
    assert got[0][2].tobytes() == got[1][2].tobytes() and np.array_equal(got[0][3], got[1][3]) and len(got[0][2]) > 20
    for b in (mine, theirs, batch, gene, indep):
        b.close()


def _busy(gpu):
    out = (C.c_uint64 * 4)()
    assert gpu.capi.lib().gmg_debug_cache_stats(out) == 0
    return int(out[0])


def test_errors_leave_nothing_behind(gpu, source):
    reads, batch = source
    good = [(5, 3, 20, -1), (8, 2000, 300, 1)]
    gc.collect()
    gpu.capi.lib().gmg_synchronize(None)
    before = _busy(gpu)
    for bad in [(9, 0, 1, 1), (5, 33, 1, 1), (5, 0, 34, -1), (5, 0, 3, 0), (5, -1, 3, 1), (5, 2, -1, 1)]:
        with pytest.raises(gpu.GmgError, match="region 1 ") as e:
            batch.extract([good[0], bad, (9, 9, 9, 0)])
        assert e.value.code == ERANGE
        assert _busy(gpu) == before
    sub = batch.extract(good)
    assert _busy(gpu) == before + 3                      # packed words, offsets, tile table
    _check(sub, _want(reads, good))
    sub.close()
    empty = batch.extract([])
    assert empty.n_reads == 0 and empty.total_bases == 0
    packed, off = empty.download()
    assert list(off) == [0] and not packed.any()
    empty.close()
    assert _busy(gpu) == before
    h = C.c_void_p()
    arr = (gpu.capi.GeneRegion * 1)(gpu.capi.GeneRegion(5, 0, 3, 1))
    assert gpu.capi.lib().gmg_reads_extract(batch.h, arr, 1, 2, None, None, 0, C.byref(h)) == EINVAL      # an unknown flag
    assert gpu.capi.lib().gmg_reads_extract(batch.h, arr, 1, 0, None, None, 3, C.byref(h)) == EINVAL      # a list without arrays
    assert _busy(gpu) == before


@pytest.fixture(scope="module")
def subset(gpu):
    """the committed subset of NC_000915.longorfs under extract -t: the genome ingested on the device, the regions, the list"""
    data = open(os.path.join(DATA, "NC_000915.fna"), "rb").read()
    genome, _, _ = gpu.Reads.from_fasta_bytes(data)
    coords = xo.parse_coords(os.path.join(xo.EX, "nc_subset.coords"))
    regions, _ = gpu.extract_plan([0, genome.total_bases], [(0,) + c[1:3] for c in coords], gpu.COORD_SKIP_STOP)
    recorded = xo.parse_out(os.path.join(xo.EX, "nc_subset.t.out"))
    yield genome, regions, gpu.fasta_ambiguous(data), recorded
    genome.close()


def test_extracted_subset_is_subscript_of_the_recorded_text(gpu, subset):
    genome, regions, amb, recorded = subset
    for reversed in (False, True):
        sub = genome.extract(regions, reversed=reversed, amb=amb)
        _check(sub, [[xo.code(ch) for ch in (text[::-1] if reversed else text)] for _, text in recorded])
        sub.close()
    plain = xo.unpack(*genome.extract(regions).download())
    assert sum(p != [xo.code(ch) for ch in text] for p, (_, text) in zip(plain, recorded)) == 4       # what the list is for


@pytest.mark.parametrize("shape", [(12, 7, 3), (6, 3, 1)])
def test_training_from_the_extracted_batch(gpu, subset, shape, tmp_path):
    """gmg_icm_train_reads on the extracted, reversed batch = gmg_icm_train on the same strings from the host = the reference's
    build-icm -r on the recorded extract -t text, file for file"""
    genome, regions, amb, recorded = subset
    W, D, P = shape
    sub = genome.extract(regions, reversed=True, amb=amb)
    a, b, c = str(tmp_path / "device.icm"), str(tmp_path / "host.icm"), str(tmp_path / "ref.icm")
    gpu.icm_train_reads(sub, W, D, P).write(a)
    gpu.Icm.train([text.lower()[::-1] for _, text in recorded], W, D, P).write(b)
    sub.close()
    assert open(a, "rb").read() == open(b, "rb").read()
    ref = built_binary("oracle", "_ref", "build-icm")
    with open(os.path.join(xo.EX, "nc_subset.t.out"), "rb") as fp:
        subprocess.run([ref, "-r", "-w", str(W), "-d", str(D), "-p", str(P), c], stdin=fp, check=True, timeout=300)
    assert open(a, "rb").read() == open(c, "rb").read()
