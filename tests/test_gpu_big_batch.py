"""Every region, segment and gather entry point on a batch of more than 2^32 bases (tests/big_batch.py: 4,143 reads, 2^32 + 2^21 +
21,332 bases, 1 GiB of packed words, uploaded once).  gmg_reads_upload takes any batch whose reads are shorter than 2^31 bases; every
kernel that turns (read, position) into a job-wide base index has to do so in 64 bits.  One test per kernel family: regions,
segments, runs and indices inside the three probe groups -- across base 2^31 and base 2^32 inside the reads that straddle them,
round their read's end on both strands, in the last reads of the batch -- compared

    1. with the Python restatements and the C oracle applied to the probe strings, byte for byte and integer for integer, and
    2. with the same call on a small batch that holds the 45 probe reads only, renumbered.

tests/test_big_batch_host.py proves on the CPU that each expectation changes when the source index is taken modulo 2^32 or modulo
2^31.  Nothing here downloads the big batch; the largest result fetched is gmg_window_counts' table (86 MB)."""
import os

import numpy as np
import pytest

import big_batch as bb
import entropy_oracle as eo
import extract_oracle as xo
import features_cases as fc
import fixed_oracle as fo
from conftest import DATA

pytestmark = pytest.mark.gpu

DIST_TOL = 1e-13                                        # tests/test_gpu_entropy.py's bound on |device - host| distance, derived there
LENS = [bb.GROUP_LENS[j % bb.K] for j in range(bb.N_PROBES)]
N_WINDOW_ROWS = bb.N_WINDOW_ROWS                         # 4,311,155 rows of gmg_window_counts (1000, 997); must stay below 5 M


@pytest.fixture(scope="module")
def layout():
    return bb.Layout()


@pytest.fixture(scope="module")
def big(gpu, layout):
    reads = gpu.Reads(layout.packed(), layout.offsets)
    assert reads.total_bases == layout.total > bb.M32
    yield reads
    reads.close()


@pytest.fixture(scope="module")
def small(gpu):
    reads = gpu.Reads(*xo.pack([c.tolist() for c in bb.probe_codes()]))
    yield reads
    reads.close()


@pytest.fixture(scope="module")
def strings():
    return bb.probe_codes()


@pytest.fixture(scope="module")
def seen(layout):
    return [layout.index_of(j) for j in range(bb.N_PROBES)]


def _same_batch(sub, want):
    """offsets, every packed word, the zero bits behind the last base and the zero guard word; -> the downloaded words"""
    packed, off = sub.download()
    words, woff = xo.pack(want)
    assert np.array_equal(off, woff)
    assert len(packed) == len(words) and packed[-1] == 0
    bad = np.nonzero(packed != words)[0]
    assert len(bad) == 0, "first differing word %d of %d: %08x, expected %08x" % (bad[0], len(bad), packed[bad[0]], words[bad[0]])
    return packed


def _amb(index_fn):
    raw = np.array([int(index_fn([p])[0]) for p in bb.AMB_PAIRS], np.uint64)
    order = np.argsort(raw, kind="stable")
    return raw[order], np.array(bb.AMB_CODES, np.uint8)[order]


def test_select_extract_splice_read_their_source_in_64_bits(gpu, layout, big, small, strings, seen):
    """the new batch's words and offsets: select (a permutation with repeats), extract (both strands, modulo the read, reversed, the
    list of ambiguous bases with indices beyond 2^32), splice (every kind of run, reversed)"""
    amb_big, amb_small = _amb(layout.big_index), _amb(bb.small_index)
    assert amb_big[0][-1] > bb.M32
    runs_small, sro = bb.splice_arrays()
    runs_big, _ = bb.splice_arrays(layout.probe_read)
    regions = bb.extract_regions()
    calls = [(lambda r, k: r.select(layout.probe_read[bb.select_order()] if k else bb.select_order()), bb.expect_select(strings))]
    for rev in (False, True):
        calls.append((lambda r, k, rev=rev: r.extract(layout.big(regions) if k else regions, reversed=rev, amb=amb_big if k else amb_small),
                      bb.expect_extract(layout, strings, seen, rev)))
        calls.append((lambda r, k, rev=rev: r.splice(runs_big if k else runs_small, sro, reversed=rev), bb.expect_splice(strings, rev)))
    for call, want in calls:
        a, b = call(big, True), call(small, False)
        try:
            assert np.array_equal(_same_batch(a, want), _same_batch(b, want))
        finally:
            a.close()
            b.close()


def test_write_side_a_new_batch_beyond_2_32_bases(gpu, layout, big, strings):
    """one select of ALL reads with the probe groups moved round the three slots: the new batch is itself beyond 2^32 bases (its
    tiles and words are indexed beyond 2^32 / 1024 and 2^32 / 16) and stays on the device; a second select pulls the probe reads out
    of it, also a filler read from either side of every group"""
    moved = bb.Layout((2, 0, 1))
    src_of = np.arange(layout.n_reads, dtype=np.uint64)
    src_of[moved.probe_read] = layout.probe_read        # read moved.probe_read[j] of the new batch is probe j
    new = big.select(src_of)
    try:
        assert new.n_reads == layout.n_reads and new.total_bases == layout.total
        edge = [int(moved.probe_read[bb.K * g]) - 1 for g in range(3)] + [int(moved.probe_read[bb.K * g + bb.K - 1]) + 1 for g in moved.slots[:2]]
        idx = np.concatenate([moved.probe_read, edge]).astype(np.uint64)
        sub = new.select(idx)
        try:
            filler = [(([3, 3, 0, 0] * (bb.FILL // 4))[:int(moved.lens[r])]) for r in edge]
            _same_batch(sub, [s.tolist() for s in strings] + filler)
        finally:
            sub.close()
    finally:
        new.close()


@pytest.fixture(scope="module")
def nc(gpu, oracle):
    path = os.path.join(DATA, "NC_000915.icm")
    return gpu.Icm.open(path), oracle.read(path)


def test_segment_entry_points(gpu, oracle, nc, layout, big, small, strings):
    """gmg_segment_frame_score, gmg_segment_cumscore, gmg_score_string, gmg_segment_partial_prob per frame and gmg_all_frame_score, all
    four orientations, NC_000915.icm: equal to the oracle on the buffers cut from the probe strings, double for double"""
    model, o_model = nc
    rows = bb.segment_rows()
    per, allf = bb.expect_segments(oracle, o_model, strings)
    prefix, frames = bb.all_frame_args()
    got = {}
    for name, reads, r in (("big", big, layout.big(rows)), ("small", small, rows)):
        segs = gpu.Segments(reads, r)
        out = []
        for f in range(3):
            out.append((segs.split(gpu.segment_frame_score(model, reads, segs, f)), segs.split(gpu.segment_cumscore(model, reads, segs, f)),
                        gpu.score_string(model, reads, segs, f), gpu.segment_partial_prob(model, reads, segs, f)))
        got[name] = (out, gpu.all_frame_score(model, reads, segs, prefix, frames))
        segs.close()
    for name in ("big", "small"):
        out, ga = got[name]
        for f in range(3):
            fs, cum, tot, part = out[f]
            for i, (w_fs, w_cum, w_tot, w_part) in enumerate(per[f]):
                assert np.array_equal(fs[i], w_fs) and np.array_equal(cum[i], w_cum), (name, f, rows[i])
                assert tot[i] == w_tot and part[i] == w_part, (name, f, rows[i])
        for i, w in enumerate(allf):
            assert np.array_equal(ga[i], w), (name, rows[i])


def test_fixed_score(gpu, oracle, layout, big, small, strings):
    """gmg_fixed_score, a model of length 12 and depth 5 trained on the genome: bit-equal to the numpy oracle"""
    g = open(os.path.join(DATA, "NC_000915.fna"), "rb").read().split(b"\n", 1)[1].replace(b"\n", b"")
    train = [g[s:s + bb.FIXED_L] for s in range(1000, 1000 + 600 * 37, 37)]
    mine = gpu.FixedIcm.train(train, 5, -1, None)
    subs = fo.train(oracle, train, bb.FIXED_L, 5, None)
    want = fo.score(subs, list(range(bb.FIXED_L)), bb.fixed_windows(strings))
    rows = bb.fixed_rows()
    for reads, r in ((big, layout.big(rows)), (small, rows)):
        segs = gpu.Segments(reads, r)
        got = gpu.fixed_score(mine, reads, segs)
        segs.close()
        assert np.array_equal(got.view(np.uint64), want.view(np.uint64))


def test_score_reads_strings_whole_batch(gpu, oracle, layout, big, small, strings):
    """one period-1 model, the default (fused) form, on ALL reads: the probe reads' rows equal the oracle on both strands; filler
    rows of equal length are equal to each other (the filler is its own reverse complement: both columns too)"""
    path = os.path.join(DATA, "cluster-1.icm")
    model, o_model = gpu.Icm.open(path), oracle.read(path)
    got = gpu.score_reads_strings([model], big)[0]
    want = bb.expect_strings(oracle, o_model, strings)
    assert np.array_equal(got[layout.probe_read], want)
    assert np.array_equal(gpu.score_reads_strings([model], small)[0], want)
    lens = layout.lens.astype(np.int64)
    for n in np.unique(lens[~layout.is_probe]):
        rows = got[(lens == n) & ~layout.is_probe]
        assert np.all(rows == rows[0, 0]) and np.isfinite(rows[0, 0]) and rows[0, 0] == oracle.score_string(o_model, ("ttaa" * (int(n) // 4)), 0)


def test_find_orfs_and_their_entropy(gpu, oracle, layout, big, small, strings):
    """gmg_find_orfs keeps its result on the device, gmg_entropy_orfs reads the ORFs' bases: the probes' ORFs equal Find_Orfs, filler
    reads have none and read_orf_off says so; counts exact, distances as tests/test_gpu_entropy.py compares them"""
    want = bb.expect_orfs(oracle, strings)
    flat = np.concatenate(want)
    aa = eo.tables()[11]
    regions = bb.orf_regions(want, LENS)
    want_counts = bb.expect_entropy_counts(strings, regions, aa)
    host = eo.finish_rows(want_counts)
    for reads, read_of in ((big, layout.probe_read), (small, np.arange(bb.N_PROBES))):
        res = gpu.OrfResult(reads, min_gene_len=bb.MIN_GENE_LEN, allow_truncated=False)
        try:
            orfs, off = res.fetch()
            assert len(orfs) == len(flat)                # nothing outside the probes
            per_read = np.diff(off.astype(np.int64))
            assert np.array_equal(per_read[read_of], [len(w) for w in want]) and per_read.sum() == len(flat)
            assert np.array_equal(orfs["read"], np.repeat(read_of, [len(w) for w in want]))
            assert np.array_equal(np.stack([orfs["frame"], orfs["stop_position"], orfs["gene_len"], orfs["orf_len"]], 1), flat)
            counts, dist = gpu.entropy_orfs(reads, res, aa.encode(), eo.POS, eo.NEG)
        finally:
            res.close()
        assert np.array_equal(counts, want_counts)
        _same_distances(dist, host)


def _same_distances(dist, host):
    assert np.array_equal(np.isnan(dist), np.isnan(host))
    ok = ~np.isnan(host[:, 0])
    worst = float(np.max(np.abs(dist[ok, :2] - host[ok, :2]))) if ok.any() else 0.0
    print("largest |device - host| distance: %.3g over %d regions" % (worst, int(ok.sum())))
    assert worst <= DIST_TOL
    for pd, nd, ratio in dist[ok]:
        assert ratio == ((1.0 if pd == 0.0 else 1e3) if nd == 0.0 else pd / nd)


def test_entropy_regions_and_genes_audit(gpu, layout, big, small, strings, seen):
    aa = eo.tables()[11]
    regions = bb.entropy_region_rows()
    want_counts = bb.expect_entropy_counts(strings, regions, aa)
    host = eo.finish_rows(want_counts)
    for reads, r in ((big, layout.big(regions)), (small, regions)):
        counts, dist = gpu.entropy_regions(reads, [tuple(x) for x in np.asarray(r).tolist()], aa.encode(), eo.POS, eo.NEG)
        assert np.array_equal(counts, want_counts)
        _same_distances(dist, host)
    # gmg_genes_audit with a list of ambiguous bases whose entries lie beyond 2^32
    regions = bb.audit_region_rows()
    recs, inner, hist = bb.expect_audit(layout, strings, seen)
    for reads, r, amb in ((big, layout.big(regions), layout.big_index(bb.AMB_PAIRS)), (small, regions, bb.small_index(bb.AMB_PAIRS))):
        got, got_inner, got_hist = gpu.genes_audit(reads, r, amb=amb)
        for name in ("first_codon", "last_codon", "start_which", "stop_which", "n_inner_stops", "inner_begin", "last_back_stop", "next_stop"):
            assert got[name].tolist() == [x[name] for x in recs], name
        assert got_inner.tolist() == inner and got_hist.tolist() == hist


def _check_windows(gpu, lay, reads, want_probe):
    off, counts = gpu.window_counts(reads, bb.WINDOW, bb.SKIP, amb=lay.big_index(bb.AMB_PAIRS))
    assert len(counts) == N_WINDOW_ROWS < 5_000_000 and int(off[-1]) == N_WINDOW_ROWS
    off = off.astype(np.int64)
    for j, w in enumerate(want_probe):
        r = lay.probe_read[j]
        assert np.array_equal(counts[off[r]:off[r + 1]], w), j
    lens = lay.lens.astype(np.int64)
    for n in np.unique(lens[~lay.is_probe]):
        want = bb.filler_windows(int(n), bb.WINDOW, bb.SKIP, lay.filler)
        which = np.nonzero((lens == n) & ~lay.is_probe)[0]
        assert np.all(off[which + 1] - off[which] == len(want))
        rows = counts[(off[which][:, None] + np.arange(len(want))[None, :]).ravel()].reshape(len(which), len(want), 5)
        bad = np.nonzero((rows != want[None]).any(axis=(1, 2)))[0]
        assert len(bad) == 0, "filler read %d (of %d bases) differs from the closed form" % (which[bad[0]], n)


def test_window_counts(gpu, layout, big, small, strings, seen):
    """(W, S) = (1000, 997), a list of ambiguous bases beyond 2^32: 4,311,155 rows; the probes' rows equal the ring buffer's, every
    filler read's rows the closed form"""
    want = bb.expect_windows(layout, strings, seen)
    _check_windows(gpu, layout, big, want)
    off, counts = gpu.window_counts(small, bb.WINDOW, bb.SKIP, amb=bb.small_index(bb.AMB_PAIRS))
    assert np.array_equal(counts, np.concatenate(want)) and np.array_equal(np.diff(off.astype(np.int64)), [len(w) for w in want])


def test_window_counts_where_the_running_sums_have_wrapped(gpu, strings):
    """the same on the all-t batch: the running count of t passes 2^32 inside the filler read behind the second group, so that read's
    rows take the difference of sums on either side of the wrap and the last group lies behind it"""
    lay = bb.Layout(filler="t")
    reads = gpu.Reads(lay.packed(), lay.offsets)
    try:
        seen = [lay.index_of(j) for j in range(bb.N_PROBES)]
        _check_windows(gpu, lay, reads, bb.expect_windows(lay, strings, seen))
    finally:
        reads.close()


def test_regions_uncovered(gpu, layout, big, small):
    """intervals in probe reads: their gaps equal the restatement's, every other read is one whole-read gap (an empty read: none)"""
    iv = bb.uncovered_intervals()
    want, want_off = bb.expect_uncovered(LENS)
    gaps, off = gpu.regions_uncovered(small, iv)
    assert gaps.tolist() == [list(g) for g in want] and off.tolist() == want_off
    gaps, off = gpu.regions_uncovered(big, layout.big(iv))
    off = off.astype(np.int64)
    assert len(gaps) == len(want) + int((~layout.is_probe).sum())
    for j in range(bb.N_PROBES):
        r = layout.probe_read[j]
        assert [[j] + g[1:] for g in gaps[off[r]:off[r + 1]].tolist()] == [list(g) for g in want[want_off[j]:want_off[j + 1]]], j
        assert np.all(gaps[off[r]:off[r + 1], 0] == r)
    fill = np.nonzero(~layout.is_probe)[0]
    assert np.all(off[fill + 1] - off[fill] == 1)
    assert np.array_equal(gaps[off[fill]], np.stack([fill, np.zeros_like(fill), layout.lens[fill].astype(np.int64), np.ones_like(fill)], 1))


def test_features_count(gpu, layout, big, small, strings, seen):
    """genes in probe reads of the groups at and beyond 2^32 only, opaque indices beyond 2^32: both tables bit-equal to the
    restatement of train_features.py on those reads"""
    genes, sd = bb.feature_inputs(layout, strings, seen)
    want_g, want_n = bb.expect_features(layout, strings, seen)
    rows = bb.feature_rows(genes)
    opq_big = layout.big_index(bb.OPAQUE_PAIRS)
    assert opq_big[0] > bb.M32 - bb.BELOW[1] and opq_big[-1] > bb.M32
    for reads, r, opq in ((big, layout.big(rows), opq_big), (small, rows, bb.small_index(bb.OPAQUE_PAIRS))):
        got_g, got_n, info = gpu.features_count(reads, [tuple(x) for x in np.asarray(r).tolist()], opq)
        assert fc.same_table(got_g, want_g) == [] and fc.same_table(got_n, want_n) == []


def test_tophits_scores(gpu, oracle, layout, big, small, strings):
    """gmg_tophits_scores (the strings sums into the handle's scratch, then the best models of every read): the probes' rows equal
    phymm_oracle's selection over the oracle's own sums; the sums the handle scored with equal them too"""
    import phymm_oracle as po
    paths = [os.path.join(DATA, "cluster-%d.icm" % i) for i in (0, 1, 2)]
    models = [gpu.Icm.open(p) for p in paths]
    want_sums = np.stack([bb.expect_strings(oracle, oracle.read(p), strings) for p in paths])
    wk, wm = po.tophits_numpy(po.merged_keys(want_sums), 2)
    for reads, read_of in ((big, layout.probe_read), (small, np.arange(bb.N_PROBES))):
        h = gpu.TopHits(reads, 2)
        try:
            sums = h.scores(models, return_sums=True)
            keys, slots = h.fetch()
        finally:
            h.close()
        assert np.array_equal(sums[:, read_of], want_sums)
        assert np.array_equal(slots[read_of], wm) and np.array_equal(keys[read_of], wk)
