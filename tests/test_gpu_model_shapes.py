"""Every device scoring path on ICM shapes other than window 12 / depth 7, bit for bit against the CPU oracle -- which
tests/test_oracle_shapes.py pins to the reference on exactly these model files (tests/model_zoo.py writes them; their hashes are
the ones of the reference's build-icm).

  fast class (depth 7, W = 4, 8, 13, 15; 4 / 7 raw and as its `clean` twin): k_frame6t / k_frame6p, the GENE32 rows, k_orf_fused, the strings
      main pass -- W is a run-time value in all of them (first_rel, the shift bytes, the 2 (W - 1) head lanes, the dense_part offsets)
  any-shape class (16 / 7, 16 / 8, 12 / 8, 12 / 9, 20 / 5, 12 / 1, 12 / 4, 2 / 1; periodicity 1, 2 and 4 where the entry point takes them)

Read set per model: lengths 0, 1, W - 2, W - 1, W, W + 1, 2 (W - 1), 2 W - 1, 150 ragged reads of 1 .. 900 bases, one of 1,500 and
one of 2,100 bases; and a uniform batch of 500-base reads.  No tolerance anywhere.  Run with -m gpu."""
import os

import numpy as np
import pytest

import model_zoo
from test_gpu_mg_err import dev_err_rows
from test_gpu_parity import ORF_PATHS, ORF_WALK
from test_oracle_mg import err_rows

pytestmark = pytest.mark.gpu

GENE = model_zoo.FAST3 + ["s3_w4_d7_clean"] + model_zoo.ANY3                                # periodicity 3: every entry point
ALL = GENE + model_zoo.FAST1 + model_zoo.ANY1 + model_zoo.OTHER_P
GCS = [0.3, 0.36, 0.42, 0.5, 0.55, 0.61, 0.7]                                              # the 7-model null set
KW = dict(min_gene_len=30)


@pytest.fixture(scope="module")
def models(gpu, oracle, tmp_path_factory):
    nulls = [oracle.tables(oracle.indep(gc)) for gc in GCS + [0.45, 0.4]]      # every null model these tests upload
    zoo = model_zoo.zoo(gpu, oracle, tmp_path_factory.mktemp("zoo"), null_tables=nulls)
    assert set(ALL) == set(zoo)
    yield zoo
    model_zoo.free(oracle, zoo)


def random_reads(rng, lengths):
    return ["".join("acgt"[c] for c in rng.integers(0, 4, size=int(n))) for n in lengths]


def read_set(W, seed):
    """(ragged batch, uniform batch): the lengths around the window first"""
    rng = np.random.default_rng(seed)
    edge = [0, 1, max(W - 2, 0), W - 1, W, W + 1, 2 * (W - 1), 2 * W - 1]
    ragged = random_reads(rng, edge + [int(x) for x in rng.integers(1, 901, size=150)] + [1500, 2100])
    assert any(len(s) < W - 1 for s in ragged) and any(len(s) == W - 1 for s in ragged)
    return ragged, random_reads(rng, [500] * 40)


def revcomp(s):
    return s[::-1].translate(str.maketrans("acgt", "tgca"))


def shape_of(icm):
    return icm.params[:3]


def mg_rows(starts):
    return [(int(s["j"]), int(s["pos"]), int(s["which"]), int(s["truncated"]), int(s["first"]), float(s["score"])) for s in starts]


# ---------------------------------------------------------------- the six-frame table

@pytest.mark.parametrize("name", GENE + ["c4_p4_d2_w3"])
def test_six_frame_table(gpu, oracle, models, name):
    """gmg_frame_score6, gmg_frame_score6_nulls (seven null models) and the table gmg_mg_score_reads hands back: every read, all
    six rows.  (periodicity 4: rows use frames 0, 1, 2 of the four, as Score_All_Frames would)"""
    icm, om, _ = models[name]
    W, _, P = shape_of(icm)
    for seqs in read_set(W, 100 + W):
        reads = gpu.Reads.from_strings(seqs)
        indep, o_indep = gpu.Icm.indep(0.45), oracle.indep(0.45)
        want = [oracle.score_all_frames(om, o_indep, s) for s in seqs]
        got = gpu.frame_score6(icm, indep, reads)
        for r, s in enumerate(seqs):
            lo, hi = int(reads.offsets[r]), int(reads.offsets[r + 1])
            assert np.array_equal(got[:, lo:hi], want[r]), (name, "frame_score6", r, len(s))
        if P == 3:
            buf = gpu.api._DeviceBuffer(6 * max(reads.total_bases, 1) * 8)
            gpu.mg_score_reads(icm, indep, reads, frame_scores=buf, **KW)
            table = buf.to_host(np.float64, 6 * reads.total_bases).reshape(6, -1)
            buf.free()
            assert np.array_equal(table, got), (name, "mg_score_reads (frame_scores=)")
        read_null = (np.arange(len(seqs)) * 3 % len(GCS)).astype(np.uint32)
        got = gpu.frame_score6(icm, gpu.NullSet.build(GCS), reads, read_null=read_null)
        o_nulls = [oracle.indep(gc) for gc in GCS]
        for r, s in enumerate(seqs):
            lo, hi = int(reads.offsets[r]), int(reads.offsets[r + 1])
            assert np.array_equal(got[:, lo:hi], oracle.score_all_frames(om, o_nulls[read_null[r]], s)), (name, "nulls", r, len(s))


# ---------------------------------------------------------------- glimmer-mg's front half

@pytest.mark.parametrize("name", GENE)
def test_front_half_and_its_variants(gpu, oracle, models, name):
    """gmg_mg_score_reads: records and start lists of EVERY read against the oracle; then mg_fused 0 / 1 x mg_tile 0 / 1 / 2 / 4 x
    mg_gene32 0 / 1 / 2: every byte equal to the first result"""
    icm, om, _ = models[name]
    W = shape_of(icm)[0]
    indep, o_indep, prm = gpu.Icm.indep(0.45), oracle.indep(0.45), oracle.mg_params(**KW)
    n_starts = n_acc = 0
    for seqs in read_set(W, 200 + W):
        reads = gpu.Reads.from_strings(seqs)
        first = gpu.mg_score_reads(icm, indep, reads, **KW)
        orfs, starts, off = first
        for r, s in enumerate(seqs):
            want_orfs, scored = oracle.mg_read(om, o_indep, s.encode(), prm)
            mine = orfs[int(off[r]):int(off[r + 1])]
            assert np.array_equal(np.stack([mine["frame"], mine["stop_position"], mine["gene_len"], mine["orf_len"]], 1).reshape(-1, 4), want_orfs)
            for o, (out, want) in zip(mine, scored):
                st = starts[o["start_begin"]:o["start_begin"] + o["n_starts"]]
                assert mg_rows(st) == [(w.j, w.pos, w.which, w.truncated, w.first, w.score) for w in want], (name, r, len(s))
                assert (o["lo"], o["hi"], o["first_j"], o["accepted"] != 0, o["orf_is_truncated"]) == \
                       (out.lo, out.hi, out.first_j, bool(out.accepted), out.orf_is_truncated)
                assert o["best_score"] == out.best_score
                n_starts += len(want)
                n_acc += int(out.accepted)
        for fused in (0, 1):
            for tile in (0, 1, 2, 4):
                for g32 in (0, 1, 2):
                    with gpu.option("mg_fused", fused), gpu.option("mg_tile", tile), gpu.option("mg_gene32", g32):
                        got = gpu.mg_score_reads(icm, indep, reads, **KW)
                    for a, b in zip(got, first):
                        assert a.tobytes() == b.tobytes(), (name, fused, tile, g32)
    assert n_starts >= 100 and n_acc >= 10, (n_starts, n_acc)


# ---------------------------------------------------------------- the error branch

@pytest.mark.parametrize("mode", ["indels", "subs"])
@pytest.mark.parametrize("name", GENE)
def test_error_branch_and_its_variants(gpu, oracle, models, name, mode):
    """glimmer-mg -i / -s: every fifth read against the oracle's recursion; mg_err_wave 0 / 1 / 2 / 3, mg_err_flat and mg_err_tile 1
    byte-identical on all reads"""
    icm, om, _ = models[name]
    W = shape_of(icm)[0]
    ekw = dict(allow_indels=True) if mode == "indels" else dict(allow_subs=True)
    indep, o_indep, prm, ep = gpu.Icm.indep(0.45), oracle.indep(0.45), oracle.mg_params(**KW), oracle.mg_err_params(**ekw)
    n_starts = n_children = 0
    for seqs in read_set(W, 300 + W):
        reads = gpu.Reads.from_strings(seqs)
        first = gpu.mg_score_reads(icm, indep, reads, **KW, **ekw)
        orfs, starts, off, errs = first
        for r in range(0, len(seqs), 5):
            want_orfs, _, scored = oracle.mg_read_errors(om, o_indep, seqs[r].encode(), prm, ep)
            mine = orfs[int(off[r]):int(off[r + 1])]
            assert np.array_equal(np.stack([mine["frame"], mine["stop_position"], mine["gene_len"], mine["orf_len"]], 1).reshape(-1, 4), want_orfs)
            for o, (out, want) in zip(mine, scored):
                sl = slice(o["start_begin"], o["start_begin"] + o["n_starts"])
                assert dev_err_rows(starts[sl], errs[sl]) == err_rows(want), (name, mode, r)
                assert (int(o["lo"]), int(o["hi"]), int(o["accepted"])) == (out.lo, out.hi, out.accepted)
                n_starts += len(want)
                n_children += sum(1 for w in want if w.n_errors)
        for opts in ({"mg_err_wave": 0, "mg_err_tile": 0}, {"mg_err_wave": 1, "mg_err_tile": 0}, {"mg_err_wave": 2, "mg_err_tile": 0},
                     {"mg_err_wave": 3, "mg_err_tile": 0}, {"mg_err_flat": 1}, {"mg_err_tile": 1}):
            old = {k: gpu.get_option(k) for k in opts}
            try:
                for k, v in opts.items():
                    gpu.set_option(k, v)
                got = gpu.mg_score_reads(icm, indep, reads, **KW, **ekw)
            finally:
                for k, v in old.items():
                    gpu.set_option(k, v)
            for a, b in zip(got, first):
                assert a.tobytes() == b.tobytes(), (name, mode, opts)
    assert n_starts >= 100 and n_children >= 10, (n_starts, n_children)


# ---------------------------------------------------------------- glimmer3's Score_Orfs

@pytest.mark.parametrize("path", sorted(ORF_PATHS))
@pytest.mark.parametrize("name", GENE)
def test_score_orfs_every_path(gpu, oracle, models, name, path, request_finalizers):
    """random in-range ORFs (both strands, also lengths that are no multiple of 3) on the ragged reads, NaNs in the running sums
    before they are written: every field of every start and result against the oracle's Score_Orfs"""
    gpu.set_option("orfs_exact_path", ORF_PATHS[path])
    gpu.set_option("orfs_walk8", ORF_WALK.get(path, 4))
    gpu.set_option("orfs_q_poison", 1)
    request_finalizers.append(lambda: (gpu.set_option("orfs_exact_path", 0), gpu.set_option("orfs_walk8", 4), gpu.set_option("orfs_q_poison", 0)))
    icm, om, _ = models[name]
    W = shape_of(icm)[0]
    seqs = [s for s in read_set(W, 400 + W)[0] if len(s) >= 3]
    reads = gpu.Reads.from_strings(seqs)
    rng = np.random.default_rng(W)
    rows = []
    for r, s in enumerate(seqs):
        n = len(s)
        for _ in range(5):
            ln = int(rng.integers(3, n + 1))
            if rng.random() < 0.8:
                ln = max(ln - ln % 3, 3)
            lo = int(rng.integers(0, n - ln + 1))
            rows.append((r, 1 + lo % 3, lo + ln + 1, ln) if rng.random() < 0.5 else (r, -1 - lo % 3, lo - 2, ln))
    rows = np.array(rows)
    kw = dict(min_gene_len=30, allow_truncated=True, ignore_score_len=200)
    res, starts = gpu.score_orfs(icm, gpu.Icm.indep(0.4), reads, rows, **kw)
    o_indep, prm = oracle.indep(0.4), oracle.orf_params(**kw)
    n_genes = 0
    for (r, frame, stop, ln), got in zip(rows, res):
        n, out, want = oracle.score_orf(om, o_indep, seqs[r], int(frame), int(stop), int(ln), prm)
        assert (got["first_j"], got["best_j"], got["best_pos"], got["orf_is_truncated"]) == (out.first_j, out.best_j, out.best_pos, out.orf_is_truncated)
        assert got["best_score"] == out.best_score, (name, path, r)
        if n < 0:
            assert got["n_starts"] == 0 and not got["is_tentative_gene"]
            continue
        assert got["n_starts"] == n and bool(got["is_tentative_gene"]) == bool(out.is_tentative_gene)
        assert got["gene_score"] == out.gene_score or (np.isnan(got["gene_score"]) and np.isnan(out.gene_score))
        st = starts[got["start_begin"]:got["start_begin"] + n]
        assert [(s["j"], s["pos"], s["which"], s["truncated"], s["first"], s["score"]) for s in st] == \
               [(w.j, w.pos, w.which, w.truncated, w.first, w.score) for w in want], (name, path, r)
        n_genes += int(out.is_tentative_gene)
    assert n_genes >= 20, n_genes


# ---------------------------------------------------------------- whole-read Score_String under many models

def test_strings_every_shape_in_one_call(gpu, oracle, models, tmp_path):
    """gmg_score_reads_strings: periodicity-1 and periodicity-3 (and 2 and 4) models of every shape in ONE call, the fused form and
    the two-pass form, both strands of every read against the oracle.  The fused form needs every read to have 86 bases or more:
    `long` is such a ragged batch (118 kbases: several rounds of 32,768 bases, reads across round boundaries, the last read inside
    the batch's last partial chunk); the other two batches (reads from 0 bases on; 40 x 500) take what the library gives them.
    Witness that `long` reaches the fused form's per-read redo: a twin of the 8 / 7 / 1 model with ONE value of exponent field 108
    (below what the fused form takes) scores next to it in the same call."""
    import shutil
    import struct
    names = ALL
    rng = np.random.default_rng(502)
    ragged, uniform = read_set(15, 500)
    long = random_reads(rng, [86, 87, 2 * 15 - 1 + 86] + [int(x) for x in rng.integers(86, 1400, size=160)] + [4097, 100])
    assert min(len(s) for s in long) >= 86 and sum(len(s) for s in long) > 3 * 32768
    icms = [models[n][0] for n in names]
    oms = [models[n][1] for n in names]
    src = models["s1_w8_d7"][2]
    twin = str(tmp_path / "s1_w8_d7_e108.icm")
    shutil.copyfile(src, twin)
    at = int(model_zoo.records(open(src, "rb").read())[-1])                  # the last record: a leaf
    with open(twin, "r+b") as fp:
        fp.seek(at)
        fp.write(struct.pack("<f", -1.5 * 2.0 ** (108 - 127)))
    icms.append(gpu.Icm.open(twin))
    oms.append(oracle.read(twin))
    assert model_zoo.exponent_range(*oracle.tables(oms[-1]))[0] == 108 and model_zoo.exponent_range(*oracle.tables(models["s1_w8_d7"][1]))[0] >= 109
    for seqs in (random_reads(np.random.default_rng(501), range(0, 42)) + ragged, uniform, long):      # (every length around every window)
        reads = gpu.Reads.from_strings(seqs)
        with gpu.option("strings_fused", 1):
            fused = gpu.score_reads_strings(icms, reads)
        with gpu.option("strings_fused", 0):
            two_pass = gpu.score_reads_strings(icms, reads)
        assert fused.tobytes() == two_pass.tobytes()
        for k, om in enumerate(oms):
            for r, s in enumerate(seqs):
                assert fused[k, r, 0] == oracle.score_string(om, s, 0), (k, r, len(s))
                assert fused[k, r, 1] == oracle.score_string(om, revcomp(s), 0), (k, r, len(s))
    assert len({shape_of(models[n][0]) for n in names}) >= 15


# ---------------------------------------------------------------- the segment kernels and the window distribution

@pytest.mark.parametrize("name", ALL)
def test_segment_kernels_and_windows(gpu, oracle, models, name):
    """cumulative score, frame score, score string and partial probability: all four orientations, frames 0 .. P - 1, the
    completed-tree form and the plain descent (seg_plain); Full_Window_Distrib / _Prob on random windows"""
    icm, om, _ = models[name]
    W, _, P = shape_of(icm)
    rng = np.random.default_rng(600 + W)
    seqs = random_reads(rng, [700, 50, 2 * W - 1, W, W - 1, max(W - 2, 1), 1])
    reads = gpu.Reads.from_strings(seqs)
    rows = []
    for r, s in enumerate(seqs):
        for orient in range(4):
            rows.append((r, 0, len(s), orient))
            for _ in range(3):
                ln = int(rng.integers(0, len(s) + 1))
                rows.append((r, int(rng.integers(0, len(s) - ln + 1)), ln, orient))
    segs = gpu.Segments(reads, rows)
    bufs = [oracle.buffer(seqs[r], lo, ln, orient) for r, lo, ln, orient in rows]
    assert any(len(b) < W - 1 for b in bufs) and any(len(b) == W - 1 for b in bufs)
    for plain in (0, 1):
        with gpu.option("seg_plain", plain):
            for f in range(P):
                cum = segs.split(gpu.segment_cumscore(icm, reads, segs, f))
                per = segs.split(gpu.segment_frame_score(icm, reads, segs, f))
                tot = gpu.score_string(icm, reads, segs, f)
                part = gpu.segment_partial_prob(icm, reads, segs, f)
                for i, buf in enumerate(bufs):
                    assert np.array_equal(cum[i], oracle.cumulative_score(om, buf, f)), (name, plain, f, i)
                    assert np.array_equal(per[i], oracle.frame_score(om, buf, f)), (name, plain, f, i)
                    assert tot[i] == oracle.score_string(om, buf, f), (name, plain, f, i)
                    if len(buf):
                        assert part[i] == oracle.partial_window(om, len(buf) - 1, buf, f), (name, plain, f, i)
    codes = rng.integers(0, 4, size=(512, W)).astype(np.uint8)
    for f in range(P):
        dist, prob = gpu.window_distrib(icm, codes, np.full(len(codes), f, np.int32))
        for i in range(len(codes)):
            p, d = oracle.full_window(om, bytes(b"acgt"[c] for c in codes[i]), f)
            assert prob[i] == p and np.array_equal(dist[i].view(np.uint32), d.view(np.uint32)), (name, f, i)


# ---------------------------------------------------------------- groups of models in one call

@pytest.mark.parametrize("mix", ["mixed_shapes", "all_w15"])
@pytest.mark.parametrize("mode", ["default", "indel"])
def test_groups_of_other_shapes(gpu, oracle, models, mix, mode):
    """gmg_mg_score_groups: one call whose groups mix 12 / 7, 15 / 7, 8 / 7, 12 / 4 and 16 / 8 models (not all_fast), and one whose
    groups are all 15 / 7 models (all_fast at a W other than 12) = gmg_mg_score_reads group by group, byte for byte; every
    fifth read against the oracle"""
    data = os.path.join(model_zoo.GOLD, "data")
    if mix == "mixed_shapes":
        nc = os.path.join(data, "NC_000915.icm")
        pairs = [(gpu.Icm.open(nc), oracle.read(nc)), models["s3_w15_d7"][:2], models["s3_w8_d7"][:2], models["syn_d4"][:2],
                 models["c3_w16_d8_r"][:2]]
        assert [shape_of(p[0])[:2] for p in pairs] == [(12, 7), (15, 7), (8, 7), (12, 4), (16, 8)]
    else:
        twin = models["s3_w15_d7"]                               # (eligible as it is: model_zoo.zoo asserts it)
        pairs = [(gpu.Icm.open(twin[2]), twin[1]) for _ in range(3)]
    rng = np.random.default_rng(len(mix) + len(mode))
    lens = [0, 1, 13, 14, 15, 16, 28, 29] + [int(x) for x in rng.integers(1, 900, 400)] + [1500, 2100]
    if mode == "indel":
        lens = lens[:120] + [1500]
    seqs = random_reads(rng, lens)
    n = len(seqs)
    cuts = [0, n // 7, n // 7 + 1, n // 3, n // 3, n // 2, (3 * n) // 4, n]
    groups = [(pairs[g % len(pairs)][0], cuts[g], cuts[g + 1]) for g in range(len(cuts) - 1)]
    group_of = np.searchsorted(cuts, np.arange(n), side="right") - 1
    reads = gpu.Reads.from_strings(seqs)
    nulls = gpu.NullSet.build(GCS)
    read_null = rng.integers(0, len(GCS), n).astype(np.uint32)
    kw = dict(min_gene_len=60, allow_indels=mode == "indel")
    whole = gpu.mg_score_reads(None, nulls, reads, read_null=read_null, groups=groups, **kw)
    n_orfs = 0
    for m, b, e in groups:
        if b == e:
            continue
        part = gpu.mg_score_reads(m, nulls, reads.select(np.arange(b, e, dtype=np.uint64)), read_null=read_null[b:e], **kw)
        o0, o1 = int(whole[2][b]), int(whole[2][e])
        mine = whole[0][o0:o1].copy()
        assert len(mine) == len(part[0])
        if len(mine) == 0:
            continue
        s0 = int(mine["start_begin"][0])
        s1 = int(mine["start_begin"][-1]) + int(mine["n_starts"][-1])
        mine["read"] -= b
        mine["start_begin"] -= s0
        assert mine.tobytes() == part[0].tobytes(), (mix, mode, b, e)
        assert whole[1][s0:s1].tobytes() == part[1].tobytes(), (mix, mode, b, e)
        if mode == "indel":
            assert whole[3][s0:s1].tobytes() == part[3].tobytes(), (mix, mode, b, e)
        n_orfs += len(mine)
    assert n_orfs == len(whole[0]) > 100
    prm = oracle.mg_params(min_gene_len=60)
    ep = oracle.mg_err_params(allow_indels=True)
    n_starts = 0
    for r in range(0, n, 5):
        om = pairs[(group_of[r]) % len(pairs)][1]
        o_indep = oracle.indep(GCS[read_null[r]])
        mine = whole[0][int(whole[2][r]):int(whole[2][r + 1])]
        if mode == "indel":
            _, _, scored = oracle.mg_read_errors(om, o_indep, seqs[r].encode(), prm, ep)
            assert len(mine) == len(scored)
            for o, (out, want) in zip(mine, scored):
                sl = slice(o["start_begin"], o["start_begin"] + o["n_starts"])
                assert dev_err_rows(whole[1][sl], whole[3][sl]) == err_rows(want), (mix, r)
                n_starts += len(want)
        else:
            _, scored = oracle.mg_read(om, o_indep, seqs[r].encode(), prm)
            assert len(mine) == len(scored)
            for o, (out, want) in zip(mine, scored):
                st = whole[1][o["start_begin"]:o["start_begin"] + o["n_starts"]]
                assert mg_rows(st) == [(w.j, w.pos, w.which, w.truncated, w.first, w.score) for w in want], (mix, r)
                assert o["best_score"] == out.best_score and bool(o["accepted"]) == bool(out.accepted)
                n_starts += len(want)
    assert n_starts >= 100
