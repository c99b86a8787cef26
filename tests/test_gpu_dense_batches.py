"""Batches dense in short reads and in ORFs through every batched entry point, at the caps each kernel keeps per tile, wave or
round (tests/dense_batches.py: the builders, the table of caps and the preconditions; tests/test_dense_batches_host.py shows the
preconditions without a GPU).  Every comparison is against the CPU oracle read by read -- integer fields equal, doubles bit for
bit -- or, where the oracle has no say (the packed words of a selection, gathered table rows), against numpy.  Each test asserts
the precondition of its batch before it calls the device; a batch that misses its cap fails, it does not skip.  Run with -m gpu."""
import os

import numpy as np
import pytest

import dense_batches as db
import model_zoo
from conftest import DATA
from test_gpu_mg_err import dev_err_rows
from test_gpu_parity import ORF_PATHS
from test_gpu_train import check_levels
from test_oracle_mg import err_rows

pytestmark = pytest.mark.gpu

NC = os.path.join(DATA, "NC_000915.icm")
GICM = os.path.join(DATA, "seqs.cluster-4.run1.filt.gicm")
SYN_D4 = os.path.join(model_zoo.TRAIN, "syn_d4.icm")                # window 12, depth 4: the any-shape kernels
GC = 0.47
GCS37 = [float(x) for x in np.linspace(0.26, 0.74, 37)]
UNIFORM = ["short_uniform[%d]" % L for L in db.UNIFORM_LENGTHS]
BUILDERS = dict({"short_ragged": db.short_ragged, "short_ragged_long": db.short_ragged_long, "orf_dense": db.orf_dense,
                 "strings_86": db.strings_86, "strings_85": db.strings_85, "strings_86_rounds": db.strings_86_rounds},
                **{"short_uniform[%d]" % L: (lambda L=L: db.short_uniform(L)) for L in db.UNIFORM_LENGTHS})
ERR_MODES = {"indels": (dict(allow_indels=True), False), "indels_q": (dict(allow_indels=True), True), "subs": (dict(allow_subs=True), False)}
ERR_PATHS = {"wave": {"mg_err_wave": 1, "mg_err_tile": 0}, "wave-walk": {"mg_err_wave": 2, "mg_err_tile": 0},
             "wave-mixed": {"mg_err_wave": 3, "mg_err_tile": 0}, "tile": {"mg_err_tile": 1},
             "level": {"mg_err_tile": 0, "mg_err_wave": 0}, "flat": {"mg_err_flat": 1}}     # as test_error_branch_every_orf_vs_oracle sets them

_cache = {}


def cached(key, make):
    """a reference is computed once and shared; nothing changes it afterwards"""
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def batch(name):
    return cached(("batch", name), BUILDERS[name])


def device_reads(gpu, name):
    return cached(("reads", name), lambda: gpu.Reads.from_strings(batch(name)))


def o_model(oracle, path):
    return cached(("o_model", path), lambda: oracle.read(path))


def d_model(gpu, path):
    return cached(("d_model", path), lambda: gpu.Icm.open(path))


def precondition(oracle, name):
    """the precondition of the batch, from offsets and the oracle alone; AssertionError when the batch misses its cap"""
    def check():
        seqs = batch(name)
        if name == "short_ragged":
            db.require_short_ragged(seqs)
            db.require_orfbits_window(seqs)
            for err in (False, True):
                db.require_orfs_per_64_reads(oracle, seqs, err, **db.MG_KW)
            for nulls in (False, True):
                db.require_front_half_tiles(oracle, seqs, nulls, **db.MG_KW)
            db.require_error_tiles(oracle, seqs, **db.MG_KW)
        elif name == "short_ragged_long":
            db.require_short_ragged_long(seqs)
            db.require_orfbits_window(seqs)
            db.require_orfs_per_64_reads(oracle, seqs, False, **db.MG_KW)
            for nulls in (False, True):
                db.require_front_half_tiles(oracle, seqs, nulls, **db.MG_KW)
        elif name == "orf_dense":
            db.require_orf_dense(oracle, seqs, **db.MG_KW)
        elif name in ("strings_86", "strings_85"):
            db.require_strings_round(seqs, name == "strings_86")
        elif name == "strings_86_rounds":
            db.require_strings_full_rounds(seqs)
        else:
            L = len(seqs[0])
            assert len(seqs) == 2000 and {len(s) for s in seqs} == {L}
            if L < 11:
                db.require_all_heads(seqs, 12)
            assert 504 // L > 6 and (L > 3 or 504 // L > 64)             # whole reads under a one-wave tile's bases: more than MT_NC, and (1 .. 3 bases) than MG_TILE_READS
        return True
    return cached(("pre", name), check)


@pytest.fixture
def options(gpu):
    """set(dict): library switches for the rest of the test"""
    old = {}

    def set_(opts):
        for k, v in opts.items():
            old.setdefault(k, gpu.get_option(k))
            gpu.set_option(k, v)
    yield set_
    for k, v in old.items():
        gpu.set_option(k, v)


# ---------------------------------------------------------------- comparing a result of the front half with the oracle's

def want_default(oracle, name, path, per_read=None):
    """the oracle's front half of every read of the batch: [(orfs [n, 4], [(fields of MgOut, start rows)])]; per_read: (GC values,
    read_null, read_ignore_score_len) of the classification mode"""
    def make():
        om, out = o_model(oracle, path), []
        nulls = [oracle.indep(gc) for gc in per_read[0]] if per_read else [oracle.indep(GC)]
        for r, s in enumerate(batch(name)):
            isl = int(per_read[2][r]) if per_read else db.MG_KW["ignore_score_len"]
            prm = oracle.mg_params(min_gene_len=db.MG_KW["min_gene_len"], ignore_score_len=isl)
            orfs, scored = oracle.mg_read(om, nulls[int(per_read[1][r]) if per_read else 0], s.encode(), prm)
            out.append((orfs, [((o.lo, o.hi, o.first_j, bool(o.accepted), o.orf_is_truncated, o.best_score),
                                [(w.j, w.pos, w.which, w.truncated, w.first, w.score) for w in st]) for o, st in scored]))
        return out
    return cached(("want", name, path, per_read is not None), make)


def mg_rows(starts):
    return [(int(s["j"]), int(s["pos"]), int(s["which"]), int(s["truncated"]), int(s["first"]), float(s["score"])) for s in starts]


def assert_front_half(got, want, tag):
    orfs, starts, off = got[:3]
    assert int(off[-1]) == len(orfs) == sum(len(w[0]) for w in want), tag
    n_starts = n_acc = 0
    for r, (want_orfs, scored) in enumerate(want):
        mine = orfs[int(off[r]):int(off[r + 1])]
        assert np.array_equal(np.stack([mine["frame"], mine["stop_position"], mine["gene_len"], mine["orf_len"]], 1).reshape(-1, 4), want_orfs), (tag, r)
        assert np.all(mine["read"] == r), (tag, r)
        for o, (fields, rows) in zip(mine, scored):
            st = starts[int(o["start_begin"]):int(o["start_begin"]) + int(o["n_starts"])]
            assert mg_rows(st) == rows, (tag, r)
            assert (int(o["lo"]), int(o["hi"]), int(o["first_j"]), o["accepted"] != 0, int(o["orf_is_truncated"]), float(o["best_score"])) == fields, (tag, r)
            n_starts += len(rows)
            n_acc += int(fields[3])
    assert n_starts == len(starts), tag
    return n_starts, n_acc


def want_errors(oracle, name, mode, path=NC):
    """the oracle's error branch of every read: [(orfs, [((lo, hi, accepted, best score, first_j), rows with error lists)])]"""
    def make():
        ekw, with_q = ERR_MODES[mode]
        seqs = batch(name)
        quals = db.quality_12_percent(seqs, 19) if with_q else [None] * len(seqs)
        om, o_indep = o_model(oracle, path), oracle.indep(GC)
        prm, ep = oracle.mg_params(**db.MG_KW), oracle.mg_err_params(**ekw)
        out = []
        for s, q in zip(seqs, quals):
            orfs, _, scored = oracle.mg_read_errors(om, o_indep, s.encode(), prm, ep, q)
            out.append((orfs, [((o.lo, o.hi, o.accepted, o.best_score if o.accepted else None, o.first_j if o.accepted else None), err_rows(st))
                               for o, st in scored]))
        quality = np.concatenate(quals).astype(np.uint8) if with_q else None
        return out, quality
    return cached(("want_err", name, mode, path), make)


def assert_error_branch(got, want, tag):
    orfs, starts, off, errs = got
    assert int(off[-1]) == len(orfs) == sum(len(w[0]) for w in want), tag
    n_starts = n_children = 0
    for r, (want_orfs, scored) in enumerate(want):
        mine = orfs[int(off[r]):int(off[r + 1])]
        assert np.array_equal(np.stack([mine["frame"], mine["stop_position"], mine["gene_len"], mine["orf_len"]], 1).reshape(-1, 4), want_orfs), (tag, r)
        for o, (fields, rows) in zip(mine, scored):
            sl = slice(int(o["start_begin"]), int(o["start_begin"]) + int(o["n_starts"]))
            assert dev_err_rows(starts[sl], errs[sl]) == rows, (tag, r)
            assert (int(o["lo"]), int(o["hi"]), int(o["accepted"])) == fields[:3], (tag, r)
            if fields[2]:
                assert (float(o["best_score"]), int(o["first_j"])) == fields[3:], (tag, r)
            n_starts += len(rows)
            n_children += sum(1 for w in rows if w[5])
    assert n_starts == len(starts) == len(errs), tag
    return n_starts, n_children


# ---------------------------------------------------------------- 1. the six-frame table

def plain_frame_score6(gpu, gene, null, reads):
    """gmg_frame_score6 itself (gpu.frame_score6 goes through the strided entry point)"""
    buf = gpu.api._DeviceBuffer(6 * max(reads.total_bases, 1) * 8)
    rc = gpu.capi.lib().gmg_frame_score6(gene.device(), null.device(), reads.h, buf.ptr, None)
    assert rc == 0, gpu.capi.lib().gmg_last_error()
    assert gpu.capi.lib().gmg_synchronize(None) == 0
    out = buf.to_host(np.float64, 6 * reads.total_bases).reshape(6, reads.total_bases)
    buf.free()
    return out


@pytest.mark.parametrize("model", [NC, SYN_D4], ids=["w12_d7", "w12_d4_generic"])
@pytest.mark.parametrize("name", ["short_ragged"] + UNIFORM)
def test_six_frame_table_of_every_read(gpu, oracle, name, model):
    """gmg_frame_score6, gmg_frame_score6_strided (stride total + 1: odd or even, never the batch's own) and gmg_frame_score6_nulls
    (37 GC values, a random one per read): all six rows of every read.  Hundreds of reads per 2,048-base chunk; with 1 .. 3
    bases (and in the first half of short_ragged) every base is a partial-window head of k_frame6p, eight reads per block."""
    assert precondition(oracle, name)
    seqs, reads = batch(name), device_reads(gpu, name)
    off = db.offsets(seqs)
    icm, om = d_model(gpu, model), o_model(oracle, model)
    assert icm.params[:3] == ((12, 7, 3) if model == NC else (12, 4, 3))
    o_indep = oracle.indep(GC)
    want = cached(("six", name, model), lambda: np.concatenate([oracle.score_all_frames(om, o_indep, s) for s in seqs], axis=1))
    assert want.shape == (6, reads.total_bases)
    indep = gpu.Icm.indep(GC)
    for tag, got in (("plain", plain_frame_score6(gpu, icm, indep, reads)), ("strided", gpu.frame_score6(icm, indep, reads, row_stride=reads.total_bases + 1))):
        bad = np.flatnonzero((got != want).any(axis=0))
        assert len(bad) == 0, (tag, name, "first base that differs", int(bad[0]), "of read", int(np.searchsorted(off, bad[0], side="right") - 1))
    rng = np.random.default_rng(len(name))
    read_null = rng.integers(0, len(GCS37), size=len(seqs)).astype(np.uint32)
    o_nulls = [oracle.indep(gc) for gc in GCS37]
    want_n = np.concatenate([oracle.score_all_frames(om, o_nulls[k], s) for k, s in zip(read_null, seqs)], axis=1)
    got = gpu.frame_score6(icm, gpu.NullSet.build(GCS37), reads, read_null=read_null)
    bad = np.flatnonzero((got != want_n).any(axis=0))
    assert len(bad) == 0, ("nulls", name, int(bad[0]), int(np.searchsorted(off, bad[0], side="right") - 1))
    assert not np.array_equal(want, want_n)


# ---------------------------------------------------------------- 2. the front half, default mode

FRONT = ["short_ragged", "short_ragged_long", "short_uniform[12]", "short_uniform[40]"]


@pytest.mark.parametrize("name", FRONT)
def test_front_half_every_read_and_every_kernel_choice(gpu, oracle, name):
    """gmg_mg_score_reads with min_gene_len 6 and ignore_score_len 12: every read's ORF records and start lists in push order against
    the oracle.  The two ragged batches: under every tiling these options give, some windows receive more reads than the MG_TILE_READS = 64
    a tile takes (the surplus goes to the per-lane kernel, MgPlan.rest), and some tile's reads carry more than MT_ORFS = 64 ORFs (stages
    3 and 4 of k_mg_tile_starts loop).  The two uniform batches make no such claim: their tiles take whole reads by arithmetic, fewer than
    64 under the default plan.  Then mg_fused 0 / 1 x
    mg_tile 0 / 1 / 2 / 4 x mg_gene32 0 / 2 x mg_orfs_bits 0 / 1 x mg_orfs_events 0 / 1 / 2: every byte as with the defaults."""
    assert precondition(oracle, name)
    reads, icm, indep = device_reads(gpu, name), d_model(gpu, NC), gpu.Icm.indep(GC)
    first = gpu.mg_score_reads(icm, indep, reads, **db.MG_KW)
    n_starts, n_acc = assert_front_half(first, want_default(oracle, name, NC), name)
    assert n_starts > 1000 and n_acc > 500, (n_starts, n_acc)
    for fused in (0, 1):
        for tile in (0, 1, 2, 4):
            for g32 in (0, 2):
                for bits in (0, 1):
                    for events in (0, 1, 2):
                        with gpu.option("mg_fused", fused), gpu.option("mg_tile", tile), gpu.option("mg_gene32", g32), \
                                gpu.option("mg_orfs_bits", bits), gpu.option("mg_orfs_events", events):
                            got = gpu.mg_score_reads(icm, indep, reads, **db.MG_KW)
                        for a, b in zip(got, first):
                            assert a.tobytes() == b.tobytes(), (name, fused, tile, g32, bits, events)


@pytest.mark.parametrize("gene32", [2, 0])
@pytest.mark.parametrize("fused", [1, 0])
@pytest.mark.parametrize("name", FRONT)
def test_front_half_with_a_null_model_and_an_ignore_score_len_per_read(gpu, oracle, name, fused, gene32):
    """nulls / read_null / read_ignore_score_len (2^31 - 1, 12 or 20 per read): every read against the oracle with its own null model
    and its own length.  A fused tile of the GENE32 form with a null model per read holds MT_NC = 6 reads: every batch here has more
    reads than that under a tile's bases (the ragged ones by require_front_half_tiles, the uniform ones because 504 // L > 6)."""
    assert precondition(oracle, name)
    seqs = batch(name)
    rng = np.random.default_rng(7 + len(name))
    per_read = cached(("per_read", name), lambda: (GCS37, rng.integers(0, len(GCS37), len(seqs)).astype(np.uint32),
                                                   rng.choice([2 ** 31 - 1, 12, 20], len(seqs)).astype(np.int32)))
    assert len(set(per_read[2].tolist())) == 3
    kw = dict(db.MG_KW)
    del kw["ignore_score_len"]
    with gpu.option("mg_fused", fused), gpu.option("mg_gene32", gene32):
        got = gpu.mg_score_reads(d_model(gpu, NC), gpu.NullSet.build(GCS37), device_reads(gpu, name), read_null=per_read[1],
                                 read_ignore_score_len=per_read[2], **kw)
    n_starts, n_acc = assert_front_half(got, want_default(oracle, name, NC, per_read), (name, fused, gene32))
    assert n_starts > 1000 and n_acc > 500


@pytest.mark.parametrize("bits", [1, 0])
@pytest.mark.parametrize("name", FRONT)
def test_find_orfs_alone(gpu, oracle, name, bits):
    """gmg_find_orfs against the oracle's Find_Orfs.  The two ragged batches: some windows of the bit-mask finder (9.5 mean read lengths)
    hold the begins of more than the OB_GROUP = 10 reads a wave walks at a time; a uniform batch has exactly 10 reads per window"""
    assert precondition(oracle, name)
    seqs = batch(name)
    kw = dict(min_gene_len=6, allow_truncated=True)
    with gpu.option("mg_orfs_bits", bits):
        orfs, off = gpu.find_orfs(device_reads(gpu, name), **kw)
    prm = oracle.mg_params(**kw)
    want = cached(("find", name), lambda: [oracle.find_orfs(s, prm) for s in seqs])
    assert int(off[-1]) == len(orfs) == sum(map(len, want)) > 2000
    for r, w in enumerate(want):
        mine = orfs[int(off[r]):int(off[r + 1])]
        assert np.array_equal(np.stack([mine["frame"], mine["stop_position"], mine["gene_len"], mine["orf_len"]], 1).reshape(-1, 4), w), (name, r)
        assert np.all(mine["read"] == r)


# ---------------------------------------------------------------- 3. the error branch

@pytest.mark.parametrize("path", sorted(ERR_PATHS))
@pytest.mark.parametrize("mode", sorted(ERR_MODES))
@pytest.mark.parametrize("name", ["short_ragged", "orf_dense"])
def test_error_branch_every_start_with_its_error_list(gpu, oracle, name, mode, path, options):
    """-i (Set_Quality_454), -i with a quality array (12 % of the bases below 19) and -s, through the wave kernels, the tile kernel,
    the level kernels and the per-ORF kernel: every start of every ORF with its error list, in push order.  short_ragged: tiles closed
    by their ET_MAXR = 64th read and tiles with more than ET_MAXO = 192 ORF records (require_error_tiles).  orf_dense: reads with more than EW_MAXO = 64 ORF records on one
    strand -- nloc of the wave kernels counts the records of one (read, strand) that Find_Orfs kept, accepted or not -- so a forced
    wave path gives up (`overflow`) and the whole batch repeats on the level kernels."""
    assert precondition(oracle, name)
    want, quality = want_errors(oracle, name, mode)
    options(ERR_PATHS[path])
    got = gpu.mg_score_reads(d_model(gpu, NC), gpu.Icm.indep(GC), device_reads(gpu, name), quality=quality, **db.MG_KW, **ERR_MODES[mode][0])
    n_starts, n_children = assert_error_branch(got, want, (name, mode, path))
    assert n_starts > 2000 and n_children > 400, (n_starts, n_children)


@pytest.mark.parametrize("mode", sorted(ERR_MODES))
def test_default_error_path_survives_the_orf_count_overflow(gpu, oracle, mode):
    """orf_dense with the library's own choice of kernels (one wave per (read, strand)): the count pass meets reads with more than 64
    ORF records per strand and the call repeats on the level kernels -- the same bytes as the level kernels asked for directly, and
    the oracle's lists"""
    assert precondition(oracle, "orf_dense")
    want, quality = want_errors(oracle, "orf_dense", mode)
    reads, icm, indep = device_reads(gpu, "orf_dense"), d_model(gpu, NC), gpu.Icm.indep(GC)
    assert (gpu.get_option("mg_err_wave"), gpu.get_option("mg_err_flat")) == (1, 0) and gpu.get_option("mg_err_tile") <= 0
    kw = dict(db.MG_KW, quality=quality, **ERR_MODES[mode][0])
    default = gpu.mg_score_reads(icm, indep, reads, **kw)
    with gpu.option("mg_err_wave", 0), gpu.option("mg_err_tile", 0):
        level = gpu.mg_score_reads(icm, indep, reads, **kw)
    for a, b in zip(default, level):
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()
    assert_error_branch(default, want, ("orf_dense", mode, "default"))
    for acc in (False, True):                                             # ... and on the accepted ORFs only, twice the same bytes
        a = gpu.mg_score_reads(icm, indep, reads, accepted_only=acc, **kw)
        with gpu.option("mg_err_wave", 0), gpu.option("mg_err_tile", 0):
            b = gpu.mg_score_reads(icm, indep, reads, accepted_only=acc, **kw)
        for x, y in zip(a, b):
            assert x.tobytes() == y.tobytes(), acc


# ---------------------------------------------------------------- 4. whole-read string sums

def fused_takes(oracle, om):
    """what gmg_score_reads_strings asks of a model before it sums inside the main pass, from the oracle's tables"""
    lo, hi, odd = model_zoo.exponent_range(*oracle.tables(om))
    return not odd and lo >= 109 and hi - lo <= 23


@pytest.mark.parametrize("name", ["strings_86", "strings_85"])
def test_string_sums_at_the_length_that_opens_the_fused_form(gpu, oracle, name):
    """gmg_score_reads_strings on 900 reads of 86 bases (and a few of 87 and 88: not uniform, so the fused form finds its reads through
    s_roff), and the same with one read of 85 bases, which takes the two-pass form.  strings_fused 1 against 0 byte for byte, every read
    and its reverse complement against the oracle, two periodicity-1 models.  (A batch this small gives every work-group one chunk:
    rounds of about 25 reads.  Full rounds: test_string_sums_with_full_rounds.)"""
    assert precondition(oracle, name)
    seqs, reads = batch(name), device_reads(gpu, name)
    paths = [os.path.join(DATA, "cluster-0.icm"), os.path.join(DATA, "cluster-3.icm")]
    oms = [o_model(oracle, p) for p in paths]
    assert all(om.contents.periodicity == 1 and fused_takes(oracle, om) for om in oms)
    icms = [d_model(gpu, p) for p in paths]
    with gpu.option("strings_fused", 1):
        fused = gpu.score_reads_strings(icms, reads)
    with gpu.option("strings_fused", 0):
        two_pass = gpu.score_reads_strings(icms, reads)
    assert fused.tobytes() == two_pass.tobytes()
    for k, om in enumerate(oms):
        for r, s in enumerate(seqs):
            assert fused[k, r, 0] == oracle.score_string(om, s, 0), (name, k, r)
            assert fused[k, r, 1] == oracle.score_string(om, db.revcomp(s), 0), (name, k, r)


def test_string_sums_with_full_rounds(gpu, oracle):
    """92,000 reads of 86 to 88 bases: every work-group of the fused form gets 16 chunks or more, so it runs full rounds of 14 chunks
    (28,672 bases, 334 or 335 reads with an accumulator in LDS: as many as reads of 86 bases or more can put into a round -- NR_MAX =
    384 is out of reach of any batch), partial rounds, and reads that straddle rounds and work-groups.  strings_fused 1 against 0 byte
    for byte under two periodicity-1 models; against the oracle every read and its reverse complement under the first model, every
    eighth read under the second."""
    assert precondition(oracle, "strings_86_rounds")
    seqs, reads = batch("strings_86_rounds"), device_reads(gpu, "strings_86_rounds")
    paths = [os.path.join(DATA, "cluster-0.icm"), os.path.join(DATA, "cluster-3.icm")]
    oms = [o_model(oracle, p) for p in paths]
    assert all(om.contents.periodicity == 1 and fused_takes(oracle, om) for om in oms)
    icms = [d_model(gpu, p) for p in paths]
    with gpu.option("strings_fused", 1):
        fused = gpu.score_reads_strings(icms, reads)
    with gpu.option("strings_fused", 0):
        two_pass = gpu.score_reads_strings(icms, reads)
    bad = np.flatnonzero((fused.view(np.uint64) != two_pass.view(np.uint64)).reshape(2, len(seqs), 2).any(axis=(0, 2)))
    assert len(bad) == 0, ("first read whose sums differ between the two forms", int(bad[0]), "of", len(bad))
    for k, (om, step) in enumerate(zip(oms, (1, 8))):
        want = np.array([(oracle.score_string(om, s, 0), oracle.score_string(om, db.revcomp(s), 0)) for s in seqs[::step]])
        bad = np.flatnonzero((fused[k, ::step] != want).any(axis=1))
        assert len(bad) == 0, ("model", k, "first read that differs from the oracle", int(bad[0]) * step, "of", len(bad))


@pytest.mark.parametrize("name", ["short_ragged"] + UNIFORM)
def test_string_sums_of_short_reads(gpu, oracle, name):
    """every read and its reverse complement under a periodicity-1 model (the strings main pass; hundreds of reads per chunk, reads
    shorter than the window) and under a periodicity-3 model, which takes the segment kernel"""
    assert precondition(oracle, name)
    seqs, reads = batch(name), device_reads(gpu, name)
    paths = [os.path.join(DATA, "cluster-2.icm"), NC]
    oms = [o_model(oracle, p) for p in paths]
    assert [om.contents.periodicity for om in oms] == [1, 3]
    got = gpu.score_reads_strings([d_model(gpu, p) for p in paths], reads)
    assert got.shape == (2, len(seqs), 2)
    for k, om in enumerate(oms):
        for r, s in enumerate(seqs):
            assert got[k, r, 0] == oracle.score_string(om, s, 0), (name, k, r, len(s))
            assert got[k, r, 1] == oracle.score_string(om, db.revcomp(s), 0), (name, k, r, len(s))


# ---------------------------------------------------------------- 5. a selection of short reads

def test_selection_packed_words_offsets_and_table(gpu, oracle):
    """gmg_reads_select with 5,000 indices into short_ragged: most 1,024-base tiles of the new batch hold more than the SEL_R = 32
    reads a wave keeps in LDS (the lane finishes its word base by base).  The packed words and offsets of the new batch are those of
    Reads.from_strings on the same strings (every word, the partial last one included: the code zeroes what lies beyond the
    batch's bases); its six-frame table is the source batch's table, rows gathered with numpy."""
    assert precondition(oracle, "short_ragged")
    seqs, reads = batch("short_ragged"), device_reads(gpu, "short_ragged")
    idx = db.selection(len(seqs))
    db.require_selection(seqs, idx)
    sub = reads.select(idx)
    packed, off = sub.download()
    chosen = [seqs[int(i)] for i in idx]
    want_packed, want_off = gpu.api.pack_strings(chosen)
    assert np.array_equal(off, want_off) and np.array_equal(off.astype(np.int64), db.offsets(chosen))
    words = (int(off[-1]) + 15) // 16
    assert len(packed) >= words
    bad = np.flatnonzero(packed[:words] != want_packed[:words])
    assert len(bad) == 0, ("first word that differs", int(bad[0]), "of", words)
    ref = gpu.Reads.from_strings(chosen).download()
    assert np.array_equal(ref[0], packed) and np.array_equal(ref[1], off)
    icm, indep = d_model(gpu, NC), gpu.Icm.indep(GC)
    full = gpu.frame_score6(icm, indep, reads)
    src = db.offsets(seqs)
    gather = np.concatenate([np.arange(src[int(i)], src[int(i) + 1]) for i in idx])
    got = gpu.frame_score6(icm, indep, sub)
    assert got.shape == (6, len(gather)) and np.array_equal(got, full[:, gather])
    assert np.array_equal(full, cached(("six", "short_ragged", NC), lambda: np.concatenate(
        [oracle.score_all_frames(o_model(oracle, NC), oracle.indep(GC), s) for s in seqs], axis=1)))


# ---------------------------------------------------------------- 6. the glimmer3 side

@pytest.mark.parametrize("path", ["events", "exact", "fused"])
def test_score_orfs_on_the_orfs_of_short_reads(gpu, oracle, path, options):
    """the ORFs gmg_find_orfs reports on short_ragged_long (thousands of them three to thirteen codons long, next to those of the
    long reads) through gmg_score_orfs: every result and every start against the oracle's Score_Orfs"""
    assert precondition(oracle, "short_ragged_long")
    seqs, reads = batch("short_ragged_long"), device_reads(gpu, "short_ragged_long")
    found, _ = gpu.find_orfs(reads, min_gene_len=6, allow_truncated=True)
    rows = np.stack([found["read"].astype(np.int64), found["frame"], found["stop_position"], found["orf_len"]], 1)
    prm_f = oracle.mg_params(min_gene_len=6, allow_truncated=True)
    want_rows = cached(("g3_rows",), lambda: np.concatenate(
        [np.concatenate([np.full((len(o), 1), r, np.int64), o[:, [0, 1, 3]]], axis=1) for r, o in enumerate(oracle.find_orfs(s, prm_f) for s in seqs)]))
    assert np.array_equal(rows, want_rows) and len(rows) > 5000
    options({"orfs_exact_path": ORF_PATHS[path], "orfs_q_poison": 1})
    kw = dict(min_gene_len=6, allow_truncated=True, ignore_score_len=12)
    res, starts = gpu.score_orfs(d_model(gpu, NC), gpu.Icm.indep(GC), reads, rows, **kw)
    om, o_indep, prm = o_model(oracle, NC), oracle.indep(GC), oracle.orf_params(**kw)

    def make():
        out = []
        for r, frame, stop, ln in rows:
            n, o, st = oracle.score_orf(om, o_indep, seqs[r], int(frame), int(stop), int(ln), prm)
            out.append((n, (o.first_j, o.best_j, o.best_pos, o.orf_is_truncated, o.best_score), bool(o.is_tentative_gene), o.gene_score,
                        [(w.j, w.pos, w.which, w.truncated, w.first, w.score) for w in st]))
        return out
    n_genes = n_starts = 0
    for i, (got, (n, fields, gene, gene_score, want)) in enumerate(zip(res, cached(("g3_want",), make))):
        assert (int(got["first_j"]), int(got["best_j"]), int(got["best_pos"]), int(got["orf_is_truncated"]), float(got["best_score"])) == fields, (path, i)
        if n < 0:
            assert got["n_starts"] == 0 and not got["is_tentative_gene"], (path, i)
            continue
        assert got["n_starts"] == n and bool(got["is_tentative_gene"]) == gene, (path, i)
        assert got["gene_score"] == gene_score or (np.isnan(got["gene_score"]) and np.isnan(gene_score)), (path, i)
        st = starts[int(got["start_begin"]):int(got["start_begin"]) + n]
        assert mg_rows(st) == want, (path, i)
        n_genes += int(gene)
        n_starts += n
    assert n_genes > 500 and n_starts > 2000, (n_genes, n_starts)


# ---------------------------------------------------------------- 7. one group per read

@pytest.mark.parametrize("mode", ["default", "indels"])
def test_one_group_per_read(gpu, oracle, mode):
    """gmg_mg_score_groups with one group per read on the 9 .. 40-base half of short_ragged: three models in rotation (12 / 7, 12 / 7
    and the 12 / 4 model train/syn_d4.icm), more than 50 groups per 2,048-base chunk (a group change at every read), a null model
    per read.  Every read against the oracle with its group's model and its own null model."""
    seqs = batch("short_ragged")[1500:]
    db.require_groups(seqs)
    paths = [NC, GICM, SYN_D4]
    oms = [o_model(oracle, p) for p in paths]
    assert [(om.contents.model_len, om.contents.model_depth, om.contents.periodicity) for om in oms] == [(12, 7, 3), (12, 7, 3), (12, 4, 3)]
    reads = cached(("reads", "groups"), lambda: gpu.Reads.from_strings(seqs))
    groups = [(d_model(gpu, paths[r % 3]), r, r + 1) for r in range(len(seqs))]
    rng = np.random.default_rng(70)
    gcs = GCS37[::4]
    read_null = rng.integers(0, len(gcs), len(seqs)).astype(np.uint32)
    o_nulls = [oracle.indep(gc) for gc in gcs]
    prm, ep = oracle.mg_params(**db.MG_KW), oracle.mg_err_params(allow_indels=True)
    got = gpu.mg_score_reads(None, gpu.NullSet.build(gcs), reads, read_null=read_null, groups=groups, allow_indels=mode == "indels", **db.MG_KW)
    want = []
    for r, s in enumerate(seqs):
        om, o_indep = oms[r % 3], o_nulls[int(read_null[r])]
        if mode == "indels":
            orfs, _, scored = oracle.mg_read_errors(om, o_indep, s.encode(), prm, ep)
            want.append((orfs, [((o.lo, o.hi, o.accepted, o.best_score if o.accepted else None, o.first_j if o.accepted else None), err_rows(st))
                                for o, st in scored]))
        else:
            orfs, scored = oracle.mg_read(om, o_indep, s.encode(), prm)
            want.append((orfs, [((o.lo, o.hi, o.first_j, bool(o.accepted), o.orf_is_truncated, o.best_score),
                                 [(w.j, w.pos, w.which, w.truncated, w.first, w.score) for w in st]) for o, st in scored]))
    n_starts, _ = (assert_error_branch if mode == "indels" else assert_front_half)(got, want, ("groups", mode))
    assert n_starts > 3000, n_starts


# ---------------------------------------------------------------- 8. training counts

@pytest.mark.parametrize("deep_levels", ["atomics", "sorted"])
def test_training_counts_of_strings_shorter_than_the_window(gpu, oracle, deep_levels):
    """3,000 training strings of 0 .. 15 bases for a 12 / 7 / 3 model: the pair counts of every level, with device-wide atomics and
    with the sort by table, against the oracle's (check_levels of tests/test_gpu_train.py)"""
    strings = db.training_strings()
    db.require_training_strings(strings, 12)
    with gpu.option("train_sort_min", 0 if deep_levels == "sorted" else 2 ** 40):
        check_levels(gpu, oracle, strings, 12, 7, 3)
