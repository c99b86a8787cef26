"""The device block cache's books balance: an entry point that has ended, with every handle it returned freed, holds no
block of the cache (gmg_debug_cache_stats' busy count is back where it was) -- on the ordinary path and on every error
path that arguments alone can reach after blocks are out.  A block handed out and not given back would stay busy for the
life of the process.  The handles that take their blocks from hipMalloc are invisible to the cache: their holders keep a
count of their own (gmg_debug_owned_blocks), which has to come back as well.  Tiny inputs: the counts are what is checked
here, the values are the other tests'."""
import contextlib
import ctypes as C
import gc
import os

import numpy as np
import pytest

import model_zoo
from conftest import DATA

pytestmark = pytest.mark.gpu

EINVAL, EBADMODEL, ERANGE = -1, -5, -6
ROWS = [(0, 0, 30, 0), (3, 5, 33, 1), (7, 2, 21, 2)]      # segments of the module's batch: (read, lo, len, orient)


def busy_blocks(gpu):
    out = (C.c_uint64 * 4)()
    assert gpu.capi.lib().gmg_debug_cache_stats(out) == 0
    return int(out[0])


def owned_blocks(gpu):
    out = C.c_uint64()
    assert gpu.capi.lib().gmg_debug_owned_blocks(C.byref(out)) == 0
    return int(out.value)


@contextlib.contextmanager
def balanced(gpu):
    """the body runs the entry point and frees what it returned; the cache then holds as many busy blocks as before, and the
    handles' holders as many blocks of hipMalloc's"""
    gc.collect()
    assert gpu.capi.lib().gmg_synchronize(None) == 0
    before, owned = busy_blocks(gpu), owned_blocks(gpu)
    yield
    gc.collect()
    assert gpu.capi.lib().gmg_synchronize(None) == 0
    assert busy_blocks(gpu) == before
    assert owned_blocks(gpu) == owned


def random_seqs(seed, lo, hi, n=8):
    rng = np.random.default_rng(seed)
    return ["".join("acgt"[c] for c in rng.integers(0, 4, size=int(k))) for k in rng.integers(lo, hi + 1, size=n)]


@pytest.fixture(scope="module")
def seqs():
    return random_seqs(11, 40, 120)


@pytest.fixture(scope="module")
def reads(gpu, seqs):
    r = gpu.Reads.from_strings(seqs)
    yield r
    r.close()


@pytest.fixture(scope="module")
def nc(gpu):
    m = gpu.Icm.open(os.path.join(DATA, "NC_000915.icm"))
    m.device()
    yield m
    m.close()


@pytest.fixture(scope="module")
def nulls(gpu):
    ns = gpu.NullSet.build([0.35, 0.6])
    ns.icms[0].device()
    yield ns
    ns.close()


def test_the_counter_sees_a_block_that_is_out(gpu, reads):
    """(the check of the check: a batch built on the device holds blocks of the cache until it is freed)"""
    gpu.capi.lib().gmg_synchronize(None)
    before = busy_blocks(gpu)
    sub = reads.select([0, 1])
    assert busy_blocks(gpu) == before + 3               # packed words, offsets, tile table
    sub.close()
    assert busy_blocks(gpu) == before


def test_reads_select(gpu, reads):
    with balanced(gpu):
        sub = reads.select([3, 0, 7, 3, 5])
        assert sub.n_reads == 5
        sub.close()
    with balanced(gpu):                                 # refused after the index list, the lengths and the offsets are on the device
        with pytest.raises(gpu.GmgError, match="names a read beyond the batch") as e:
            reads.select([1, 8, 2])
        assert e.value.code == ERANGE


def zero_probability_model(gpu, tmp_path):
    """cluster-2.icm with the logarithm of a zero probability (icm.cc:1345-1349) in its first record: the two-pass form"""
    raw = bytearray(open(os.path.join(DATA, "cluster-2.icm"), "rb").read())
    v = np.frombuffer(raw, "<f4", 4, 174 + 4).copy()
    v[2] = np.float32(-3.4028234663852886e38)
    raw[174 + 4:174 + 20] = v.tobytes()
    path = tmp_path / "zero.icm"
    path.write_bytes(bytes(raw))
    return gpu.Icm.open(str(path))


@pytest.mark.parametrize("case", ["default-shape", "zero-probability", "segment-path", "second-model-null"])
def test_score_reads_strings(gpu, reads, tmp_path, case):
    default = gpu.Icm.open(os.path.join(DATA, "cluster-2.icm"))
    models = {"default-shape": [default], "second-model-null": [default],
              "zero-probability": [zero_probability_model(gpu, tmp_path)] if case == "zero-probability" else None,
              "segment-path": [gpu.Icm.open(os.path.join(model_zoo.TRAIN, "c3_p1_d5_w9.icm"))]}[case]
    for m in models:
        m.device()
    # the sums folded into the main pass need reads of 86 bases or more; the other cases take the module's batch
    batch = gpu.Reads.from_strings(random_seqs(12, 86, 120)) if case == "default-shape" else reads
    with balanced(gpu):
        if case == "second-model-null":                 # refused after the first model's scratch exists
            arr = (C.c_void_p * 2)(models[0].device(), None)
            buf = gpu.api._DeviceBuffer(2 * batch.n_reads * 2 * 8)
            assert gpu.capi.lib().gmg_score_reads_strings(arr, 2, batch.h, buf.ptr, None) == EINVAL
            buf.free()
        else:
            assert gpu.score_reads_strings(models, batch).shape == (1, batch.n_reads, 2)
    if batch is not reads:
        batch.close()
    for m in models:
        m.close()


@pytest.mark.parametrize("case", ["per-read-nulls", "two-groups"])
def test_mg_score_reads(gpu, reads, nc, nulls, case):
    read_null = np.arange(reads.n_reads, dtype=np.uint32) % 2
    groups = [(nc, 0, 3), (nc, 3, reads.n_reads)] if case == "two-groups" else None
    with balanced(gpu):
        orfs, starts, off = gpu.mg_score_reads(None if groups else nc, nulls, reads, min_gene_len=30, read_null=read_null, groups=groups)
        assert len(off) == reads.n_reads + 1 and len(orfs) > 0


@pytest.mark.parametrize("options", [{}, {"mg_err_wave": 2, "mg_err_wave_q": 4}], ids=["default", "stack-overflow"])
def test_mg_error_branch(gpu, nc, options):
    """stack-overflow: a wave's call stack of four entries (the stack walker's; a strand of these reads has up to eight ORFs) is
    full at once, the call ends and repeats on the level kernels"""
    seqs = random_seqs(13, 90, 120)
    batch = gpu.Reads.from_strings(seqs)
    indep = gpu.Icm.indep(0.5)
    indep.device()
    quality = np.full(batch.total_bases, 10, np.uint8)  # (every base may branch)
    with contextlib.ExitStack() as stack:
        for k, v in options.items():
            stack.enter_context(gpu.option(k, v))
        with balanced(gpu):
            orfs, starts, off, errs = gpu.mg_score_reads(nc, indep, batch, min_gene_len=30, allow_indels=True, quality=quality,
                                                         indel_suffix_score_threshold=-2.5)
            assert len(starts) == len(errs) and int(errs["n"].max()) > 0
    batch.close()
    indep.close()


def test_model_set_load_and_finish_with_a_refused_file(gpu):
    syn = open(os.path.join(model_zoo.TRAIN, "syn_d4.icm"), "rb").read()
    small = open(os.path.join(model_zoo.TRAIN, "c4_d1_w2.icm"), "rb").read()
    with balanced(gpu):
        ms = gpu.ModelSet.load([syn, syn[:174 + 22 * 400 + 10], small])         # the second one ends inside a record
        with pytest.raises(gpu.GmgError) as e:
            ms.finish()
        assert e.value.code == EBADMODEL and e.value.bad_file == 1
        ms.close()
    with balanced(gpu):
        ms = gpu.ModelSet.load([syn, small, syn]).finish()
        assert gpu.model_info(ms.model(1)) == (2, 1, 3, 5)
        ms.close()


@pytest.mark.parametrize("piece_min", [None, 0])
def test_fasta_ingest(gpu, seqs, piece_min):
    data = b"".join(b">r%d some words\n%s\n" % (i, s.encode()) for i, s in enumerate(seqs))
    with contextlib.ExitStack() as stack:
        if piece_min is not None:                       # the upload in pieces, every piece packed as it arrives
            stack.enter_context(gpu.option("ingest_piece_min", piece_min))
        with balanced(gpu):
            batch, headers, _ = gpu.Reads.from_fasta_bytes(data)
            assert batch.n_reads == len(seqs) and batch.total_bases == sum(map(len, seqs)) and headers[2] == b"r2 some words"
            batch.close()


def test_entropy_regions(gpu, reads):
    pos, neg = gpu.entropy_default_profiles()
    with balanced(gpu):
        counts, dist = gpu.entropy_regions(reads, [(0, 0, 30, 1), (1, 38, 36, -1), (7, 2, 3, 1)], gpu.xlate_table(11), pos, neg)
        assert counts.shape == (3, 20) and int(counts[0].sum()) <= 10


def test_score_orfs_on_a_batch_of_fewer_than_eight_bases(gpu, nc):
    """six bases in all: the walk kernels' eight-wide loads of the gene rows end in the rows' spare entries"""
    batch = gpu.Reads.from_strings(["atgtaa"])
    indep = gpu.Icm.indep(0.5)
    indep.device()
    with balanced(gpu):
        res, starts = gpu.score_orfs(nc, indep, batch, np.array([[0, 1, 4, 3]]), min_gene_len=6, allow_truncated=True)
        assert len(res) == 1
    batch.close()
    indep.close()


# ---- one case per handle type: create, use, use again (a buffer that is too small is replaced where arguments reach that), free

def test_the_owned_counter_sees_a_block_that_is_out(gpu, reads):
    """(the check of the other check: top hits hold keys, models and the flag from hipMalloc until they are freed)"""
    before = owned_blocks(gpu)
    th = gpu.TopHits(reads, 2)
    assert owned_blocks(gpu) == before + 3
    th.close()
    assert owned_blocks(gpu) == before


def test_model(gpu, reads):
    with balanced(gpu):
        m = gpu.Icm.open(os.path.join(DATA, "NC_000915.icm"))
        m.device()
        for _ in range(2):
            assert gpu.score_reads_strings([m], reads).shape == (1, reads.n_reads, 2)
        m.close()


@pytest.mark.parametrize("how", ["from-models", "from-tables"])
def test_null_set(gpu, reads, nc, how):
    read_null = np.arange(reads.n_reads, dtype=np.uint32) % 2
    with balanced(gpu):
        ns = gpu.NullSet([gpu.Icm.indep(0.35), gpu.Icm.indep(0.6)]) if how == "from-models" else gpu.NullSet.build([0.35, 0.6])
        ns.icms[0].device()
        for _ in range(2):
            orfs, starts, off = gpu.mg_score_reads(nc, ns, reads, min_gene_len=30, read_null=read_null)
            assert len(off) == reads.n_reads + 1
        ns.close()
        for m in ns.icms:
            m.close()


def test_segments(gpu, reads, nc):
    with balanced(gpu):
        segs = gpu.Segments(reads, ROWS)
        for _ in range(2):
            assert len(gpu.segment_cumscore(nc, reads, segs, 1)) == segs.total_len
        segs.close()
    with balanced(gpu):                                 # (refused before anything is on the device)
        with pytest.raises(gpu.GmgError) as e:
            gpu.Segments(reads, [(0, 0, 30, 0), (8, 0, 1, 0)])
        assert e.value.code == ERANGE


def test_uploaded_reads(gpu, seqs, nc):
    with balanced(gpu):
        batch = gpu.Reads.from_strings(seqs)
        for _ in range(2):
            assert gpu.score_reads_strings([nc], batch).shape == (1, batch.n_reads, 2)
        batch.close()
    # a batch wrapped around device arrays is refused once its guarded copy of the words exists: the offsets end elsewhere
    packed, off = gpu.api.pack_strings(seqs)
    d_packed, d_off = gpu.api._DeviceBuffer.from_host(packed), gpu.api._DeviceBuffer.from_host(off)
    with balanced(gpu):
        h = C.c_void_p()
        assert gpu.capi.lib().gmg_reads_wrap_device(d_packed.ptr, d_off.ptr, len(seqs), int(off[-1]) - 1, C.byref(h)) == EINVAL
        assert gpu.capi.lib().gmg_reads_wrap_device(d_packed.ptr, d_off.ptr, len(seqs), int(off[-1]), C.byref(h)) == 0
        assert gpu.capi.lib().gmg_reads_free(h) == 0
    d_packed.free()
    d_off.free()


def test_single(gpu, nc):
    """100 bases, then 5,000: the staging of the first call (4,096 bases) is replaced"""
    lib = gpu.capi.lib()
    with balanced(gpu):
        st = C.c_void_p()
        assert lib.gmg_single_create(C.byref(st)) == 0
        for n in (100, 5000):
            text = random_seqs(n, n, n, 1)[0].encode()
            r, g, d_out = C.c_void_p(), C.c_void_p(), C.c_void_p()
            assert lib.gmg_single_stage(st, text, n, 0, C.byref(r), C.byref(g), C.byref(d_out)) == 0
            assert lib.gmg_segment_cumscore(nc.device(), r, g, 1, d_out, None) == 0
            got = np.zeros(n, np.float64)
            assert lib.gmg_single_fetch(st, got.ctypes.data, n) == 0
            assert np.all(np.isfinite(got)) and got.min() < 0
        assert lib.gmg_single_fetch(st, None, 1 << 20) == EINVAL
        assert lib.gmg_single_free(st) == 0


def test_fixed_model(gpu, reads):
    sub = [(np.full(1, -1, np.int16), np.zeros((1, 4), np.float32), 0), (np.full(5, -1, np.int16), np.zeros((5, 4), np.float32), 0)]
    with balanced(gpu):
        m = gpu.FixedModel([1, 0], sub)
        segs = gpu.Segments(reads, ROWS)
        for _ in range(2):
            assert len(gpu.fixed_score(m, reads, segs)) == segs.n
        segs.close()
        m.close()


@pytest.mark.parametrize("exact_path", [0, 2, 1], ids=["events", "fused", "any-shape"])
def test_orf_batch(gpu, nc, exact_path):
    """every path's first-use arrays, two calls on one batch of ORFs (the second asks for more starts)"""
    lib = gpu.capi.lib()
    batch = gpu.Reads.from_strings(["atgaaacccgggtttatgaaacccgggtttaaatag" * 3, "ttgcccaaagggtaa"])
    indep = gpu.Icm.indep(0.5)
    indep.device()
    o = np.zeros(2, gpu.api.ORF_DTYPE)
    o["read"], o["frame"], o["stop_position"], o["orf_len"] = [0, 1], [1, 1], [106, 13], [105, 12]
    with gpu.option("orfs_exact_path", exact_path), balanced(gpu):
        h, max_starts = C.c_void_p(), C.c_uint64()
        assert lib.gmg_orfs_upload(batch.h, o.ctypes.data, len(o), C.byref(max_starts), C.byref(h)) == 0
        for min_gene_len in (90, 6):
            prm = gpu.capi.OrfParams(min_gene_len, 1, 0, 2**31 - 1, -6.0, 3)
            for i, c in enumerate(("atg", "gtg", "ttg")):
                prm.start_codon[i].value = c.encode()
            n_st = C.c_uint64()
            assert lib.gmg_score_orfs_begin(nc.device(), indep.device(), batch.h, h, C.byref(prm), C.byref(n_st), None) == 0
            res, starts = np.zeros(len(o), gpu.api.ORF_RESULT_DTYPE), np.zeros(max(int(n_st.value), 1), gpu.api.START_DTYPE)
            assert lib.gmg_score_orfs_fetch(h, res.ctypes.data, starts.ctypes.data, None) == 0
        other = gpu.Reads.from_strings(["acgt" * 30])   # refused with the batch's arrays out: not the reads the ORFs were uploaded against
        assert lib.gmg_score_orfs_begin(nc.device(), indep.device(), other.h, h, C.byref(prm), C.byref(n_st), None) == EINVAL
        other.close()
        assert lib.gmg_orf_batch_free(h) == 0
    with balanced(gpu):                                 # refused: the second ORF leaves its read
        o["orf_len"][1] = 300
        assert lib.gmg_orfs_upload(batch.h, o.ctypes.data, len(o), None, C.byref(h)) == ERANGE
    batch.close()
    indep.close()


def test_top_hits(gpu, reads, nc):
    """format_rows with B = 1 and then B = 3 replaces the lengths, the offsets and the text"""
    rng = np.random.default_rng(5)
    with balanced(gpu):
        th = gpu.TopHits(reads, 2)
        for B in (1, 3):
            sums = -rng.random((B, reads.n_reads, 2)) * 100
            assert th.format_rows(sums).count(b"\n") == B
            th.update_sums(sums, first_model=B, informative=np.ones(B, np.uint8))
        th.scores([nc], first_model=7)
        assert th.fetch()[1].shape == (reads.n_reads, 2)
        # refused with the handle's scratch out: a sum without a %.4f key; a text buffer that is too small
        bad = np.full((4, reads.n_reads, 2), np.nan)
        with pytest.raises(gpu.GmgError) as e:
            th.update_sums(bad, informative=np.ones(4, np.uint8))
        assert e.value.code == ERANGE
        buf, out, size = gpu.api._DeviceBuffer.from_host(sums), np.zeros(8, np.uint8), C.c_size_t(8)
        assert gpu.capi.lib().gmg_tophits_format_rows(th.h, buf.ptr, 3, 0, out.ctypes.data, C.byref(size), None) == ERANGE
        assert size.value > 8
        buf.free()
        th.close()


def test_trainer(gpu, reads):
    """train_sort_min = 0: the levels whose counters do not fit the LDS (3 and up for windows of 12) take the sorted path, whose
    arrays come on first use and are used again"""
    with gpu.option("train_sort_min", 0), balanced(gpu):
        t = gpu.Trainer(reads, 12, 4, 3)
        for level in range(5):
            mip_prev = np.full((3, 4 ** (level - 1)), 10 - level, np.int16) if level else None
            counts = t.level_counts(level, mip_prev)
            assert counts.shape == (3, 4 ** level, 11, 16) and int(counts.sum()) > 0
        t.close()
    with balanced(gpu):                                 # refused with the trainer's arrays out: a level out of order, a bad position
        t = gpu.Trainer(reads, 12, 2, 3)
        for level, mip_prev, code in [(1, np.zeros((3, 1), np.int16), EINVAL), (0, None, 0), (1, np.full((3, 1), 11, np.int16), EBADMODEL)]:
            if code:
                with pytest.raises(gpu.GmgError) as e:
                    t.level_counts(level, mip_prev)
                assert e.value.code == code
            else:
                t.level_counts(level, mip_prev)
        t.close()


def test_letters(gpu, seqs):
    """the text of two regions, then of six: the second does not fit the first one's buffer"""
    off = np.zeros(len(seqs) + 1, np.uint64)
    off[1:] = np.cumsum([len(s) for s in seqs])
    prm = gpu.text_params(60)
    few = [(0, 0, 30, 1), (1, 38, 36, -1)]
    more = few + [(r, 0, len(seqs[r]), 1) for r in (2, 3, 4, 5)]
    with balanced(gpu):
        l = gpu.Letters("".join(seqs).encode(), off)
        for regions in (few, more):
            heads = [b">g%d\n" % k for k in range(len(regions))]
            text = l.regions_text(regions, heads, prm)
            assert text.count(b">") == len(regions)
            ptr, size = l.regions_text_device(regions, heads, prm)
            assert size == len(text) and gpu.memcpy_d2h(ptr, size) == text
        # refused with the handle's arrays out: a region beyond its read; a host buffer that is too small
        with pytest.raises(gpu.GmgError) as e:
            l.regions_text([(0, 0, 1000, 1)], [b">x\n"], prm)
        assert e.value.code == ERANGE
        with pytest.raises(gpu.GmgError) as e:
            l.regions_text(more, heads, prm, capacity=10)
        assert e.value.code == ERANGE
        l.close()


def test_model_set_member_scores(gpu, reads):
    syn = open(os.path.join(model_zoo.TRAIN, "syn_d4.icm"), "rb").read()
    with balanced(gpu):
        ms = gpu.ModelSet.load([syn, syn]).finish()
        for k in range(2):
            assert gpu.score_reads_strings([ms.model(k)], reads).shape == (1, reads.n_reads, 2)
        ms.close()
