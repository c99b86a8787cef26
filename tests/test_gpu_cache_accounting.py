"""The device block cache's books balance: an entry point that has ended, with every handle it returned freed, holds no
block of the cache (gmg_debug_cache_stats' busy count is back where it was) -- on the ordinary path and on every error
path that arguments alone can reach after blocks are out.  A block handed out and not given back would stay busy for the
life of the process.  Tiny inputs: the count is what is checked here, the values are the other tests'."""
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


def busy_blocks(gpu):
    out = (C.c_uint64 * 4)()
    assert gpu.capi.lib().gmg_debug_cache_stats(out) == 0
    return int(out[0])


@contextlib.contextmanager
def balanced(gpu):
    """the body runs the entry point and frees what it returned; the cache then holds as many busy blocks as before"""
    gc.collect()
    assert gpu.capi.lib().gmg_synchronize(None) == 0
    before = busy_blocks(gpu)
    yield
    gc.collect()
    assert gpu.capi.lib().gmg_synchronize(None) == 0
    assert busy_blocks(gpu) == before


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
