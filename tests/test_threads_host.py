"""The host-thread contract where no device is needed: gmg_last_error() is the calling thread's own text, and the
host-only entry points give the same bytes from four threads at once as from one.  ctypes releases the GIL around every call, so
Python threads overlap inside the library."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import thread_cases as tc
from conftest import DATA, GOLD

N_FAILING = 2000
ROUNDS = 50


def test_error_text_is_the_calling_threads_own(gmg):
    """four threads fail 2,000 times each with a key of their own and read exactly that key back after every call; a fifth makes
    only calls that succeed and never sees a text at all"""
    lib = gmg.capi.lib()
    done = []

    def body(t, barrier):
        barrier.wait()
        if t == tc.N_THREADS:
            v = C.c_longlong()
            while len(done) < tc.N_THREADS:
                assert lib.gmg_get_option(b"strings_fused", C.byref(v)) == 0 and lib.gmg_base_code(ord("g")) == 2
                assert lib.gmg_packed_words(33) == 4
                text = lib.gmg_last_error()
                assert text == b"", "a thread that never failed reads %r" % text
            return
        try:
            for i in range(N_FAILING):
                key = b"no_such_%d_%d" % (t, i)
                assert lib.gmg_set_option(key, 1) == -1
                text = lib.gmg_last_error()
                assert b"'" + key + b"'" in text, "thread %d, call %d reads %r" % (t, i, text)
        finally:
            done.append(t)

    tc.run_threads(tc.N_THREADS + 1, body)
    assert sorted(done) == list(range(tc.N_THREADS))


# ---- the host-only entry points: (name, call) with call() -> bytes ------------------------------------------------------------------

def _bytes(*parts):
    out = []
    for p in parts:
        if isinstance(p, np.ndarray):
            out.append(b"%s%r" % (p.dtype.str.encode(), p.shape) + np.ascontiguousarray(p).tobytes())
        elif isinstance(p, bytes):
            out.append(p)
        elif isinstance(p, str):
            out.append(p.encode())
        else:
            out.append(repr(p).encode())
    return b"|".join(out)


def reference_pack(raw, first):
    """gmg_pack_bases restated: a c g t keep their meaning, r d -> g, w k -> t, everything else -> c; 16 bases per word"""
    code = np.ones(256, np.uint32)
    for chars, v in (("aA", 0), ("cC", 1), ("gGrRdD", 2), ("tTwWkK", 3)):
        for ch in chars:
            code[ord(ch)] = v
    words = np.zeros((first + len(raw) + 15) // 16 + 1, np.uint32)
    for i, ch in enumerate(raw):
        g = first + i
        words[g >> 4] |= code[ch] << np.uint32(2 * (g & 15))
    return words


@pytest.fixture(scope="module")
def genome_data(tmp_path_factory):
    sys.path.insert(0, GOLD)
    import make_genome_data
    d = str(tmp_path_factory.mktemp("genomeData"))
    mixed = make_genome_data.write_class_variants(d)
    make_genome_data.build(os.path.join(d, ".genomeData"), [os.path.join(DATA, "seqs.class.txt"), mixed])
    return d


def host_calls(gmg, seqs_fa):
    """the small inputs of the entry points' own host tests"""
    api, lib = gmg.api, gmg.capi.lib()
    rng = np.random.default_rng(3)
    raw = rng.integers(1, 256, size=4096, dtype=np.uint8).tobytes()
    fasta = b"junk\n" + b"".join(b">r%d has > inside\nACGT>mid%d\nAC\nGT\n\n" % (i, i) for i in range(200))
    icm = open(os.path.join(DATA, "NC_000915.icm"), "rb").read()
    class_text = open(os.path.join(DATA, "seqs.class.txt")).read()
    hdrs = seqs_fa[0][:300]
    counts = rng.integers(0, 40, size=(16, 20)).astype(np.int32)
    pos, neg = api.entropy_default_profiles()
    three = 0.05 + 0.05 + 0.05
    table = api.FeatureTable([1, 0, 0, 7, 123456789012], (10, 0, 3), (2.5, sum([1.0 / 6] * 6), 1.0, 2.5),
                             ([0.15, three] + [0.0] * 50 + [7.25], [], [0.0] * 50 + [1e-9, 0.25, 0.35, 12345678.96]))
    off3 = np.array([0, 50, 120], np.uint64)

    def pack():
        words = np.zeros(int(lib.gmg_packed_words(7 + len(raw))), np.uint32)
        assert lib.gmg_pack_bases(raw, len(raw), 7, words.ctypes.data) == 0
        return _bytes(words)

    def split():
        cuts = np.zeros(64, np.uint64)
        n = lib.gmg_fasta_split(fasta, len(fasta), 700, cuts.ctypes.data_as(C.c_void_p), 63)
        return _bytes(n, cuts[:n + 1])

    def classes():
        cls = api.Classes(class_text, ".genomeData")
        try:
            return _bytes(cls.n_reads, cls.n_icms, cls.n_classes, cls.n_missing_gc, *cls.plan(hdrs))
        finally:
            cls.close()

    return [
        ("gmg_pack_bases", pack),
        ("gmg_extract_plan", lambda: _bytes(*api.extract_plan([0, 250, 250, 600], [(0, 251, 255, 1), (0, 0, 3, 1), (0, 1, 250, 1), (2, 100, 200, -1)],
                                                               api.COORD_USE_DIR))),
        ("gmg_uncovered_plan", lambda: _bytes(api.uncovered_plan([0, 40, 100], [(0, 5, 14, 1), (0, 26, 28, 1), (1, 39, 2, 1), (1, 7, 30, -1)]))),
        ("gmg_edits_plan", lambda: _bytes(*api.edits_plan(off3, [(1, 1, 60, 1, [3], [10, 11], [20]), (0, 1, 30, 1, [], [], []), (1, 1, 60, -1, [], [5], [])]))),
        ("gmg_shard_plan", lambda: _bytes(gmg.shard.shard_plan(np.cumsum([0] + list(range(1, 400))), 8))),
        ("gmg_fasta_split", split),
        ("gmg_fasta_shard_ranges", lambda: _bytes(gmg.shard.fasta_shard_ranges(fasta, 5))),
        ("gmg_xlate_table", lambda: _bytes(*[api.xlate_table(code) for code in (1, 4, 11)])),
        ("gmg_stop_codons_by_code", lambda: _bytes(*[api.stop_codons_by_code(code) for code in (1, 4, 11)])),
        ("gmg_entropy_from_counts", lambda: _bytes(api.entropy_from_counts(counts, pos, neg))),
        ("gmg_features_format", lambda: _bytes(*[api.features_format(table, "NON", what, 50) for what in range(7)])),
        ("gmg_icm_bytes_info", lambda: _bytes(api.icm_bytes_info(icm), api.icm_bytes_info(icm[:174]))),
        ("gmg_classes_load + gmg_classes_plan", classes),
    ], (raw, 7)


def test_host_only_entry_points_concurrent_equal_serial(gmg, seqs_fa, genome_data, monkeypatch):
    """four threads run the whole list 50 times, each in an order of its own; every output is byte-equal to the same call made
    before any thread started.  gmg_pack_bases builds its table at its first use: its expected words are restated here, and (when
    this file runs on its own) its very first calls are the concurrent ones"""
    monkeypatch.chdir(genome_data)                                    # (the ICM files' order depends on their names, directory included)
    calls, (raw, first) = host_calls(gmg, seqs_fa)
    assert len(calls) == 13
    want = {name: fn() for name, fn in calls if name != "gmg_pack_bases"}
    words = reference_pack(raw, first)
    want["gmg_pack_bases"] = _bytes(words[:int(gmg.capi.lib().gmg_packed_words(first + len(raw)))])
    assert all(len(v) > 8 for v in want.values())
    bad = []

    def body(t, barrier):
        barrier.wait()
        for k in range(ROUNDS):
            for i in range(len(calls)):
                name, fn = calls[(i + t * 3 + k) % len(calls)]
                if fn() != want[name]:
                    bad.append((t, k, name))

    tc.run_threads(tc.N_THREADS, body)
    assert not bad, "differs from the serial call: %s" % ", ".join("%s (thread %d, round %d)" % (n, t, k) for t, k, n in bad[:8])
    assert dict((name, fn()) for name, fn in calls) == want           # ... and serially afterwards, gmg_pack_bases included
