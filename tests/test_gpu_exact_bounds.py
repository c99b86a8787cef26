"""The three exactness predicates of the reordered sums, AT their bounds (models and reads: tests/exact_models.py; that `edge` is
exact on the reference alone: tests/test_exact_bounds.py):
  edge   clog (R + 2) + max_exp - min_exp == 28: the fused tile kernel, the error branch on running sums and GENE32 may run
  past   the same model, one read lengthened so that clog grows by one: they may not
  wide   a spread one larger: they may not
and for gmg_score_reads_strings min_exp 109 / 108 x spread 23 / 24 with reads whose |sum| falls on both sides of the per-read
test.  Whatever path the library picks, every result must equal the oracle's bit for bit, and every variant the first result."""
import numpy as np
import pytest

import exact_models
from test_gpu_mg_err import dev_err_rows
from test_gpu_parity import ORF_PATHS, ORF_WALK
from test_oracle_mg import err_rows

pytestmark = pytest.mark.gpu
KW = dict(min_gene_len=30)
CASES = ["edge", "past", "wide"]


@pytest.fixture(scope="module")
def doctored(gpu, oracle, tmp_path_factory):
    d = tmp_path_factory.mktemp("exact")
    out = {}
    for which in CASES:
        path = exact_models.mg_model(oracle, which, d)
        out[which] = (gpu.Icm.open(path), oracle.read(path), exact_models.mg_reads(which))
    for name in exact_models.STRINGS:
        path = exact_models.strings_model(name, d)
        out[name] = (gpu.Icm.open(path), oracle.read(path))
    yield out
    for v in out.values():
        v[0].close()
        oracle.L.orc_model_free(v[1])


def mg_rows(starts):
    return [(int(s["j"]), int(s["pos"]), int(s["which"]), int(s["truncated"]), int(s["first"]), float(s["score"])) for s in starts]


@pytest.mark.parametrize("which", CASES)
def test_front_half_at_the_bound(gpu, oracle, doctored, which):
    """gmg_mg_score_reads with one null model per read: every read against the oracle, then every mg_fused x mg_tile x mg_gene32
    variant byte for byte"""
    icm, om, seqs = doctored[which]
    reads = gpu.Reads.from_strings(seqs)
    read_null = (np.arange(len(seqs)) % len(exact_models.GCS)).astype(np.uint32)
    nulls = gpu.NullSet.build(exact_models.GCS)
    prm = oracle.mg_params(**KW)
    first = gpu.mg_score_reads(icm, nulls, reads, read_null=read_null, **KW)
    orfs, starts, off = first
    n_starts = 0
    for r, s in enumerate(seqs):
        want_orfs, scored = oracle.mg_read(om, oracle.indep(exact_models.GCS[read_null[r]]), s.encode(), prm)
        mine = orfs[int(off[r]):int(off[r + 1])]
        assert np.array_equal(np.stack([mine["frame"], mine["stop_position"], mine["gene_len"], mine["orf_len"]], 1).reshape(-1, 4), want_orfs)
        for o, (out, want) in zip(mine, scored):
            st = starts[o["start_begin"]:o["start_begin"] + o["n_starts"]]
            assert mg_rows(st) == [(w.j, w.pos, w.which, w.truncated, w.first, w.score) for w in want], (which, r)
            assert o["best_score"] == out.best_score and bool(o["accepted"]) == bool(out.accepted)
            n_starts += len(want)
    assert n_starts >= 100
    for fused in (0, 1):
        for tile in (0, 1, 2, 4):
            for g32 in (0, 1, 2):
                with gpu.option("mg_fused", fused), gpu.option("mg_tile", tile), gpu.option("mg_gene32", g32):
                    got = gpu.mg_score_reads(icm, nulls, reads, read_null=read_null, **KW)
                for a, b in zip(got, first):
                    assert a.tobytes() == b.tobytes(), (which, fused, tile, g32)


@pytest.mark.parametrize("mode", ["indels", "subs"])
@pytest.mark.parametrize("which", CASES)
def test_error_branch_at_the_bound(gpu, oracle, doctored, which, mode):
    """-i / -s (err_exact decides between running sums and walks): every read against the oracle, every variant byte for byte"""
    icm, om, seqs = doctored[which]
    reads = gpu.Reads.from_strings(seqs)
    ekw = dict(allow_indels=True) if mode == "indels" else dict(allow_subs=True)
    indep, o_indep, prm, ep = gpu.Icm.indep(0.5), oracle.indep(0.5), oracle.mg_params(**KW), oracle.mg_err_params(**ekw)
    first = gpu.mg_score_reads(icm, indep, reads, **KW, **ekw)
    orfs, starts, off, errs = first
    n_starts = 0
    for r, s in enumerate(seqs):
        _, _, scored = oracle.mg_read_errors(om, o_indep, s.encode(), prm, ep)
        mine = orfs[int(off[r]):int(off[r + 1])]
        assert len(mine) == len(scored)
        for o, (out, want) in zip(mine, scored):
            sl = slice(o["start_begin"], o["start_begin"] + o["n_starts"])
            assert dev_err_rows(starts[sl], errs[sl]) == err_rows(want), (which, mode, r)
            assert int(o["accepted"]) == out.accepted
            n_starts += len(want)
    assert n_starts >= 100
    for opts in ({"mg_err_wave": 0, "mg_err_tile": 0}, {"mg_err_wave": 1, "mg_err_tile": 0}, {"mg_err_wave": 2, "mg_err_tile": 0},
                 {"mg_err_wave": 3, "mg_err_tile": 0}, {"mg_err_flat": 1}, {"mg_err_tile": 1}, {"mg_err_skip": 0}):
        old = {k: gpu.get_option(k) for k in opts}
        try:
            for k, v in opts.items():
                gpu.set_option(k, v)
            got = gpu.mg_score_reads(icm, indep, reads, **KW, **ekw)
        finally:
            for k, v in old.items():
                gpu.set_option(k, v)
        for a, b in zip(got, first):
            assert a.tobytes() == b.tobytes(), (which, mode, opts)


@pytest.mark.parametrize("path", sorted(ORF_PATHS))
@pytest.mark.parametrize("which", CASES)
def test_score_orfs_at_the_bound(gpu, oracle, doctored, which, path, request_finalizers):
    gpu.set_option("orfs_exact_path", ORF_PATHS[path])
    gpu.set_option("orfs_walk8", ORF_WALK.get(path, 4))
    gpu.set_option("orfs_q_poison", 1)
    request_finalizers.append(lambda: (gpu.set_option("orfs_exact_path", 0), gpu.set_option("orfs_walk8", 4), gpu.set_option("orfs_q_poison", 0)))
    icm, om, seqs = doctored[which]
    reads = gpu.Reads.from_strings(seqs)
    rng = np.random.default_rng(5)
    rows = []
    for r, s in enumerate(seqs):
        n = len(s)
        rows.append((r, 1 + 0 % 3, n + 1 - n % 3, n - n % 3))                      # (the whole read: the longest sums)
        for _ in range(5):
            ln = int(rng.integers(3, n + 1))
            if rng.random() < 0.8:
                ln = max(ln - ln % 3, 3)
            lo = int(rng.integers(0, n - ln + 1))
            rows.append((r, 1 + lo % 3, lo + ln + 1, ln) if rng.random() < 0.5 else (r, -1 - lo % 3, lo - 2, ln))
    rows = np.array(rows)
    kw = dict(min_gene_len=30, allow_truncated=True, start_threshold=-1e300)
    res, starts = gpu.score_orfs(icm, gpu.Icm.indep(0.5), reads, rows, **kw)
    o_indep, prm = oracle.indep(0.5), oracle.orf_params(**kw)
    n_starts = 0
    for (r, frame, stop, ln), got in zip(rows, res):
        n, out, want = oracle.score_orf(om, o_indep, seqs[r], int(frame), int(stop), int(ln), prm)
        assert (got["first_j"], got["best_j"], got["best_pos"]) == (out.first_j, out.best_j, out.best_pos)
        assert got["best_score"] == out.best_score, (which, path, r)
        if n < 0:
            assert got["n_starts"] == 0
            continue
        assert got["n_starts"] == n
        assert got["gene_score"] == out.gene_score or (np.isnan(got["gene_score"]) and np.isnan(out.gene_score))
        st = starts[got["start_begin"]:got["start_begin"] + n]
        assert [(s["j"], s["pos"], s["which"], s["truncated"], s["first"], s["score"]) for s in st] == \
               [(w.j, w.pos, w.which, w.truncated, w.first, w.score) for w in want], (which, path, r)
        n_starts += n
    assert n_starts >= 100


def test_strings_at_the_bounds(gpu, oracle, doctored):
    """min_exp 109 / 108 x spread 23 / 24 in ONE call (only 109 / 23 may take the fused form; its reads with |sum| >= 2^11 go to the
    per-read redo): fused and two-pass, both strands of every read against the oracle"""
    names = sorted(exact_models.STRINGS)
    seqs = exact_models.strings_reads()
    reads = gpu.Reads.from_strings(seqs)
    icms = [doctored[n][0] for n in names]
    with gpu.option("strings_fused", 1):
        fused = gpu.score_reads_strings(icms, reads)
    with gpu.option("strings_fused", 0):
        two_pass = gpu.score_reads_strings(icms, reads)
    assert fused.tobytes() == two_pass.tobytes()
    rc = str.maketrans("acgt", "tgca")
    for k, n in enumerate(names):
        om = doctored[n][1]
        for r, s in enumerate(seqs):
            assert fused[k, r, 0] == oracle.score_string(om, s, 0), (n, r, len(s))
            assert fused[k, r, 1] == oracle.score_string(om, s[::-1].translate(rc), 0), (n, r, len(s))
    big = np.abs(fused[names.index("s109_23"), :, 0])
    assert (big < 2.0 ** 10).sum() >= 10 and (big >= 2.0 ** 11).sum() >= 10
