"""gmg_tophits_* (include/gmg.h) and integration/phymm_gpu against tests/phymm_oracle.py: crafted sums through the top-hits
update and the device formatter, the program on a synthetic .genomeData built from the committed ICMs (raw matrix byte for byte,
class file as a map, every batch size), and a large batch against the numpy form of score_insert."""
import os
import subprocess

import numpy as np
import pytest

import phymm_oracle as po
from conftest import DATA, ROOT

pytestmark = pytest.mark.gpu


def revcomp(s):
    """the reverse complement gmg_score_reads_strings scores: of the read after the load-time normalisation (lower case, any
    other character a 'c'; seqs.fa holds one 'Y').  Phymm's own reverse-complement script is not part of the reference."""
    s = "".join(c if c in "acgt" else "c" for c in s.lower())
    return s[::-1].translate(str.maketrans("acgt", "tgca"))


def text_key(t):
    return int(t.replace(".", ""))


def crafted_sums(rng, n, B):
    """[B, n, 2] scores full of what the printed text makes hard: halfway values q/32 and their neighbours, +-0 and values
    that print -0.0000, equal keys on both strands, exact ties between models"""
    q = rng.integers(-40000, 40000, size=(B, n, 2))
    s = q / 32.0
    pick = rng.integers(0, 8, size=(B, n, 2))
    s = np.where(pick == 1, np.nextafter(s, np.inf), s)
    s = np.where(pick == 2, np.nextafter(s, -np.inf), s)
    s = np.where(pick == 3, rng.choice([0.0, -0.0, -4e-5, 4e-5, -1e-9], size=s.shape), s)
    s = np.where(pick == 4, rng.normal(-600, 100, size=s.shape), s)
    same = rng.integers(0, 6, size=(B, n)) == 0                      # both strands print the same text
    s[..., 1] = np.where(same, s[..., 0], s[..., 1])
    near = rng.integers(0, 6, size=(B, n)) == 0
    s[..., 1] = np.where(near, np.nextafter(s[..., 0], np.inf), s[..., 1])
    for b in range(1, B, 5):                                         # a model that repeats an earlier one: ties between models
        s[b] = s[b - 1]
    return s


def oracle_slots(sums, T, informative, forward_only):
    B, n, _ = sums.shape
    out = []
    for r in range(n):
        slots, text = [None] * T, {}
        for b in range(B):
            if informative is not None and not informative[b]:
                continue
            text[b] = po.merged_text(sums[b, r, 0], None if forward_only else sums[b, r, 1])
            po.score_insert(slots, float(text[b]), b)
        out.append([(text[g], g) for _, g in slots])
    return out


def test_update_sums_equals_score_insert_on_the_printed_text(gpu):
    rng = np.random.default_rng(11)
    n, B = 300, 36
    sums = crafted_sums(rng, n, B)
    reads = gpu.Reads.from_strings(["acgt"] * n)
    for T in range(1, 9):
        inf = (rng.integers(0, 4, B) != 0).astype(np.uint8) if T % 2 else None
        for fwd_only in (False, True):
            h = gpu.TopHits(reads, T)
            h.update_sums(sums[:13], 0, None if inf is None else inf[:13], fwd_only)      # the database in two batches
            h.update_sums(sums[13:], 13, None if inf is None else inf[13:], fwd_only)
            keys, models = h.fetch()
            want = oracle_slots(sums, T, inf, fwd_only)
            for r in range(n):
                w = want[r]
                assert list(models[r]) == [g for _, g in w], (T, fwd_only, r)
                assert list(keys[r]) == [text_key(t) for t, _ in w], (T, fwd_only, r)
            h.close()


def test_update_sums_fills_unsorted_and_refuses_unkeyable_values(gpu):
    reads = gpu.Reads.from_strings(["acgt"])
    h = gpu.TopHits(reads, 3)
    h.update_sums(np.array([[[-5.0, -9.0]], [[-1.0, -9.0]], [[-3.0, -9.0]]]))
    assert list(h.fetch()[1][0]) == [0, 1, 2]                          # arrival order
    h.update_sums(np.array([[[-4.0, -9.0]]]), 3)
    assert list(h.fetch()[1][0]) == [3, 0, 1]
    h.update_sums(np.array([[[-1.0, -3.4e38]]]), 4, forward_only=True)   # the reverse strand is not read with -f
    assert list(h.fetch()[1][0]) == [4, 3, 0]
    for bad in ((np.nan, -1.0), (-1.0, -3.4e38), (-1.0, -np.inf), (4.6e11, -1.0)):
        with pytest.raises(gpu.GmgError):                              # (the slots are undefined after a refusal)
            h.update_sums(np.array([[bad]]), 5)
        with pytest.raises(gpu.GmgError):
            h.format_rows(np.array([[bad]]))
    with pytest.raises(gpu.GmgError):
        gpu.TopHits(reads, 17)


def test_format_rows_equals_the_printed_matrix(gpu):
    rng = np.random.default_rng(12)
    for n, B in ((1, 3), (257, 9), (5000, 4)):
        sums = crafted_sums(rng, n, B)
        sums[0, 0] = (-123456789.98765, 0.1)
        reads = gpu.Reads.from_strings(["acgt"] * n)
        h = gpu.TopHits(reads, 1)
        for fwd_only in (False, True):
            got = h.format_rows(sums, fwd_only)
            want = "".join("\t".join(po.merged_text(sums[b, r, 0], None if fwd_only else sums[b, r, 1]) for r in range(n)) + "\n"
                           for b in range(B))
            assert got == want.encode(), (n, B, fwd_only)


# ------------------------------------------------------------------------------------------------------------------------------
# the program
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def phymm_exe(gmg, tmp_path_factory):
    return po.phymm_binary(str(tmp_path_factory.mktemp("phymm_bin")))


def run(exe, cwd, *args):
    env = dict(os.environ, LD_LIBRARY_PATH=os.path.join(ROOT, "glimmer-mg_amd", "lib"))
    res = subprocess.run([exe, *args], cwd=cwd, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    return res


# link name -> model file: duplicates under other names force exact ties between models
LAYOUT = {
    "HP_strainA/NC_000915.icm": "NC_000915.icm",
    "HP_strainA/cluster-0.icm": "cluster-0.icm",
    "HP_strainA/cluster-0.gene.icm": "cluster-1.icm",          # skipped: ".gene."
    "B_strain/NC_100001.icm": "cluster-1.icm",
    "B_strain/NC_100002.x.icm": "cluster-2.icm",
    "B_strain/NC_100003.icm": "cluster-0.icm",                  # = HP_strainA/cluster-0: ties
    "C_strain/NC_200001.icm": "cluster-3.icm",                  # its whole directory is ignored
    "D_strain/NC_300001.icm": "cluster-4.icm",
    "D_strain/NC_300002.icm": "cluster-5.icm",                  # ignored by its full path
    "D_strain/readme.txt": "cluster-5.icm",                     # not an ICM
    ".hidden/NC_400001.icm": "cluster-5.icm",                   # a dot directory: not scanned
    ".userAdded/U_strain/NC_500001.icm": "cluster-5.icm",
    ".userAdded/U_strain/NC_500002.icm": "cluster-4.icm",       # = D_strain/NC_300001: ties
}
IGNORE = "C_strain\n.genomeData/D_strain/NC_300002.icm\nnot_there\n"


@pytest.fixture(scope="module")
def phymm_case(tmp_path_factory, oracle, seqs_fa):
    """the synthetic database, the reads and the oracle's raw files (both strands, forward only)"""
    root = tmp_path_factory.mktemp("phymm_run")
    for link, model in LAYOUT.items():
        p = root / ".genomeData" / link
        os.makedirs(p.parent, exist_ok=True)
        os.symlink(os.path.join(DATA, model), p)
    (root / "ignore.txt").write_text(IGNORE)
    os.symlink(os.path.join(DATA, "seqs.fa"), root / "seqs.fa")
    icms = po.icm_list(str(root), "icm", IGNORE.splitlines())
    assert len(icms) == 8 and ".genomeData/.userAdded/U_strain/NC_500001.icm" in icms
    ids = [h.split()[0] for h in seqs_fa[0]]
    seqs = seqs_fa[1]
    committed = {}
    for i in range(6):
        committed["cluster-%d.icm" % i] = [float(line.split()[1]) for line in open(os.path.join(DATA, "icm-%d.scores.tmp" % i))]
    fwd, rev, cache = [], [], {}
    for p in icms:
        model = LAYOUT[p[len(".genomeData/"):]]
        if model not in cache:
            m = oracle.read(os.path.join(DATA, model))
            f = committed.get(model) or [oracle.score_string(m, s, 0) for s in seqs]
            cache[model] = (f, [oracle.score_string(m, revcomp(s), 0) for s in seqs])
        fwd.append(cache[model][0])
        rev.append(cache[model][1])
    return root, icms, ids, po.raw_file(icms, ids, fwd, rev), po.raw_file(icms, ids, fwd)


def test_program_raw_matrix_and_class_file(phymm_exe, phymm_case):
    root, icms, ids, want_both, want_fwd = phymm_case
    for args, want in (([], want_both), (["-f"], want_fwd)):
        for batch in ("1", "3", str(len(icms))):
            for T in (1, 3, 5):
                res = run(phymm_exe, root, *args, "-i", "ignore.txt", "-t", str(T), "--batch-models", batch, "seqs.fa")
                assert res.returncode == 0, res.stderr
                got = (root / "rawPhymmOutput_seqs_fa.txt").read_text()
                assert got == want, (args, batch, T)
                classes, _ = po.classify(want, T)
                assert po.read_class_file(root / "seqs.class.txt") == classes, (args, batch, T)
                assert [ln.split("\t")[0] for ln in open(root / "seqs.class.txt")] == ids          # read order
    # informative genomes, and no matrix
    inf = {"HP_strainA|NC_000915", "B_strain|NC_100003", "U_strain|NC_500002", "D_strain|NC_300001"}
    (root / "inf.txt").write_text("\n".join(sorted(inf)) + "\n")
    os.remove(root / "rawPhymmOutput_seqs_fa.txt")
    res = run(phymm_exe, root, "-i", "ignore.txt", "-t", "4", "--informative", "inf.txt", "--no-matrix", "seqs.fa")
    assert res.returncode == 0, res.stderr
    assert not os.path.exists(root / "rawPhymmOutput_seqs_fa.txt")
    assert po.read_class_file(root / "seqs.class.txt") == po.classify(want_both, 4, inf)[0]


def test_program_refusals(phymm_exe, phymm_case, tmp_path):
    root = phymm_case[0]
    cases = {
        "empty.fa": (">r1\nacgt\n>r2\n\n>r3\nggg\n", "empty sequence"),
        "dup.fa": (">r1 a\nacgt\n>r1 b\nggg\n", "appears twice"),
        "noid.fa": (">r1\nacgt\n> r2\nggg\n", "without a read ID"),
        "noid2.fa": (">\nacgt\n", "without a read ID"),
    }
    for name, (text, msg) in cases.items():
        (root / name).write_text(text)
        res = run(phymm_exe, root, "-i", "ignore.txt", name)
        assert res.returncode != 0 and msg in res.stderr, (name, res.stderr)


# ------------------------------------------------------------------------------------------------------------------------------
# a large batch
# ------------------------------------------------------------------------------------------------------------------------------
def test_200k_reads_40_models_against_numpy(gpu, tmp_path):
    import models64
    n, L, T = 200_000, 500, 5
    packed, off = gpu.synth.packed_reads(n, L, 17)
    reads = gpu.Reads(packed, off)
    models = [m for m, _ in models64.period1_models(gpu, tmp_path, 40)]
    rng = np.random.default_rng(4)
    inf = (rng.integers(0, 5, 40) != 0).astype(np.uint8)
    h = gpu.TopHits(reads, T)
    for first in range(0, 40, 16):
        h.scores(models[first:first + 16], first, inf[first:first + 16])
    keys, slots = h.fetch()
    sums = gpu.score_reads_strings(models, reads)
    wk, wm = po.tophits_numpy(po.merged_keys(sums), T, inf)
    assert np.array_equal(slots, wm) and np.array_equal(keys, wk)
    assert len(set(slots[:, 0].tolist())) > 1
