"""The entropy distance ratio on the device (glimmer-mg_amd/csrc/gmg_entropy.hip; include/gmg.h, gmg_entropy_*) against the Python
restatement of the reference's arithmetic (tests/entropy_oracle.py), and integration/long-orfs_gpu against recorded outputs of the
reference's long-orfs (tests/golden/longorfs/, tests/golden/data/NC_000915.longorfs).

The contract: the 20 counts of a region are exact; the device-finished distances differ from the host finish only through the
device's log and d * d in place of pow (d, 2) -- log good to 4 ulp moves an ep_j by about 1e-15, the distance is 1-Lipschitz in ep,
the remaining ~45 roundings act on values <= 1.1: below 5e-15, asserted as <= 1e-13 absolute -- with NaN exactly where the host
gives NaN, and the device ratio is the IEEE quotient of the device's own two distances (1.0 for 0 / 0, 1e3 for x / 0)."""
import os
import subprocess

import numpy as np
import pytest

import entropy_oracle as eo
from conftest import DATA, GOLD, built_binary

pytestmark = pytest.mark.gpu

DIST_TOL = 1e-13


def _rand_seq(rng, n):
    return "".join("acgt"[c] for c in rng.integers(0, 4, size=int(n)))


def _check(gpu, seqs, regions, aa, pos=eo.POS, neg=eo.NEG, reads=None):
    """counts exact, distances within the bound, NaN where the host finish has NaN, ratio = the quotient of the fetched distances;
    -> (counts, dist, the largest distance difference)"""
    reads = reads or gpu.Reads.from_strings(seqs)
    counts, dist = gpu.entropy_regions(reads, regions, aa.encode(), pos, neg)
    want = np.array([eo.counts(seqs[r], f, ln, s, aa) for r, f, ln, s in regions], np.int32).reshape(-1, 20)
    assert np.array_equal(counts, want)
    host = eo.finish_rows(want, pos, neg)
    assert np.array_equal(np.isnan(dist), np.isnan(host))
    ok = ~np.isnan(host[:, 0])
    worst = float(np.max(np.abs(dist[ok, :2] - host[ok, :2]))) if ok.any() else 0.0
    print("largest |device - host| distance: %.3g over %d regions" % (worst, int(ok.sum())))
    assert worst <= DIST_TOL
    for pd, nd, ratio in dist[ok]:
        assert ratio == ((1.0 if pd == 0.0 else 1e3) if nd == 0.0 else pd / nd)
    return counts, dist, worst


@pytest.fixture(scope="module")
def batch():
    """three reads of 100, 37 and 1,000 bases (offsets that are no multiples of 16), then a read of stop codons, poly-a, and one
    with stop codons inside a frame"""
    rng = np.random.default_rng(5)
    seqs = [_rand_seq(rng, 100), _rand_seq(rng, 37), _rand_seq(rng, 1000), "taatagtga" * 7, "a" * 90,
            "atggct" + "taa" + "gctgat" * 5 + "tag" + "cat" * 4 + "tga" + "ggg"]
    return seqs


def test_edge_case_regions(gpu, batch):
    """every length around the 64-codon step (63 / 64 / 65 codons, the second step's boundary), starts where a codon straddles two
    packed words, wraps on both strands, len = n, regions without a countable codon, a single amino acid (NaN), internal stops"""
    seqs = batch
    aa = eo.tables()[11]
    regions = []
    for ln in (0, 1, 2, 3, 4, 189, 192, 195, 384, 387):
        for first in (0, 13, 14, 15, 16 + 13, 32 + 14, 48 + 15):
            for strand in (1, -1):
                regions.append((2, first if strand > 0 else first + 500, ln, strand))
    for r in (0, 1, 2):
        n = len(seqs[r])
        regions += [(r, n - 1, min(n, 60), 1), (r, 0, min(n, 60), -1), (r, n - 2, 9, 1), (r, 1, 9, -1),      # wraps
                    (r, 0, n, 1), (r, n - 1, n, -1), (r, 17 % n, n, 1), (r, 5, n, -1),                        # len = n
                    (r, n - 1, 0, 1), (r, n - 1, 1, -1), (r, 0, 3, 1)]
    regions += [(3, 0, 63, 1), (3, 3, 30, 1), (3, 1, 30, 1),             # stop codons only; out of frame: amino acids
                (4, 0, 90, 1), (4, 7, 60, 1), (4, 89, 90, -1),           # poly-a: K only (NaN); its reverse strand: F only
                (5, 0, len(seqs[5]), 1), (5, 0, 57, 1), (5, len(seqs[5]) - 1, len(seqs[5]), -1)]
    counts, dist, _ = _check(gpu, seqs, regions, aa)
    k = regions.index((3, 0, 63, 1))
    assert not counts[k].any() and not np.isnan(dist[k]).any()           # ep = 0: the distances are the profiles' norms
    k = regions.index((4, 0, 90, 1))
    assert counts[k][eo.AMINO.index("K")] == 30 and counts[k].sum() == 30 and np.isnan(dist[k]).all()
    k = regions.index((5, 0, len(seqs[5]), 1))
    assert counts[k].sum() == len(seqs[5]) // 3 - 3                       # the three stop codons count nowhere


def test_either_output_may_be_null_and_n_zero(gpu, batch):
    reads = gpu.Reads.from_strings(batch)
    aa = eo.tables()[0].encode()
    regions = [(2, 14, 387, 1), (0, 99, 100, -1), (1, 3, 36, 1)]
    both = gpu.entropy_regions(reads, regions, aa, eo.POS, eo.NEG)
    only_counts = gpu.entropy_regions(reads, regions, aa, eo.POS, eo.NEG, want_dist=False)
    only_dist = gpu.entropy_regions(reads, regions, aa, eo.POS, eo.NEG, want_counts=False)
    assert only_counts[1] is None and only_dist[0] is None
    assert np.array_equal(only_counts[0], both[0]) and np.array_equal(only_dist[1].view(np.uint64), both[1].view(np.uint64))
    assert gpu.entropy_regions(reads, regions, aa, eo.POS, eo.NEG, want_counts=False, want_dist=False) == (None, None)
    counts, dist = gpu.entropy_regions(reads, [], aa, eo.POS, eo.NEG)
    assert counts.shape == (0, 20) and dist.shape == (0, 3)


def test_other_profiles_and_the_ratio_rules(gpu, batch):
    """pos == neg gives ratio 1.0 exactly; an all-zero negative profile with a region of no countable codon gives x / 0 = 1e3 and,
    with a zero positive profile as well, 0 / 0 = 1.0; random profiles stay inside the bound"""
    aa = eo.tables()[11]
    regions = [(2, 14, 387, 1), (3, 0, 63, 1), (0, 99, 99, -1)]
    _, dist, _ = _check(gpu, batch, regions, aa, eo.POS, eo.POS)
    assert np.all(dist[:, 2] == 1.0)
    zero = [0.0] * 20
    _, dist, _ = _check(gpu, batch, regions, aa, eo.POS, zero)
    assert dist[1, 1] == 0.0 and dist[1, 2] == 1e3
    _, dist, _ = _check(gpu, batch, regions, aa, zero, zero)
    assert tuple(dist[1]) == (0.0, 0.0, 1.0)
    rng = np.random.default_rng(9)
    _check(gpu, batch, regions, aa, list(rng.random(20) / 10), list(rng.random(20) / 10))


def test_all_translation_tables(gpu):
    """one read that holds the 64 codons, 64 regions of one codon per strand, under each of the 17 tables: counts exact"""
    read = "".join("acgt"[i >> 4] + "acgt"[(i >> 2) & 3] + "acgt"[i & 3] for i in range(64))
    regions = [(0, 3 * i, 3, 1) for i in range(64)] + [(0, 3 * i + 2, 3, -1) for i in range(64)]
    reads = gpu.Reads.from_strings([read])
    for code in eo.CODES:
        aa = eo.tables()[code]
        assert gpu.xlate_table(code) == aa.encode()
        counts, _, _ = _check(gpu, [read], regions, aa, reads=reads)
        for i in range(64):                                            # codon i, forward: the table's letter and nothing else
            k = eo.AMINO.find(aa[i])
            assert counts[i].sum() == (0 if k < 0 else 1) and (k < 0 or counts[i][k] == 1)


def test_entropy_of_the_orfs_of_a_find_orfs_result(gpu, oracle):
    """gmg_entropy_orfs on the device-resident result of gmg_find_orfs for 64 random circular sequences of 300 - 3,000 bases: every
    ORF's region by Entropy_Filter's rule from the fetched records, counts exact, distances within the bound; the batch holds ORFs
    that wrap on both strands (the seed is checked against the CPU oracle's Find_Orfs)"""
    rng = np.random.default_rng(1)
    seqs = [_rand_seq(rng, n) for n in rng.integers(300, 3001, 64)]
    prm = oracle.mg_params(min_gene_len=90, allow_truncated=False)
    want_orfs = [oracle.find_orfs_general(s, prm, circular=True) for s in seqs]
    assert all(w is not None for w in want_orfs)
    reads = gpu.Reads.from_strings(seqs)
    res = gpu.OrfResult(reads, min_gene_len=90, allow_truncated=False, circular=True)
    orfs, off = res.fetch()
    assert len(orfs) == sum(len(w) for w in want_orfs) > 500
    aa = eo.tables()[11]
    counts, dist = gpu.entropy_orfs(reads, res, aa.encode(), eo.POS, eo.NEG)
    regions = [(int(o["read"]),) + eo.orf_region(int(o["stop_position"]), int(o["gene_len"]), int(o["frame"]), len(seqs[int(o["read"])]))
               for o in orfs]
    wraps_fwd = sum(1 for r, f, ln, s in regions if s > 0 and f + ln > len(seqs[r]))
    wraps_rev = sum(1 for r, f, ln, s in regions if s < 0 and f - ln + 1 < 0)
    assert wraps_fwd >= 1 and wraps_rev >= 1
    want = np.array([eo.counts(seqs[r], f, ln, s, aa) for r, f, ln, s in regions], np.int32)
    assert np.array_equal(counts, want)
    host = eo.finish_rows(want)
    assert np.array_equal(np.isnan(dist), np.isnan(host))
    ok = ~np.isnan(host[:, 0])
    worst = float(np.max(np.abs(dist[ok, :2] - host[ok, :2])))
    print("largest |device - host| distance: %.3g over %d ORFs" % (worst, int(ok.sum())))
    assert worst <= DIST_TOL
    assert np.array_equal(dist[ok, 2], dist[ok, 0] / dist[ok, 1])
    # the same regions through gmg_entropy_regions: the same bits
    c2, d2 = gpu.entropy_regions(reads, regions, aa.encode(), eo.POS, eo.NEG)
    assert np.array_equal(c2, counts) and np.array_equal(d2.view(np.uint64), dist.view(np.uint64))
    only_counts, none = gpu.entropy_orfs(reads, res, aa.encode(), eo.POS, eo.NEG, want_dist=False)
    assert none is None and np.array_equal(only_counts, counts)
    res.close()


def test_error_paths(gpu, batch):
    reads = gpu.Reads.from_strings(batch)
    aa = eo.tables()[0].encode()
    n = len(batch[1])
    for bad in [(1, n, 3, 1), (1, -1, 3, 1), (1, 0, n + 1, 1), (1, 0, -3, 1), (1, 0, 3, 0), (len(batch), 0, 3, 1)]:
        with pytest.raises(gpu.GmgError) as e:
            gpu.entropy_regions(reads, [(0, 0, 30, 1), bad], aa, eo.POS, eo.NEG)
        assert e.value.code == -6, bad                                   # GMG_ERANGE
    for bad_byte in (b"a", b"\0", b"-", b"["):
        with pytest.raises(gpu.GmgError) as e:
            gpu.entropy_regions(reads, [(0, 0, 30, 1)], aa[:10] + bad_byte + aa[11:], eo.POS, eo.NEG)
        assert e.value.code == -1                                        # GMG_EINVAL
    counts, _ = gpu.entropy_regions(reads, [(1, n - 1, n, 1)], aa, eo.POS, eo.NEG)           # the largest legal values pass
    assert counts.sum() <= n // 3


# ---- integration/long-orfs_gpu against recorded outputs of the reference's long-orfs ------------------------------------------

def _genome():
    return "".join(line.strip() for line in open(os.path.join(DATA, "NC_000915.fna")) if not line.startswith(">"))


def _write_fasta(path, records):
    with open(path, "w") as f:
        for name, s in records:
            f.write(">%s\n" % name)
            for i in range(0, len(s), 70):
                f.write(s[i:i + 70] + "\n")


def _run(exe, args, cwd):
    return subprocess.run([exe, *args], cwd=str(cwd), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)


def _golden(name):
    return open(os.path.join(GOLD, "longorfs", name), "rb").read()


def test_long_orfs_gpu_on_the_whole_genome(gpu, tmp_path):
    """long-orfs_gpu -n -t 1.15 NC_000915.fna: the reference's sample-run output, byte for byte (1,161 rows)"""
    exe = built_binary("integration", "_build", "long-orfs_gpu")
    res = _run(exe, ["-n", "-t", "1.15", os.path.join(DATA, "NC_000915.fna"), "-"], tmp_path)
    assert res.returncode == 0, res.stderr.decode()[-2000:]
    assert res.stdout == open(os.path.join(DATA, "NC_000915.longorfs"), "rb").read()
    assert b"Final minimum gene length = 409" in res.stderr


@pytest.mark.parametrize("args,golden", [
    (["-n", "-t", "1.15", "-l", "-z", "4"], "s700_n_t115_l_z4.out"),
    (["-n", "-f", "-g", "300", "-w"], "s700_n_f_g300_w.out"),
    (["-t", "1.15"], "s700_t115_hdr.out"),
    (["-n", "-t", "1.15", "--length_opt", "-o", "10"], "s700_n_t115_lengthopt_o10.out"),
])
def test_long_orfs_gpu_option_sets_on_a_slice(gpu, tmp_path, args, golden):
    """the 60 kb slice at 700,000 under four option sets (linear with table 4; fixed minimum length without -t and without stop
    codons, where every printed value comes from the second device call; with the header, which echoes the relative file name;
    the total-length optimum with a 10-base overlap) against the reference's recorded output.  (-L is spelled --length_opt: the
    reference's getopt string has no 'L', so the short form ends in its usage message -- see the next test.)"""
    exe = built_binary("integration", "_build", "long-orfs_gpu")
    _write_fasta(tmp_path / "slice700000.fa", [("slice700000", _genome()[700000:760000])])
    res = _run(exe, [*args, "slice700000.fa", "-"], tmp_path)
    assert res.returncode == 0, res.stderr.decode()[-2000:]
    assert res.stdout == _golden(golden)


def test_long_orfs_gpu_where_the_reference_stops(gpu, tmp_path):
    """an 80-base record: the reference exits 1 with "No valid orfs found below entropy cutoff" and writes nothing; the short
    option -L: its own parser rejects it (exit 1, usage)"""
    exe = built_binary("integration", "_build", "long-orfs_gpu")
    _write_fasta(tmp_path / "short80.fa", [("short80", _genome()[:80])])
    res = _run(exe, ["-n", "-t", "1.15", "short80.fa", "-"], tmp_path)
    assert res.returncode == 1 and res.stdout == b""
    assert b"ERROR:  No valid orfs found below entropy cutoff" in res.stderr
    res = _run(exe, ["-n", "-t", "1.15", "-L", "-o", "10", "short80.fa", "-"], tmp_path)
    assert res.returncode == 1 and res.stdout == b"" and b"USAGE:  long-orfs" in res.stderr


def test_long_orfs_gpu_multi(gpu, tmp_path):
    """--multi on three records (the slices at 0, 700,000 and 1,600,000) and an 80-base one: per record its header line and the rows
    the reference writes for a file that holds this record alone; the short record keeps its header line and no rows"""
    exe = built_binary("integration", "_build", "long-orfs_gpu")
    g = _genome()
    _write_fasta(tmp_path / "multi.fa", [("slice%d" % at, g[at:at + 60000]) for at in (0, 700000)] + [("short80 x", g[:80])]
                 + [("slice1600000", g[1600000:1660000])])
    res = _run(exe, ["--multi", "-n", "-t", "1.15", "multi.fa", "-"], tmp_path)
    assert res.returncode == 0, res.stderr.decode()[-2000:]
    want = (b">slice0\n" + _golden("s0_n_t115.out") + b">slice700000\n" + _golden("s700000_n_t115.out") + b">short80 x\n"
            + b">slice1600000\n" + _golden("s1600000_n_t115.out"))
    assert res.stdout == want
    # without --multi: the first record alone, as the reference
    res = _run(exe, ["-n", "-t", "1.15", "multi.fa", "-"], tmp_path)
    assert res.returncode == 0 and res.stdout == _golden("s0_n_t115.out")
