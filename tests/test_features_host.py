"""The yardstick of the feature-model tests pinned to what the reference produced itself: tests/features_oracle.py, a sequential
Python 3 restatement of scripts/train_features.py, against the input / output pairs of the reference's sample-run that are held
under tests/golden/.  Plus the two host-only entry points, gmg_fasta_not_upper_acgt and gmg_features_format.  No GPU."""
import os

import numpy as np
import pytest

import features_oracle as fo
from conftest import DATA, GOLD

FEAT = os.path.join(GOLD, "features")


def held_sha(name):
    for line in open(os.path.join(FEAT, "gene_fasta.sha256")):
        digest, _, rest = line.partition("  ")
        if rest.strip() == name:
            return digest
    raise KeyError(name)


@pytest.fixture(scope="module")
def genome():
    genes, seqs = fo.load(os.path.join(GOLD, "predict", "NC_000915.run1.predict"), os.path.join(DATA, "NC_000915.fna"))
    return genes, seqs


@pytest.fixture(scope="module")
def read_seqs():
    with open(os.path.join(DATA, "seqs.fa")) as fp:
        return fo.parse_seqs(fp.read())


def cluster(k, read_seqs):
    with open(os.path.join(FEAT, "seqs.cluster-%d.run1.filt.predict" % k)) as fp:
        return fo.parse_predict(fp.read(), read_seqs)


def test_genome_feature_file_is_the_held_one(genome):
    genes, seqs = genome
    gs, ns = fo.count(genes, seqs)
    with open(os.path.join(DATA, "NC_000915.run1.features.txt")) as fp:
        held = fp.read()
    assert len(fo.sections(held)) == 12                 # six sections per table, GENE and NON
    assert fo.feature_file(gs, ns) == held


def test_genome_has_letters_outside_acgt(genome):
    genes, seqs = genome
    (seq,) = seqs.values()
    assert any(ch not in "ACGT" for ch in seq)


def test_genome_gene_strings_have_the_held_hash(genome):
    genes, seqs = genome
    assert fo.sha256(fo.gene_fasta(fo.gene_strings(genes, seqs))) == held_sha("NC_000915.run1.gene.fasta")


@pytest.mark.parametrize("k", range(6))
def test_cluster_start_sections_and_gene_strings(k, read_seqs):
    genes = cluster(k, read_seqs)
    gs, ns = fo.count(genes, read_seqs)
    with open(os.path.join(DATA, "seqs.cluster-%d.run1.filt.features.txt" % k)) as fp:
        held = fo.sections(fp.read())
    mine = fo.sections(fo.feature_file(gs, ns))
    for title in ("DIST START GENE", "DIST START NON"):
        assert mine[title] == held[title]
    records = sorted(">%s\n%s\n" % r for r in fo.gene_strings(genes, read_seqs))
    assert fo.sha256("".join(records)) == held_sha("seqs.cluster-%d.run1.filt.gene.fasta.sorted" % k)


# ---- gmg_fasta_not_upper_acgt ---------------------------------------------------------------------------------------------------

def test_not_upper_acgt(gmg):
    data = b"junk in front\n>one first\nACGTN\nacgt R\n\n>two > still header\nTT\tYA\n>empty\n>last\n*A"
    #            bases: A C G T N a c g t R | T T Y A | * A
    assert gmg.fasta_not_upper_acgt(data).tolist() == [4, 5, 6, 7, 8, 9, 12, 14]
    assert gmg.fasta_not_upper_acgt(b"").tolist() == [] and gmg.fasta_not_upper_acgt(b">h\nACGT\n").tolist() == []
    # the list contains gmg_fasta_ambiguous's (the letters outside acgtACGT), which numbers the bases in the same way
    assert set(gmg.fasta_ambiguous(data)[0].tolist()) <= set(gmg.fasta_not_upper_acgt(data).tolist())


def test_not_upper_acgt_on_the_genome(gmg, genome):
    genes, seqs = genome
    (seq,) = seqs.values()
    with open(os.path.join(DATA, "NC_000915.fna"), "rb") as fp:
        got = gmg.fasta_not_upper_acgt(fp.read())
    assert got.tolist() == [i for i, ch in enumerate(seq) if ch not in "ACGT"]


def test_not_upper_acgt_counts_beyond_the_room(gmg):
    import ctypes as C
    lib = gmg.capi.lib()
    data = b">h\nNNACGTNN\n"
    base = np.full(3, 99, np.uint64)
    n = C.c_uint64()
    assert lib.gmg_fasta_not_upper_acgt(data, len(data), base.ctypes.data_as(C.c_void_p), 2, C.byref(n)) == 0
    assert n.value == 4 and base.tolist() == [0, 1, 99]


# ---- gmg_features_format ----------------------------------------------------------------------------------------------------------

def stats_of(lengths, starts, orients, dists):
    s = fo.init_stats()
    s["lengths"] = dict(lengths)
    s["start_codons"] = dict(zip(fo.STARTS, starts))
    s["adj_orients"] = dict(zip(fo.ORIENTS, orients))
    for o, d in zip(fo.ORIENTS, dists):
        s["adj_dist"][o] = dict(d)
    return s


def table_from(gmg, stats, max_overlap):
    top = max(stats["lengths"].keys(), default=-1)
    lengths = [stats["lengths"].get(l, 0) for l in range(top + 1)]
    dist = []
    for o in fo.ORIENTS[:3]:
        d = stats["adj_dist"][o]
        dist.append([float(d.get(l, 0)) for l in range(-max_overlap, 1 + max(d.keys()))] if d else [])
    return gmg.FeatureTable(lengths, [stats["start_codons"][c] for c in fo.STARTS], [float(stats["adj_orients"][o]) for o in fo.ORIENTS], dist)


def test_format_hand_made_tables(gmg):
    three = 0.05 + 0.05 + 0.05                          # 0.15000000000000002, printed 0.2; the literal 0.15 is printed 0.1
    assert three != 0.15 and "%.1f" % three == "0.2" and "%.1f" % 0.15 == "0.1"
    sixth = sum([1.0 / 6] * 6)                          # 0.9999999999999999: %d prints 0
    stats = stats_of({0: 1, 3: 7, 4: 123456789012}, (10, 0, 3), (2.5, sixth, 1.0 / 3 + 1.0 / 3 + 1.0 / 3, 2.5),
                     ({-50: 0.15, -49: three, 2: 7.25}, {}, {0: 1e-9, 1: 0.25, 2: 0.35, 3: 12345678.96}, {}))
    for max_overlap in (50, 51):
        t = table_from(gmg, stats, max_overlap)
        assert gmg.features_format(t, "NON", gmg.FEATURES_BLOCK, max_overlap) == fo.feature_block(stats, "NON", max_overlap)
        files = fo.stat_files(stats, stats, max_overlap)
        assert gmg.features_format(t, "", gmg.FEATURES_LENGTHS, max_overlap) == files["lengths.non.txt"]
        assert gmg.features_format(t, "", gmg.FEATURES_STARTS, max_overlap) == files["starts.non.txt"]
        assert gmg.features_format(t, "", gmg.FEATURES_ORIENTS, max_overlap) == files["adj_orients.non.txt"]
        for k, (a, b) in enumerate(fo.ORIENTS[:3]):
            assert gmg.features_format(t, "", gmg.FEATURES_DIST + k, max_overlap) == files["adj_dist.%d.%d.non.txt" % (a, b)]
    block = gmg.features_format(table_from(gmg, stats, 50), "GENE", gmg.FEATURES_BLOCK, 50)
    assert "1,-1\t0\n-1,1\t1\n" in block and "-50\t0.1\n-49\t0.2\n" in block
    # an empty distance table is its title and the blank line, nothing else
    assert "DIST ADJACENT_DISTANCE_1_-1 GENE\n\nDIST ADJACENT_DISTANCE_-1_1 GENE\n-50\t0.0\n-49\t0.0\n" in block
    assert block.endswith("-1\t0.0\n0\t0.0\n1\t0.2\n2\t0.3\n3\t12345679.0\n\n")


def test_format_an_empty_table(gmg):
    t = gmg.FeatureTable([], (0, 0, 0), (0.0, 0.0, 0.0, 0.0), ([], [], []))
    assert gmg.features_format(t, "NON") == ("DIST LENGTH NON\n\nDIST START NON\nATG\t0\nGTG\t0\nTTG\t0\n\nDIST ADJACENT_ORIENTATION NON\n"
                                             "1,1\t0\n1,-1\t0\n-1,1\t0\n-1,-1\t0\n\nDIST ADJACENT_DISTANCE_1_1 NON\n\n"
                                             "DIST ADJACENT_DISTANCE_1_-1 NON\n\nDIST ADJACENT_DISTANCE_-1_1 NON\n\n")
    assert gmg.features_format(t, "", gmg.FEATURES_LENGTHS) == "" and gmg.features_format(t, "", gmg.FEATURES_DIST + 2) == ""


def test_format_refuses_bad_arguments(gmg):
    import ctypes as C
    t = gmg.FeatureTable([1], (0, 0, 0), (0.0,) * 4, ([], [], []))
    with pytest.raises(gmg.GmgError) as e:
        gmg.features_format(t, "NON", 7)
    assert e.value.code == -1
    st = t._struct()
    n = C.c_size_t(3)
    buf = C.create_string_buffer(3)
    assert gmg.capi.lib().gmg_features_format(C.byref(st), b"NON", 0, 50, buf, C.byref(n)) == -6 and n.value > 3
