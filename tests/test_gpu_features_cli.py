"""integration/train-features_gpu: scripts/train_features.py --predict P --seq S in one process.  The yardsticks: the files the
reference produced itself (tests/golden), the restatement of the script (tests/features_oracle.py) for what the held files do not
pin, and for the gene ICM the reference's build-icm -r (oracle/_ref) fed the restatement's gene strings."""
import os
import shutil
import subprocess

import pytest

import features_cases as fc
import features_oracle as fo
from conftest import built_binary, DATA, GOLD

pytestmark = pytest.mark.gpu

FEAT = os.path.join(GOLD, "features")
NC_FNA = os.path.join(DATA, "NC_000915.fna")
NC_PREDICT = os.path.join(GOLD, "predict", "NC_000915.run1.predict")
SEQS = os.path.join(DATA, "seqs.fa")


def ours(args, **kw):
    exe = built_binary("integration", "_build", "train-features_gpu")
    return subprocess.run([exe, *args], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300, **kw)


def reference_icm(records, tmp_path):
    """build-icm -r on the text of the gene strings"""
    ref = built_binary("oracle", "_ref", "build-icm")
    out = tmp_path / "ref.gicm"
    subprocess.run([ref, "-r", str(out)], input=fo.gene_fasta(records).encode("latin-1"), check=True, timeout=300)
    return open(out, "rb").read()


def run_on(tmp_path, predict, seq, *opts):
    """the tool on a copy of the predict file (its outputs land beside it) -> prefix of the outputs"""
    local = tmp_path / os.path.basename(predict)
    shutil.copy(predict, local)
    res = ours(["--predict", str(local), "--seq", seq, *opts])
    assert res.returncode == 0, res.stderr.decode()
    return os.path.splitext(str(local))[0]


_oracle = {}


def oracle_of(predict, seq, *args):
    key = (predict, seq) + args
    if key not in _oracle:
        genes, seqs = fo.load(predict, seq)
        _oracle[key] = (genes, seqs) + fo.count(genes, seqs, *args)
    return _oracle[key]


def cluster_predict(k):
    return os.path.join(FEAT, "seqs.cluster-%d.run1.filt.predict" % k)


def test_genome_feature_file_and_icm(tmp_path):
    prefix = run_on(tmp_path, NC_PREDICT, NC_FNA, "-f")
    with open(os.path.join(DATA, "NC_000915.run1.features.txt"), "rb") as fp:
        assert open(prefix + ".features.txt", "rb").read() == fp.read()
    genes, seqs, gs, ns = oracle_of(NC_PREDICT, NC_FNA)
    assert open(prefix + ".gicm", "rb").read() == reference_icm(fo.gene_strings(genes, seqs), tmp_path)


@pytest.mark.parametrize("k", range(6))
def test_cluster_feature_file(k, tmp_path):
    prefix = run_on(tmp_path, cluster_predict(k), SEQS, "-f")
    mine = open(prefix + ".features.txt").read()
    with open(os.path.join(DATA, "seqs.cluster-%d.run1.filt.features.txt" % k)) as fp:
        held = fo.sections(fp.read())
    for title in ("DIST START GENE", "DIST START NON"):
        assert fo.sections(mine)[title] == held[title]
    genes, seqs, gs, ns = oracle_of(cluster_predict(k), SEQS)
    assert mine == fo.feature_file(gs, ns)
    if k in (0, 4):
        assert open(prefix + ".gicm", "rb").read() == reference_icm(fo.gene_strings(genes, seqs), tmp_path)


def test_separate_files_and_gc(tmp_path):
    prefix = run_on(tmp_path, cluster_predict(3), SEQS, "-l", "60", "--max_overlap=40", "-z")
    genes, seqs, gs, ns = oracle_of(cluster_predict(3), SEQS, 60, 40, True)
    for suffix, text in fo.stat_files(gs, ns, 40).items():
        assert open("%s.%s" % (prefix, suffix)).read() == text, suffix
    assert open(prefix + ".gc.txt").read() == fo.gc_text(seqs)
    assert not os.path.exists(prefix + ".features.txt") and os.path.exists(prefix + ".gicm")


def test_opaque_letters_reach_the_gene_strings(tmp_path):
    """N, R and lower-case letters inside genes of both strands: the script's rc() leaves what is not ACGTacgt as it is"""
    seqs, lines = fc.opaque_letters()
    more_seqs, more_lines = fc.differential()           # (enough strings for a model)
    seqs, lines = seqs + more_seqs[:120], lines + [("f", 60, 31, -1)] + [l for l in more_lines if int(l[0][1:]) < 120]
    fa, predict = tmp_path / "opaque.fa", tmp_path / "opaque.run1.predict"
    fa.write_text("".join(">%s\n%s\n" % (h, "\n".join(s[i:i + 60] for i in range(0, len(s), 60))) for h, s in seqs))
    text, last = "", None
    for hdr, a, b, frame in lines:
        if hdr != last:
            text += ">%s\n" % hdr
            last = hdr
        text += "orf%05d %8d %8d %+d %8.2f\n" % (len(text), a, b, frame, 3.0)
    predict.write_text(text)
    res = ours(["--predict", str(predict), "--seq", str(fa), "-f", "-l", "0"])
    assert res.returncode == 0, res.stderr.decode()
    genes, sd = fo.load(str(predict), str(fa))
    gs, ns = fo.count(genes, sd, 0)
    records = fo.gene_strings(genes, sd)
    assert any("R" in s for _, s in records) and any("N" in s for _, s in records) and any("a" in s or "t" in s for _, s in records)
    assert open(tmp_path / "opaque.run1.features.txt").read() == fo.feature_file(gs, ns)
    assert open(tmp_path / "opaque.run1.gicm", "rb").read() == reference_icm(records, tmp_path)


def test_icm_only_and_min_icm(tmp_path):
    local = tmp_path / "c5.predict"
    shutil.copy(cluster_predict(5), local)
    (tmp_path / "c5.gicm").write_text("stale")
    res = ours(["--predict", str(local), "--seqs", SEQS, "--icm", "--min_icm", "100000000"])
    assert res.returncode == 0, res.stderr.decode()
    assert (tmp_path / "c5.gicm").read_text() == "stale" and not os.path.exists(tmp_path / "c5.lengths.genes.txt")
    res = ours(["--predict", str(local), "--seqs", SEQS, "--icm"])
    assert res.returncode == 0, res.stderr.decode()
    genes, seqs, gs, ns = oracle_of(cluster_predict(5), SEQS)
    assert open(tmp_path / "c5.gicm", "rb").read() == reference_icm(fo.gene_strings(genes, seqs), tmp_path)
    assert not os.path.exists(tmp_path / "c5.lengths.genes.txt") and not os.path.exists(tmp_path / "c5.features.txt")


@pytest.mark.parametrize("opts,word", [(["--gbk", "x.gbk"], b"Biopython"), (["--rbs"], b"ELPH"), (["--indels"], b"extract_aa")])
def test_refused_options(opts, word, tmp_path):
    res = ours(["--predict", cluster_predict(4), "--seq", SEQS, *opts], cwd=tmp_path)
    assert res.returncode == 2 and word in res.stderr and res.stderr.count(b"\n") == 1


def test_refused_inputs(tmp_path):
    predict = tmp_path / "p.predict"
    fa = tmp_path / "s.fa"
    fa.write_text(">one\nACGTACGTAAACGT\n>two words\nACGTTTGACC\n>one\nACGT\n")
    predict.write_text(">two words\norf1 1 9 +1 2.0\n")
    res = ours(["--predict", str(predict), "--seq", str(fa), "-f"])
    assert res.returncode == 1 and b"'one' occurs twice" in res.stderr
    fa.write_text(">one\nACGTACGTAAACGT\n>two words\nACGTTTGACC\n")
    predict.write_text(">two words\norf1 1 9 +1 2.0\n>three\norf2 1 9 +1 2.0\n")
    res = ours(["--predict", str(predict), "--seq", str(fa), "-f"])
    assert res.returncode == 1 and b"'three'" in res.stderr
    predict.write_text(">two words\n>one\n")
    res = ours(["--predict", str(predict), "--seq", str(fa), "-f"])
    assert res.returncode == 1 and b"no gene line" in res.stderr
    assert not os.path.exists(tmp_path / "p.features.txt")
