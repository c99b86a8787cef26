"""integration/extract-aa_gpu: scripts/extract_aa.py -s S -p P in one process, and with --gicm the ICM step of train_features.py
--indels.  The yardsticks: the .ffn / .faa files the reference's script wrote (tests/golden/extract_aa: their text, or their SHA-256 where no test needs the text) and, for the gene
ICM, the reference's build-icm -r (oracle/_ref) fed that .ffn text (so.script_ffn: text that has the recorded digest)."""
import os
import subprocess

import pytest

import splice_oracle as so
from conftest import built_binary, GOLD

pytestmark = pytest.mark.gpu


def tool(*args):
    exe = built_binary("integration", "_build", "extract-aa_gpu")
    return subprocess.run([exe, *args], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)


def recorded(name, ext):
    return so.recorded_text(name, ext)


@pytest.mark.parametrize("name", sorted(so.CASES))
def test_ffn_and_faa_are_the_scripts(gpu, name, tmp_path):
    seqs, predict = so.CASES[name]
    res = tool("-s", seqs, "-p", predict, "-o", str(tmp_path / "out"))
    assert res.returncode == 0, res.stderr
    so.assert_recorded(name, ".ffn", open(tmp_path / "out.ffn", "rb").read())
    so.assert_recorded(name, ".faa", open(tmp_path / "out.faa", "rb").read())
    assert sorted(os.listdir(tmp_path)) == ["out.faa", "out.ffn"]


def test_default_prefix_is_the_sequence_file_without_its_extension(gpu, tmp_path):
    seqs, predict = so.CASES["edges"]
    local = tmp_path / "my.reads.fa"
    local.write_bytes(open(seqs, "rb").read())
    res = tool("-s", str(local), "-p", predict)
    assert res.returncode == 0, res.stderr
    assert open(tmp_path / "my.reads.ffn", "rb").read() == recorded("edges", ".ffn")
    assert os.path.exists(tmp_path / "my.reads.faa")


@pytest.mark.parametrize("name", ["glimmer-mg.indel", "edges"])
def test_gicm_is_build_icm_r_on_the_recorded_text(gpu, name, tmp_path):
    """--gicm: .gene.fasta is the .ffn text, .faa and .ffn are gone, .gicm equals the reference's build-icm -r fed the recorded
    .ffn -- blanks inside its lines and empty records included"""
    seqs, predict = so.CASES[name]
    prefix = str(tmp_path / "out")
    for ext in (".faa", ".ffn"):
        open(prefix + ext, "w").write("stale\n")
    res = tool("-s", seqs, "-p", predict, "-o", prefix, "--gicm")
    assert res.returncode == 0, res.stderr
    assert sorted(os.listdir(tmp_path)) == ["out.gene.fasta", "out.gicm"]
    so.assert_recorded(name, ".ffn", open(prefix + ".gene.fasta", "rb").read())
    ref = built_binary("oracle", "_ref", "build-icm")
    subprocess.run([ref, "-r", str(tmp_path / "ref.gicm")], input=so.script_ffn(gpu, name), check=True, timeout=300)
    assert open(prefix + ".gicm", "rb").read() == open(tmp_path / "ref.gicm", "rb").read()


def test_min_icm_counts_the_printed_characters(gpu, tmp_path):
    """the script's count: len(line.rstrip()) of every string -- blanks in front count, trailing ones do not.  One more than that
    leaves a stale .gicm untouched; exactly that many trains"""
    seqs, predict = so.CASES["edges"]
    printed = sum(len(s.rstrip()) for s in recorded("edges", ".ffn").decode().split("\n")[1::2])
    assert printed != sum(len(s) for s in recorded("edges", ".ffn").decode().split("\n")[1::2])
    prefix = str(tmp_path / "out")
    open(prefix + ".gicm", "w").write("stale\n")
    res = tool("-s", seqs, "-p", predict, "-o", prefix, "--gicm", "--min_icm", str(printed + 1))
    assert res.returncode == 0, res.stderr
    assert open(prefix + ".gicm").read() == "stale\n" and os.path.exists(prefix + ".gene.fasta")
    res = tool("-s", seqs, "-p", predict, "-o", prefix, "--gicm", "--min_icm=%d" % printed)
    assert res.returncode == 0, res.stderr
    assert open(prefix + ".gicm", "rb").read() != b"stale\n"


@pytest.mark.parametrize("predict", ["glimmer-mg.indel_q80", "classes.mixed_sub"])
def test_a_sequence_without_a_predict_record_is_refused(gpu, predict, tmp_path):
    """the two recorded runs that cover only a part of seqs.fa: the script dies with a KeyError"""
    res = tool("-s", so.CASES["glimmer-mg.indel"][0], "-p", os.path.join(GOLD, "predict", predict + ".predict"), "-o", str(tmp_path / "out"))
    assert res.returncode == 1 and os.listdir(tmp_path) == []
    err = res.stderr.decode().strip().split("\n")
    assert len(err) == 1 and "has no record" in err[0] and "read" in err[0]


def test_refusals_name_the_offender(gpu, tmp_path):
    """a gene line without its I: D: S: fields; a header that occurs twice: status 1, one line, nothing written"""
    seqs, predict = so.CASES["edges"]
    out = tmp_path / "out"
    out.mkdir()
    text = open(predict).read().split("\n")
    k = next(i for i, line in enumerate(text) if line.startswith("orf"))
    short = tmp_path / "short.predict"
    short.write_text("\n".join(text[:k] + [" ".join(text[k].split()[:5])] + text[k + 1:]))
    res = tool("-s", seqs, "-p", str(short), "-o", str(out / "x"))
    err = res.stderr.decode().strip().split("\n")
    assert res.returncode == 1 and len(err) == 1 and "I: D: S:" in err[0] and text[k].split()[0] in err[0]
    twice = tmp_path / "twice.fa"
    twice.write_text(open(seqs).read() + ">ins_last\nACGTACGT\n")
    res = tool("-s", str(twice), "-p", predict, "-o", str(out / "x"))
    err = res.stderr.decode().strip().split("\n")
    assert res.returncode == 1 and len(err) == 1 and "'ins_last' occurs twice" in err[0]
    assert os.listdir(out) == []
    res = tool("-s", seqs)
    assert res.returncode == 2
