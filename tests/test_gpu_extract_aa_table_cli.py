"""integration/extract-aa_gpu -z N / --transl_table N: the .faa under another GenBank translation table.  The fixture
(tests/golden/extract_aa/tga.fa, tga.predict: hand-written) holds genes with TGA in frame on either strand and in lower case,
which table 4 reads through as W; the yardstick is the restatement (tests/runs_text_oracle.py) under gmg_xlate_table's table."""
import os
import subprocess

import pytest

import entropy_oracle as eo
import runs_text_oracle as ro
import splice_oracle as so
from conftest import built_binary

pytestmark = pytest.mark.gpu

SEQS, PREDICT = os.path.join(so.XA, "tga.fa"), os.path.join(so.XA, "tga.predict")


def tool(*args):
    exe = built_binary("integration", "_build", "extract-aa_gpu")
    return subprocess.run([exe, *args], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)


@pytest.fixture(scope="module")
def want(gmg):
    """{table: the .faa text}, and the .ffn text, by the restatement"""
    so.CASES["tga"] = (SEQS, PREDICT)
    try:
        seqs, runs, sro, heads, front, behind = ro.case_inputs(gmg, "tga")
    finally:
        del so.CASES["tga"]
    faa = {t: ro.text(seqs, runs, sro, heads, ro.Params(ro.PROTEIN, aa=(ro.script_aa() if t == 0 else eo.tables()[t].encode())), front, behind)
           for t in (0, 4, 11)}
    return faa, ro.text(seqs, runs, sro, heads, ro.Params(ro.DNA), front, behind)


def test_the_fixture_tells_the_tables_apart(want):
    faa, ffn = want
    assert faa[0] == faa[11] != faa[4] and faa[0].count(b"*") == 9 and b"*" not in faa[4]
    assert faa[0].replace(b"*", b"W").upper() == faa[4].upper()
    assert b"TGA" in ffn and b"tga" in ffn and b"X" in faa[4]


@pytest.mark.parametrize("option", ["-z", "--transl_table"])
def test_table_4_reads_tga_through(gpu, want, option, tmp_path):
    faa, ffn = want
    res = tool("-s", SEQS, "-p", PREDICT, "-o", str(tmp_path / "std"))
    assert res.returncode == 0, res.stderr
    res = tool("-s", SEQS, "-p", PREDICT, "-o", str(tmp_path / "myco"), *([option, "4"] if option == "-z" else [option + "=4"]))
    assert res.returncode == 0, res.stderr
    got = {name: open(tmp_path / name, "rb").read() for name in sorted(os.listdir(tmp_path))}
    assert sorted(got) == ["myco.faa", "myco.ffn", "std.faa", "std.ffn"]
    assert got["std.faa"] == faa[0] and got["myco.faa"] == faa[4] and got["std.faa"] != got["myco.faa"]
    assert got["std.ffn"] == got["myco.ffn"] == ffn


def test_table_11_is_the_default(gpu, want, tmp_path):
    res = tool("-s", SEQS, "-p", PREDICT, "-o", str(tmp_path / "out"), "-z", "11")
    assert res.returncode == 0, res.stderr
    assert open(tmp_path / "out.faa", "rb").read() == want[0][0]


@pytest.mark.parametrize("value", ["7", "24", "-1", "four", ""])
def test_a_bad_table_is_refused(gpu, value, tmp_path):
    res = tool("-s", SEQS, "-p", PREDICT, "-o", str(tmp_path / "out"), "-z", value)
    err = res.stderr.decode().strip().split("\n")
    assert res.returncode == 2 and len(err) == 1 and "translation table" in err[0], res.stderr
    assert os.listdir(tmp_path) == []
