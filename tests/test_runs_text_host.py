"""The yardstick of gmg_runs_text before any device is involved: the Python restatement (tests/runs_text_oracle.py), applied to
gmg_edits_plan's output with the script's parameters, gives the .ffn AND the .faa file scripts/extract_aa.py wrote for every
recorded case; and gmg_runs_text_params_script (host code) fills those parameters."""
import pytest

import entropy_oracle as eo
import runs_text_oracle as ro
import splice_oracle as so


@pytest.mark.parametrize("name", sorted(so.CASES))
def test_the_restatement_gives_the_recorded_files(gmg, name):
    seqs, runs, sro, heads, front, behind = ro.case_inputs(gmg, name)
    ffn = ro.text(seqs, runs, sro, heads, ro.Params(ro.DNA), front, behind)
    faa = ro.text(seqs, runs, sro, heads, ro.Params(ro.PROTEIN), front, behind)
    assert ffn.count(b"\n") == faa.count(b"\n") == 2 * len(heads) > 0
    so.assert_recorded(name, ".ffn", ffn)
    so.assert_recorded(name, ".faa", faa)


def test_the_recorded_cases_hold_what_the_translation_must_tell_apart(gmg):
    """lower-case codons, codons with a pad blank and codons with a foreign letter all occur in the recorded .faa files"""
    faa = so.recorded_text("edges", ".faa").decode()
    bodies = "".join(faa.split("\n")[1::2])
    assert "X" in bodies and any(c.islower() for c in bodies) and any(c.isupper() for c in bodies)


def test_script_parameters(gmg):
    """every field gmg_runs_text_params_script fills, against the restatement's defaults"""
    for mode in (ro.DNA, ro.PROTEIN):
        p, want = gmg.runs_text_params(mode, 0), ro.Params(mode)
        for name in ("up", "down", "sub_up", "sub_down", "literal"):
            assert bytes(getattr(p, name)) == getattr(want, name), name
        assert (p.pad, p.unknown, p.width, p.mode, bytes(p.reserved)) == (ord(" "), ord("X"), 0, mode, b"\0\0")
        assert p.aa == want.aa
    assert gmg.runs_text_params(ro.DNA, 0, width=60).width == 60
    assert bytes(p.down[c] for c in b"ATCGatcgNn*-") == b"TAGCtagcNn*-"
    assert bytes(p.sub_up[c] for c in b"ACGTcn") == b"CGCCCC" and bytes(p.sub_down[c] for c in b"ACGTcn") == b"GCGGGG"


def test_table_0_is_the_scripts_dictionary(gmg):
    """the 64 upper-case and the 64 lower-case codons of extract_aa.py's dictionary, through the library's table and the
    restatement's translation"""
    code = {a + b + c: ro.SCRIPT_CODE[16 * i + 4 * j + k] for i, a in enumerate("TCAG") for j, b in enumerate("TCAG") for k, c in enumerate("TCAG")}
    assert (code["ATG"], code["TGA"], code["TGG"], code["GCA"], code["AAA"]) == ("M", "*", "W", "A", "K") and len(code) == 64
    code.update({k.lower(): v.lower() for k, v in list(code.items())})
    prm = ro.Params(ro.PROTEIN, aa=gmg.runs_text_params(ro.PROTEIN, 0).aa)
    for codon, letter in code.items():
        assert ro.translate(codon.encode(), prm) == letter.encode(), codon
    assert ro.translate(b"tga", prm) == b"*" and ro.translate(b"AcG", prm) == b"X" and ro.translate(b"ANG ", prm) == b"X"


@pytest.mark.parametrize("table", [4, 11])
def test_other_tables_are_codon_translations(gmg, table):
    assert gmg.runs_text_params(ro.PROTEIN, table).aa == eo.tables()[table].encode()
    assert (gmg.runs_text_params(ro.PROTEIN, table).aa == ro.script_aa()) == (table == 11)


def test_a_bad_table_or_mode_is_refused(gmg):
    for table in (7, 8, 24, -1):
        with pytest.raises(gmg.GmgError) as e:
            gmg.runs_text_params(ro.PROTEIN, table)
        assert e.value.code == -1
    with pytest.raises(gmg.GmgError) as e:
        gmg.runs_text_params(2, 0)
    assert e.value.code == -1
