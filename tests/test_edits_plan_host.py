"""gmg_edits_plan (include/gmg.h; host only, no GPU needed): the edit arithmetic of the reference's scripts/extract_aa.py against
the files that script wrote (tests/golden/extract_aa, made by tests/golden/make_extract_aa.py): the plan's runs are expanded over
the letters of the sequence file in a few lines of Python (tests/splice_oracle.py) and must give the recorded .ffn byte for byte --
record names, order, strings and pad blanks (against the text where it is kept, against its SHA-256 otherwise)."""
import os

import numpy as np
import pytest

import splice_oracle as so

ERANGE = -6


def _plan(gmg, name, with_letters=True):
    fasta = so.read_fasta(so.CASES[name][0])
    headers, seqs = [h for h, _ in fasta], [s for _, s in fasta]
    genes = so.parse_predict(so.CASES[name][1], headers)
    runs, sro, rows = gmg.edits_plan(so.offsets(seqs), genes, so.odd_letters(seqs) if with_letters else None)
    return headers, seqs, genes, runs, sro, rows


@pytest.mark.parametrize("name", sorted(so.CASES))
def test_plan_reproduces_the_recorded_ffn(gmg, name):
    headers, seqs, genes, runs, sro, rows = _plan(gmg, name)
    assert len(rows) == len(genes) and int(sro[-1]) == len(runs)
    so.assert_recorded(name, ".ffn", so.ffn_text(headers, seqs, genes, runs, sro, rows).encode())


def test_the_synthetic_case_holds_what_it_is_for():
    """blanks in front of, behind and only in some strings, an empty record, a read without gene lines"""
    strings = open(os.path.join(so.XA, "edges.ffn")).read().split("\n")[1::2]
    assert any(s.startswith(" ") for s in strings) and any(s.endswith(" ") for s in strings) and "" in strings
    assert ">no_genes" in open(os.path.join(so.XA, "edges.predict")).read()
    assert not any("no_genes" in line for line in open(os.path.join(so.XA, "edges.ffn")))


def test_runs_are_few_and_stay_inside_their_reads(gmg):
    """a gene without edits is one run; every run lies inside its read, downward runs included; pads never become runs"""
    headers, seqs, genes, runs, sro, rows = _plan(gmg, "glimmer-mg.indel")
    for k, (line, start, end, strand, front, behind) in enumerate(rows):
        mine = runs[int(sro[k]):int(sro[k + 1])]
        read = genes[line][0]
        edits = sum(len(g[4]) + len(g[5]) + len(g[6]) for g in genes if g[0] == read)
        if edits == 0:
            assert len(mine) <= 1
        assert len(mine) <= 1 + 3 * edits
        for r, first, n, kind in mine.tolist():
            assert r == read and n > 0
            if kind in (so.UP, so.SUB_UP):
                assert first + n <= len(seqs[r])
            elif kind in (so.DOWN, so.SUB_DOWN):
                assert n <= first + 1 <= len(seqs[r])


def test_without_the_letter_list_the_rules_on_codes_apply(gmg):
    """no list: no literals, the same records; in code space the strings then differ from the script's in the few records that
    substitute a c or an N, or read an ambiguity letter on the reverse strand"""
    headers, seqs, genes, runs, sro, rows = _plan(gmg, "edges", with_letters=False)
    assert runs[:, 3].max() <= so.SUB_DOWN
    _, _, _, lruns, lsro, lrows = _plan(gmg, "edges")
    assert lruns[:, 3].max() >= so.LITERAL_AS_IS and rows == lrows
    codes = [[gmg.capi.lib().gmg_base_code(ord(ch)) for ch in s] for s in seqs]
    plain, exact = so.spliced(codes, runs, sro), so.spliced(codes, lruns, lsro)
    differ = [headers[genes[rows[k][0]][0]] for k in range(len(rows)) if plain[k] != exact[k]]
    assert [len(p) for p in plain] == [len(e) for e in exact]
    assert {"sub_letters", "sub_letters_rev", "letters_rev"} <= set(differ) and len(differ) < 12
    want = open(os.path.join(so.XA, "edges.ffn")).read().split("\n")[1::2]
    assert [[gmg.capi.lib().gmg_base_code(ord(ch)) for ch in w if ch != " "] for w in want] == exact


def test_errors(gmg):
    off = np.array([0, 50, 120], np.uint64)
    with pytest.raises(gmg.GmgError, match="line 1 ") as e:
        gmg.edits_plan(off, [(1, 1, 60, 1, [], [], []), (2, 1, 30, 1, [3], [], [])])
    assert e.value.code == ERANGE
    runs, sro, rows = gmg.edits_plan(off, [])
    assert len(runs) == 0 and list(sro) == [0] and rows == []
    # lines of two reads interleaved: grouped by read, file order kept inside a read
    runs, sro, rows = gmg.edits_plan(off, [(1, 1, 60, 1, [], [], []), (0, 1, 30, 1, [], [], []), (1, 1, 60, 1, [], [], [])])
    assert [r[0] for r in rows] == [1, 0, 2]
