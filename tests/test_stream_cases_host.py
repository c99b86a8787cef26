"""tests/stream_cases.py against include/gmg.h, without a device: every entry point that takes a `void *stream` has a row in the case
table of tests/test_gpu_streams.py or stands in the named exclusion list, the variants DESIGN.md 2.3 names are there, and every
constructor the section lists has its case."""
import os

import stream_cases as sc
from conftest import ROOT


def header():
    return open(os.path.join(ROOT, "include", "gmg.h")).read()


def test_every_stream_taking_prototype_has_a_row_or_a_named_exclusion():
    protos = sc.stream_prototypes(header())
    assert len(protos) >= 37 and "gmg_frame_score6" in protos and "gmg_tophits_scores" in protos      # (the parser sees them)
    covered = {r.entry for r in sc.ROWS}
    missing = [p for p in protos if p not in covered and p not in sc.EXCLUDED]
    assert not missing, "no stream case for %s" % ", ".join(missing)
    assert not covered & set(sc.EXCLUDED), "both a row and an exclusion"
    unknown = [e for e in list(covered) + list(sc.EXCLUDED) if e not in protos]
    assert not unknown, "not a stream-taking prototype of include/gmg.h: %s" % ", ".join(unknown)


def test_the_parser_reads_prototypes_not_words():
    text = """/* gmg_in_a_comment(void *stream); */
    int gmg_one(const char (*codon)[4], void *stream);
    int gmg_two(void **stream);
    int gmg_three(int a,
                  void * stream, const double **out);
    typedef struct gmg_s { int x; } gmg_s;
    int gmg_four(void *streams);"""
    assert sc.stream_prototypes(text) == ["gmg_one", "gmg_three"]


def test_the_variant_rows_are_listed():
    by_entry = {}
    for r in sc.ROWS:
        by_entry.setdefault(r.entry, []).append(r)
    assert len({r.name for r in sc.ROWS}) == len(sc.ROWS)
    mg = [r for r in by_entry["gmg_mg_score_reads"] if not r.options.get("mg_one_stream")]
    assert [r.name for r in mg] == ["mg_score_reads", "mg_score_reads_indels", "mg_score_reads_subs", "mg_score_reads_nulls"]
    assert sorted(r.options["orfs_exact_path"] for r in by_entry["gmg_score_orfs"]) == [0, 1, 2]
    assert sorted(r.options["strings_fused"] for r in by_entry["gmg_score_reads_strings"]) == [0, 1]
    assert any(r.options.get("ingest_piece_min") == 0 for r in by_entry["gmg_fasta_ingest_on"])
    assert "gmg_regions_text_device" in by_entry and "gmg_runs_text_device" in by_entry
    # every row that forks into side streams has a twin on the caller's stream alone, and no other row is excused in mode C
    for entry in sc.SIDE_STREAM_ENTRIES:
        plain = [r for r in by_entry[entry] if not r.options.get("mg_one_stream")]
        twins = [r for r in by_entry[entry] if r.options.get("mg_one_stream") == 1]
        assert plain and [t.name for t in twins] == [r.name + "_one_stream" for r in plain]
    assert sorted(sc.SIDE_STREAM_ENTRIES) == ["gmg_find_orfs", "gmg_mg_score_groups", "gmg_mg_score_reads"]


def test_the_constructors_are_listed():
    want = ["gmg_tophits_create", "gmg_null_set_upload", "gmg_null_set_from_tables", "gmg_null_set_build", "gmg_model_upload",
            "gmg_fixed_model_upload", "gmg_orfs_upload", "gmg_segments_upload", "gmg_letters_upload", "gmg_reads_upload",
            "gmg_reads_wrap_device", "gmg_reads_select", "gmg_reads_extract", "gmg_reads_splice", "gmg_trainer_create"]
    have = [e for k in sc.CTORS for e in k.entries]
    assert sorted(have) == sorted(want)
    text = header()
    for name in want:
        assert name + "(" in text.replace(" (", "(")
    assert not set(have) & set(sc.stream_prototypes(text)), "a constructor takes no stream"


def test_the_job_is_the_one_the_contract_names():
    n = sc.lengths()
    assert len(n) == 200 and n.min() == 0 and n.max() == 961 and (n == 0).sum() == 1 and sorted(n)[-2] <= 700
    assert (n[:sc.N_SEGS] >= 60).all() and sc.N_SEGS == 64 and sc.N_REGIONS == 300
