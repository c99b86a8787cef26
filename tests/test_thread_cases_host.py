"""tests/thread_cases.py against include/gmg.h and tests/stream_cases.py, without a device: every handle type of the header is
classified as mutable or const, every row of the stream table is either safe on a shared job or names the mutable
handle that keeps it on a job of its own, and the option groups partition the table."""
import os

import stream_cases as sc
import thread_cases as tc
from conftest import ROOT


def header():
    return open(os.path.join(ROOT, "include", "gmg.h")).read()


def test_every_handle_type_is_classified():
    types = tc.handle_types(header())
    assert len(types) >= 18 and "gmg_model" in types and "gmg_letters" in types and "gmg_features" in types     # (the parser sees them)
    assert "gmg_segment" not in types and "gmg_mg_params" not in types                                          # (records are no handles)
    both = set(tc.MUTABLE_HANDLES) & set(tc.CONST_HANDLES)
    assert not both, "both mutable and const: %s" % ", ".join(sorted(both))
    missing = [t for t in types if t not in tc.MUTABLE_HANDLES and t not in tc.CONST_HANDLES]
    assert not missing, "handle type in neither list of tests/thread_cases.py: %s" % ", ".join(missing)
    unknown = [t for t in tc.MUTABLE_HANDLES + tc.CONST_HANDLES if t not in types]
    assert not unknown, "not a handle type of include/gmg.h: %s" % ", ".join(unknown)


def test_the_lists_are_the_contracts():
    assert sorted(tc.MUTABLE_HANDLES) == ["gmg_letters", "gmg_model_set", "gmg_orf_batch", "gmg_single", "gmg_tophits", "gmg_trainer"]
    assert sorted(tc.CONST_HANDLES) == ["gmg_audit", "gmg_classes", "gmg_fasta", "gmg_features", "gmg_fixed_model", "gmg_gaps",
                                        "gmg_mg_result", "gmg_model", "gmg_null_set", "gmg_reads", "gmg_segments", "gmg_windows"]


def test_the_handle_parser_reads_forward_declarations_only():
    text = """/* typedef struct gmg_in_a_comment gmg_in_a_comment; */
    typedef struct gmg_a gmg_a;       /* a handle */
    typedef struct gmg_rec { int x; } gmg_rec;
    typedef struct gmg_b
        gmg_b;
    typedef struct gmg_c gmg_other;
    typedef enum gmg_e { GMG_X } gmg_e;"""
    assert tc.handle_types(text) == ["gmg_a", "gmg_b"]


def test_every_row_is_shared_or_names_its_mutable_handle():
    names = [r.name for r in sc.ROWS]
    for n in names:
        assert (n in tc.SHARED_OK) != (n in tc.OWN_JOB_ONLY), "%s: in both lists or in neither" % n
    assert not [n for n in list(tc.SHARED_OK) + list(tc.OWN_JOB_ONLY) if n not in names], "not a row of tests/stream_cases.py"
    assert set(tc.OWN_JOB_ONLY.values()) <= set(tc.MUTABLE_HANDLES)
    # what keeps a row on its own job is visible in its entry point: the text calls take the job's gmg_letters, the ORF scorer its batch
    by_name = {r.name: r for r in sc.ROWS}
    for n, handle in tc.OWN_JOB_ONLY.items():
        entry = by_name[n].entry
        assert ("_text" in entry) == (handle == "gmg_letters") and entry.startswith("gmg_score_orfs") == (handle == "gmg_orf_batch"), n
    for n in tc.SHARED_OK:
        assert "_text" not in by_name[n].entry and not by_name[n].entry.startswith("gmg_score_orfs"), n
    assert len(tc.SHARED_OK) >= 30 and "mg_score_reads" in tc.SHARED_OK and "mg_result_fetch_on" in tc.SHARED_OK


def test_every_stream_taking_entry_point_takes_part():
    """case A runs every row: the rows cover every stream-taking prototype but the named exclusions (tests/test_stream_cases_host.py
    holds the table to that), and every row is in exactly one option group"""
    protos = sc.stream_prototypes(header())
    groups = tc.option_groups()
    in_groups = [r.name for _, rows in groups for r in rows]
    assert sorted(in_groups) == sorted(r.name for r in sc.ROWS)
    assert not [p for p in protos if p not in sc.EXCLUDED and p not in {r.entry for _, rows in groups for r in rows}]
    for opts, rows in groups:
        assert all(r.options == opts for r in rows)
    keys = [tuple(sorted(opts.items())) for opts, _ in groups]
    assert len(set(keys)) == len(keys) and () in keys
    # the variants the contract names run apart from the defaults
    for want in ({"mg_one_stream": 1}, {"ingest_piece_min": 0}, {"strings_fused": 0}, {"orfs_exact_path": 1}, {"orfs_exact_path": 2}):
        assert want in [opts for opts, _ in groups], want


def test_the_same_entry_rows_are_the_ones_the_contract_names():
    by_name = {r.name: r for r in sc.ROWS}
    assert all(n in by_name for n in tc.SAME_ENTRY) and len(set(tc.SAME_ENTRY)) == len(tc.SAME_ENTRY)
    entries = {by_name[n].entry for n in tc.SAME_ENTRY}
    assert entries == {"gmg_mg_score_reads", "gmg_mg_score_groups", "gmg_find_orfs", "gmg_fasta_ingest_on", "gmg_score_orfs",
                       "gmg_features_count", "gmg_tophits_scores"}
    assert sum(by_name[n].entry == "gmg_mg_score_reads" for n in tc.SAME_ENTRY) == 4          # plain, -i, -s, per-read nulls
    assert sorted(by_name[n].options["orfs_exact_path"] for n in tc.SAME_ENTRY if by_name[n].entry == "gmg_score_orfs") == [0, 1, 2]
    assert [by_name[n].options.get("ingest_piece_min") for n in tc.SAME_ENTRY if by_name[n].entry == "gmg_fasta_ingest_on"] == [None, 0]
    assert 1 < tc.N_THREADS <= tc.MAX_THREADS == 8


def test_run_threads_turns_a_thread_that_never_ends_into_a_failure():
    """a thread that waits for something that never comes is reported after the time limit (here 0.3 s), not waited for; an
    exception in one thread releases the others from the barrier and is raised in the caller"""
    import threading
    import time

    import pytest

    never = threading.Event()
    t0 = time.monotonic()
    with pytest.raises(tc.Stuck, match="gmg-test-1"):
        tc.run_threads(2, lambda t, barrier: never.wait() if t == 1 else None, timeout=0.3)
    assert time.monotonic() - t0 < 5.0
    never.set()

    def body(t, barrier):
        if t == 0:
            raise ValueError("thread 0 says no")
        barrier.wait()                                                # (broken by thread 0: comes back at once)

    t0 = time.monotonic()
    with pytest.raises(ValueError, match="thread 0 says no"):
        tc.run_threads(3, body, timeout=30.0)
    assert time.monotonic() - t0 < 5.0
    with pytest.raises(tc.Stuck, match="barrier"):                    # a barrier that not all reach: told as such
        tc.run_threads(2, lambda t, barrier: barrier.wait() if t == 0 else None, timeout=0.3)
    seen = []
    tc.run_threads(4, lambda t, barrier: (barrier.wait(), seen.append(t)))
    assert sorted(seen) == [0, 1, 2, 3]
