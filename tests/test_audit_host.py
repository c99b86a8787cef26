"""Host-side checks of the gene-coordinate audit (no device): the Python restatement of anomaly, start-codon-distrib and entropy-score
(tests/audit_oracle.py) reproduces every output recorded from the reference's programs (tests/golden/audit/, built outside this
repository) byte for byte, none of the recorded input lines is one at which the reference leaves its buffers, the inputs the
*_gpu commands refuse are flagged, and the C ABI validates its handles and refuses to run without a device."""
import ctypes as C
import hashlib
import json
import os

import pytest

import audit_oracle as ao
from conftest import GOLD

AUDIT = os.path.join(GOLD, "audit")
CASES = json.load(open(os.path.join(AUDIT, "cases.json")))


def coords_of(case):
    """the coordinate file of a recorded case: a file under tests/golden, or the 300 moved genes of the genome's predict file"""
    if case["coords"] == "generated:nc300_moved":
        return ao.moved_genes(open(os.path.join(GOLD, "predict", "NC_000915.run1.predict")).read())
    return open(os.path.join(GOLD, case["coords"])).read()


def same_as_recorded(case, out, err):
    """stdout against the recorded digest and length (and the text, where the case keeps it), stderr against the recorded text"""
    assert err == case["stderr"].encode()
    assert len(out) == case["stdout_bytes"] and hashlib.sha256(out).hexdigest() == case["stdout_sha256"]
    assert case["stdout"] is None or out == case["stdout"].encode()


def run_restatement(case, fasta_text=None, coords_text=None, extra=()):
    args = list(case["args"]) + list(extra)
    recs = ao.fasta_records(fasta_text if fasta_text is not None else open(os.path.join(GOLD, case["fasta"])).read())
    text = coords_text if coords_text is not None else coords_of(case)
    multi = "--multi" in args
    if case["program"] == "anomaly":
        kw = dict(check_start="-s" not in args, use_dir="-d" in args, circular="-w" not in args, multi=multi)
        if "-A" in args:
            kw["starts"] = tuple(args[args.index("-A") + 1].split(","))
        if "-Z" in args:
            kw["stops"] = tuple(args[args.index("-Z") + 1].split(","))
        return ao.anomaly(recs, text, **kw)
    if case["program"] == "entropy-score":
        kw = dict(use_dir="-d" in args, circular="-w" not in args, skip_start="-s" in args or "--nostart" in args, skip_stop="--nostop" in args,
                  multi=multi)
        for opt in ("-l", "--minlen"):
            if opt in args:
                kw["min_len"] = int(args[args.index(opt) + 1])
        return ao.entropy_score(recs, text, **kw)
    return ao.start_codon_distrib(recs, text, use_dir="-d" in args, circular="-w" not in args, comma3="-3" in args, multi=multi)


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_restatement_reproduces_the_recorded_outputs(case):
    out, err, flagged = run_restatement(case)
    assert case["status"] == 0
    assert flagged == []                                 # the cap: 0 flagged lines, so no refusal can hide a mismatch
    same_as_recorded(case, out.encode(), err.encode())


def test_recorded_genome_runs_say_what_the_issue_says():
    """the short outputs as recorded; the long ones through the restatement, whose text has the recorded digest (the test above)"""
    case = {c["name"]: c for c in CASES}
    assert case["nc.anomaly"]["stderr"] == "     OK orfs =    1549\nProblem orfs =       0\n"
    assert case["nc.anomaly"]["stdout"].startswith("Bad line:  >gi|")
    assert case["nc.scd"]["stdout"] == " atg     1202   77.6%\n ttg      186   12.0%\n gtg      161   10.4%\nTotal:   1549\n"
    assert case["nc.scd.3"]["stdout"] == "0.776,0.104,0.120\n"
    rows = run_restatement(case["nc.es"])[0].splitlines()
    # the long-orfs file's own last column again -- but for the six genes that hold a letter outside acgt: long-orfs scores the
    # filtered sequence, entropy-score the raw letters, where such a codon counts nowhere
    assert len(rows) == 1161 and sum(r.split()[-1] != r.split()[-2] for r in rows) == 6
    moved = run_restatement(case["nc300.anomaly"])[0]
    assert hashlib.sha256(moved.encode()).hexdigest() == case["nc300.anomaly"]["stdout_sha256"]
    for kind in ("has bad start codon", "has bad stop codon", "next stop occurs at offset", "frame shift", "Best prefix is",
                 "Best suffix is", "No stop found in start frame", "has stop codon"):
        assert kind in moved


REFUSED = {                                              # coordinate lines on the 180-base tiny genome -> the flag
    "anomaly": [("g 10 11 +1\n", "gene length"), ("g 0 11 +1\n", "off the sequence"), ("g 355 365 +1\n", "off the sequence"),
                ("g 400 10 +1\n", "gene length")],
    "start-codon-distrib": [("g 178 10\n", "last base"), ("g 180 10\n", "last base"), ("g 2 170\n", "last base"),
                            ("g 600 10\n", "off the sequence"), ("g -300 10\n", "off the sequence")],
    "entropy-score": [("g 600 610\n", "off the sequence"), ("g -300 -290\n", "off the sequence")],
}


@pytest.mark.parametrize("program", sorted(REFUSED))
def test_inputs_the_commands_refuse_are_flagged(program):
    fasta = open(os.path.join(AUDIT, "tiny.fna")).read()
    case = {"program": program, "args": []}
    for line, why in REFUSED[program]:
        _, _, flagged = run_restatement(case, fasta, "ok 20 49\n" + line)
        assert flagged == [(1, why)], line
    _, _, flagged = run_restatement(case, fasta, "x" * 298 + " 1 9\n")
    assert flagged == [(0, "line too long")]


def test_a_gene_without_a_later_stop_is_flagged():
    """what the reference answers with assert (j < Len): recorded once, status -6 and no output, with tiny.coords under -Z tga"""
    fasta = open(os.path.join(AUDIT, "tiny.fna")).read()
    coords = open(os.path.join(AUDIT, "tiny.coords")).read()
    _, _, flagged = run_restatement({"program": "anomaly", "args": ["-s", "-Z", "tga"]}, fasta, coords)
    assert flagged and {why for _, why in flagged} == {"no later stop"}
    _, _, flagged = run_restatement({"program": "anomaly", "args": []}, ">s\nacccccccccccccccccccta\n", "g 3 8 +1\n")
    assert flagged == []                                 # found through the wrap: t a + base 1
    _, _, flagged = run_restatement({"program": "anomaly", "args": []}, ">s\nacccccccccccccccccccta\n", "g 25 30 +1\n")
    assert flagged == [(0, "walk off the sequence")]     # Start + i + j > 2 Len before a stop turns up


def test_record_restatement_on_a_worked_example():
    rec = ao.audit_region("atgccctaatgaccctag", 0, 12, 1, ("atg",), ("taa", "tga"))
    assert rec["first_codon"] == 14 and rec["stop_which"] == 1 and rec["inner"] == [6] and rec["last_back_stop"] == 6 and rec["next_stop"] == -1
    rec = ao.audit_region("atgccctaatgaccctag", 17, 6, -1, ("cta",), ("tag",))
    assert rec["start_which"] == 0 and rec["last_codon"] == ao.codon_code("ggg") and rec["next_stop"] == -1


def test_handles_are_validated_and_nothing_runs_without_a_device(gmg):
    lib = gmg.capi.lib()
    n = C.c_uint64()
    assert lib.gmg_audit_info(None, C.byref(n), None) == -1 and b"gmg_audit_info" in lib.gmg_last_error()
    assert lib.gmg_audit_fetch(None, None, None, None) == -1 and b"gmg_audit_fetch" in lib.gmg_last_error()
    assert lib.gmg_audit_free(None) == 0
    assert C.sizeof(gmg.capi.AuditParams) == 80 and gmg.GENE_AUDIT_DTYPE.itemsize == 32
    if lib.gmg_device_count() > 0:
        return
    prm = gmg.audit_params()
    h = C.c_void_p()
    assert lib.gmg_genes_audit(None, None, 0, C.byref(prm), None, 0, C.byref(h), None) == -2          # GMG_ENODEV before anything else
    assert b"gmg_genes_audit" in lib.gmg_last_error()
