"""Host-side checks of the window composition / uncovered regions work (no device): the Python restatement of window-acgt, uncovered
and entropy-fasta (tests/windows_oracle.py) reproduces every output recorded from the reference's programs (tests/golden/windows/,
built outside this repository) byte for byte, none of the recorded input lines is one at which the reference leaves its buffers, the
closed form of the windows equals the ring buffer, gmg_uncovered_plan equals the restatement's intervals, the inputs the *_gpu
commands refuse are flagged, and the C ABI validates its handles and refuses to run without a device."""
import ctypes as C
import hashlib
import json
import os

import numpy as np
import pytest

import audit_oracle as ao
import windows_oracle as wo
from conftest import GOLD

WIN = os.path.join(GOLD, "windows")
CASES = json.load(open(os.path.join(WIN, "cases.json")))


def text_of(rel):
    return open(os.path.join(GOLD, rel), newline="").read()


def same_as_recorded(case, out, err):
    """stdout against the recorded digest and length (and the text, where the case keeps it), stderr against the recorded text; the
    usage text (stderr recorded as null) is each program's own"""
    if case["stderr"] is not None:
        assert err == case["stderr"].encode()
    assert len(out) == case["stdout_bytes"] and hashlib.sha256(out).hexdigest() == case["stdout_sha256"]
    assert case["stdout"] is None or out == case["stdout"].encode()


def uncovered_options(args):
    """the reference's getopt string "2dhl:sw" and its long options, --multi of uncovered_gpu; None: a usage error"""
    kw, min_len, fasta_format, multi = {}, 0, True, False
    args = list(args)
    while args:
        a = args.pop(0)
        if a == "-2":
            fasta_format = False
        elif a in ("-d", "--dir"):
            kw["use_dir"] = True
        elif a in ("-l", "--minlen"):
            min_len = int(args.pop(0))
        elif a in ("-s", "--nostart"):
            kw["skip_start"] = True
        elif a == "--nostop":
            kw["skip_stop"] = True
        elif a in ("-w", "--nowrap"):
            kw["circular"] = False
        elif a == "--multi":
            multi = True
        else:
            return None
    return kw, min_len, fasta_format, multi


def run_restatement(case, coords_text=None, extra=()):
    """-> (stdout, stderr, flagged, status)"""
    args = list(case["args"]) + list(extra)
    if case["program"] == "window-acgt":
        percents = "-p" in args
        W, S = [int(a) for a in args if a != "-p"]
        return wo.window_acgt(text_of(case["stdin"]), W, S, percents) + (0,)
    if case["program"] == "entropy-fasta":
        return wo.entropy_fasta(text_of(case["stdin"]))
    opts = uncovered_options(args)
    if opts is None or "fasta" not in case:
        return "", None, [], 1
    kw, min_len, fasta_format, multi = opts
    recs = ao.fasta_records(text_of(case["fasta"]))
    return wo.uncovered(recs, coords_text if coords_text is not None else text_of(case["coords"]), min_len, fasta_format, multi, **kw) + (0,)


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_restatement_reproduces_the_recorded_outputs(case):
    out, err, flagged, status = run_restatement(case)
    assert flagged == []                                 # the cap: 0 flagged lines, so no refusal can hide a mismatch
    assert status == case["status"]
    same_as_recorded(case, out.encode("latin-1"), None if err is None else err.encode("latin-1"))


def test_recorded_runs_say_what_the_issue_says():
    case = {c["name"]: c for c in CASES}
    # (W, S) = (10, 2) on 15 bases: 1, 3, 5, then 7 of length 9; (4, 7): 1, 8, then 15 of length 1
    rows = [r.split()[:2] for r in case["hand.w10.s2"]["stdout"].split(">len15")[1].split(">")[0].splitlines()[2:]] if case["hand.w10.s2"]["stdout"] else None
    assert rows is None or rows == [["1", "10"], ["3", "10"], ["5", "10"], ["7", "9"]]
    out = wo.window_acgt(text_of("windows/hand.fna"), 4, 7)[0]
    rows = [r.split()[:2] for r in out.split(">len15")[1].split(">")[0].splitlines()[2:]]
    assert rows == [["1", "4"], ["8", "4"], ["15", "1"]]
    assert [(p, n) for p, n, _ in wo.window_rows("a" * 13, 4, 7)] == [(1, 4), (8, 4)]
    # an empty record still prints its two heading lines
    assert ">len0  a record of 0 bases\nPosition  Length     As     Cs     Gs     Ts  Other    %GC\n>len1 " in out
    # entropy-fasta's exit keeps the stdout of the records in front of the bad one: exit () flushes cout, to a file and to a pipe
    bad = case["ef.bad"]
    assert bad["status"] == 1 and bad["stderr"] == "odd  ten bases not divisible by 3\n" and bad["stdout"].count(">gene") == 2
    assert case["ef.hand"]["stdout"].startswith(bad["stdout"])
    # -t is no option of uncovered (its getopt string lacks it): status 1; --nostop works
    assert case["circ40.t"]["status"] == 1 and case["circ40.nostop"]["status"] == 0
    # an empty interval inside a gap splits it: bases 26 .. 28 come out as 26 and 27 .. 28 once empty_gap is among the lines
    assert ">seq00003  26 28  len=3\n" in case["circ40.d"]["stdout"]
    assert ">seq00003  26 26  len=1\n" in case["circ40e.d"]["stdout"] and ">seq00004  27 28  len=2\n" in case["circ40e.d"]["stdout"]


def test_closed_form_of_the_windows_equals_the_ring_buffer():
    for L in range(0, 81):
        seq = "a" * L
        for W in range(1, 41):
            for S in range(1, 46):
                assert [(p, n) for p, n, _ in wo.window_rows(seq, W, S)] == wo.closed_form_windows(L, W, S), (L, W, S)


UNCOVERED_CASES = [c for c in CASES if c["program"] == "uncovered" and c["status"] == 0]


def coord_rows(text, use_dir, tags=None):
    """the lines that parse, as gmg_coord rows (read, start, end, dir)"""
    rows = []
    for line in text.splitlines(True):
        f = ao.scan_fields(line, 3 if use_dir else 2, 2 if tags is not None else 1)
        if f is not None:
            rows.append((tags.index(f[0][1]) if tags is not None else 0, f[1][0], f[1][1], f[1][2] if use_dir else 0))
    return rows


def plan_flags(gmg, kw):
    return ((gmg.COORD_USE_DIR if kw.get("use_dir") else 0) | (0 if kw.get("circular", True) else gmg.COORD_NOWRAP) |
            (gmg.COORD_SKIP_START if kw.get("skip_start") else 0) | (gmg.COORD_SKIP_STOP if kw.get("skip_stop") else 0))


@pytest.mark.parametrize("case", UNCOVERED_CASES, ids=[c["name"] for c in UNCOVERED_CASES])
def test_planner_equals_the_restatement_on_the_recorded_files(gmg, case):
    kw = uncovered_options(case["args"])[0]
    L = len(ao.fasta_records(text_of(case["fasta"]))[0][1])
    text = text_of(case["coords"])
    want, _, flagged = wo.coord_intervals([L], text, **kw)
    assert flagged == [] and want
    got = gmg.uncovered_plan([0, L], coord_rows(text, kw.get("use_dir", False)), plan_flags(gmg, kw))
    assert got == want


def test_planner_on_several_records(gmg):
    recs = ao.fasta_records(text_of("windows/multi3.fna"))
    tags, lengths = [t for t, _ in recs], [len(s) for _, s in recs]
    text = text_of("windows/multi3.coords")
    for kw in ({}, dict(use_dir=True), dict(skip_start=True), dict(skip_stop=True), dict(circular=False)):
        want, _, flagged = wo.coord_intervals(lengths, text, tags=tags, **kw)
        assert flagged == [] and len(want) >= 16
        got = gmg.uncovered_plan(np.cumsum([0] + lengths), coord_rows(text, kw.get("use_dir", False), tags), plan_flags(gmg, kw))
        assert got == want


REFUSED = [                                              # (options, coordinate line on the 40-base genome)
    (dict(skip_start=True, skip_stop=True), "wrap4 39 2 +1\n"),      # the reference's own arithmetic: lo = 41, hi = 39
    ({}, "far 50 60 +1\n"), ({}, "neg -5 3 +1\n"), (dict(use_dir=True), "back 50 45 -1\n"), (dict(skip_start=True), "tiny 11 12 +1\n"),
    (dict(circular=False), "past 45 50 +1\n"),
]


@pytest.mark.parametrize("kw,line", REFUSED, ids=[l.split()[0] for _, l in REFUSED])
def test_lines_off_the_sequence_are_flagged_and_refused_by_the_planner(gmg, kw, line):
    text = "ok 5 14 +1\n" + line
    made, _, flagged = wo.coord_intervals([40], text, **kw)
    assert flagged == [(1, "off the sequence")]
    if line.startswith("wrap4"):
        # i = 38 + 3, extract_len = 4 - 6: j = 39
        assert wo.coord_intervals([40], "ok 5 14 +1\n", **kw)[0] == made
    with pytest.raises(gmg.GmgError) as e:
        gmg.uncovered_plan([0, 40], coord_rows(text, kw.get("use_dir", False)), plan_flags(gmg, kw))
    assert e.value.code == -6 and "line 1 " in str(e.value)          # GMG_ERANGE naming the line
    with pytest.raises(gmg.GmgError) as e:
        gmg.uncovered_plan([0, 40], [(1, 5, 8, 1)])
    assert e.value.code == -6


def test_inputs_the_commands_refuse_are_flagged():
    assert wo.window_acgt("acgt\n>s\nacgt\n", 2, 1)[2] == [(0, "sequence before the first header")]
    assert wo.window_acgt(">s\nac>gt\n", 2, 1)[2] == [(1, "'>' inside a sequence line")]
    assert wo.window_acgt(">s\n" + "a" * 299 + "\n", 2, 1)[2] == [(1, "line too long")]
    assert wo.window_acgt(">s\n" + "a" * 298 + "\n", 2, 1)[2] == []
    assert wo.window_acgt(">s\nac\0gt\n", 2, 1)[2] == [(1, "NUL byte")]
    assert wo.uncovered([("s", "a" * 40)], "x" * 298 + " 1 9\n")[2] == [(0, "line too long")]
    assert wo.uncovered([("s", "a" * 40), ("t", "c" * 9)], "g u 1 9\n", multi=True)[2] == [(0, "unknown sequence")]
    assert wo.entropy_fasta(">s\nacg\0tt\n")[2] == [(0, "NUL byte")]


def test_handles_are_validated_and_nothing_runs_without_a_device(gmg):
    lib = gmg.capi.lib()
    n = C.c_uint64()
    for name, args in (("gmg_windows_info", (None, C.byref(n), None)), ("gmg_windows_fetch", (None, None, None)),
                       ("gmg_windows_device", (None, None, None)), ("gmg_gaps_info", (None, C.byref(n))), ("gmg_gaps_fetch", (None, None, None))):
        assert getattr(lib, name)(*args) == -1 and name.encode() in lib.gmg_last_error()
    assert lib.gmg_windows_free(None) == 0 and lib.gmg_gaps_free(None) == 0
    assert lib.gmg_uncovered_plan(None, 0, None, 0, 0, None, None) == -1
    off = np.array([0, 40], np.uint64)
    assert lib.gmg_uncovered_plan(off.ctypes.data_as(C.c_void_p), 1, None, 0, 32, None, C.byref(n)) == -1      # an unknown flag
    if lib.gmg_device_count() > 0:
        return
    h = C.c_void_p()
    assert lib.gmg_window_counts(None, 10, 2, None, 0, C.byref(h), None) == -2           # GMG_ENODEV before anything else
    assert b"gmg_window_counts" in lib.gmg_last_error()
    assert lib.gmg_regions_uncovered(None, None, 0, 0, C.byref(h), None) == -2
    assert b"gmg_regions_uncovered" in lib.gmg_last_error()
