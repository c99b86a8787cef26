"""integration/window-acgt_gpu, integration/uncovered_gpu and integration/entropy-fasta_gpu against every output recorded from the
reference's programs (tests/golden/windows/): stdout, stderr and the exit status byte for byte; uncovered_gpu --multi against the
single runs with the tag counter carried over; every refusal."""
import os
import re
import subprocess

import pytest

import audit_oracle as ao
import windows_oracle as wo
from conftest import GOLD, built_binary
from test_windows_host import CASES, REFUSED, WIN, run_restatement, same_as_recorded

pytestmark = pytest.mark.gpu

EXE = {"window-acgt": "window-acgt_gpu", "uncovered": "uncovered_gpu", "entropy-fasta": "entropy-fasta_gpu"}


def _run(program, args, stdin=None):
    exe = built_binary("integration", "_build", EXE[program])
    res = subprocess.run([exe] + [str(a) for a in args], stdin=open(stdin, "rb") if stdin else subprocess.DEVNULL, stdout=subprocess.PIPE,
                         stderr=subprocess.PIPE, timeout=120)
    return res.returncode, res.stdout, res.stderr


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_commands_reproduce_the_recorded_outputs(gpu, case):
    args = list(case["args"])
    if "fasta" in case:
        args += [os.path.join(GOLD, case["fasta"]), os.path.join(GOLD, case["coords"])]
    rc, out, err = _run(case["program"], args, os.path.join(GOLD, case["stdin"]) if "stdin" in case else None)
    assert rc == case["status"], err.decode()[-500:]
    if case["stderr"] is None:
        assert b"USAGE:" in err and out == b""         # (getopt's own line about the option may stand in front of it)
    if case["stdout_bytes"] < (1 << 20):
        assert out.decode("latin-1") == run_restatement(case)[0]     # (the restatement's text has the recorded digest: a readable difference first)
    same_as_recorded(case, out, err)


def test_entropy_fasta_keeps_the_records_in_front_of_the_bad_one_on_a_file_too(gpu, tmp_path):
    """the recorded run had its stdout on a file and on a pipe: both keep the two records in front of the 10-base one"""
    exe = built_binary("integration", "_build", EXE["entropy-fasta"])
    case = next(c for c in CASES if c["name"] == "ef.bad")
    with open(tmp_path / "out", "wb") as fo:
        res = subprocess.run([exe], stdin=open(os.path.join(WIN, "ef_bad.fna"), "rb"), stdout=fo, stderr=subprocess.PIPE, timeout=120)
    assert res.returncode == 1 and res.stderr.decode() == case["stderr"]
    assert open(tmp_path / "out").read() == case["stdout"]


@pytest.mark.parametrize("opts", [[], ["-d"], ["-2", "-l", "4"], ["-s"], ["--nostop"], ["-w"]], ids=["plain", "d", "2l4", "s", "nostop", "w"])
def test_uncovered_multi_equals_the_single_runs_with_the_tags_carried_over(gpu, tmp_path, opts):
    fasta, coords = os.path.join(WIN, "multi3.fna"), os.path.join(WIN, "multi3.coords")
    rc, out, err = _run("uncovered", opts + ["--multi", fasta, coords])
    assert rc == 0, err.decode()
    want = run_restatement({"program": "uncovered", "args": opts + ["--multi"], "fasta": "windows/multi3.fna", "coords": "windows/multi3.coords"})
    assert want[2] == [] and (out.decode(), err.decode()) == want[:2]
    singles, carried = "", 0
    recs = ao.fasta_records(open(fasta).read())
    assert len(recs) == 3
    for tag, letters in recs:
        fa, co = tmp_path / (tag + ".fna"), tmp_path / (tag + ".coords")
        fa.write_text(">%s\n%s\n" % (tag, letters))
        co.write_text("".join(" ".join(f for k, f in enumerate(line.split()) if k != 1) + "\n" for line in open(coords) if line.split()[1] == tag))
        rc, o, e = _run("uncovered", opts + [fa, co])
        if not letters:
            assert rc == 0 and o == b""                  # an empty record: no gap
            continue
        assert rc == 0, e.decode()
        o = o.decode()
        singles += re.sub(r"seq(\d{5})", lambda m: "seq%05d" % (int(m.group(1)) + carried), o)
        carried += len(re.findall(r"seq\d{5}", o))
    assert out.decode() == singles and carried > 2       # (two records have letters: the counter ran on)


def _refused(program, args, stdin=None):
    rc, out, err = _run(program, args, stdin)
    assert rc == 1 and out == b"" and err.count(b"\n") == 1 and err.startswith(b"ERROR:  "), (args, rc, out[:200], err[:500])
    return err.decode()


def test_window_acgt_refusals(gpu, tmp_path):
    for k, (text, why) in enumerate([("acgt\n>s\nacgt\n", "in front of the first header"), (">s\nac>gt\n", "'>' inside"),
                                     (">s\n" + "a" * 299 + "\n", "299 characters"), (">s\nac\0gt\n", "NUL")]):
        fa = tmp_path / ("bad%d.fna" % k)
        fa.write_bytes(text.encode())
        assert wo.window_acgt(text, 2, 1)[2] != []
        assert why in _refused("window-acgt", ["2", "1"], fa)
    fa = tmp_path / "ok.fna"
    fa.write_text(">s\n" + "a" * 298 + "\n")
    rc, out, err = _run("window-acgt", ["100", "100"], fa)
    assert rc == 0 and out.decode() == wo.window_acgt(fa.read_text(), 100, 100)[0]
    for args in (["0", "1"], ["3", "0"], ["--", "-5", "2"]):
        assert "Bad window" in _refused("window-acgt", args, fa)
    rc, out, err = _run("window-acgt", ["-5", "2"], fa)  # getopt takes -5 for an option: the usage, as the reference
    assert rc == 1 and out == b"" and b"USAGE:" in err
    rc, out, err = _run("window-acgt", ["5"], fa)        # too few arguments: the usage, status 1
    assert rc == 1 and out == b"" and err.startswith(b"USAGE:")
    rc, out, err = _run("window-acgt", ["3", "2"])       # an empty standard input prints nothing
    assert rc == 0 and out == b"" and err == b""


def test_uncovered_refusals(gpu, tmp_path):
    fasta = os.path.join(WIN, "circ40.fna")
    for k, (kw, line) in enumerate(REFUSED):
        co = tmp_path / ("refused%d.coords" % k)
        co.write_text("ok 5 14 +1\n" + line)
        opts = (["-d"] if kw.get("use_dir") else []) + (["-s"] if kw.get("skip_start") else []) + (["--nostop"] if kw.get("skip_stop") else []) + \
               ([] if kw.get("circular", True) else ["-w"])
        assert line.strip() in _refused("uncovered", opts + [fasta, co])
    co = tmp_path / "long.coords"
    co.write_text("x" * 298 + " 1 9\n")
    assert "299 characters" in _refused("uncovered", [fasta, co])
    co = tmp_path / "tag.coords"
    co.write_text("g m0 3 20 +1\ng nosuch 3 20 +1\n")
    assert "g nosuch 3 20 +1" in _refused("uncovered", ["--multi", os.path.join(WIN, "multi3.fna"), co])
    fa = tmp_path / "nul.fna"
    fa.write_bytes(b">s\nacgt\0acgt\n")
    co.write_text("g 1 3\n")
    assert "NUL" in _refused("uncovered", [fa, co])
    rc, out, err = _run("uncovered", ["-l", "3", fasta, "-"])           # the coordinates from an empty standard input: one gap, the sequence
    assert rc == 0 and out.decode() == wo.uncovered(ao.fasta_records(open(fasta).read()), "", 3)[0] and out.startswith(b">seq00001  1 40  len=40\n")


def test_entropy_fasta_refusals(gpu, tmp_path):
    fa = tmp_path / "nul.fna"
    fa.write_bytes(b">s\nacg\0tt\n")
    assert "NUL" in _refused("entropy-fasta", [], fa)
    fa.write_bytes(b">s\natgaaataa\n>  ")                # Fasta_Read drops the header the file ends in, and so does the device's parser
    rc, out, err = _run("entropy-fasta", [], fa)
    assert rc == 0 and out.decode() == wo.entropy_fasta(">s\natgaaataa\n")[0] and err == b""
