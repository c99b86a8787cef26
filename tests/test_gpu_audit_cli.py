"""integration/anomaly_gpu, integration/start-codon-distrib_gpu and integration/entropy-score_gpu against every output recorded from the reference's programs
(tests/golden/audit/): stdout, stderr and the exit status byte for byte; --multi against the single runs; every refusal."""
import os
import subprocess

import pytest

import audit_oracle as ao
from conftest import GOLD, built_binary
from test_audit_host import AUDIT, CASES, REFUSED, coords_of, run_restatement, same_as_recorded

pytestmark = pytest.mark.gpu

EXE = {"anomaly": "anomaly_gpu", "start-codon-distrib": "start-codon-distrib_gpu", "entropy-score": "entropy-score_gpu"}


def _run(program, args):
    exe = built_binary("integration", "_build", EXE[program])
    res = subprocess.run([exe] + [str(a) for a in args], stdin=subprocess.DEVNULL, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                         timeout=120)
    return res.returncode, res.stdout, res.stderr


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_commands_reproduce_the_recorded_outputs(gpu, tmp_path, case):
    coords = tmp_path / "case.coords"
    coords.write_text(coords_of(case))
    rc, out, err = _run(case["program"], case["args"] + [os.path.join(GOLD, case["fasta"]), coords])
    assert rc == case["status"] == 0, err.decode()[-500:]
    assert out.decode() == run_restatement(case)[0]      # (the restatement's text has the recorded digest: a readable difference first)
    same_as_recorded(case, out, err)


@pytest.mark.parametrize("opts", [[], ["-d"], ["-A", "atg,gtg"]], ids=["plain", "d", "A"])
def test_anomaly_multi_equals_the_single_runs_in_line_order(gpu, tmp_path, opts):
    fasta, coords = os.path.join(AUDIT, "multi4.fna"), os.path.join(AUDIT, "multi4.coords")
    rc, out, err = _run("anomaly", opts + ["--multi", fasta, coords])
    assert rc == 0, err.decode()
    want = run_restatement({"program": "anomaly", "args": opts + ["--multi"]}, open(fasta).read(), open(coords).read())
    assert want[2] == [] and (out.decode(), err.decode()) == want[:2]
    singles, ok, problem = b"", 0, 0
    recs = ao.fasta_records(open(fasta).read())
    assert len(recs) == 4
    for tag, letters in recs:
        fa, co = tmp_path / (tag + ".fna"), tmp_path / (tag + ".coords")
        fa.write_text(">%s\n%s\n" % (tag, letters))
        co.write_text("".join(" ".join(f for k, f in enumerate(line.split()) if k != 1) + "\n"
                              for line in open(coords) if line.split()[1] == tag))
        rc, o, e = _run("anomaly", opts + [fa, co])
        assert rc == 0, e.decode()
        singles += o
        ok += int(e.decode().split("\n")[0].split("=")[1])
        problem += int(e.decode().split("\n")[1].split("=")[1])
    assert out == singles and len(out) > 1000
    assert err.decode() == "     OK orfs = %7d\nProblem orfs = %7d\n" % (ok, problem)


def test_start_codon_distrib_multi_counts_every_record(gpu, tmp_path):
    fasta, coords = os.path.join(AUDIT, "multi4.fna"), os.path.join(AUDIT, "multi4.coords")
    for opts in ([], ["-d"], ["-3", "-w"]):
        rc, out, err = _run("start-codon-distrib", opts + ["--multi", fasta, coords])
        assert rc == 0, err.decode()
        want = run_restatement({"program": "start-codon-distrib", "args": opts + ["--multi"]}, open(fasta).read(), open(coords).read())
        assert want[2] == [] and (out.decode(), err.decode()) == want[:2]
    n_lines = len(open(coords).readlines())
    rc, out, _ = _run("start-codon-distrib", ["--multi", fasta, coords])
    assert out.decode().endswith("Total: %6d\n" % n_lines)
    rc, out, err = _run("start-codon-distrib", ["-3", fasta, "-"])      # the coordinates from an empty standard input
    assert rc == 0 and out == b"0.000,0.000,0.000\n"


def test_entropy_score_multi_equals_the_single_runs_in_line_order(gpu, tmp_path):
    fasta, coords = os.path.join(AUDIT, "multi4.fna"), os.path.join(AUDIT, "multi4.coords")
    for opts in ([], ["-d", "--nostart", "--minlen", "12"]):
        rc, out, err = _run("entropy-score", opts + ["--multi", fasta, coords])
        assert rc == 0, err.decode()
        want = run_restatement({"program": "entropy-score", "args": opts + ["--multi"]}, open(fasta).read(), open(coords).read())
        assert want[2] == [] and "nan" not in want[0] and (out.decode(), err.decode()) == want[:2]
        singles = b""
        for tag, letters in ao.fasta_records(open(fasta).read()):
            fa, co = tmp_path / (tag + ".fna"), tmp_path / (tag + ".coords")
            fa.write_text(">%s\n%s\n" % (tag, letters))
            co.write_text("".join(line for line in open(coords) if line.split()[1] == tag))
            rc, o, e = _run("entropy-score", opts + ["--multi", fa, co])
            assert rc == 0, e.decode()
            singles += o
        assert out == singles and out.count(b"\n") > 40
    rc, out, err = _run("entropy-score", ["-2", fasta, coords])          # in the getopt string, rejected like any unknown option
    assert rc == 1 and out == b"" and err.startswith(b"USAGE:")
    rc, out, err = _run("entropy-score", ["-t", fasta, coords])          # no short -t: only --nostop
    assert rc == 1 and out == b""


def _refused(program, args):
    rc, out, err = _run(program, args)
    assert rc == 1 and out == b"" and err.count(b"\n") == 1 and err.startswith(b"ERROR:  "), (args, rc, out[:200], err[:500])
    return err.decode()


@pytest.mark.parametrize("program", sorted(REFUSED))
def test_refusals(gpu, tmp_path, program):
    fasta = os.path.join(AUDIT, "tiny.fna")
    for k, (line, _) in enumerate(REFUSED[program]):
        co = tmp_path / ("refused%d.coords" % k)
        co.write_text("ok 20 49\n" + line)
        assert line.strip() in _refused(program, [fasta, co])
    co = tmp_path / "long.coords"
    co.write_text("x" * 298 + " 1 9\n")
    assert "299 characters" in _refused(program, [fasta, co])
    co = tmp_path / "tag.coords"
    co.write_text("g rec0 3 20 +1\ng nosuch 3 20 +1\n")
    assert "g nosuch 3 20 +1" in _refused(program, ["--multi", os.path.join(AUDIT, "multi4.fna"), co])


def test_anomaly_refusals_of_its_own(gpu, tmp_path):
    fasta, coords = os.path.join(AUDIT, "tiny.fna"), os.path.join(AUDIT, "tiny.coords")
    assert "-t is refused" in _refused("anomaly", ["-t", fasta, coords])
    assert "there is none behind it" in _refused("anomaly", ["-s", "-Z", "tga", fasta, coords])         # the reference aborts here
    fa, co = tmp_path / "s.fna", tmp_path / "s.coords"
    fa.write_text(">s\nacccccccccccccccccccta\n")
    co.write_text("g 25 30 +1\n")
    assert "passes the end of the sequence twice" in _refused("anomaly", [fa, co])
    co.write_text("g 3 8 +1\n")
    rc, out, err = _run("anomaly", [fa, co])
    assert rc == 0 and b"next stop occurs at offset 18  Gene_Len = 6  diff = +15" in out
    for bad in (["-A", "atg,at"], ["-Z", "tan"], ["-A", ",".join(["atg"] * 9)]):
        assert "cod" in _refused("anomaly", bad + [fasta, coords])
