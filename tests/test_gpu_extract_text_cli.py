"""integration/extract_gpu and integration/multi-extract_gpu against the reference's own outputs: the training set of its sample
run (by digest), every recording of tests/golden/extract (the text, or per-record digests), the -2 format, unparsable lines,
coordinates from standard input and the lines the plan refuses."""
import hashlib
import os
import subprocess

import pytest

import extract_oracle as xo
import text_oracle as to
from conftest import DATA, built_binary
from test_text_host import EX, IDS, NC, RECORDED, SEQS, SLICE

pytestmark = pytest.mark.gpu

EXE = {"extract": "extract_gpu", "multi-extract": "multi-extract_gpu"}
# sha256 of sample-run/glimmer3/results/NC_000915.train of the reference: `extract -t NC_000915.fna NC_000915.longorfs`
TRAIN_DIGEST = open(os.path.join(EX, "NC_000915.train.sha256")).read().split()[0]


def run(program, args, stdin=None):
    exe = built_binary("integration", "_build", EXE[program])
    res = subprocess.run([exe] + [str(a) for a in args], stdin=stdin or subprocess.DEVNULL, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                         timeout=120)
    return res.returncode, res.stdout, res.stderr


def ex(name):
    return os.path.join(EX, name)


def test_training_set_of_the_sample_run(gpu):
    rc, out, err = run("extract", ["-t", NC, os.path.join(DATA, "NC_000915.longorfs")])
    assert rc == 0 and err == b""
    assert len(out) == 1307331 and out.count(b">") == 1161
    assert hashlib.sha256(out).hexdigest() == TRAIN_DIGEST == "cc2a8150bdee945b6484648b373d1c795116c181284274a6f5ec53361b56c511"
    assert to.body_lines_ok(out.decode())


@pytest.mark.parametrize("program,opts,seq_file,coords_file,recording", RECORDED[:3], ids=IDS[:3])
def test_recorded_texts(gpu, program, opts, seq_file, coords_file, recording):
    rc, out, err = run(program, opts + [seq_file, ex(coords_file)])
    assert rc == 0 and err == b""
    assert out == open(ex(recording), "rb").read()
    assert to.body_lines_ok(out.decode())


@pytest.mark.parametrize("program,opts,seq_file,coords_file,recording", RECORDED[3:], ids=IDS[3:])
def test_recorded_digests(gpu, program, opts, seq_file, coords_file, recording):
    rc, out, err = run(program, opts + [seq_file, ex(coords_file)])
    assert rc == 0 and err == b""
    text = out.decode()
    assert to.body_lines_ok(text)
    got = [(h, len(t), xo.sha(t)) for h, t in _records(text)]
    assert got == [(h, n, d) for h, n, d in xo.recorded(recording)] and len(got) >= 8


def _records(text):
    out = []
    for line in text.splitlines():
        if line.startswith(">"):
            out.append([line[1:].split(), ""])
        else:
            out[-1][1] += line
    return out


@pytest.mark.parametrize("program,opts,seq_file,coords_file,recording", [
    ("extract", ["-2"], SLICE, "slice_wrap.coords", "slice_wrap.2.out"),
    ("extract", ["-2", "-t"], SLICE, "slice_wrap.coords", "slice_wrap.2_t.out"),
    ("multi-extract", ["-2"], SEQS, "seqs_multi.coords", "seqs_multi.2.out"),
    ("multi-extract", ["-2", "-t"], SEQS, "seqs_multi.coords", "seqs_multi.2_t.out")], ids=["extract-2", "extract-2-t", "multi-2", "multi-2-t"])
def test_two_field_format(gpu, program, opts, seq_file, coords_file, recording):
    rc, out, err = run(program, opts + [seq_file, ex(coords_file)])
    assert rc == 0 and err == b""
    assert out == open(ex(recording), "rb").read()
    assert all(len(line.split(" ")[0]) > 0 for line in out.decode().splitlines())


def test_unparsable_lines_are_reported_and_skipped(gpu):
    rc, out, err = run("extract", [SLICE, ex("slice_bad.coords")])
    assert rc == 0
    assert err == open(ex("slice_bad.err"), "rb").read() and err.count(b"ERROR:  Skipped following coord line\n") == 4
    assert out == open(ex("slice_bad.out"), "rb").read() and out.count(b">") == 4


def test_coordinates_from_standard_input(gpu):
    for program, opts, seq_file, coords_file, recording in RECORDED[1:3]:
        with open(ex(coords_file), "rb") as fp:
            rc, out, err = run(program, opts + [seq_file, "-"], stdin=fp)
        assert rc == 0 and err == b"" and out == open(ex(recording), "rb").read()


def test_lines_the_plan_refuses(gpu, tmp_path):
    """more letters than the sequence holds (the reference laps the circle), a start one wrap does not bring onto the sequence:
    status 1, the plan's message and the line, nothing on stdout"""
    for k, (program, seq_file, line) in enumerate([("extract", SLICE, "far 4100 4150 1\n"), ("extract", SLICE, "lap 10 2100 1\n"),
                                                   ("multi-extract", SEQS, "g read0 1 100000 1\n")]):
        co = tmp_path / ("refused%d.coords" % k)
        co.write_text(("fine 10 90 1\n" if program == "extract" else "f read0 10 90 1\n") + line)
        rc, out, err = run(program, ["-d", seq_file, co])
        assert rc == 1 and out == b"" and err.startswith(b"ERROR:  gmg_extract_plan: line 1") and line.encode() in err, err


def test_usage(gpu):
    for program in EXE:
        rc, out, err = run(program, [SLICE])
        assert rc == 1 and out == b"" and err.startswith(b"USAGE:")
        rc, out, err = run(program, ["-x", SLICE, ex("slice_wrap.coords")])
        assert rc == 1 and out == b""
        rc, out, err = run(program, ["-h"])
        assert rc == 0 and out == b"" and err.startswith(b"USAGE:")
