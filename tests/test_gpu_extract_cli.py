"""integration/build-icm_gpu: `extract <opts> seq coords | build-icm <opts> out.icm` in one process.  The yardstick is the
reference's build-icm (oracle/_ref) on RECORDED output of the reference's extract / multi-extract (tests/golden/extract)."""
import os
import subprocess

import pytest

import extract_oracle as xo
from conftest import built_binary, DATA

pytestmark = pytest.mark.gpu

NC = os.path.join(DATA, "NC_000915.fna")
SEQS = os.path.join(DATA, "seqs.fa")
SLICE = os.path.join(xo.EX, "slice2000.fna")


def ex(name):
    return os.path.join(xo.EX, name)


def reference(recorded, opts, out):
    ref = built_binary("oracle", "_ref", "build-icm")
    with open(recorded, "rb") as fp:
        subprocess.run([ref, *opts, str(out)], stdin=fp, check=True, timeout=300)
    return open(out, "rb").read()


def ours(args, **kw):
    exe = built_binary("integration", "_build", "build-icm_gpu")
    return subprocess.run([exe, *args], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300, **kw)


@pytest.mark.parametrize("opts", [["-r"], ["-r", "-t"], ["-r", "-w", "8", "-d", "4", "-p", "1"], ["-w", "8", "-d", "4", "-p", "1", "-t"]],
                         ids=["binary", "text", "shape-8-4-1", "shape-8-4-1-text-forward"])
def test_extract_equals_the_reference_pipe(opts, tmp_path):
    want = reference(ex("nc_subset.t.out"), opts, tmp_path / "ref.icm")
    res = ours([*opts, "--extract", "-t", NC, ex("nc_subset.coords"), str(tmp_path / "gpu.icm")])
    assert res.returncode == 0, res.stderr.decode()
    assert open(tmp_path / "gpu.icm", "rb").read() == want


def test_multi(tmp_path):
    want = reference(ex("seqs_multi.t.out"), ["-r"], tmp_path / "ref.icm")
    res = ours(["-r", "--extract", "--multi", "-t", SEQS, ex("seqs_multi.coords"), str(tmp_path / "gpu.icm")])
    assert res.returncode == 0, res.stderr.decode()
    assert open(tmp_path / "gpu.icm", "rb").read() == want


def test_list_of_three_jobs(tmp_path):
    jobs = [(["-t", NC, ex("nc_subset.coords")], "nc_subset.t.out"), ([SLICE, ex("slice_wrap.coords")], "slice_wrap.out"),
            (["--multi", "-t", SEQS, ex("seqs_multi.coords")], "seqs_multi.t.out")]
    with open(tmp_path / "jobs.txt", "w") as fp:
        fp.write("# one job per line\n\n")
        for k, (args, _) in enumerate(jobs):
            fp.write(" ".join(args + [str(tmp_path / ("list%d.icm" % k))]) + "\n")
    res = ours(["-r", "-w", "9", "-d", "5", "--list", str(tmp_path / "jobs.txt")])
    assert res.returncode == 0, res.stderr.decode()
    for k, (args, recorded) in enumerate(jobs):
        single = ours(["-r", "-w", "9", "-d", "5", "--extract", *args, str(tmp_path / ("single%d.icm" % k))])
        assert single.returncode == 0, single.stderr.decode()
        got = open(tmp_path / ("list%d.icm" % k), "rb").read()
        assert got == open(tmp_path / ("single%d.icm" % k), "rb").read()
        assert got == reference(ex(recorded), ["-r", "-w", "9", "-d", "5"], tmp_path / "ref.icm")


def test_no_stops_option_is_refused(tmp_path):
    res = ours(["-F", "--extract", "-t", NC, ex("nc_subset.coords"), str(tmp_path / "x.icm")])
    assert res.returncode == 2 and b"-F" in res.stderr
    assert not os.path.exists(tmp_path / "x.icm")


def test_unparsable_line_is_reported_and_skipped(tmp_path):
    lines = open(ex("slice_wrap.coords")).read().splitlines()
    coords = tmp_path / "coords.txt"
    coords.write_text("\n".join(lines[:3] + ["w_bad twelve 40", "lonely"] + lines[3:]) + "\n")
    res = ours(["-r", "--extract", SLICE, str(coords), str(tmp_path / "gpu.icm")])
    assert res.returncode == 0, res.stderr.decode()
    assert res.stderr.count(b"ERROR:  Skipped following coord line\n") == 2 and b"w_bad twelve 40\n" in res.stderr
    assert open(tmp_path / "gpu.icm", "rb").read() == reference(ex("slice_wrap.out"), ["-r"], tmp_path / "ref.icm")


def test_coordinate_beyond_the_sequence(tmp_path):
    coords = tmp_path / "coords.txt"
    coords.write_text("fine 10 90\nfar 4100 4150\n")
    res = ours(["--extract", SLICE, str(coords), str(tmp_path / "gpu.icm")])
    assert res.returncode == 1 and b"far 4100 4150" in res.stderr and b"line 1" in res.stderr


def test_without_extract_it_is_build_icm(tmp_path):
    want = reference(ex("slice_wrap.out"), ["-r", "-w", "7", "-d", "3"], tmp_path / "ref.icm")
    with open(ex("slice_wrap.out"), "rb") as fp:
        res = ours(["-r", "-w", "7", "-d", "3", str(tmp_path / "gpu.icm")], stdin=fp)
    assert res.returncode == 0, res.stderr.decode()
    assert open(tmp_path / "gpu.icm", "rb").read() == want
