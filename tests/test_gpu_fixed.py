"""Fixed-length ICMs on the device: gmg_fixed_score against the numpy oracle (tests/fixed_oracle.py) bit for bit, the refusals,
training byte-identical to the reference's build-fixed, and the drop-in programs (build-fixed_dropin, score-fixed_dropin,
score-fixed_gpu) byte-identical to the reference's output (tests/golden/fixed)."""
import hashlib
import json
import os
import subprocess

import numpy as np
import pytest

import fixed_oracle as fo
from conftest import GOLD, ROOT, built_binary

pytestmark = pytest.mark.gpu

FIX = os.path.join(GOLD, "fixed")
CASES = json.load(open(os.path.join(FIX, "cases.json")))
MODELS = {m["name"]: m for m in CASES["models"]}
NC_ICM = os.path.join(GOLD, "data", "NC_000915.icm")
COMP = np.array([3, 2, 1, 0], np.uint8)


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    """the FASTA inputs of the goldens, rebuilt (tests/test_fixed_host.py checks their sha256)"""
    return fo.make_inputs(os.path.join(GOLD, "data", "NC_000915.fna"), str(tmp_path_factory.mktemp("fixed_inputs")))


@pytest.fixture(scope="module")
def genome():
    return b"".join(line.strip() for line in open(os.path.join(GOLD, "data", "NC_000915.fna"), "rb") if not line.startswith(b">"))


def _windows(genome, L, n, seed):
    rng = np.random.default_rng(seed)
    return [genome[s:s + L] for s in rng.integers(0, len(genome) - L, n)]


def _buffer(codes, lo, ln, orient):
    b = codes[lo:lo + ln]
    if orient in (1, 3):
        b = b[::-1]
    if orient in (2, 3):
        b = COMP[b]
    return b


def _model_pair(gpu, oracle, genome, L, depth, perm, seed):
    """the same model trained by the library (device counting) and by the oracle"""
    train = _windows(genome, L, 600, seed)
    mine = gpu.FixedIcm.train(train, depth, -1, perm)
    subs = fo.train(oracle, train, L, depth, perm)
    return mine, subs, (perm if perm is not None else list(range(L)))


SHAPES = [(1, 0, "none"), (2, 1, "rev"), (3, 2, "rand"), (5, 7, "rand"), (7, 3, "none"), (12, 5, "rand"), (16, 7, "rev"),
          (24, 5, "none"), (24, 7, "rand"), (31, 4, "rand"), (32, 7, "rev"), (32, 6, "rand")]


@pytest.mark.parametrize("L,depth,kind", SHAPES)
def test_fixed_score_matches_oracle(gpu, oracle, genome, L, depth, kind):
    rng = np.random.default_rng(L * 100 + depth)
    perm = None if kind == "none" else list(range(L - 1, -1, -1)) if kind == "rev" else [int(x) for x in rng.permutation(L)]
    mine, subs, p = _model_pair(gpu, oracle, genome, L, depth, perm, L + depth)
    # ragged reads, windows at many offsets in all four orientations, segments longer than L
    lens = rng.integers(L, L + 90, 40)
    reads = [genome[s:s + int(n)] for s, n in zip(rng.integers(0, len(genome) - 200, 40), lens)]
    reads = [bytes(r.lower()) if k % 3 == 0 else r for k, r in enumerate(reads)]
    codes = [fo.codes([r])[0] for r in reads]
    rows = []
    for r, n in enumerate(lens):
        for lo in range(0, int(n) - L + 1, 3):
            ln = int(rng.integers(L, int(n) - lo + 1))
            rows.append((r, lo, ln, int(rng.integers(0, 4))))
    R = gpu.Reads.from_strings(reads)
    S = gpu.Segments(R, rows)
    win = np.stack([_buffer(codes[r], lo, ln, o)[:L] for r, lo, ln, o in rows])
    for lo, hi in [(0, L), (0, 0), (L // 2, L), (0, max(L // 3, 1)), (L - 1, L)]:
        got = gpu.fixed_score(mine, R, S, lo, hi)
        want = fo.score(subs, p, win, lo, hi)
        assert np.array_equal(got.view(np.uint64), want.view(np.uint64)), (lo, hi)
    # the batch entry point of the class and the one-window path (Score_Window) agree with it
    strings = [bytes(reads[r][lo:lo + ln]) for r, lo, ln, o in rows[:200] if o == 0]
    got = mine.score(strings)
    assert np.array_equal(got, fo.score(subs, p, fo.codes(strings)))


def test_fixed_score_grid_edges(gpu, oracle, genome):
    """N = 1 up to more than a million windows (partial work-groups, a grid that is not resident at once)"""
    mine, subs, p = _model_pair(gpu, oracle, genome, 24, 7, [int(x) for x in np.random.default_rng(5).permutation(24)], 77)
    n_max = 1_100_003
    R = gpu.Reads.from_strings([genome[:n_max + 23]])
    allwin = np.lib.stride_tricks.sliding_window_view(fo.codes([genome[:n_max + 23]])[0], 24)
    for n in (1, 63, 64, 65, 511, 512, 513, 70_001, n_max):
        rows = np.zeros((n, 4), np.uint32)
        rows[:, 1] = np.arange(n)
        rows[:, 2] = 24
        S = gpu.Segments(R, rows)
        want = fo.score(subs, p, allwin[:n])
        got = gpu.fixed_score(mine, R, S)
        assert np.array_equal(got.view(np.uint64), want.view(np.uint64)), n
        S.close()


def test_refusals(gpu, genome):
    mine = gpu.FixedIcm.train(_windows(genome, 12, 100, 3), 3)
    R = gpu.Reads.from_strings([genome[:100]])
    with pytest.raises(gpu.GmgError) as e:
        gpu.fixed_score(mine, R, gpu.Segments(R, [(0, 0, 12, 0), (0, 50, 11, 1)]))
    assert e.value.code == -6
    with pytest.raises(gpu.GmgError) as e:
        gpu.fixed_score(mine, R, gpu.Segments(R, [(0, 0, 12, 0)]), 5, 13)
    assert e.value.code == -1
    mip = np.full(1, -1, np.int16)
    prob = np.zeros((1, 4), np.float32)
    sub = [(mip, prob, 0), (np.full(5, -1, np.int16), np.zeros((5, 4), np.float32), 0)]
    for perm, subs in [([0, 0], sub), ([0, 2], sub), ([1, 0], [sub[0], (sub[1][0], sub[1][1], 2)]),
                       ([0] * 33, [sub[0]] * 33)]:
        with pytest.raises(gpu.GmgError) as e:
            gpu.FixedModel(perm, subs)
        assert e.value.code == -5
    m = gpu.FixedModel([1, 0], sub)
    assert m.info()[:2] == (2, 0)


@pytest.mark.parametrize("name", [m["name"] for m in CASES["models"]])
def test_train_byte_identical(gpu, inputs, name, tmp_path):
    m = MODELS[name]
    f = gpu.FixedIcm.train(fo.read_fasta_strings(inputs[m["train"]]), m["depth"], m["special"], m["perm"])
    out = tmp_path / "m.fix"
    f.write(str(out), binary=not m["text"])
    assert hashlib.sha256(out.read_bytes()).hexdigest() == m["sha256"]
    if not m["text"]:
        L = m["length"]
        assert f.params == (L, m["depth"], m["special"], 0, m["perm"] or list(range(L)))


def _run(argv, stdin_path):
    with open(stdin_path, "rb") as fp:
        r = subprocess.run(argv, stdin=fp, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    return r.returncode, r.stdout, r.stderr


@pytest.fixture(scope="module")
def fix_models(gpu, inputs, tmp_path_factory):
    """every golden model made by build-fixed_dropin (byte-identical to the reference's), by name"""
    exe = built_binary("integration", "_build", "build-fixed_dropin")
    d = tmp_path_factory.mktemp("fix")
    out = {}
    for m in CASES["models"]:
        argv = [exe, *m["opts"]] + (["-p", ",".join(map(str, m["perm"]))] if m["perm"] else [])
        rc, data, err = _run(argv, inputs[m["train"]])
        assert rc == 0, err
        assert hashlib.sha256(data).hexdigest() == m["sha256"], m["name"]
        out[m["name"]] = str(d / (m["name"] + ".fix"))
        open(out[m["name"]], "wb").write(data)
    return out


def test_build_fixed_dropin(fix_models, inputs):
    assert len(fix_models) == len(CASES["models"])
    exe = built_binary("integration", "_build", "build-fixed_dropin")
    for e in CASES["build_errors"]:
        rc, out, err = _run([exe, *e["opts"]], inputs[e["input"]])
        assert rc == e["status"] and len(out) == e["stdout_bytes"], e["name"]
        assert err.decode().replace(exe, "build-fixed") == e["stderr"], e["name"]


@pytest.mark.parametrize("prog", ["score-fixed_dropin", "score-fixed_gpu"])
def test_score_fixed_programs(fix_models, inputs, prog):
    exe = built_binary("integration", "_build", prog)
    for r in CASES["score_runs"]:
        args = r["opts"] + [fix_models[r["pos"]]] + ([NC_ICM if r["neg"] == "NC_000915.icm" else fix_models[r["neg"]]] if r["neg"] else [])
        rc, out, err = _run([exe, *args], inputs[r["input"]])
        assert hashlib.sha256(out).hexdigest() == r["stdout_sha256"] and out.count(b"\n") == r["stdout_lines"], (prog, r["name"])
        assert err.decode() == r["stderr"], (prog, r["name"])
        assert rc == r["status"], (prog, r["name"])


def test_score_fixed_gpu_matches_dropin_on_200k(fix_models, genome, tmp_path):
    rng = np.random.default_rng(200_000)
    path = tmp_path / "many.fa"
    with open(path, "wb") as fp:
        for k, s in enumerate(rng.integers(0, len(genome) - 40, 200_000)):
            w = genome[s:s + int(rng.integers(24, 31))]
            fp.write(b">w%d\n%s\n" % (k, w.lower() if k % 2 else w))
    outs = []
    for prog in ("score-fixed_dropin", "score-fixed_gpu"):
        exe = built_binary("integration", "_build", prog)
        outs.append(_run([exe, fix_models["L24_d5"], fix_models["L24_d7_rand"]], str(path)))
    assert outs[0][0] == outs[1][0] == 0
    assert outs[0][1] == outs[1][1] and outs[0][1].count(b"\n") == 200_000
