"""Pins the CPU oracle's SCORER (oracle/gmg_oracle.c) to the reference on model shapes other than window 12 / depth 7:
tests/golden/shapes_<name>.npz holds what the reference's ICM_t gave with the model its own build-icm trained
(oracle/gen_golden_shapes.py).  Here the oracle trains the same model (its file must have the recorded hash), reads that file and
scores the same reads: Score_All_Frames, Score_String, Partial_Window_Prob, Cumulative_Score_String and the window distribution
must agree bit for bit -- values for the first reads and every short read, a SHA-256 over all reads.  Only then does a
device-against-oracle comparison on these shapes (tests/test_gpu_model_shapes.py) prove anything.  CPU only."""
import hashlib
import os

import numpy as np
import pytest

import model_zoo
from conftest import DATA, GOLD

NAMES = model_zoo.TRAINED + model_zoo.COMMITTED


@pytest.fixture(scope="module")
def model_dir(tmp_path_factory):
    return tmp_path_factory.mktemp("shapes")


@pytest.fixture(scope="module")
def read_sets(oracle, gmg, seqs_fa):
    _, short = gmg.read_fasta(os.path.join(DATA, "short_reads.fa"))
    assert sorted(set(len(s) for s in short)) == list(range(1, 41))
    return [oracle.filter_lower(s) for s in seqs_fa[1]], [oracle.filter_lower(s) for s in short]


@pytest.fixture(params=NAMES)
def shape(request, oracle, gmg, model_dir):
    name = request.param
    path = model_zoo.model_file(oracle, gmg, name, model_dir)          # (asserts the recorded size and hash of a trained file)
    g = np.load(os.path.join(GOLD, "shapes_%s.npz" % name))
    assert hashlib.sha256(open(path, "rb").read()).hexdigest() == str(g["model_sha256"])
    m = oracle.read(path)
    c = m.contents
    assert (c.model_len, c.model_depth, c.periodicity) == (int(g["W"]), int(g["D"]), int(g["P"]))
    yield name, m, g
    oracle.L.orc_model_free(m)


def test_every_shape_of_the_issue_is_pinned():
    shapes = {(c["model_len"], c["model_depth"], c["periodicity"]) for c in (model_zoo.CASES[n] for n in NAMES)}
    assert {(8, 7, 3), (13, 7, 3), (15, 7, 3), (4, 7, 3), (16, 7, 3), (12, 8, 3), (12, 9, 3), (20, 5, 3), (12, 1, 3),
            (8, 7, 1), (15, 7, 1), (16, 7, 1), (3, 2, 4), (6, 3, 2), (9, 5, 1), (2, 1, 3), (12, 4, 3)} <= shapes


def test_score_all_frames(shape, oracle, read_sets):
    name, m, g = shape
    if int(g["P"]) < 3:
        assert "frames_seqs" not in g.files                 # (Frame_Score asserts frame < periodicity: the reference has no such table)
        return
    seqs, short = read_sets
    indep = oracle.indep(float(g["gc"]))
    h = hashlib.sha256()
    for r, s in enumerate(seqs):
        out = oracle.score_all_frames(m, indep, s)
        if r < g["frames_seqs"].shape[0]:
            assert np.array_equal(out, g["frames_seqs"][r]), (name, r)
        h.update(out.tobytes())
    assert h.hexdigest() == str(g["frames_seqs_sha256"])
    off = 0
    for s in short:
        want = g["frames_short"][off:off + 6 * len(s)].reshape(6, len(s))
        assert np.array_equal(oracle.score_all_frames(m, indep, s), want), (name, len(s))
        off += 6 * len(s)
    assert off == g["frames_short"].size


def test_score_string(shape, oracle, read_sets):
    name, m, g = shape
    P = int(g["P"])
    seqs, short = read_sets
    frames = [0 if P == 1 else f % P for f in range(3)]
    h = hashlib.sha256()
    for r, s in enumerate(seqs):
        out = np.array([oracle.score_string(m, s, f) for f in frames])
        if r < g["sstring_seqs"].shape[0]:
            assert np.array_equal(out, g["sstring_seqs"][r]), (name, r)
        h.update(out.tobytes())
    assert h.hexdigest() == str(g["sstring_seqs_sha256"])
    for r, s in enumerate(short):
        assert np.array_equal(np.array([oracle.score_string(m, s, f) for f in frames]), g["sstring_short"][r]), (name, len(s))


def test_partial_window(shape, oracle, read_sets):
    name, m, g = shape
    W, P = int(g["W"]), int(g["P"])
    seqs, short = read_sets
    h = hashlib.sha256()
    for r in range(64):
        out = np.array([[oracle.partial_window(m, i, seqs[r], f) for i in range(W - 1)] for f in range(P)]).reshape(P, W - 1)
        if r < g["partial_seqs"].shape[0]:
            assert np.array_equal(out, g["partial_seqs"][r]), (name, r)
        h.update(out.tobytes())
    assert h.hexdigest() == str(g["partial_seqs_sha256"])
    off = 0
    for s in short:
        lim = min(W - 1, len(s))
        out = np.array([[oracle.partial_window(m, i, s, f) for i in range(lim)] for f in range(P)]).reshape(P, lim)
        assert np.array_equal(out.ravel(), g["partial_short"][off:off + P * lim]), (name, len(s))
        off += P * lim
    assert off == g["partial_short"].size


def cumulative_score_string(oracle, m, s, f):
    """Cumulative_Score_String (icm.cc:409-452): 0, then the running sums of Cumulative_Score"""
    return np.concatenate([[0.0], oracle.cumulative_score(m, s, f)])


def test_cumulative_score(shape, oracle, read_sets):
    name, m, g = shape
    W, P = int(g["W"]), int(g["P"])
    seqs, short = read_sets
    h = hashlib.sha256()
    for r in range(16):
        out = np.stack([cumulative_score_string(oracle, m, seqs[r], f) for f in range(P)])
        if r < g["cumstr_seqs"].shape[0]:
            assert np.array_equal(out, g["cumstr_seqs"][r]), (name, r)
        h.update(out.tobytes())
    assert h.hexdigest() == str(g["cumstr_seqs_sha256"])
    off = 0
    for s in short:
        if len(s) < W - 1:                                  # (the reference scores the first W - 1 bases whatever the length: not dumped)
            continue
        for f in range(P):
            assert np.array_equal(cumulative_score_string(oracle, m, s, f), g["cumstr_short"][off:off + len(s) + 1]), (name, len(s), f)
            off += len(s) + 1
    assert off == g["cumstr_short"].size


def test_window_distribution(shape, oracle):
    name, m, g = shape
    for i in range(g["windows"].shape[0]):
        w = g["windows"][i].tobytes()
        for f in range(int(g["P"])):
            p, dist = oracle.full_window(m, w, f)
            assert p == g["window_prob"][i, f], (name, i, f)
            assert np.array_equal(dist.view(np.uint32), g["window_dist"][i, f].view(np.uint32)), (name, i, f)


@pytest.mark.parametrize("name", model_zoo.FAST3 + model_zoo.FAST1)
def test_clean_twins_are_eligible(name, oracle, gmg, model_dir):
    """the helper's proof, without a device: the twin's values are negative normal floats within the exponent spread the
    reordered sums need for a 2,100-base read; a raw model in which something had to be replaced is not eligible (w 4 / d 7: the
    witness of the sequential fall-back), the others are their own twins"""
    path = model_zoo.model_file(oracle, gmg, name, model_dir)
    twin = str(model_dir / (name + "_twin.icm"))
    replaced = model_zoo.write_clean_twin(path, twin)
    assert (replaced > 0) == (name == "s3_w4_d7")
    nulls = [oracle.tables(oracle.indep(gc)) for gc in (0.3, 0.4, 0.5, 0.6, 0.7)]
    raw, tw = oracle.read(path), oracle.read(twin)
    ok, why = model_zoo.clean_is_eligible(oracle, tw, nulls)
    assert ok, why
    assert model_zoo.clean_is_eligible(oracle, raw, nulls)[0] == (replaced == 0)
    a, b = oracle.tables(raw), oracle.tables(tw)
    assert np.array_equal(a[0], b[0])
    same = a[1].view(np.uint32) == b[1].view(np.uint32)
    assert int((~same).sum()) == replaced and np.all(b[1][~same] == model_zoo.CLEAN_VALUE) and np.all(model_zoo.is_odd(a[1][~same]))
