"""Models of shapes other than window 12 / depth 7 for the scoring tests (tests/test_oracle_shapes.py, tests/test_gpu_model_shapes.py).

  zoo(gmg, oracle, tmp_dir) -> {name: (device Icm, oracle model, path)}

Every trained model comes from oracle.train_model on the training set of its entry in tests/golden/train/cases.json and is written
as an .icm file whose SHA-256 must be the one recorded there -- the hash of the file the reference's build-icm wrote
(oracle/gen_golden_shapes.py).  gmg.Icm.open and oracle.read then read that file: both sides score the same bytes, and those
bytes are the ones the reference scored for tests/golden/shapes_<name>.npz.

FAST: the shapes the fast kernels take (depth 7, 3 <= W <= 15).  A trained table may hold logarithms of zero probabilities
(-FLT_MAX, icm.cc:1345-1349), which send a model to the exact sequential paths, so each of them also has a `<name>_clean` twin:
the same file with every value that is positive, denormal, infinite or below -1e30 replaced by float32 (ln 1e-4).
clean_is_eligible() proves from the tables, in numpy, that the twin meets what the reordered-sum paths ask for.  The raw model
stays in the set.  With these training sets only the w 4 / d 7 model has such values (two: a window of four bases cannot hold
what the long ORFs never contain) -- it is the witness of the sequential fall-back and the only one with a twin; the other raw
files are eligible as they are, which zoo() asserts with the caller's null tables.
"""
import hashlib
import json
import os
import struct

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden")
TRAIN = os.path.join(GOLD, "train")
CASES = {c["name"]: c for c in json.load(open(os.path.join(TRAIN, "cases.json")))}

FAST3 = ["s3_w8_d7", "s3_w13_d7", "s3_w15_d7", "s3_w4_d7"]                # periodicity 3: k_frame6t / k_frame6p, GENE32, k_orf_fused
FAST1 = ["s1_w8_d7", "s1_w15_d7"]                                          # periodicity 1: the strings main pass
ANY3 = ["s3_w16_d7", "s3_w12_d8", "s3_w12_d9", "s3_w20_d5", "s3_w12_d1", "c3_w16_d8_r", "syn_d4", "c4_d1_w2"]
ANY1 = ["s1_w16_d7", "c3_p1_d5_w9"]
OTHER_P = ["c4_p4_d2_w3", "c3_p2_d3_w6_r"]                                 # periodicity 4 and 2
TRAINED = FAST3 + FAST1 + ["s3_w16_d7", "s3_w12_d8", "s3_w12_d9", "s3_w20_d5", "s3_w12_d1", "s1_w16_d7"]
TRAINED_UNPINNED = ["c3_w16_d8_r"]                                          # 16 / 8: the trainer's golden case; no scoring vectors of the reference
COMMITTED = ["syn_d4", "c4_d1_w2", "c3_p1_d5_w9", "c4_p4_d2_w3", "c3_p2_d3_w6_r"]
CLEAN_VALUE = np.float32(np.log(1e-4))
LONGEST_READ = 2100                                                         # the longest read of the GPU tests' read sets

_files = {}


def model_file(oracle, gmg, name, tmp_dir):
    """path of the model's .icm file: the committed one, or the oracle's training written to tmp_dir (hash checked)"""
    case = CASES[name]
    if case["whole"]:
        return os.path.join(TRAIN, name + ".icm")
    if name in _files and os.path.exists(_files[name]):
        return _files[name]
    from test_oracle_train import training_strings
    m = oracle.train_model(training_strings(case, gmg), case["model_len"], case["model_depth"], case["periodicity"])
    path = os.path.join(str(tmp_dir), name + ".icm")
    assert oracle.L.orc_model_write(m, path.encode()) == 0
    oracle.L.orc_model_free(m)
    data = open(path, "rb").read()
    assert len(data) == case["bytes"] and hashlib.sha256(data).hexdigest() == case["sha256"], name
    _files[name] = path
    return path


def records(buf):
    """binary .icm (icm.cc:614-726): 150 header bytes, six int32, then records {int32 id, 4 float32, int16 mip}, -1 at the end
    -> byte offsets of every record's four floats"""
    off, at = 174, []
    while True:
        (nid,) = struct.unpack_from("<i", buf, off)
        if nid < 0:
            return np.array(at, np.int64)
        at.append(off + 4)
        off += 22


def is_odd(v):
    """values the reordered sums cannot take: what gmg_model_upload calls odd (positive, denormal, infinite / NaN) and the
    logarithm of a zero probability"""
    b = v.view(np.uint32)
    ex = (b >> 23) & 0xff
    nonzero = (b << 1) != 0
    return nonzero & (((b >> 31) == 0) | (ex == 0) | (ex == 255) | (v < np.float32(-1e30)))


def write_clean_twin(src, dst):
    raw = bytearray(open(src, "rb").read())
    at = records(raw)
    vals = np.stack([np.frombuffer(raw, "<f4", 4, int(o)) for o in at]).copy()
    bad = is_odd(vals)
    vals[bad] = CLEAN_VALUE
    for o, v in zip(at[bad.any(axis=1)], vals[bad.any(axis=1)]):
        raw[int(o):int(o) + 16] = v.astype("<f4").tobytes()
    open(dst, "wb").write(bytes(raw))
    return int(bad.sum())


def exponent_range(mip, prob):
    """(min_exp, max_exp, odd) over the values of existing nodes, zeros left out -- as gmg_model_upload counts them"""
    v = prob[mip != -2].ravel()
    b = v.view(np.uint32)
    v = v[(b << 1) != 0]
    ex = (v.view(np.uint32) >> 23) & 0xff
    return int(ex.min()), int(ex.max()), bool(is_odd(v).any() or (v > 0).any())


def clog(longest_read):
    c = 0
    while (1 << c) < longest_read + 2:
        c += 1
    return c


def clean_is_eligible(oracle, o_model, null_tables, longest_read=LONGEST_READ):
    """the twin's tables, and the null models', hold negative normal floats only, and clog + max_exp - min_exp <= 28 for the
    longest read: the condition of mg_plan and of gmg_score_orfs' events path"""
    lo, hi, odd = exponent_range(*oracle.tables(o_model))
    for mip, prob in null_tables:
        a, b, o = exponent_range(mip, prob)
        lo, hi, odd = min(lo, a), max(hi, b), odd or o
    return (not odd) and clog(longest_read) + hi - lo <= 28, (lo, hi, odd)


def zoo(gmg, oracle, tmp_dir, names=None, null_tables=()):
    """{name: (device Icm, oracle model, path)}.  A fast-class model in which write_clean_twin had something to replace also brings
    its `_clean` twin (otherwise the twin would be the same bytes).  null_tables: oracle.tables() of every null model the caller
    uploads -- with them, every fast-class model that is meant to reach the reordered sums (the twin, or the raw model when it
    has no twin) is asserted eligible for LONGEST_READ here, so that a test cannot pass on the sequential path unnoticed"""
    out = {}
    for name in (names if names is not None else TRAINED + TRAINED_UNPINNED + COMMITTED):
        path = model_file(oracle, gmg, name, tmp_dir)
        out[name] = (gmg.Icm.open(path), oracle.read(path), path)
        if name in FAST3 + FAST1:
            twin = os.path.join(str(tmp_dir), name + "_clean.icm")
            best = name
            if write_clean_twin(path, twin) > 0:
                out[name + "_clean"] = (gmg.Icm.open(twin), oracle.read(twin), twin)
                best = name + "_clean"
            else:
                os.remove(twin)
            ok, why = clean_is_eligible(oracle, out[best][1], null_tables)
            assert ok, (best, why)
    return out


def free(oracle, models):
    for icm, om, _ in models.values():
        icm.close()
        oracle.L.orc_model_free(om)
