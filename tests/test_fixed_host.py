"""Fixed-length ICMs, host side (no GPU): .fix parsing and its refusals through gmg_fixed_icm_read, the reference's
"too short" / "Bad range" checks through gmg_fixed_icm_score, the new ABI symbols, and the test oracle (tests/fixed_oracle.py)
against the reference's build-fixed / score-fixed output (tests/golden/fixed, made by tools/gen_golden_fixed.py; the FASTA inputs
are rebuilt from NC_000915.fna by fixed_oracle.make_inputs)."""
import hashlib
import json
import os
import re
import struct

import numpy as np
import pytest

import fixed_oracle as fo
from conftest import GOLD, ROOT

FIX = os.path.join(GOLD, "fixed")
CASES = json.load(open(os.path.join(FIX, "cases.json")))
MODELS = {m["name"]: m for m in CASES["models"]}
RUNS = {r["name"]: r for r in CASES["score_runs"]}
WHOLE_BIN = [m["name"] for m in CASES["models"] if m["whole"]]


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    return fo.make_inputs(os.path.join(GOLD, "data", "NC_000915.fna"), str(tmp_path_factory.mktemp("fixed_inputs")))


def test_inputs_rebuilt(inputs):
    assert {n: hashlib.sha256(open(p, "rb").read()).hexdigest() for n, p in inputs.items()} == CASES["inputs"]


def _bytes(name):
    return open(os.path.join(FIX, name + ".fix"), "rb").read()


@pytest.mark.parametrize("name", WHOLE_BIN)
def test_golden_header_and_permutation(gmg, name, tmp_path):
    m = MODELS[name]
    data = _bytes(name)
    assert hashlib.sha256(data).hexdigest() == m["sha256"]
    perm = m["perm"] if m["perm"] is not None else list(range(m["length"]))
    f = gmg.FixedIcm.open(os.path.join(FIX, name + ".fix"))
    assert f.params == (m["length"], m["depth"], m["special"], 0, perm)
    p = fo.parse_fix(data)
    assert (p["length"], p["depth"], p["special"], p["perm"]) == (m["length"], m["depth"], m["special"], perm)
    want = ">ver=2.00  len=%d  depth=%d  special=%d  type=0  %s\n" % (m["length"], m["depth"], m["special"], ",".join(map(str, perm)))
    assert p["header"] == want.encode()
    # sub-model i: model_len i+1, depth min(i, max_depth)
    assert [d for _, _, d in p["subs"]] == [min(i, m["depth"]) for i in range(m["length"])]


def _edited(tmp_path, name, fn):
    data = bytearray(_bytes(name))
    fn(data)
    p = tmp_path / ("edited_" + name + ".fix")
    p.write_bytes(bytes(data))
    return str(p)


def test_refusals(gmg, tmp_path):
    bad_version = _edited(tmp_path, "L12_d3_rand", lambda d: struct.pack_into("<i", d, 150, 199))
    with pytest.raises(gmg.GmgError, match=r"Bad ICM version = 199  should be 200") as e:
        gmg.FixedIcm.open(bad_version)
    assert e.value.code == -5
    too_long = _edited(tmp_path, "L12_d3_rand", lambda d: struct.pack_into("<i", d, 158, 33))
    with pytest.raises(gmg.GmgError, match=r"length = 33  must be 1 \.\. 32"):
        gmg.FixedIcm.open(too_long)
    # a permutation that repeats an entry (the reference does not check: undefined behaviour there)
    dup = _edited(tmp_path, "L12_d3_rand", lambda d: struct.pack_into("<i", d, 174 + 4, struct.unpack_from("<i", d, 174)[0]))
    with pytest.raises(gmg.GmgError, match=r"not a bijection of 0\.\.11"):
        gmg.FixedIcm.open(dup)
    out_of_range = _edited(tmp_path, "L2_d3_rev", lambda d: struct.pack_into("<i", d, 174, 2))
    with pytest.raises(gmg.GmgError, match=r"not a bijection"):
        gmg.FixedIcm.open(out_of_range)
    truncated = _edited(tmp_path, "L12_d3_rand", lambda d: d.__delitem__(slice(5000, None)))
    with pytest.raises(gmg.GmgError):
        gmg.FixedIcm.open(truncated)
    with pytest.raises(gmg.GmgError, match=r"Could not open file"):
        gmg.FixedIcm.open(str(tmp_path / "missing.fix"))
    text = tmp_path / "text.fix"                # a -t model: text where the binary header belongs
    text.write_bytes(b"ver=2.00  len=12  depth=3  special=-1  type=0  " + b",".join(b"%d" % i for i in range(12)) + b"\n" * 200)
    with pytest.raises(gmg.GmgError):
        gmg.FixedIcm.open(str(text))


def test_window_checks_without_a_device(gmg):
    """the reference's messages come from host checks that run before any device work"""
    f = gmg.FixedIcm.open(os.path.join(FIX, "L12_d3_rand.fix"))
    perm = MODELS["L12_d3_rand"]["perm"]
    w = b"acgtacgtac"                                   # 10 of 12 bases
    shown = bytes(w[p] for p in perm[:next(i for i, p in enumerate(perm) if p >= len(w))])
    with pytest.raises(gmg.GmgError, match=re.escape('ERROR:  String "%s" too short in Score_Window' % shown.decode())) as e:
        f.score([b"acgtacgtacgt", w])
    assert e.value.code == -6
    # subrange_score only checks [lo, hi): below the first '\0' of the permuted window nothing is reported
    first = next(i for i, p in enumerate(perm) if p >= len(w))
    with pytest.raises(gmg.GmgError, match="too short"):
        f.score([w], first, first + 1)
    with pytest.raises(gmg.GmgError, match=r"Bad range  lo = 3  hi = 13  in subrange_score") as e:
        f.score([b"acgtacgtacgt"], 3, 13)
    assert e.value.code == -1


def test_abi_symbols(gmg):
    lib = gmg.capi.lib()
    names = ["gmg_fixed_model_upload", "gmg_fixed_model_free", "gmg_fixed_model_info", "gmg_fixed_score",
             "gmg_fixed_icm_read", "gmg_fixed_icm_train", "gmg_fixed_icm_write", "gmg_fixed_icm_params", "gmg_fixed_icm_score",
             "gmg_fixed_icm_device_model", "gmg_fixed_icm_free"]
    for n in names:
        assert hasattr(lib, n) and n in gmg.capi.PROTOTYPES
    decl = open(os.path.join(ROOT, "include", "gmg.h")).read() + open(os.path.join(ROOT, "include", "gmg_icm.h")).read()
    for n in names:
        assert re.search(r"\b%s\(" % n, decl), n
    hh = open(os.path.join(ROOT, "glimmer-mg_amd", "host", "icm.hh")).read()
    for cls in ("enum  ICM_Model_t", "class  Fixed_Length_ICM_t", "class  Fixed_Length_ICM_Training_t", "Permute_Data", "Permute_String"):
        assert cls in hh


def _trained(oracle, inputs, name):
    m = MODELS[name]
    strings = fo.read_fasta_strings(inputs[m["train"]])
    perm = m["perm"] if m["perm"] is not None else list(range(m["length"]))
    return fo.train(oracle, strings, m["length"], m["depth"], m["perm"]), perm


def test_oracle_training_matches_reference_tables(oracle, inputs):
    """the oracle's sub-models, trained on the permuted prefixes, are the reference's tables bit for bit"""
    for name in ("L1_d3", "L2_d3_rev", "L12_d3_rand", "L24_d3_rev"):
        subs, _ = _trained(oracle, inputs, name)
        ref = fo.parse_fix(_bytes(name))["subs"]
        for (m1, p1, d1), (m2, p2, d2) in zip(subs, ref):
            assert d1 == d2 and np.array_equal(m1, m2) and np.array_equal(p1.view(np.uint32), p2.view(np.uint32)), name


@pytest.mark.parametrize("run", ["default", "simple", "null_neg", "L1_L2", "short"])
def test_oracle_scores_match_score_fixed(oracle, inputs, run):
    r = RUNS[run]
    pos, pperm = _trained(oracle, inputs, r["pos"])
    neg = _trained(oracle, inputs, r["neg"]) if r["neg"] else None
    strings = fo.read_fasta_strings(inputs[r["input"]])
    need = max(len(pos), len(neg[0]) if neg else 0)
    n = next((k for k, s in enumerate(strings) if len(s) < need), len(strings))
    c = fo.codes(strings[:n])
    ps = fo.score(pos, pperm, c)
    ns = fo.score(neg[0], neg[1], c) if neg else np.zeros(n)
    got = "".join(fo.score_line(k, ps[k], ns[k], len(strings[k]), "-s" in r["opts"]) for k in range(n))
    assert hashlib.sha256(got.encode()).hexdigest() == r["stdout_sha256"] and got.count("\n") == r["stdout_lines"]
    assert (r["status"] != 0) == (n < len(strings))
