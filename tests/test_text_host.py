"""The yardstick of gmg_regions_text before the device is involved (no GPU needed): the Python restatement of the record rule
(tests/text_oracle.py) reproduces the recorded texts of the reference's extract / multi-extract byte for byte and every
per-record digest of the runs kept as digests; gmg_text_params_reference is the reference's Complement; a text call's size
query and refusals work on the host."""
import os

import numpy as np
import pytest

import extract_oracle as xo
import text_oracle as to
from conftest import DATA

EX = xo.EX
NC = os.path.join(DATA, "NC_000915.fna")
SEQS = os.path.join(DATA, "seqs.fa")
SLICE = os.path.join(EX, "slice2000.fna")

# (program, options, sequence file, coordinate file, recording)
RECORDED = [
    ("extract", ["-t"], NC, "nc_subset.coords", "nc_subset.t.out"),
    ("extract", [], SLICE, "slice_wrap.coords", "slice_wrap.out"),
    ("multi-extract", ["-t"], SEQS, "seqs_multi.coords", "seqs_multi.t.out"),
    ("extract", [], NC, "nc_subset.coords", "nc_subset.sha256"),
    ("extract", ["-s", "-t", "-l", "300"], NC, "nc_subset.coords", "nc_subset.s_t_l300.sha256"),
    ("extract", ["-w"], NC, "nc_subset.coords", "nc_subset.w.sha256"),
    ("extract", ["-d"], NC, "nc_subset.coords", "nc_subset.d.sha256"),
    ("extract", ["-t"], SLICE, "slice_wrap.coords", "slice_wrap.t.sha256"),
    ("extract", ["-s"], SLICE, "slice_wrap.coords", "slice_wrap.s.sha256"),
    ("extract", ["-w", "-l", "3"], SLICE, "slice_wrap.coords", "slice_wrap.w_l3.sha256"),
    ("extract", ["-d"], SLICE, "slice_dir.coords", "slice_dir.d.sha256"),
    ("extract", ["-d", "-s", "-t"], SLICE, "slice_dir.coords", "slice_dir.d_s_t.sha256"),
    ("multi-extract", ["-s", "-l", "60"], SEQS, "seqs_multi.coords", "seqs_multi.s_l60.sha256"),
]
IDS = [r[4] for r in RECORDED]


def restated(gmg, program, opts, seq_file, coords_file):
    return to.run(gmg, program, opts, open(seq_file, "rb").read(), open(os.path.join(EX, coords_file)).read())


def in_recorded_order(records, recording):
    """the restatement's records in the order of the recording's headers (multi-extract: the order among the lines of one tag is
    std::sort's); ids are unique in every coordinate file here"""
    by_id = dict(records)
    assert len(by_id) == len(records)
    want = [h[0] for h, _, _ in xo.recorded(recording)]
    assert sorted(want) == sorted(by_id)
    return [by_id[i] for i in want]


@pytest.mark.parametrize("program,opts,seq_file,coords_file,recording", RECORDED[:3], ids=IDS[:3])
def test_restatement_reproduces_the_recorded_texts(gmg, program, opts, seq_file, coords_file, recording):
    records, err = restated(gmg, program, opts, seq_file, coords_file)
    assert err == ""
    got = "".join(in_recorded_order(records, recording))
    assert got == open(os.path.join(EX, recording)).read()
    assert to.body_lines_ok(got) and got.count(">") == len(records) >= 14


@pytest.mark.parametrize("program,opts,seq_file,coords_file,recording", RECORDED[3:], ids=IDS[3:])
def test_restatement_reproduces_every_recorded_digest(gmg, program, opts, seq_file, coords_file, recording):
    records, err = restated(gmg, program, opts, seq_file, coords_file)
    assert err == ""
    want = xo.recorded(recording)
    for rec, (hdr, length, digest) in zip(in_recorded_order(records, recording), want):
        head, _, body = rec.partition("\n")
        assert head[1:].split() == hdr
        letters = body.replace("\n", "")
        assert len(letters) == length and xo.sha(letters) == digest, hdr
        assert body == to.record("", letters)           # (the lines are the rule's)
    assert len(want) >= 8


def test_record_rule_at_the_line_width():
    for n, want in [(0, "\n"), (1, "a\n"), (59, "a" * 59 + "\n"), (60, "a" * 60 + "\n"), (61, "a" * 60 + "\na\n"),
                    (120, "a" * 60 + "\n" + "a" * 60 + "\n"), (121, "a" * 60 + "\n" + "a" * 60 + "\na\n")]:
        assert to.record("", "a" * n) == want
    assert to.record(">h\n", "acgtacg", 3) == ">h\nacg\ntac\ng\n" and to.record("t ", "acgtacg", 0) == "t acgtacg\n"


def test_reference_tables(gmg):
    """fwd: every byte itself.  rev: the restatement's complement for every byte below 128 that is no upper-case letter outside
    the IUPAC set (the reference's table keeps the case there, 'N': src/Common/gene.cc:15-19); 'n' from 128 on"""
    p = gmg.text_params(60)
    assert p.width == 60 and p.reserved == 0 and bytes(p.fwd) == bytes(range(256))
    rev = bytes(p.rev)
    for ch in range(128):
        c = chr(ch)
        if c.isupper() and c.lower() not in xo._PAIRS:
            assert rev[ch] == ord("N"), c
        else:
            assert chr(rev[ch]) == xo.complement(c), c
    assert rev[128:] == b"n" * 128
    assert gmg.text_params(0, rev=bytes(range(256))).rev[65] == 65


def test_text_calls_fail_loudly_without_a_device(gmg):
    """no GPU, no text: gmg_letters_upload is GMG_ENODEV before gmg_init (this module never initialises a device)"""
    handle = gmg.capi.C.c_void_p()
    off = np.array([0, 4], np.uint64)
    rc = gmg.capi.lib().gmg_letters_upload(b"acgt", off.ctypes.data, 1, gmg.capi.C.byref(handle))
    if rc == 0:                                          # (the session's GPU tests ran first and initialised the device)
        gmg.capi.lib().gmg_letters_free(handle)
    else:
        assert rc == -2 and not handle.value
