"""gmg_icm_bytes_info (include/gmg.h): the header of a binary .icm from its bytes, on the host -- the part of the device loader
(gmg_model_set_load) that needs no GPU.  The shape must be what struct reads at byte 150, the blob size what gmg_model_upload's
layout gives for that shape (recomputed here from the description in csrc/gmg_internal.h), the refusals Try_Input's."""
import glob
import os
import struct

import pytest

import model_zoo
from conftest import DATA

TRAIN = model_zoo.TRAIN


def binary_models():
    files = sorted(glob.glob(os.path.join(DATA, "*.icm")) + glob.glob(os.path.join(DATA, "*.gicm")) + glob.glob(os.path.join(TRAIN, "*.icm")))
    return [f for f in files if open(f, "rb").read(1) == b">"]             # (the text form starts with "ver = ")


def align(x, a):
    return (x + a - 1) // a * a


def blob_tables(W, D, P, N):
    """[(table, first byte)] + [("end", size)] of a model's device blob: mip int8 [P][N] | prob [P][N][4] | cshift [P][cstride] |
    crow [P][ctot][4] + a zero row | chalf [P][2][4^D][2] | dense [P][4^W] | dense_part [P][(4^W - 4) / 3] (+ 4 bytes); every table
    at a multiple of 256; the fast tables for W <= 16 and D <= 8, the direct ones for W <= 6"""
    fast, dense = W <= 16 and D <= 8, W <= 6
    n_internal, ctot, leaves = (4 ** D - 1) // 3, (4 ** (D + 1) - 1) // 3, 4 ** D
    cstride = align(max(n_internal, 1), 16)
    n_dense = 4 ** W if dense else 0
    n_part = (n_dense - 4) // 3 if dense else 0
    out = [("mip", 0)]
    out.append(("prob", align(P * N, 256)))
    out.append(("cshift", align(out[-1][1] + P * N * 16, 256)))
    out.append(("crow", align(out[-1][1] + (P * cstride if fast else 0), 256)))
    out.append(("chalf", align(out[-1][1] + (P * ctot * 16 + 16 if fast else 0), 256)))
    out.append(("dense", align(out[-1][1] + (P * leaves * 16 if fast else 0), 256)))
    out.append(("dense_part", align(out[-1][1] + P * n_dense * 4, 256)))
    out.append(("end", align(out[-1][1] + P * n_part * 4 + 4, 256)))
    return out


def blob_size(W, D, P, N):
    return blob_tables(W, D, P, N)[-1][1]


def test_header_and_blob_size_of_every_committed_binary_model(gmg):
    files = binary_models()
    assert len(files) >= 17 and any(f.endswith(".gicm") for f in files)
    shapes = set()
    for path in files:
        data = open(path, "rb").read()
        ver, idl, W, D, P, N = struct.unpack_from("<6i", data, 150)
        assert (ver, idl) == (200, 150), path
        assert len(model_zoo.records(data)) >= P                            # (a binary stream that model_zoo.records walks to its end)
        got = gmg.icm_bytes_info(data)
        assert got[:4] == (W, D, P, N), path
        assert got[4] == blob_size(W, D, P, N), path
        assert gmg.icm_bytes_info(data[:174])[:4] == (W, D, P, N)          # only the header is read
        shapes.add((W, D, P))
    assert {(12, 7, 3), (12, 7, 1), (2, 1, 3), (3, 2, 4), (6, 3, 2)} <= shapes


def test_header_refusals_carry_the_readers_messages(gmg):
    good = bytearray(open(os.path.join(DATA, "cluster-4.icm"), "rb").read())

    def patched(at, value):
        b = bytearray(good)
        b[at:at + 4] = struct.pack("<i", value)
        return bytes(b)

    cases = [(bytes(good[:100]), "ERROR reading ICM header"),
             (bytes(good[:160]), "ERROR reading parameters"),
             (patched(150, 199), "Bad ICM version = 199  should be 200"),
             (patched(154, 149), "Bad ID_STRING_LEN = 149  should be 150"),
             (patched(162, -1), "ERROR:  bad ICM parameters")]
    for data, msg in cases:
        with pytest.raises(gmg.GmgError, match=msg) as e:
            gmg.icm_bytes_info(data)
        assert e.value.code == -5
    with pytest.raises(gmg.GmgError, match="ERROR reading ICM header"):
        gmg.icm_bytes_info(b"")


def test_text_format_is_refused_as_the_reader_refuses_it(gmg, tmp_path):
    path = os.path.join(TRAIN, "c4_text_d3_r.icm")
    data = open(path, "rb").read()
    with pytest.raises(gmg.GmgError) as from_file:
        gmg.Icm.open(path)
    with pytest.raises(gmg.GmgError) as from_bytes:
        gmg.icm_bytes_info(data)
    assert str(from_bytes.value) == str(from_file.value)


def test_shapes_the_kernels_do_not_take_have_no_blob_size(gmg):
    """len 33, depth 13, fewer nodes than the depth needs: gmg_model_upload's refusals, met when the blob size is asked for"""
    good = bytearray(open(os.path.join(DATA, "cluster-4.icm"), "rb").read())
    for at, value, msg in ((158, 33, "unsupported shape"), (162, 13, "unsupported shape"), (170, 21844, "num_nodes=21844 < 21845")):
        b = bytearray(good[:174])
        b[at:at + 4] = struct.pack("<i", value)
        with pytest.raises(gmg.GmgError, match=msg):
            gmg.icm_bytes_info(bytes(b))
