"""gmg_model_set_* (include/gmg.h, csrc/gmg_models.hip): binary .icm files parsed and flattened on the device.  The reference of
every check is the host path on the same bytes -- gmg_icm_open + gmg_icm_device_model (Try_Input, then gmg_model_upload): the device
blob byte for byte, the value statistics, the shape, the scores through three entry points, Try_Input's refusals with their
messages, a load on a second stream beside scoring on the null stream, and phymm_gpu with and without --host-load."""
import ctypes as C
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import model_zoo
import phymm_oracle as po
from conftest import DATA, ROOT
from test_model_bytes_host import blob_tables

pytestmark = pytest.mark.gpu

TRAINED = ["s3_w16_d7", "s3_w12_d8", "s3_w12_d1", "s3_w4_d7", "s1_w15_d7", "s3_w20_d5", "s3_w12_d9"]
SAMPLE = ["cluster-0.icm", "NC_000915.icm", "seqs.cluster-4.run1.filt.gicm"]
HEAD, REC = 174, 22


def first_difference(got, want, shape):
    """None, or where two blobs differ first: (table, byte inside it)"""
    if got == want:
        return None
    if len(got) != len(want):
        return "sizes", len(got), len(want)
    a, b = np.frombuffer(got, np.uint8), np.frombuffer(want, np.uint8)
    at = int(np.flatnonzero(a != b)[0])
    name, start = [(n, o) for n, o in blob_tables(*shape) if o <= at][-1]
    return name, at - start, int(a[at]), int(b[at])


def host_side(gpu, path):
    icm = gpu.Icm.open(path)
    return icm, gpu.model_blob(icm), gpu.model_value_stats(icm), gpu.model_info(icm)


def assert_member_equals_host(gpu, member, host, what):
    _, blob, stats, info = host
    assert gpu.model_info(member) == info, what
    assert first_difference(gpu.model_blob(member), blob, info) is None, what
    assert gpu.model_value_stats(member) == stats, what


@pytest.fixture(scope="module")
def members(gpu, oracle, tmp_path_factory):
    """{name: (path, host Icm, host blob, host stats, host info, member of ONE set)} -- every file goes up in a single load"""
    tmp = tmp_path_factory.mktemp("model_set")
    paths = {n: model_zoo.model_file(oracle, gpu, n, tmp) for n in model_zoo.COMMITTED + TRAINED}
    paths.update({n: os.path.join(DATA, n) for n in SAMPLE})
    names = list(paths)
    ms = gpu.ModelSet.load([open(paths[n], "rb").read() for n in names]).finish()
    assert len(ms) == len(names)
    out = {n: (paths[n],) + host_side(gpu, paths[n]) + (ms.model(k),) for k, n in enumerate(names)}
    yield out
    ms.close()
    for v in out.values():
        v[1].close()


def test_every_member_equals_the_host_path_byte_for_byte(gpu, members):
    shapes = set()
    for name, (path, icm, blob, stats, info, member) in members.items():
        assert_member_equals_host(gpu, member, (icm, blob, stats, info), name)
        shapes.add((info[0] <= 16 and info[1] <= 8, info[0] <= 6, info[2]))
    # fast and not, with direct tables and without, periodicity 1 .. 4
    assert {(True, False, 3), (True, False, 1), (False, False, 3), (True, True, 3), (True, True, 4), (True, True, 2)} <= shapes
    assert members["s3_w12_d9"][4][1] == 9                                           # depth 9: no fast tables


def test_scores_through_set_members_are_bit_identical(gpu, members, seqs_fa):
    reads = gpu.Reads.from_strings(seqs_fa[1][:200])
    indep = gpu.Icm.indep(0.5)
    rows = [(r, 0, len(s), o) for r, s in enumerate(seqs_fa[1][:200]) for o in (gpu.FORWARD, gpu.REVCOMP) if r % 7 == 0]
    segs = gpu.Segments(reads, rows)
    for name in ("NC_000915.icm", "s1_w15_d7", "c4_d1_w2"):
        _, icm, _, _, info, member = members[name]
        if info[2] >= 3:
            assert np.array_equal(gpu.frame_score6(member, indep, reads), gpu.frame_score6(icm, indep, reads)), name
        else:                                           # Frame_Score asserts frame < periodicity: both refuse alike
            for m in (member, icm):
                with pytest.raises(gpu.GmgError, match="periodicity must be >= 3"):
                    gpu.frame_score6(m, indep, reads)
        assert np.array_equal(gpu.score_reads_strings([member], reads), gpu.score_reads_strings([icm], reads)), name
        assert np.array_equal(gpu.segment_cumscore(member, reads, segs, 0), gpu.segment_cumscore(icm, reads, segs, 0)), name


# ------------------------------------------------------------------------------------------------------------------------------
# file edges and refusals, each on a copy of syn_d4.icm (12 / 4 / 3, every node present: 3 x 341 records and the end marker)
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def syn():
    data = open(os.path.join(model_zoo.TRAIN, "syn_d4.icm"), "rb").read()
    W, D, P, N = struct.unpack_from("<4i", data, 158)
    assert (W, D, P, N) == (12, 4, 3, 341) and len(data) == HEAD + REC * P * N + 4
    return data


def record(data, r):
    return data[HEAD + REC * r:HEAD + REC * (r + 1)]


def subtree(root, N):
    ids, level = [], [root]
    while level:
        ids += level
        level = [4 * i + 1 + b for i in level for b in range(4) if 4 * i + 1 + b < N]
    return set(ids)


def test_file_edges_give_the_host_paths_model(gpu, syn, tmp_path):
    N = 341
    gone = subtree(2, N) | subtree(19, N)
    assert len(gone) == 85 + 21
    cases = {
        "no_end_marker": syn[:-4],
        "junk3": syn + b"\x01\x02\x03",
        "junk40": syn + bytes(range(200, 240)),
        "subtree_deleted": syn[:HEAD] + b"".join(record(syn, r) for r in range(3 * N) if not (r // N == 1 and r % N in gone)) + syn[-4:],
        "more_nodes": syn[:170] + struct.pack("<i", N + 7) + syn[HEAD:],
    }
    with gpu.ModelSet.load(list(cases.values())) as ms:
        ms.finish()
        for k, (name, data) in enumerate(cases.items()):
            path = tmp_path / (name + ".icm")
            path.write_bytes(data)
            host = host_side(gpu, path)
            assert_member_equals_host(gpu, ms.model(k), host, name)
            if name == "subtree_deleted":
                mip = np.frombuffer(host[1], np.int8, 3 * N)
                assert all(mip[N + i] == -2 for i in gone)
            host[0].close()


def with_record(data, r, rec):
    return data[:HEAD + REC * r] + rec + data[HEAD + REC * (r + 1):]


def test_refusals_name_the_file_and_carry_the_readers_message(gpu, syn, tmp_path):
    N, W = 341, 12
    r = 341 + 77                                        # a record of the second sub-model
    swapped = with_record(with_record(syn, r, record(syn, r + 1)), r + 1, record(syn, r))
    cases = {
        "cut_in_prob": syn[:HEAD + REC * r + 10],
        "cut_in_mip": syn[:HEAD + REC * r + 21],
        "id_beyond_nodes": with_record(syn, r, struct.pack("<i", N) + record(syn, r)[4:]),
        "one_submodel_short": syn[:HEAD + REC * 2 * N] + syn[-4:],
        "one_root_too_many": syn[:-4] + record(syn, 0) + syn[-4:],
        "swapped": swapped,
        "mip_is_W": with_record(syn, r, record(syn, r)[:20] + struct.pack("<h", W)),
    }
    own = {"swapped": r"node 77 follows node 78 in sub-model 1: ids must increase inside a sub-model.*gmg_icm_open",
           "mip_is_W": r"gmg_model_upload: mut_info_pos 12 at slot %d outside \[-2,11\]" % r}
    good = [syn, open(os.path.join(DATA, "cluster-0.icm"), "rb").read(), open(os.path.join(model_zoo.TRAIN, "c4_d1_w2.icm"), "rb").read()]
    for at, (name, data) in enumerate(cases.items()):
        at %= 4
        batch = good[:at] + [data] + good[at:]
        ms = gpu.ModelSet.load(batch)
        with pytest.raises(gpu.GmgError) as e:
            ms.finish()
        assert e.value.code == -5 and e.value.bad_file == at, name
        if name in own:
            assert re.search(own[name], str(e.value)), (name, str(e.value))
        else:                                           # Try_Input's own words for this file
            path = tmp_path / (name + ".icm")
            path.write_bytes(data)
            with pytest.raises(gpu.GmgError) as host:
                gpu.Icm.open(path)
            assert str(e.value) == str(host.value), name
        with pytest.raises(gpu.GmgError):
            ms.model(0)
        ms.close()
        ms.close()
    expect = {"cut_in_prob": "ERROR reading icm node = 77  period = 1", "cut_in_mip": "ERROR reading mut_info_pos for node = 77  period = 1",
              "id_beyond_nodes": "ERROR reading icm node = 341  period = 1", "one_submodel_short": "ERROR:  Too few nodes for periodicity = 3",
              "one_root_too_many": "ERROR reading icm node = 0  period = 3"}
    for name, msg in expect.items():                    # (the words themselves, not only their equality with the host's)
        ms = gpu.ModelSet.load([cases[name]])
        with pytest.raises(gpu.GmgError, match=re.escape(msg)):
            ms.finish()
        ms.close()
    # the swapped file is one the host reads (the last record of an id wins there); a good load after the refusals is correct
    path = tmp_path / "syn.icm"
    path.write_bytes(syn)
    host = host_side(gpu, path)
    with gpu.ModelSet.load([syn]) as ms:
        assert_member_equals_host(gpu, ms.finish().model(0), host, "after the refusals")
    host[0].close()
    # what _load itself refuses, on the host: a bad header inside a batch
    with pytest.raises(gpu.GmgError, match=r"Bad ICM version = 199  should be 200 \(file 1 of the batch\)"):
        gpu.ModelSet.load([syn, syn[:150] + struct.pack("<i", 199) + syn[154:]])
    with pytest.raises(gpu.GmgError, match="ERROR reading ICM header"):
        gpu.ModelSet.load([syn[:100]])


def test_load_on_a_second_stream_beside_scoring_on_the_null_stream(gpu, members, seqs_fa):
    lib = gpu.capi.lib()
    reads = gpu.Reads.from_strings(seqs_fa[1][:200])
    a_names, b_names = ["cluster-0.icm", "s1_w15_d7"], ["c3_p1_d5_w9", "cluster-0.icm", "s1_w15_d7"]
    stream = C.c_void_p()
    gpu.api._ck(lib.gmg_stream_create(C.byref(stream)))
    try:
        with gpu.ModelSet.load([open(members[n][0], "rb").read() for n in a_names]) as a:
            a.finish()
            b = gpu.ModelSet.load([open(members[n][0], "rb").read() for n in b_names], stream=stream)       # queued, not waited for
            got_a = gpu.score_reads_strings([a.model(k) for k in range(len(a))], reads)
            b.finish()
            got_b = gpu.score_reads_strings([b.model(k) for k in range(len(b))], reads)
            b.close()
        assert np.array_equal(got_a, gpu.score_reads_strings([members[n][1] for n in a_names], reads))
        assert np.array_equal(got_b, gpu.score_reads_strings([members[n][1] for n in b_names], reads))
    finally:
        gpu.api._ck(lib.gmg_stream_destroy(stream))


# ------------------------------------------------------------------------------------------------------------------------------
# phymm_gpu: the device loader (default) against --host-load on a synthetic .genomeData (the layout of tests/test_gpu_phymm.py)
# ------------------------------------------------------------------------------------------------------------------------------
LAYOUT = {
    "HP_strainA/NC_000915.icm": "NC_000915.icm",
    "HP_strainA/cluster-0.icm": "cluster-0.icm",
    "HP_strainA/cluster-0.gene.icm": "cluster-1.icm",          # skipped: ".gene."
    "B_strain/NC_100001.icm": "cluster-1.icm",
    "B_strain/NC_100002.x.icm": "cluster-2.icm",
    "B_strain/NC_100003.icm": "cluster-0.icm",
    "C_strain/NC_200001.icm": "cluster-3.icm",                  # its whole directory is ignored
    "D_strain/NC_300001.icm": "cluster-4.icm",
    "D_strain/NC_300002.icm": "cluster-5.icm",                  # ignored by its full path
    ".userAdded/U_strain/NC_500001.icm": "cluster-5.icm",
    ".userAdded/U_strain/NC_500002.icm": "cluster-4.icm",
}
IGNORE = "C_strain\n.genomeData/D_strain/NC_300002.icm\n"


def test_phymm_gpu_writes_the_same_files_with_either_loader(gmg, tmp_path_factory, tmp_path):
    exe = po.phymm_binary(str(tmp_path_factory.mktemp("phymm_bin")))
    for link, model in LAYOUT.items():
        p = tmp_path / ".genomeData" / link
        os.makedirs(p.parent, exist_ok=True)
        os.symlink(os.path.join(DATA, model), p)
    (tmp_path / "ignore.txt").write_text(IGNORE)
    os.symlink(os.path.join(DATA, "seqs.fa"), tmp_path / "seqs.fa")
    icms = po.icm_list(str(tmp_path), "icm", IGNORE.splitlines())
    assert len(icms) == 8
    env = dict(os.environ, LD_LIBRARY_PATH=os.path.join(ROOT, "glimmer-mg_amd", "lib"))

    def run(*args):
        res = subprocess.run([exe, *args, "-i", "ignore.txt", "seqs.fa"], cwd=tmp_path, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                             text=True, timeout=300)
        assert res.returncode == 0, res.stderr
        out = (tmp_path / "rawPhymmOutput_seqs_fa.txt").read_bytes(), (tmp_path / "seqs.class.txt").read_bytes()
        os.remove(tmp_path / "rawPhymmOutput_seqs_fa.txt")
        os.remove(tmp_path / "seqs.class.txt")
        return out

    want = run("--host-load")
    assert want[0].startswith(b"BEGIN_ICM_LIST\n") and want[1].count(b"\n") == want[0].split(b"BEGIN_READID_LIST\n")[1].split(b"END_READID_LIST")[0].count(b"\n")
    for batch in ("1", "3", str(len(icms))):
        assert run("--batch-models", batch) == want, batch
        assert run("--batch-models", batch, "--host-load") == want, batch
    # a bad file dies with its path and the reader's message, with either loader
    bad = tmp_path / ".genomeData" / "B_strain" / "NC_100004.icm"
    bad.write_bytes(open(os.path.join(DATA, "cluster-1.icm"), "rb").read()[:HEAD + REC * 1000 + 10])
    for args in ([], ["--host-load"]):
        res = subprocess.run([exe, *args, "-i", "ignore.txt", "seqs.fa"], cwd=tmp_path, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                             text=True, timeout=300)
        assert res.returncode != 0 and ".genomeData/B_strain/NC_100004.icm" in res.stderr and "ERROR reading icm node = " in res.stderr, res.stderr
