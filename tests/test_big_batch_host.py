"""The fixture of tests/test_gpu_big_batch.py, checked on the CPU (tests/big_batch.py): the reads fall where the layout says, the
filler holds no ORF, and -- the sensitivity condition -- every expectation the GPU module asserts changes when the source index is
taken modulo 2^32, and when it is taken modulo 2^31.  So a kernel that cuts a job-wide base index to 32 bits fails every one of
those tests; none of them can pass by accident of the probes."""
import os

import numpy as np
import pytest

import big_batch as bb
import entropy_oracle as eo
import fixed_oracle as fo
import windows_oracle as wo
from conftest import DATA

MODULI = (bb.M32, bb.M31)


@pytest.fixture(scope="module")
def layout():
    return bb.Layout()


@pytest.fixture(scope="module")
def views(layout):
    """{modulus or None: (strings, seen)}"""
    return {m: (layout.strings(m), [layout.index_of(j, m) for j in range(bb.N_PROBES)]) for m in (None,) + MODULI}


def _differs(a, b):
    """do two expectations differ (nested lists / tuples / arrays / numbers / dicts)?"""
    if isinstance(a, dict):
        return a.keys() != b.keys() or any(_differs(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return len(a) != len(b) or any(_differs(x, y) for x, y in zip(a, b))
    if isinstance(a, np.ndarray):
        return a.shape != np.shape(b) or a.tobytes() != np.asarray(b, a.dtype).tobytes()
    return a != b


def _sensitive(views, fn):
    """fn (strings, seen) gives another expectation under either modulus than with the true index"""
    true = fn(*views[None])
    for m in MODULI:
        assert _differs(true, fn(*views[m])), "the expectation does not notice a source index taken modulo 2^%d" % (m.bit_length() - 1)
    return true


def test_reads_fall_where_the_layout_says(layout):
    off, pr = layout.offsets, layout.probe_read
    assert layout.total == bb.M32 + bb.TAIL_FILL * bb.FILL + 2 * bb.GROUP_BASES - bb.BELOW[1] and layout.total > bb.M32
    assert layout.n_reads == 2 * 2048 + bb.TAIL_FILL + bb.N_PROBES
    lens = np.diff(off.astype(np.int64))
    assert lens.max() == bb.FILL < bb.M31                                     # no read has 2^31 bases
    assert np.all(lens[~layout.is_probe] % 4 == 0) and np.all(off[:-1][~layout.is_probe] % np.uint64(4) == 0)
    for slot, edge in ((0, bb.M31), (1, bb.M32)):
        first = pr[bb.K * slot]
        assert int(off[first]) == edge - bb.BELOW[slot] and int(off[first + 1]) == edge - bb.BELOW[slot] + 3000      # it straddles the edge
        assert not layout.is_probe[first - 1] and layout.is_probe[first]
    assert int(off[pr[2 * bb.K + bb.K - 1] + 1]) == layout.total and pr[-1] == layout.n_reads - 1      # the batch ends with a probe read
    for g in range(3):
        assert list(lens[pr[bb.K * g]:pr[bb.K * g] + bb.K]) == list(bb.GROUP_LENS)
        assert lens[pr[bb.K * g + 1]] == 0 and lens[pr[bb.K * g + 2]] == 0     # two empty reads side by side
    assert np.array_equal(off[pr], layout.probe_base.astype(np.uint64))


def test_packed_words_are_the_codes(layout):
    """the materialised words against codes_at on both sides of every group, at the batch's ends and at random places"""
    words = layout.packed()
    assert len(words) == (layout.total + 15) // 16 + 1 and words[-1] == 0
    rng = np.random.default_rng(3)
    g = [rng.integers(0, layout.total, 5000), np.arange(0, 4096), np.arange(layout.total - 4096, layout.total)]
    g += [np.arange(s - 64, s + bb.GROUP_BASES + 64) for s in layout.slot_start[:2]]
    g = np.concatenate(g).astype(np.int64)
    got = (words[g >> 4] >> (2 * (g & 15)).astype(np.uint32)) & 3
    assert np.array_equal(got, layout.codes_at(g))
    for j, s in enumerate(layout.strings()):
        assert np.array_equal(s, bb.probe_codes()[j])
    assert layout.total % 16 == 0 or words[layout.total // 16] >> (2 * (layout.total % 16)) == 0


def test_permuted_layout_keeps_the_geometry(layout):
    moved = bb.Layout((2, 0, 1))
    assert np.array_equal(moved.offsets, layout.offsets) and not np.array_equal(moved.probe_read, layout.probe_read)
    assert sorted(moved.probe_read) == sorted(layout.probe_read)
    for m in MODULI:                                     # the probes pulled out of the permuted batch notice a truncated index too
        assert _differs([s.tolist() for s in moved.strings()], [s.tolist() for s in moved.strings(m)])
    assert not _differs([s.tolist() for s in moved.strings()], [s.tolist() for s in layout.strings()])


def test_filler_holds_no_orf(oracle, layout):
    """taa in all three frames every 12 bases, the text its own reverse complement: no ORF in a filler read, alone or with its
    neighbours (the kernels see reads, the restatement here also sees three of them as one string)"""
    read = "ttaa" * (bb.FILL // 4)
    assert bb.revcomp(read[:48]) == read[:48]
    assert all(any(read[i:i + 3] == "taa" for i in range(f, f + 12, 3)) for f in range(3))
    for mgl in (bb.MIN_GENE_LEN, 75, 3):
        prm = oracle.mg_params(min_gene_len=mgl, allow_truncated=False)
        for s in (read, read[:bb.FILL - bb.BELOW[0]], read * 3):
            assert len(oracle.find_orfs_general(s, prm)) == 0
    assert text_of(layout, 1 << 20, 24) == "ttaa" * 6


def text_of(layout, g, n):
    return bb.text(layout.codes_at(np.arange(g, g + n)))


def test_filler_window_rows_closed_form():
    for L in (bb.FILL - 12316, 4000, 996, 1000):
        for filler in ("ttaa", "t"):
            s = (filler * L)[:L]
            want = np.array([c for _, _, c in wo.window_rows(s, bb.WINDOW, bb.SKIP)], np.int32).reshape(-1, 5)
            assert np.array_equal(bb.filler_windows(L, bb.WINDOW, bb.SKIP, filler), want)
    n_rows = sum(len(wo.closed_form_windows(int(n), bb.WINDOW, bb.SKIP)) for n in bb.Layout().lens)
    assert n_rows == bb.N_WINDOW_ROWS < 5_000_000        # 86 MB of rows: what the GPU test fetches


def test_all_t_batch_wraps_its_running_t_count():
    """in the all-t batch the count of t in front of a base passes 2^32 inside the filler read behind slot 1 (a group that begins
    2,100 bases below base 2^32 cannot have 2^32 t in front of it): that read's rows have a sum on either side of the wrap, and the
    whole of slot 2 lies behind it"""
    lay = bb.Layout(filler="t")
    t_in = [int((lay.group_codes[g] == 3).sum()) for g in range(3)]
    behind_slot1 = lay.slot_start[1] + bb.GROUP_BASES
    t_behind_slot1 = behind_slot1 - 2 * bb.GROUP_BASES + t_in[lay.slots[0]] + t_in[lay.slots[1]]
    assert t_behind_slot1 < bb.M32 < t_behind_slot1 + bb.FILL
    assert not lay.is_probe[lay.probe_read[bb.K * lay.slots[1] + bb.K - 1] + 1]


# ---- the sensitivity condition, one test per GPU test ---------------------------------------------------------------------------------

def test_sensitive_select_extract_splice(layout, views):
    _sensitive(views, lambda s, seen: bb.expect_select(s))
    for rev in (False, True):
        _sensitive(views, lambda s, seen: bb.expect_extract(layout, s, seen, rev))
        _sensitive(views, lambda s, seen: bb.expect_splice(s, rev))
    # the listed bases decide codes of the true expectation: without the list it is another one
    assert _differs(bb.expect_extract(layout, *views[None]), bb.expect_extract(layout, views[None][0], [np.full(len(x), -1) for x in views[None][1]]))


def test_sensitive_per_group(layout, views):
    """stronger than the condition asks: the regions of the group at 2^31 alone notice modulo 2^31, those of the two groups at and
    beyond 2^32 notice either modulus"""
    true, a32, a31 = (bb.expect_extract(layout, *views[m]) for m in (None, bb.M32, bb.M31))
    per = len(true) // 3
    for g in range(3):
        sl = slice(per * g, per * (g + 1))
        assert _differs(true[sl], a31[sl])
        assert (g == 0) != _differs(true[sl], a32[sl])


def test_sensitive_segment_scorers(oracle, views):
    model = oracle.read(os.path.join(DATA, "NC_000915.icm"))
    true = bb.expect_segments(oracle, model, views[None][0])
    for m in MODULI:
        per, allf = bb.expect_segments(oracle, model, views[m][0])
        for f in range(3):
            for k in range(4):                           # each of the four per-segment entry points on its own
                assert _differs([row[k] for row in true[0][f]], [row[k] for row in per[f]])
        assert _differs(true[1], allf)


def test_sensitive_fixed_score(oracle, views):
    g = open(os.path.join(DATA, "NC_000915.fna"), "rb").read().split(b"\n", 1)[1].replace(b"\n", b"")
    train = [g[s:s + bb.FIXED_L] for s in range(1000, 1000 + 600 * 37, 37)]
    subs = fo.train(oracle, train, bb.FIXED_L, 5, None)
    _sensitive(views, lambda s, seen: fo.score(subs, list(range(bb.FIXED_L)), bb.fixed_windows(s)))


def test_sensitive_strings_sums(oracle, views):
    model = oracle.read(os.path.join(DATA, "cluster-1.icm"))
    _sensitive(views, lambda s, seen: bb.expect_strings(oracle, model, s))


def test_sensitive_tophits(oracle, views):
    import phymm_oracle as po
    models = [oracle.read(os.path.join(DATA, "cluster-%d.icm" % i)) for i in (0, 1, 2)]
    true = _sensitive(views, lambda s, seen: list(po.tophits_numpy(po.merged_keys(np.stack([bb.expect_strings(oracle, m, s) for m in models])), 2)))
    assert len(set(true[1][:, 0].tolist())) > 1          # not one model for every read


def test_sensitive_orfs_and_entropy(oracle, views):
    lens = [bb.GROUP_LENS[j % bb.K] for j in range(bb.N_PROBES)]
    aa = eo.tables()[11]
    true = _sensitive(views, lambda s, seen: [o.tolist() for o in bb.expect_orfs(oracle, s)])
    assert sum(len(o) for o in true) >= 30
    _sensitive(views, lambda s, seen: bb.expect_entropy_counts(s, bb.orf_regions(bb.expect_orfs(oracle, views[None][0]), lens), aa))
    _sensitive(views, lambda s, seen: bb.expect_entropy_counts(s, bb.entropy_region_rows(), aa))


def test_sensitive_audit_windows_uncovered_features(layout, views):
    recs, inner, hist = _sensitive(views, lambda s, seen: bb.expect_audit(layout, s, seen))
    assert len(inner) > 50 and any(r["next_stop"] >= 0 for r in recs)
    rows = _sensitive(views, lambda s, seen: bb.expect_windows(layout, s, seen))
    assert sum(int(r[:, 4].sum()) for r in rows) > 0     # listed bases are counted as "other"
    true = bb.expect_uncovered(bb.seen_lengths(layout))
    for m in MODULI:
        assert _differs(true, bb.expect_uncovered(bb.seen_lengths(layout, m)))
    _sensitive(views, lambda s, seen: bb.expect_features(layout, s, seen))


# ---- tests/test_gpu_big_text.py ----------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def letter_views():
    lay = bb.LetterLayout()
    return lay, {m: lay.letter_strings(m) for m in (None,) + MODULI}


def test_letters_fall_where_the_layout_says(letter_views):
    lay, views = letter_views
    assert [len(s) for s in views[None]] == [bb.GROUP_LENS[j % bb.K] for j in range(bb.N_PROBES)]
    assert all(s == p.tobytes() for s, p in zip(views[None], bb.probe_letters()))
    assert lay.letters_at(np.arange(8)).tobytes() == b"ttaattaa" and lay.total % 4 == 0
    assert lay.letters_at(np.array([lay.slot_start[1] - 1, lay.slot_start[1]])).tobytes() == b"a" + views[None][bb.K * lay.slots[1]][:1]
    assert set(b"".join(views[None])) == set(bb.ALPHABET)


def test_sensitive_regions_text_and_runs_text(letter_views):
    """every parametrised case of the source-side tests: both widths, both modes"""
    _, views = letter_views
    for width in (0, 60):
        true = bb.expect_regions_text(views[None], width)
        assert len(true) > 2 * 16384                     # more than a work-group's tile of text
        for mode in (0, 1):
            true_runs = bb.expect_runs_text(views[None], mode, width)
            for m in MODULI:
                assert true != bb.expect_regions_text(views[m], width)
                assert true_runs != bb.expect_runs_text(views[m], mode, width)
    faa = bb.expect_runs_text(views[None], 1, 0)
    assert b"X" in faa and any(c in faa for c in b"acdefghiklmnpqrstvwy") and any(c in faa for c in b"ACDEFGHIKLMNPQRSTVWY")


def test_output_side_slices_notice_a_wrapped_text_offset():
    """the text of the output-side tests is longer than 2^32 bytes, the slices lie where they are said to lie, and what stands at
    a byte of the slices at and beyond 2^32 differs from what stands 2^32 bytes earlier (a text offset cut to 32 bits writes there)"""
    off = bb.out_record_offsets(bb.REGION_BODY)
    total = int(off[-1])
    assert total > bb.M32 and total < 10 * (1 << 30)
    (a31, n31), (a32, n32), (a_end, n_end) = bb.out_slices(total)
    assert a31 < bb.M31 < a31 + n31 and a32 < bb.M32 < a32 + n32 and a_end + n_end == total and a_end > bb.M32
    for record_of in (bb.out_region_record, bb.out_runs_record):
        k = 100_001
        assert len(record_of(k)) == int(off[k + 1] - off[k])
        for a, n in ((bb.M32, a32 + n32 - bb.M32), (a_end, n_end)):
            assert bb.expect_out_slice(off, record_of, a, n) != bb.expect_out_slice(off, record_of, a - bb.M32, n)
        assert bb.expect_out_slice(off, record_of, bb.M31, 4096) != bb.expect_out_slice(off, record_of, 0, 4096)
