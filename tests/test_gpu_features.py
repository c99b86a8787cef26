"""gmg_features_count against the sequential restatement of scripts/train_features.py (tests/features_oracle.py) on the smallest
batches at which the kernels can go wrong (tests/features_cases.py).  Integers equal, doubles bit-equal: no tolerance anywhere."""
import numpy as np
import pytest

import features_cases as fc
import features_oracle as fo

pytestmark = pytest.mark.gpu

_cases = {}


def case(name):
    if name not in _cases:
        seqs, lines = fc.CASES[name]()
        genes, sd = fc.oracle_inputs(seqs, lines)
        _cases[name] = (seqs, genes, sd) + fc.abi_inputs(seqs, genes)
    return _cases[name]


@pytest.fixture(scope="module")
def device_reads(gpu):
    """every case's batch, uploaded once"""
    held = {}

    def get(name):
        if name not in held:
            held[name] = gpu.Reads.from_strings(case(name)[3])
        return held[name]
    yield get
    for r in held.values():
        r.close()


@pytest.mark.parametrize("name,min_length,max_overlap,drop_tga", fc.RUNS, ids=["%s-l%d-o%d%s" % (n, l, o, "-z" if z else "") for n, l, o, z in fc.RUNS])
def test_counts_equal_the_restatement(gpu, device_reads, name, min_length, max_overlap, drop_tga):
    seqs, genes, sd, reads, rows, opaque = case(name)
    gs, ns = fo.count(genes, sd, min_length, max_overlap, drop_tga)
    got_g, got_n, info = gpu.features_count(device_reads(name), rows, opaque, min_length, max_overlap, drop_tga)
    assert fc.same_table(got_g, fc.table_of(gs, max_overlap)) == []
    assert fc.same_table(got_n, fc.table_of(ns, max_overlap)) == []
    # ... and the text made from the device's result is the script's
    text = gpu.features_format(got_g, "GENE", gpu.FEATURES_BLOCK, max_overlap) + gpu.features_format(got_n, "NON", gpu.FEATURES_BLOCK, max_overlap)
    assert text == fo.feature_file(gs, ns, max_overlap)


def terms_of(name, min_length=75, max_overlap=50):
    seqs, genes, sd, reads, rows, opaque = case(name)
    trace = []
    gs, ns = fo.count(genes, sd, min_length, max_overlap, False, trace)
    return ns, trace


def test_six_terms_of_a_sixth_are_added_in_order(gpu, device_reads):
    """the case is built so that the order decides a printed digit: checked on the CPU first, then asked of the device"""
    ns, trace = terms_of("six_starts")
    terms = [1.0 / n for o, d, n in trace if o == (1, -1)]
    assert [n for o, d, n in trace if o == (1, -1)] == [6] * 6
    in_order = 0.0
    for t in terms:
        in_order += t
    assert int(in_order) == 0 and int(fc.pairwise(terms)) == 1
    assert ns["raw_orients"][(1, -1)] == in_order
    seqs, genes, sd, reads, rows, opaque = case("six_starts")
    got_g, got_n, info = gpu.features_count(device_reads("six_starts"), rows, opaque)
    assert got_n.orient_raw[1] == in_order and info["n_records"] == 6
    assert "1,-1\t0\n" in gpu.features_format(got_n, "NON", gpu.FEATURES_ORIENTS)
    assert "35\t1.0\n" in gpu.features_format(got_n, "NON", gpu.FEATURES_DIST + 1)


def test_the_cases_hold_what_they_are_named_for():
    """num_starts 3, 6, 7 and 10 all occur; the overlap cuts fall where the batch puts them (CPU only)"""
    ns, trace = terms_of("many_starts")
    assert {n for o, d, n in trace} == {3, 6, 7, 10}
    counts = [len(terms_of("overlaps", 15, mo)[1]) for mo in (11, 12, 13, 16)]
    assert counts[0] < counts[1] < counts[2] < counts[3]
    seqs, genes, sd, reads, rows, opaque = case("long_orf")
    gs, ns = fo.count(genes, sd)
    assert max(ns["lengths"]) >= 400 and max(gs["lengths"]) >= 400


def test_reads_without_genes_add_nothing(gpu):
    seqs, genes, sd, reads, rows, opaque = case("mostly_without_genes")
    keep = [k for k, (hdr, _) in enumerate(seqs) if hdr in genes]
    renumber = {old: new for new, old in enumerate(keep)}
    sub = [reads[k] for k in keep]
    sub_rows = [(renumber[r], s, a, b, sc) for r, s, a, b, sc in rows]
    full, part = gpu.Reads.from_strings(reads), gpu.Reads.from_strings(sub)
    a = gpu.features_count(full, rows, opaque, 0, 50)
    b = gpu.features_count(part, sub_rows, None, 0, 50)
    for x, y in zip(a[:2], b[:2]):
        assert np.array_equal(x.lengths, y.lengths) and np.array_equal(x.starts, y.starts) and x.orient_raw.tobytes() == y.orient_raw.tobytes()
        assert all(p.tobytes() == q.tobytes() for p, q in zip(x.dist, y.dist))
    full.close()
    part.close()


def test_too_many_records_is_refused(gpu, device_reads, request_finalizers):
    seqs, genes, sd, reads, rows, opaque = case("differential")
    old = gpu.get_option("mg_max_entries")
    request_finalizers.append(lambda: gpu.set_option("mg_max_entries", old))
    gpu.set_option("mg_max_entries", 900)               # the 643 genes pass, the 996 records do not
    with pytest.raises(gpu.GmgError) as e:
        gpu.features_count(device_reads("differential"), rows, opaque)
    assert e.value.code == -7 and "records" in str(e.value)
    gpu.set_option("mg_max_entries", 100)
    with pytest.raises(gpu.GmgError) as e:
        gpu.features_count(device_reads("differential"), rows, opaque)
    assert e.value.code == -7
    gpu.set_option("mg_max_entries", old)
    gpu.features_count(device_reads("differential"), rows, opaque)


def test_bad_gene_lists_are_refused(gpu, device_reads):
    seqs, genes, sd, reads, rows, opaque = case("single_gene")
    r = device_reads("single_gene")
    for bad, code in (([(0, 1, 10, 400, 1)], -6), ([(0, 1, -1, 40, 1)], -6), ([(3, 1, 1, 40, 1)], -6), ([], -1)):
        with pytest.raises(gpu.GmgError) as e:
            gpu.features_count(r, bad, None)
        assert e.value.code == code
    two = gpu.Reads.from_strings(["ACGTACGTAA", "ACGTACGTAA"])
    with pytest.raises(gpu.GmgError) as e:              # the genes of a read must be consecutive
        gpu.features_count(two, [(0, 1, 0, 9, 1), (1, 1, 0, 9, 1), (0, -1, 0, 9, 1)], None)
    assert e.value.code == -1
    two.close()
