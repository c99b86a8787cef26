"""Inputs for the tests of gmg_features_count (tests/test_gpu_features.py): the smallest batches at which the kernels can go wrong,
and the glue between the oracle's structures (tests/features_oracle.py) and the C ABI's.

A case is (seqs, lines): seqs = [(header, letters)] in file order, lines = [(header, a, b, frame)] the gene lines of a predict file
(1-based coordinates as glimmer prints them, the sign of `frame` the strand), in file order.
"""
import random

import numpy as np

import features_oracle as fo


def oracle_inputs(seqs, lines):
    sd = dict(seqs)
    assert len(sd) == len(seqs)
    genes = {}
    for hdr, a, b, frame in lines:
        genes.setdefault(hdr, []).append(fo.gene_of(["orf", str(a), str(b), str(frame)], len(sd[hdr])))
    return genes, sd


def abi_inputs(seqs, genes):
    """-> (letters of every read, [(read, strand, start, end, start_codon)] grouped by read, opaque base indices)"""
    index = {hdr: k for k, (hdr, _) in enumerate(seqs)}
    rows = [(index[hdr], g.strand, g.start, g.end, g.start_codon) for hdr, hgenes in genes.items() for g in hgenes]
    blob = "".join(s for _, s in seqs)
    opaque = np.array([i for i, ch in enumerate(blob) if ch not in "ACGT"], np.uint64)
    return [s for _, s in seqs], rows, opaque


def table_of(stats, max_overlap):
    """the oracle's stats in the layout of gmg_features_table: (lengths, starts, orient, orient_raw, [dist x 3])"""
    top = max(stats["lengths"].keys(), default=-1)
    lengths = np.array([stats["lengths"].get(l, 0) for l in range(top + 1)], np.int64)
    starts = np.array([stats["start_codons"][c] for c in fo.STARTS], np.int64)
    orient = np.array([float(stats["adj_orients"][o]) for o in fo.ORIENTS], np.float64)
    raw = np.array([float(stats["raw_orients"][o]) for o in fo.ORIENTS], np.float64)
    dist = []
    for o in fo.ORIENTS[:3]:
        d = stats["adj_dist"][o]
        dist.append(np.array([float(d.get(l, 0)) for l in range(-max_overlap, 1 + max(d.keys()))] if d else [], np.float64))
    return lengths, starts, orient, raw, dist


def same_table(got, want):
    """got: a gmg FeatureTable; want: table_of().  Integers equal, doubles bit-equal.  -> list of the fields that differ"""
    lengths, starts, orient, raw, dist = want
    bad = []
    if not np.array_equal(got.lengths, lengths):
        bad.append("lengths")
    if not np.array_equal(got.starts, starts):
        bad.append("starts")
    if got.orient.tobytes() != orient.tobytes():
        bad.append("orient %r != %r" % (got.orient.tolist(), orient.tolist()))
    if got.orient_raw.tobytes() != raw.tobytes():
        bad.append("orient_raw %r != %r" % (got.orient_raw.tolist(), raw.tolist()))
    for k in range(3):
        if got.dist[k].tobytes() != dist[k].tobytes():
            bad.append("dist[%d]" % k)
    return bad


def fill(L, codons, letter="C"):
    """a sequence of `letter` with the given {position: letters} written over it (a run of C holds no start or stop on either strand)"""
    s = [letter] * L
    for pos, text in codons.items():
        assert pos >= 0 and pos + len(text) <= L
        s[pos:pos + len(text)] = list(text)
    return "".join(s)


def at_rich(rng, L, opaque=0.0):
    s = rng.choices("ATGC", weights=(35, 35, 15, 15), k=L)
    for i in range(L):
        if rng.random() < opaque:
            s[i] = rng.choice(["N", "R", s[i].lower()])
    return "".join(s)


def random_lines(rng, hdr, L, n):
    out = []
    for _ in range(n):
        start0 = rng.randint(-3, L)
        end0 = rng.randint(max(start0, 0), L + 3)
        if rng.random() < 0.5:
            out.append((hdr, start0 + 1, end0, rng.choice((1, 2, 3))))
        else:
            out.append((hdr, end0, start0 + 1, -rng.choice((1, 2, 3))))
    return out


# ---- the hand-made batches --------------------------------------------------------------------------------------------------------

def tiny():
    """lengths 0, 1, 2, 3, 5, 6 with and without genes: only the pseudo-stops L, L + 1, L + 2 (and a stop at L - 3 = 0)"""
    seqs, lines = [], []
    for k, s in enumerate(["", "A", "TA", "TAA", "ATG", "ATGTA", "ATGTAA", "TAGATG", "TTGTGA"]):
        seqs.append(("g%d" % k, s))
        seqs.append(("n%d" % k, s))                     # the same letters, no gene line: adds nothing
        lines.append(("g%d" % k, 1, len(s), 1) if k % 2 == 0 else ("g%d" % k, len(s), 1, -1))
    seqs.append(("two", "ATGTAA"))
    lines += [("two", -1, 3, 2), ("two", 9, 4, -3)]      # both ends outside
    return seqs, lines


def ends_and_fronts():
    """a stop codon at 0 and at L - 3; frames that run off the front with ci = -1, -2, -3: the pseudo-start counts for lengths, and for
    the bins of the neighbours, not for starts"""
    s = fill(90, {0: "TAA", 30: "ATG", 40: "TTG", 50: "GTG", 60: "TAG", 67: "TGA", 74: "TAA", 87: "TAG"})
    return [("a", s), ("b", s[1:]), ("c", s[2:]), ("d", fo.rc(s))], \
           [("a", 76, 84, 1), ("b", 5, 20, 2), ("c", 80, 70, -1), ("d", 3, 11, 1), ("d", 60, 20, -2)]


def mostly_without_genes():
    """odd read lengths, so that reads start at every offset inside a packed word; most reads have no gene line"""
    rng = random.Random(11)
    seqs, lines = [], []
    for k in range(97):
        L = rng.choice((17, 33, 49, 21, 75, 131, 5, 1))
        seqs.append(("r%d" % k, at_rich(rng, L)))
        if k % 7 == 3:
            lines += random_lines(rng, "r%d" % k, L, rng.randint(1, 2))
    return seqs, lines


def gene_is_the_orf():
    """a gene whose end - 3 is a stop item (the item is dropped), alone and between two others"""
    s = fill(150, {3: "ATG", 18: "TAA", 40: "ATG", 70: "TAG", 100: "TTG", 130: "TGA"})
    return [("one", s), ("three", s)], [("one", 4, 21, 1), ("three", 4, 21, 1), ("three", 41, 73, 2), ("three", 101, 133, 3)]


def overlaps():
    """run under max_overlap 11, 12, 13 and 16.  `suc`: a stop at 69 inside a gene that starts at 60: succeeding overlap 12, with starts
    upstream.  `pre`: a gene that ends at 60, starts at 47 and 44 in another frame whose stop lies behind the gene: preceding overlaps 13
    and 16, one on either side of the cut for 13 <= max_overlap < 16."""
    suc = fill(140, {9: "ATG", 24: "GTG", 39: "ATG", 60: "ATG", 69: "TAG", 108: "TAA"})
    pre = fill(140, {30: "ATG", 57: "TAA", 44: "ATGATG", 62: "TAA", 20: "TAG"})
    return [("suc", suc), ("pre", pre), ("suc_rc", fo.rc(suc)), ("pre_rc", fo.rc(pre))], \
           [("suc", 61, 111, 1), ("pre", 31, 60, 1), ("suc_rc", 140 - 60, 140 - 111 + 1, -1), ("pre_rc", 140 - 30, 140 - 60 + 1, -1)]


def nested_and_unordered():
    """nested genes and genes out of positional order in the file: the ends are not monotone, their prefix maximum is"""
    rng = random.Random(5)
    L = 600
    s = at_rich(rng, L)
    lines = [("x", 11, 400, 1), ("x", 41, 100, 2), ("x", 380, 120, -1), ("x", 450, 520, 3), ("x", 300, 330, 1), ("x", 590, 530, -2),
             ("x", 20, 29, 1)]
    return [("x", s), ("y", s)], lines + [("y", 500, 560, 1), ("y", 100, 10, -1), ("y", 130, 300, 2)]


def single_gene():
    rng = random.Random(6)
    return [("solo", at_rich(rng, 333))], [("solo", 100, 201, 1)]


def opaque_letters():
    """N, R and lower-case letters in every codon position of a start and of a stop, on both strands; genes whose start codon holds one"""
    fwd = fill(240, {0: "TAA", 6: "NTG", 12: "ANG", 18: "ATN", 24: "atg", 30: "ATG", 36: "RAA", 42: "TRA", 48: "TAR", 54: "taa", 60: "TAG",
                     66: "ATN", 99: "TAA", 120: "aTG", 150: "TGA", 170: "CAT", 180: "CAN", 190: "cat", 200: "TTA", 210: "TNA", 231: "TAG"})
    seqs = [("f", fwd), ("r", fo.rc(fwd)), ("plain", fwd.upper().replace("N", "A").replace("R", "G"))]
    lines = [("f", 67, 102, 1), ("f", 121, 153, 2), ("f", 31, 63, 3), ("f", 192, 160, -1), ("r", 20, 80, 1), ("r", 174, 139, -1),
             ("plain", 67, 102, 1), ("plain", 192, 160, -1)]
    return seqs, lines


def starts_read(n_starts, gene_strand):
    """400 bases: a closed ORF with n_starts ATGs, all of them long enough, in front of one gene: one item with num_starts = n_starts"""
    codons = {21: "TAA", 24 + 3 * (n_starts + 40): "TAG"}
    for k in range(n_starts):
        codons[24 + 3 * k] = "ATG"
    return fill(400, codons), (201, 320, 1) if gene_strand > 0 else (320, 201, -1)


def six_starts():
    """one item with six starts in front of a reverse-strand gene: the (1,-1) bins take six terms of 1/6, whose sum in order is
    0.9999999999999999 -- printed 0 by %d -- and 1.0 when added pairwise"""
    s, g = starts_read(6, -1)
    return [("six", s)], [("six",) + g]


def many_starts():
    """items with num_starts = 3, 6, 7 and 10 feeding the same bins"""
    seqs, lines = [], []
    for k, (n, strand) in enumerate([(3, 1), (6, -1), (7, -1), (10, 1), (3, -1), (7, 1), (10, -1), (6, 1), (3, -1)]):
        s, g = starts_read(n, strand)
        seqs.append(("m%d" % k, s))
        lines.append(("m%d" % k,) + g)
    return seqs, lines


def long_orf():
    """3,001 bases with an ORF of 420 codons, AT-rich around it"""
    rng = random.Random(3001)
    body = "ATG" + "".join(rng.choice(("GCT", "AAA", "CTG", "GAT", "ATG", "TTC", "GGC", "CAG")) for _ in range(419)) + "TAA"
    s = at_rich(rng, 700) + body + at_rich(rng, 3001 - 700 - len(body))
    assert len(s) == 3001
    return [("long", s)], [("long", 701, 700 + len(body), 1), ("long", 2600, 2201, -1), ("long", 100, 400, 2), ("long", 2990, 3004, 1)]


def differential():
    """300 random sequences of 0 - 900 bases, AT-rich so that ORFs run long, 0 - 4 random genes each, some letters opaque"""
    rng = random.Random(20261019)
    seqs, lines = [], []
    for k in range(300):
        L = rng.randint(0, 900)
        seqs.append(("d%d" % k, at_rich(rng, L, 0.004 if k % 3 == 0 else 0.0)))
        lines += random_lines(rng, "d%d" % k, L, rng.randint(0, 4))
    return seqs, lines


CASES = {"tiny": tiny, "ends_and_fronts": ends_and_fronts, "mostly_without_genes": mostly_without_genes, "gene_is_the_orf": gene_is_the_orf,
         "overlaps": overlaps, "nested_and_unordered": nested_and_unordered, "single_gene": single_gene, "opaque_letters": opaque_letters,
         "six_starts": six_starts, "many_starts": many_starts, "long_orf": long_orf, "differential": differential}

# (case, min_length, max_overlap, drop_tga)
RUNS = [("tiny", 75, 50, False), ("tiny", 0, 50, False), ("tiny", 0, 0, True),
        ("ends_and_fronts", 75, 50, False), ("ends_and_fronts", 0, 50, False), ("ends_and_fronts", 9, 50, True),
        ("mostly_without_genes", 75, 50, False), ("mostly_without_genes", 0, 0, False),
        ("gene_is_the_orf", 75, 50, False), ("gene_is_the_orf", 12, 50, False),
        ("overlaps", 15, 11, False), ("overlaps", 15, 12, False), ("overlaps", 15, 13, False), ("overlaps", 15, 16, False), ("overlaps", 0, 15, False),
        ("nested_and_unordered", 75, 50, False), ("nested_and_unordered", 30, 0, False),
        ("single_gene", 75, 50, False),
        ("opaque_letters", 75, 50, False), ("opaque_letters", 0, 50, False), ("opaque_letters", 0, 50, True),
        ("six_starts", 75, 50, False), ("many_starts", 75, 50, False), ("many_starts", 75, 200, False),
        ("long_orf", 75, 50, False), ("long_orf", 75, 50, True), ("long_orf", 0, 50, False), ("long_orf", 300, 50, False), ("long_orf", 75, 0, False),
        ("differential", 75, 50, False), ("differential", 0, 50, True), ("differential", 300, 0, False)]


def pairwise(terms):
    """the same terms added as a balanced tree"""
    terms = list(terms)
    while len(terms) > 1:
        terms = [terms[i] + terms[i + 1] if i + 1 < len(terms) else terms[i] for i in range(0, len(terms), 2)]
    return terms[0] if terms else 0.0
