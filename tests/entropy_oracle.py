"""The entropy distance ratio of long-orfs / glimmer3 -E restated in Python (test infrastructure): Entropy_Distance_Ratio
(src/Glimmer/long-orfs.cc:301-351), Counts_To_Entropy_Profile (src/Common/gene.cc:1095-1135), Codon_Translation (gene.cc:1016-1080,
its answers read from tests/golden/codon_translation.txt), Forward_Strand_Transfer / Reverse_Strand_Transfer (gene.cc:1237-1260,
1533-1556) and Filter (gene.cc:1139-1175).  math.log / math.pow / math.sqrt are the C library's, the functions the reference calls;
every sum runs in index order."""
import math
import os

import numpy as np

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
AMINO = "ACDEFGHIKLMNPQRSTVWY"                           # the letters IS_AMINO marks, in count order
CODES = (0, 1, 2, 3, 4, 5, 6, 9, 10, 11, 12, 13, 14, 15, 16, 21, 22, 23)
# DEFAULT_POS_ENTROPY_PROF / DEFAULT_NEG_ENTROPY_PROF (src/Common/gene.hh:47-52)
POS = (0.08468, 0.01606, 0.05739, 0.05752, 0.04328, 0.07042, 0.02942, 0.05624, 0.04442, 0.05620,
       0.03029, 0.03975, 0.05116, 0.04098, 0.05989, 0.08224, 0.05660, 0.06991, 0.02044, 0.03310)
NEG = (0.07434, 0.03035, 0.05936, 0.04729, 0.05662, 0.07704, 0.05777, 0.05328, 0.03360, 0.05581,
       0.01457, 0.03718, 0.04594, 0.05977, 0.08489, 0.05990, 0.04978, 0.07227, 0.01050, 0.01974)
_FILTER = {"a": "a", "c": "c", "g": "g", "t": "t", "r": "g", "y": "c", "s": "c", "w": "t", "m": "c", "k": "t",
           "b": "c", "d": "g", "h": "c", "v": "c"}
_COMP = {"a": "t", "c": "g", "g": "c", "t": "a"}
_tables = None


def tables():
    """code -> the 64 letters of Codon_Translation, index 16*b0 + 4*b1 + b2 with a=0 c=1 g=2 t=3 (the reference's `sub`)"""
    global _tables
    if _tables is None:
        _tables = {}
        with open(os.path.join(GOLD, "codon_translation.txt")) as fh:
            for line in fh:
                code, letters = line.split()
                assert len(letters) == 64
                _tables[int(code)] = letters
    return _tables


def filter_seq(seq):
    """Filter (tolower (ch)) of every character, as the reference's loaders apply it"""
    return "".join(_FILTER.get(ch, "c") for ch in seq.lower())


def region_bases(seq, first, length, strand):
    """the `length` bases from 0-based `first`: upwards (strand > 0) or downwards and complemented, modulo len(seq)"""
    n = len(seq)
    assert 0 <= first < n
    if strand > 0:
        return "".join(seq[(first + i) % n] for i in range(length))
    return "".join(_COMP[seq[(first - i) % n]] for i in range(length))


def counts(seq, first, length, strand, aa):
    """the 20 amino-acid counts of a region of a filtered sequence under the 64-letter table aa"""
    buf = region_bases(seq, first, length, strand)
    out = [0] * 20
    for i in range(0, length, 3):
        codon = buf[i:i + 3]
        if len(codon) < 3:                               # the reference reads the string's NUL there: 'X'
            continue
        letter = aa["acgt".index(codon[0]) * 16 + "acgt".index(codon[1]) * 4 + "acgt".index(codon[2])]
        k = AMINO.find(letter)
        if letter != "*" and k >= 0:
            out[k] += 1
    return out


def finish(count, pos=POS, neg=NEG):
    """Counts_To_Entropy_Profile + the distances and the ratio -> (pos_dist, neg_dist, ratio)"""
    total = 0.0
    for c in count:
        total += int(c)
    if total == 0.0:
        ep = [0.0] * 20
    else:
        ep = [int(c) / total for c in count]
        s = 0.0
        for j in range(20):
            ep[j] = 0.0 if ep[j] <= 0.0 else -1.0 * ep[j] * math.log(ep[j])
            s += ep[j]
        ep = [e / s if s != 0.0 else float("nan") for e in ep]      # 0 / 0: NaN in C, an exception in Python
    pd = nd = 0.0
    for j in range(20):
        pd += math.pow(ep[j] - pos[j], 2)
        nd += math.pow(ep[j] - neg[j], 2)
    pd, nd = math.sqrt(pd), math.sqrt(nd)
    if nd == 0.0:
        return pd, nd, 1.0 if pd == 0.0 else 1e3
    return pd, nd, pd / nd


def finish_rows(count_rows, pos=POS, neg=NEG):
    return np.array([finish(c, pos, neg) for c in count_rows], np.float64).reshape(-1, 3)


def orf_region(stop_position, gene_len, frame, n):
    """Entropy_Filter's region of an ORF (long-orfs.cc:370-377) -> (first, len, strand), first 0-based"""
    start = stop_position - gene_len if frame > 0 else stop_position + gene_len + 2
    while start < 1:                                     # On_Seq_1
        start += n
    while n < start:
        start -= n
    return start - 1, gene_len, 1 if frame > 0 else -1


def longorfs_rows(path):
    """the coordinate rows of a long-orfs output -> [(start, stop, frame, ratio text)]"""
    rows = []
    with open(path) as fh:
        for line in fh:
            f = line.split()
            if len(f) == 5 and f[0].isdigit() and f[3][0] in "+-":
                rows.append((int(f[1]), int(f[2]), int(f[3]), f[4]))
    return rows


def row_region(start, stop, frame, n):
    """the region Output_Orfs scored for a row WITH its stop codon (long-orfs.cc:1092-1118) -> (first, len, strand)"""
    length = ((stop - start) if frame > 0 else (start - stop)) % n - 2
    return start - 1, length, 1 if frame > 0 else -1
