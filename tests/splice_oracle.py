"""What the tests of gmg_edits_plan / gmg_reads_splice / extract-aa_gpu share (tests only): the two input files as
scripts/extract_aa.py reads them, the letters outside upper-case ACGT, and the expansion of a plan's runs -- over the letters of
the reads into the text of a .ffn file, over the codes of the reads into the strings of a spliced batch.  Written from the
semantics in include/gmg.h, not from the library's code."""
import hashlib
import os

import numpy as np

from conftest import GOLD, DATA

XA = os.path.join(GOLD, "extract_aa")
UP, DOWN, SUB_UP, SUB_DOWN, LITERAL, LITERAL_AS_IS = 0, 1, 2, 3, 4, 8
_RC = str.maketrans("ATCGatcg", "TAGCtagc")

# name -> (sequence file, predict file): the three recorded runs that cover every read of seqs.fa, and the synthetic case
CASES = {
    "glimmer-mg.indel": (os.path.join(DATA, "seqs.fa"), os.path.join(GOLD, "predict", "glimmer-mg.indel.predict")),
    "glimmer-mg.sub": (os.path.join(DATA, "seqs.fa"), os.path.join(GOLD, "predict", "glimmer-mg.sub.predict")),
    "classes.indel": (os.path.join(DATA, "seqs.fa"), os.path.join(GOLD, "predict", "classes.indel.predict")),
    "edges": (os.path.join(XA, "edges.fa"), os.path.join(XA, "edges.predict")),
}


def recorded_text(name, ext):
    """the bytes of a file the script wrote, where they are kept as text (the synthetic case), else None"""
    path = os.path.join(XA, name + ext)
    return open(path, "rb").read() if os.path.exists(path) else None


def assert_recorded(name, ext, data):
    """data is, byte for byte, the file the script wrote: against its text, or against its SHA-256 in recorded.sha256 where only
    that is kept (tests/golden/make_extract_aa.py writes both; run it to get the text of a file that differs)"""
    data = bytes(data)
    digests = dict(line.split()[::-1] for line in open(os.path.join(XA, "recorded.sha256")))
    want = recorded_text(name, ext)
    if want is not None:
        if data != want:
            g, w = data.split(b"\n"), want.split(b"\n")
            k = next((i for i in range(min(len(g), len(w))) if g[i] != w[i]), min(len(g), len(w)))
            raise AssertionError("%s%s line %d (%r):\n got %r\nwant %r" % (name, ext, k + 1, w[k - 1] if k % 2 and k < len(w) else b"",
                                                                           g[k] if k < len(g) else None, w[k] if k < len(w) else None))
    else:
        assert name + ext in digests, "no recorded output %s%s" % (name, ext)
    if name + ext in digests:
        assert hashlib.sha256(data).hexdigest() == digests[name + ext], "%s%s differs from the script's file (%d bytes here)" % (name, ext, len(data))


def script_ffn(gmg, name):
    """the .ffn text the script wrote for a case, as bytes: the kept file, or -- where only its SHA-256 is kept -- the expansion of
    gmg_edits_plan's runs over the letters of the sequence file (host only), which IS that text once it has the recorded digest"""
    want = recorded_text(name, ".ffn")
    if want is None:
        fasta = read_fasta(CASES[name][0])
        headers, seqs = [h for h, _ in fasta], [s for _, s in fasta]
        genes = parse_predict(CASES[name][1], headers)
        want = ffn_text(headers, seqs, genes, *gmg.edits_plan(offsets(seqs), genes, odd_letters(seqs))).encode()
        assert_recorded(name, ".ffn", want)
    return want


def read_fasta(path):
    """[(header, letters)] as the script reads the file: the line behind '>' and the other lines, right-stripped"""
    out = []
    for line in open(path):
        if line[0] == ">":
            out.append([line[1:].rstrip(), ""])
        else:
            out[-1][1] += line.rstrip()
    return [(h, s) for h, s in out]


def parse_predict(path, headers):
    """gene lines in file order: [(read, column 2, column 3, frame, insertions, deletions, substitutions)], positions as written"""
    index = {h: k for k, h in enumerate(headers)}
    genes, read = [], None
    for line in open(path):
        if line[0] == ">":
            read = index[line[1:].rstrip()]
            genes = [g for g in genes if g[0] != read]   # (a header that comes again starts over, as the script's dict does)
            continue
        a = line.split()
        lists = [[int(x) for x in f[2:].split(",")] if len(f) > 2 else [] for f in a[5:8]]
        genes.append((read, int(a[1]), int(a[2]), int(a[3]), lists[0], lists[1], lists[2]))
    return genes


def offsets(seqs):
    return np.concatenate([[0], np.cumsum([len(s) for s in seqs])]).astype(np.uint64)


def odd_letters(seqs):
    """(job-wide base indices, letters) of every base that is no upper-case A C G T"""
    base, letters, k = [], bytearray(), 0
    for s in seqs:
        for ch in s:
            if ch not in "ACGT":
                base.append(k)
                letters.append(ord(ch))
            k += 1
    return np.array(base, np.uint64), bytes(letters)


def run_text(seqs, run):
    read, first, n, kind = (int(x) for x in run)
    if kind >= LITERAL_AS_IS:
        return seqs[read][first] * n
    if kind >= LITERAL:
        return "ACGT"[kind & 3] * n
    s = seqs[read]
    text = s[first:first + n] if kind in (UP, SUB_UP) else s[first - n + 1:first + 1][::-1]
    assert len(text) == n
    if kind in (SUB_UP, SUB_DOWN):
        text = "".join("G" if ch == "C" else "C" for ch in text)
    return text.translate(_RC) if kind in (DOWN, SUB_DOWN) else text


def ffn_text(headers, seqs, genes, runs, sro, rows):
    """the .ffn file of a plan: record names from the adjusted coordinates, strings from the runs and the pad counts"""
    out = []
    for k, (line, start, end, strand, front, behind) in enumerate(rows):
        text = "".join(run_text(seqs, r) for r in runs[int(sro[k]):int(sro[k + 1])])
        out.append(">%s_%d,%d_%s\n%s\n" % (headers[genes[line][0]], start, end, "+" if strand > 0 else "-", " " * front + text + " " * behind))
    return "".join(out)


def run_codes(reads, run):
    """a run over the 2-bit codes of the reads: 3 - code downwards; the substitution c -> g, anything else -> c, before that"""
    read, first, n, kind = (int(x) for x in run)
    if kind >= LITERAL:
        return [kind & 3] * n
    c = reads[read]
    codes = c[first:first + n] if kind in (UP, SUB_UP) else c[first - n + 1:first + 1][::-1]
    assert len(codes) == n
    if kind in (SUB_UP, SUB_DOWN):
        codes = [2 if x == 1 else 1 for x in codes]
    return [3 - x for x in codes] if kind in (DOWN, SUB_DOWN) else list(codes)


def spliced(reads, runs, sro, reversed=False):
    out = []
    for k in range(len(sro) - 1):
        w = [x for r in runs[int(sro[k]):int(sro[k + 1])] for x in run_codes(reads, r)]
        out.append(w[::-1] if reversed else w)
    return out
