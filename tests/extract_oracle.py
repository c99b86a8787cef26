"""Python restatement of what extract / multi-extract followed by build-icm's Subscript do (tests only): Fasta_Read's records, the
reference's complement of a letter, the 2-bit code of a letter, the strings of regions in character space and in code space.
Written from the semantics in include/gmg.h, not from the library's code."""
import hashlib
import os

import numpy as np

from conftest import GOLD, DATA                          # noqa: F401

EX = os.path.join(GOLD, "extract")

# Complement (ch): the IUPAC pairs keep their case; any other letter, digit or punctuation gives 'n', except the five characters
# the table leaves alone
_PAIRS = {"a": "t", "c": "g", "g": "c", "t": "a", "r": "y", "y": "r", "k": "m", "m": "k", "b": "v", "v": "b", "d": "h", "h": "d",
          "s": "s", "w": "w", "n": "n"}


def complement(ch):
    if ch in " *-._":
        return ch
    low = ch.lower()
    if low in _PAIRS and ch.isalpha() and ord(ch) < 128:
        c = _PAIRS[low]
        return c.upper() if ch.isupper() else c
    return "n"


def code(ch):
    """Subscript (ch) = code (tolower (Filter (ch))): a 0, c 1, g 2, t 3; r, d -> g; w, k -> t; everything else -> c"""
    return {"a": 0, "c": 1, "g": 2, "r": 2, "d": 2, "t": 3, "w": 3, "k": 3}.get(ch.lower() if ord(ch) < 128 else "n", 1)


def records(data):
    """[(first header token or b'', sequence str)] of a FASTA file's bytes by the rules gmg_fasta_ingest applies: a '>' outside a
    header line starts a record, the header ends with its line, every later byte that is neither '>' nor white space is a base"""
    out, state, hdr = [], "pre", bytearray()
    for b in bytes(data):
        ch = chr(b)
        if ch == ">":
            if state != "hdr":
                out.append([None, []])
                hdr = bytearray()
                state = "hdr"
            else:
                hdr.append(b)
        elif state == "hdr":
            if ch == "\n":
                out[-1][0] = bytes(hdr)
                state = "seq"
            else:
                hdr.append(b)
        elif state == "seq" and ch not in " \t\n\r\x0b\x0c":
            out[-1][1].append(ch)
    for r in out:
        if r[0] is None:
            r[0] = bytes(hdr)
    return [(h, "".join(s)) for h, s in out]


def ambiguous(data):
    """(job-wide base indices, Subscript (Complement (letter))) of every base outside acgtACGT"""
    base, rev, k = [], [], 0
    for _, s in records(data):
        for ch in s:
            if ch not in "acgtACGT":
                base.append(k)
                rev.append(code(complement(ch)))
            k += 1
    return np.array(base, np.uint64), np.array(rev, np.uint8)


def parse_out(path):
    """the records extract / multi-extract printed: [(header fields, sequence)]"""
    out = []
    for line in open(path).read().splitlines():
        if line.startswith(">"):
            out.append([line[1:].split(), []])
        else:
            out[-1][1].append(line)
    return [(h, "".join(s)) for h, s in out]


def recorded(name):
    """[(header fields, length, sha256 of the letters)] of a recorded run: from its text (*.out) or, where no test needs the
    text itself, from the digests kept in its place (*.sha256: header fields, a tab, the digest of the record's letters)"""
    path = os.path.join(EX, name)
    if name.endswith(".out"):
        rows = [(h, hashlib.sha256(t.encode()).hexdigest()) for h, t in parse_out(path)]
    else:
        rows = [(line.split("\t")[0].split(), line.split("\t")[1]) for line in open(path).read().splitlines()]
    return [(h, int(h[-1].split("=")[1]), d) for h, d in rows]


def sha(text):
    return hashlib.sha256(text.encode()).hexdigest()


def region_chars(seq, first, n, strand):
    """what the reference prints for a region: the letters upwards, or Complement of the letters downwards, modulo the sequence"""
    L = len(seq)
    if strand > 0:
        return "".join(seq[(first + i) % L] for i in range(n))
    return "".join(complement(seq[(first - i) % L]) for i in range(n))


def region_codes(codes, first, n, strand, patches=None, base0=0):
    """the same in code space: 3 - code downwards, except where patches {job-wide base: code} says otherwise"""
    L = len(codes)
    if strand > 0:
        return [codes[(first + i) % L] for i in range(n)]
    out = []
    for i in range(n):
        p = (first - i) % L
        out.append(patches[base0 + p] if patches and base0 + p in patches else 3 - codes[p])
    return out


def parse_coords(path, multi=False):
    """coordinate lines as the reference's sscanf reads them: (tag, start, end[, dir]) or with multi (id, tag, start, end[, dir])"""
    rows = []
    for line in open(path).read().splitlines():
        f = line.split()
        k = 2 if multi else 1
        rows.append(tuple(f[:k]) + (int(f[k]), int(f[k + 1])) + ((int(f[k + 2]),) if len(f) > k + 2 and _is_int(f[k + 2]) else ()))
    return rows


def _is_int(s):
    try:
        int(s)
        return True
    except ValueError:
        return False


def unpack(packed, off):
    """the strings of a downloaded batch as lists of codes"""
    packed = np.asarray(packed, np.uint32)
    total = int(off[-1])
    if total == 0:
        return [[] for _ in range(len(off) - 1)]
    idx = np.arange(total, dtype=np.uint64)
    flat = (packed[(idx >> np.uint64(4)).astype(np.int64)] >> ((idx & np.uint64(15)) * np.uint64(2)).astype(np.uint32)) & np.uint32(3)
    return [flat[int(off[k]):int(off[k + 1])].tolist() for k in range(len(off) - 1)]


def pack(strings):
    """code lists -> (packed words with one zero guard word, offsets), the layout gmg_reads_upload takes"""
    off = np.zeros(len(strings) + 1, np.uint64)
    off[1:] = np.cumsum([len(s) for s in strings])
    total = int(off[-1])
    flat = np.zeros(((total + 15) // 16 + 1) * 16, np.uint32)
    if total:
        flat[:total] = np.concatenate([np.asarray(s, np.uint32) for s in strings if len(s)])
    words = (flat.reshape(-1, 16) << (2 * np.arange(16, dtype=np.uint32))).sum(axis=1, dtype=np.uint64).astype(np.uint32)
    return words, off
