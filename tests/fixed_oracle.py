"""CPU oracle of the fixed-length ICMs (Fixed_Length_ICM_t, src/ICM/icm.cc:1466-1836) for the tests: .fix parsing in Python,
training through the plain-C oracle's ICM trainer (oracle_py.train_model, one sub-model per prefix length) and a numpy restatement
of Score_Window / subrange_score over many windows at once (the descent of Full_Window_Prob, values added in double in
sub-model order)."""
import os
import struct

import numpy as np

ID_STRING_LEN = 150


def _sub_model(data, at):
    """one ICM_t in a .fix stream at byte `at` -> (mip int16 [N], prob float32 [N, 4], depth, model_len, periodicity, end)"""
    W, D, P, N = struct.unpack_from("<4i", data, at + ID_STRING_LEN + 8)
    at += ID_STRING_LEN + 24
    mip = np.zeros(P * N, np.int16)
    prob = np.zeros((P * N, 4), np.float32)
    present = np.zeros(P * N, bool)
    period = -1
    while True:
        (node,) = struct.unpack_from("<i", data, at)
        at += 4
        if node < 0:
            break
        if node == 0:
            period += 1
        prob[period * N + node] = np.frombuffer(data, np.float32, 4, at)
        (mip[period * N + node],) = struct.unpack_from("<h", data, at + 16)
        present[period * N + node] = True
        at += 18
    absent = ~present
    absent[np.arange(P) * N] = False
    mip[absent] = -2
    return mip, prob, D, W, P, at


def parse_fix(data):
    """-> dict(length, depth, special, type, perm, subs = [(mip, prob, depth)], header = the 150-byte line up to its NUL)"""
    version, idlen, L, depth, special, mtype = struct.unpack_from("<6i", data, ID_STRING_LEN)
    assert version == 200 and idlen == ID_STRING_LEN
    perm = list(struct.unpack_from("<%di" % L, data, ID_STRING_LEN + 24))
    at = ID_STRING_LEN + 24 + 4 * L
    subs = []
    for i in range(L):
        mip, prob, D, W, P, at = _sub_model(data, at)
        assert (W, P) == (i + 1, 1)
        subs.append((mip, prob, D))
    assert at == len(data)
    return {"length": L, "depth": depth, "special": special, "type": mtype, "perm": perm, "subs": subs,
            "header": data[:ID_STRING_LEN].split(b"\0")[0]}


def permute(s, perm):
    """Permute_String on bytes of at least len(perm) characters"""
    return bytes(s[p] for p in perm)


def train(orc, strings, L, max_depth, perm=None):
    """Fixed_Length_ICM_Training_t::Train_Model on the oracle's trainer -> subs [(mip, prob, depth)]"""
    lower = [orc.filter_lower(s) for s in strings]
    if perm is not None:
        lower = [permute(s, perm) for s in lower]
    subs = []
    for i in range(1, L + 1):
        d = min(i - 1, max_depth)
        m = orc.train_model([s[:i] for s in lower], W=i, D=d, P=1)
        mip, prob = orc.model_tables(m)
        subs.append((mip[0].astype(np.int16), prob[0].astype(np.float32), d))
    return subs


CODE = np.full(256, 1, np.uint8)          # tolower (Filter (ch)) then Subscript: every byte is a base ('\0' included)
for _c, _v in zip(b"acgtrdwk", (0, 1, 2, 3, 2, 2, 3, 3)):
    CODE[_c] = CODE[ord(chr(_c).upper())] = _v


def codes(windows):
    """list of bytes (each >= L characters) or uint8 array [n, >= L] of characters -> uint8 codes [n, L_max]"""
    if isinstance(windows, np.ndarray):
        return CODE[windows]
    n = max(len(w) for w in windows)
    a = np.zeros((len(windows), n), np.uint8)
    for k, w in enumerate(windows):
        a[k, :len(w)] = np.frombuffer(w, np.uint8)
    return CODE[a]


def score(subs, perm, win_codes, lo=0, hi=None):
    """subrange_score (lo, hi) of every window: win_codes uint8 [n, >= L] (the buffer B, codes 0..3) -> float64 [n]"""
    L = len(subs)
    hi = L if hi is None else hi
    P = win_codes[:, :L][:, np.asarray(perm, np.int64)].astype(np.int64)
    n = P.shape[0]
    rows = np.arange(n)
    total = np.zeros(n, np.float64)
    for i in range(lo, hi):
        mip, prob, D = subs[i]
        mip = mip.astype(np.int64)
        node = np.zeros(n, np.int64)
        active = np.ones(n, bool)
        for _ in range(D):
            pos = mip[node]
            active &= pos != -1
            up = active & (pos < -1)
            node[up] = np.where(node[up] > 0, (node[up] - 1) // 4, 0)
            active &= ~up
            a = np.nonzero(active)[0]
            node[a] = 4 * node[a] + P[a, pos[a]] + 1
        cut = mip[node] < -1
        node[cut] = np.where(node[cut] > 0, (node[cut] - 1) // 4, 0)
        total = total + prob[node, P[rows, i]].astype(np.float64)
    return total


def score_line(k, pos, neg, length, simple):
    """one line of score-fixed's output (score-fixed.cc:94-101)"""
    if simple:
        return "%6d %3d\n" % (k, 1 if pos >= neg else -1)
    ap, an = pos / length, neg / length
    return "%5d:  %10.4f %9.5f   %10.4f %9.5f   %9.5f\n" % (k + 1, pos, ap, neg, an, ap - an)


def read_fasta_strings(path):
    """score-fixed's Read_String: every non-space byte after a header line, up to the next '>'"""
    out = []
    for rec in open(path, "rb").read().split(b">")[1:]:
        out.append(b"".join(rec.split(b"\n", 1)[1].split()) if b"\n" in rec else b"")
    return out


# ---- the FASTA inputs of tests/golden/fixed, rebuilt from NC_000915.fna (tools/gen_golden_fixed.py records their sha256) ----

class Rng:
    """splitmix64: a fixed, library-independent stream, so that the inputs come out the same wherever they are rebuilt"""

    def __init__(self, seed):
        self.s = seed & 0xFFFFFFFFFFFFFFFF

    def below(self, n):
        self.s = (self.s + 0x9E3779B97F4A7C15) & 0xFFFFFFFFFFFFFFFF
        z = self.s
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & 0xFFFFFFFFFFFFFFFF
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & 0xFFFFFFFFFFFFFFFF
        return (z ^ (z >> 31)) % n

    def permutation(self, n):
        p = list(range(n))
        for i in range(n - 1, 0, -1):
            j = self.below(i + 1)
            p[i], p[j] = p[j], p[i]
        return p


def _mess(s, rng, k):
    """string k of a set: every third one lower case, every seventh one with an ambiguity code"""
    s = bytearray(s.lower() if k % 3 == 0 else s)
    if k % 7 == 3:
        s[rng.below(len(s))] = b"nNryswmkbdhv"[rng.below(12)]
    return bytes(s)


def _fasta(seqs, prefix):
    out = []
    for k, s in enumerate(seqs):
        out.append(b">%s%d\n" % (prefix.encode(), k))
        out.extend(s[i:i + 60] + b"\n" for i in range(0, len(s), 60))
    return b"".join(out)


INPUT_LENGTHS = (1, 2, 12, 24, 32)


def make_inputs(fna, out_dir):
    """train_<L>.fa for L in INPUT_LENGTHS (3000 windows of the genome, mixed case, a few ambiguity codes), score.fa (400 strings of
    24 - 40 characters, some with '*' or '5'), short.fa (a 20-base string among score.fa's first 40), bad_len.fa (training strings
    of two lengths) -> {file name: path}"""
    g = b"".join(line.strip() for line in open(fna, "rb") if not line.startswith(b">"))
    rng = Rng(20261015)
    starts = [rng.below(len(g) - 64) for _ in range(3000)]
    files = {}
    for L in INPUT_LENGTHS:
        files["train_%d.fa" % L] = _fasta([_mess(g[s:s + L], rng, k) for k, s in enumerate(starts)], "t%d_" % L)
    sc = []
    for k in range(400):
        s = rng.below(len(g) - 64)
        w = bytearray(_mess(g[s:s + 24 + rng.below(17)], rng, k))
        if k % 50 == 11:
            w[rng.below(len(w))] = ord("*")
        if k % 50 == 23:
            w[rng.below(len(w))] = ord("5")
        sc.append(bytes(w))
    files["score.fa"] = _fasta(sc, "s")
    files["short.fa"] = _fasta(sc[:30] + [sc[30][:20]] + sc[31:40], "s")
    files["bad_len.fa"] = _fasta([g[s:s + 12] for s in starts[:20]] + [g[5:16]] + [g[s:s + 12] for s in starts[20:30]], "b")
    paths = {}
    for name, data in files.items():
        paths[name] = os.path.join(out_dir, name)
        with open(paths[name], "wb") as fp:
            fp.write(data)
    return paths
