"""A batch slightly longer than 2^32 bases, and what every entry point must return on it (tests only; no GPU here).

The layout.  Filler reads of exactly 2^20 bases of the period-4 text ttaattaa... (packed word 0x0F0F0F0F, so the filler is one np.full;
its own reverse complement; taa in all three frames every 12 bases, so Find_Orfs reports no ORF in it), a few shorter filler reads
(lengths that are multiples of 4) that position three groups of random reads over acgt, the PROBES:

    slot 0   begins 1,500 bases below base 2^31: its first read straddles 2^31
    slot 1   begins 2,100 bases below base 2^32: its first read straddles 2^32
    slot 2   the last reads of the batch: the guard words behind the data are reached

Every group holds reads of GROUP_LENS bases: the straddling read of 3,000 bases first, two empty reads side by side, the lengths
around a packed word and a tile, 5,000 bases for window rows, and 7 bases that bring the group to a multiple of 4 bases (the filler
behind a group then still begins in phase: any of its words that begins at a multiple of 4 is the same word).  Group g comes from
seed SEEDS[g]; a Layout says which group sits in which slot (the permuted layout of the write-side test moves them round).

The aliasing condition.  codes_at (g) answers the base of any job-wide index, the filler analytically.  strings (modulus) gives the
probe reads as a kernel would see them whose source index went through 32 bits: base B + p of a read is read from (B + p) mod 2^32,
or mod 2^31 -- the latter stands for an index that went through a signed 32-bit variable, except where such an index turns
negative, which would fault instead.  Every expectation of the GPU tests is a function of those strings (and, for the lists of
ambiguous bases, of the job-wide index each position is read from), so it can be produced three times: tests/test_big_batch_host.py
checks that the two aliased forms differ from the true one for every case -- a truncated index fails every GPU test.

Expectations come from the Python restatements (extract_oracle, splice_oracle, text_oracle, runs_text_oracle, windows_oracle,
audit_oracle, entropy_oracle, features_oracle, fixed_oracle, phymm_oracle) and the C oracle (oracle_py) applied to the probe strings,
never from the library.  The second half of the file is the same layout in letters and the output-side text cases of
tests/test_gpu_big_text.py."""
import numpy as np

import audit_oracle as ao
import entropy_oracle as eo
import extract_oracle as xo
import features_cases as fc
import features_oracle as feo
import splice_oracle as so
import windows_oracle as wo

M31, M32 = 1 << 31, 1 << 32
FILL = 1 << 20
GROUP_LENS = (3000, 0, 0, 1, 2, 15, 16, 17, 86, 500, 1023, 1024, 1025, 5000, 7)
K = len(GROUP_LENS)
GROUP_BASES = sum(GROUP_LENS)                            # 11,716
SEEDS = (9101, 9102, 9103)
BELOW = (1500, 2100)                                     # slot 0 begins BELOW[0] under 2^31, slot 1 BELOW[1] under 2^32
TAIL_FILL = 2                                            # whole filler reads between slot 1 and slot 2
N_PROBES = 3 * K
FWD, REV, COMP, REVCOMP = 0, 1, 2, 3
assert GROUP_BASES % 4 == 0 and all(b % 4 == 0 for b in BELOW)

_probe_codes = None


def probe_codes():
    """the 45 probe reads as uint8 code arrays (a 0, c 1, g 2, t 3): probe j = K * group + k"""
    global _probe_codes
    if _probe_codes is None:
        _probe_codes = []
        for seed in SEEDS:
            rng = np.random.default_rng(seed)
            _probe_codes += [rng.integers(0, 4, size=n).astype(np.uint8) for n in GROUP_LENS]
    return _probe_codes


def text(codes):
    return "".join("acgt"[c] for c in codes)


class Layout:
    """slots[s] = the probe group in slot s; filler "ttaa" or "t" """

    def __init__(self, slots=(0, 1, 2), filler="ttaa"):
        assert sorted(slots) == [0, 1, 2] and filler in ("ttaa", "t")
        self.slots, self.filler = tuple(slots), filler
        self.fill_word = 0x0F0F0F0F if filler == "ttaa" else 0xFFFFFFFF
        lens, self.probe_read, self.slot_start, self.is_probe = [], [0] * N_PROBES, [], []
        pos = 0

        def fill_to(target):
            nonlocal pos
            assert target >= pos and (target - pos) % 4 == 0
            whole, rest = divmod(target - pos, FILL)
            for n in [FILL] * whole + ([rest] if rest else []):
                lens.append(n)
                self.is_probe.append(False)
            pos = target

        def group(s):
            nonlocal pos
            self.slot_start.append(pos)
            for k, n in enumerate(GROUP_LENS):
                self.probe_read[K * self.slots[s] + k] = len(lens)
                lens.append(n)
                self.is_probe.append(True)
            pos += GROUP_BASES

        fill_to(M31 - BELOW[0])
        group(0)
        fill_to(M32 - BELOW[1])
        group(1)
        fill_to(pos + TAIL_FILL * FILL)
        group(2)
        self.lens = np.array(lens, np.uint64)
        self.offsets = np.zeros(len(lens) + 1, np.uint64)
        np.cumsum(self.lens, out=self.offsets[1:])
        self.n_reads, self.total = len(lens), int(self.offsets[-1])
        self.is_probe = np.array(self.is_probe)
        self.probe_read = np.array(self.probe_read, np.int64)
        self.probe_base = self.offsets[self.probe_read].astype(np.int64)      # job-wide index of base 0 of probe j
        codes = probe_codes()
        self.group_codes = [np.concatenate(codes[K * g:K * g + K]) for g in range(3)]

    def codes_at(self, g):
        """the codes of the job-wide indices g (any int array, all inside the batch)"""
        g = np.asarray(g, np.int64)
        assert g.size == 0 or (g.min() >= 0 and g.max() < self.total)
        out = np.where(g % 4 < 2, 3, 0).astype(np.uint8) if self.filler == "ttaa" else np.full(g.shape, 3, np.uint8)
        for s, start in enumerate(self.slot_start):
            m = (g >= start) & (g < start + GROUP_BASES)
            out[m] = self.group_codes[self.slots[s]][g[m] - start]
        return out

    def index_of(self, j, modulus=None):
        """the job-wide index every position of probe j is read from"""
        g = self.probe_base[j] + np.arange(GROUP_LENS[j % K], dtype=np.int64)
        return g if modulus is None else g % modulus

    def strings(self, modulus=None):
        """the probe reads (code arrays) as read through the job-wide index, or through that index modulo `modulus`"""
        return [self.codes_at(self.index_of(j, modulus)) for j in range(N_PROBES)]

    def packed(self):
        """the packed words of the whole batch (gmg_reads_upload's layout: one guard word behind the data)"""
        words = np.full((self.total + 15) // 16 + 1, self.fill_word, np.uint32)
        words[self.total // 16:] = 0
        tail = self.total % 16                           # (the batch ends with a probe read: no filler in the last word)
        for s, start in enumerate(self.slot_start):
            w0, w1 = start // 16, (start + GROUP_BASES + 15) // 16
            g = np.arange(16 * w0, 16 * w1, dtype=np.int64)
            inside = g < self.total
            c = np.zeros(len(g), np.uint32)
            c[inside] = self.codes_at(g[inside])
            words[w0:w1] = (c.reshape(-1, 16) << (2 * np.arange(16, dtype=np.uint32))).sum(axis=1, dtype=np.uint64).astype(np.uint32)
        assert tail == 0 or words[self.total // 16] >> (2 * tail) == 0
        return words

    def big(self, rows, col=0):
        """rows whose column `col` names a probe (the small batch's numbering) -> the same rows naming the read of this batch"""
        a = np.array(rows, np.int64).reshape(len(rows), -1)
        a[:, col] = self.probe_read[a[:, col]]
        return a

    def big_index(self, pairs):
        """[(probe, position)] -> job-wide indices in this batch, ascending"""
        return np.array(sorted(int(self.probe_base[j]) + p for j, p in pairs), np.uint64)


def small_offsets():
    off = np.zeros(N_PROBES + 1, np.uint64)
    off[1:] = np.cumsum([GROUP_LENS[j % K] for j in range(N_PROBES)])
    return off


def small_index(pairs):
    off = small_offsets()
    return np.array(sorted(int(off[j]) + p for j, p in pairs), np.uint64)


def filler_windows(L, W, S, filler="ttaa"):
    """the closed form of gmg_window_counts' rows for a filler read of L bases (a multiple of 4 that begins in phase)"""
    ws = wo.closed_form_windows(L, W, S)
    a = np.array([p - 1 for p, _ in ws], np.int64)
    e = a + np.array([n for _, n in ws], np.int64)
    rows = np.zeros((len(ws), 5), np.int32)
    if filler == "t":
        rows[:, 3] = e - a
    else:
        t_before = lambda x: 2 * (x // 4) + np.minimum(x % 4, 2)      # the t among bases 0 .. x - 1 of ttaattaa...
        rows[:, 3] = t_before(e) - t_before(a)
        rows[:, 0] = (e - a) - rows[:, 3]
    return rows


# ---------------------------------------------------------------------------------------------------------------------------------
# The cases.  Reads are named by probe number j = K * group + k (the small batch's read index); Layout.big () renumbers them.
# Every expect_* takes the probe strings as the kernel would see them (Layout.strings (modulus)) and, where a list of job-wide
# indices goes in, `seen` = for every probe the job-wide index each position is read from (Layout.index_of (j, modulus)).
# ---------------------------------------------------------------------------------------------------------------------------------

CROSS = {0: BELOW[0], 1: BELOW[1], 2: 1700}             # position of the straddling read at which 2^31 / 2^32 is crossed (slot 2: none)


def _per_group(fn):
    return [row for g in range(3) for row in fn(K * g, CROSS[g])]


def extract_regions():
    """(probe, first, len, strand): across 2^31 / 2^32 both ways, round the read's end both ways, whole reads of every length"""
    def rows(j0, x):
        out = [(j0, x - 40, 100, 1), (j0, x + 50, 120, -1), (j0, x - 1, 1, 1), (j0, x, 1, -1), (j0, 2990, 60, 1), (j0, 10, 60, -1),
               (j0, 0, 3000, 1), (j0, 2999, 3000, -1), (j0 + 13, 4990, 1025, 1), (j0 + 13, 3, 1040, -1)]
        for k in (3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 14):
            n = GROUP_LENS[k]
            out += [(j0 + k, 0, n, 1), (j0 + k, n - 1, n, -1), (j0 + k, n // 2, n, 1)]
        return out
    return _per_group(rows)


AMB_PAIRS = [(K * g + k, p) for g in range(3) for k, p in ((0, CROSS[g] - 3), (0, CROSS[g] + 2), (0, 5), (0, 2995), (8, 40), (13, 4), (13, 4999))]
AMB_CODES = [(3 * i + 1) % 4 for i in range(len(AMB_PAIRS))]


def _amb_by_position(layout, seen):
    """{probe: {position: code}}: the listed bases as a kernel finds them that looks its source index up in the list"""
    listed = {int(layout.probe_base[j]) + p: c for (j, p), c in zip(AMB_PAIRS, AMB_CODES)}
    return {j: {p: listed[int(g)] for p, g in enumerate(seen[j]) if int(g) in listed} for j in range(N_PROBES)}


def expect_extract(layout, strings, seen, reversed=False):
    patches = _amb_by_position(layout, seen)
    out = []
    for j, first, n, strand in extract_regions():
        w = xo.region_codes(strings[j].tolist(), first, n, strand, patches[j], 0)
        out.append(w[::-1] if reversed else w)
    return out


def select_order():
    rng = np.random.default_rng(77)
    return [int(x) for x in rng.permutation(N_PROBES)] + [0, K, 2 * K, 0, 13, K + 13]


def expect_select(strings):
    return [strings[j].tolist() for j in select_order()]


def splice_strings():
    """[[run, ...], ...], a run = (probe, first, len, kind): runs of every kind across 2^31 / 2^32, strings that mix the groups"""
    out = []
    for g in range(3):
        j0, x = K * g, CROSS[g]
        h = K * ((g + 1) % 3)
        out += [[(j0, x - 30, 70, so.UP), (h + 9, 499, 300, so.DOWN), (0, 0, 5, so.LITERAL + 2), (j0, x + 20, 50, so.SUB_DOWN)],
                [(j0, x + 600, 1200, so.DOWN)], [(j0, x - 17, 33, so.SUB_UP), (j0 + 13, 4999, 5000, so.DOWN)], [],
                [(j0 + 3, 0, 1, so.UP), (j0 + 4, 1, 2, so.DOWN), (j0 + 12, 0, 1025, so.UP), (h, x, 1, so.SUB_DOWN)]]
    return out


def splice_arrays(read_of=None):
    strs = splice_strings()
    runs = np.array([r for s in strs for r in s], np.int64).reshape(-1, 4)
    if read_of is not None:
        lit = runs[:, 3] >= so.LITERAL
        runs[~lit, 0] = read_of[runs[~lit, 0]]
    sro = np.concatenate([[0], np.cumsum([len(s) for s in strs])]).astype(np.uint64)
    return runs.astype(np.uint32), sro


def expect_splice(strings, reversed=False):
    runs, sro = splice_arrays()
    return so.spliced([s.tolist() for s in strings], runs, sro, reversed)


def segment_rows():
    """(probe, lo, len, orient): all four orientations across 2^31 / 2^32, whole short reads, a segment of one base"""
    def rows(j0, x):
        out = [(j0, x - 200 + 7 * o, 400, o) for o in range(4)] + [(j0, 0, 3000, REVCOMP), (j0, x - 1, 2, FWD), (j0, x, 1, COMP)]
        out += [(j0 + k, 0, GROUP_LENS[k], (k + j0) % 4) for k in (3, 5, 6, 7, 8, 10, 11, 12)]
        return out + [(j0 + 13, 4000 - 100 * o, 1000, o) for o in range(4)]
    return _per_group(rows)


def segment_buffers(orc, strings):
    return [orc.buffer(text(strings[j]), lo, ln, o) for j, lo, ln, o in segment_rows()]


def expect_segments(orc, model, strings):
    """per frame 0..2: (Frame_Score, Cumulative_Score, Score_String, Partial_Window_Prob of the last base) of every segment's buffer;
    then All_Frame_Score with prefix and frame varying"""
    bufs = segment_buffers(orc, strings)
    per = [[(orc.frame_score(model, b, f), orc.cumulative_score(model, b, f), orc.score_string(model, b, f),
             orc.partial_window(model, len(b) - 1, b, f)) for b in bufs] for f in range(3)]
    prefix, frames = all_frame_args()
    allf = [orc.all_frame_score(model, b, int(p), int(fr)) for b, p, fr in zip(bufs, prefix, frames)]
    return per, allf


def all_frame_args():
    rows = segment_rows()
    lens = np.array([r[2] for r in rows], np.int64)
    prefix = np.maximum(lens - (np.arange(len(rows)) % 5), 0).astype(np.uint32)
    frames = np.array([(1, 2, 3, -1, -2, -3)[i % 6] for i in range(len(rows))], np.int32)
    return prefix, frames


FIXED_L = 12


def fixed_rows():
    return [r for r in segment_rows() if r[2] >= FIXED_L]


def fixed_windows(strings):
    comp = np.array([3, 2, 1, 0], np.uint8)
    win = []
    for j, lo, ln, o in fixed_rows():
        b = strings[j][lo:lo + ln]
        b = b[::-1] if o in (REV, REVCOMP) else b
        win.append((comp[b] if o in (COMP, REVCOMP) else b)[:FIXED_L])
    return np.stack(win)


def revcomp(s):
    return s[::-1].translate(str.maketrans("acgt", "tgca"))


def expect_strings(orc, model, strings):
    """whole-read Score_String, frame 0, of every probe and of its reverse complement"""
    return np.array([[orc.score_string(model, text(s), 0), orc.score_string(model, revcomp(text(s)), 0)] for s in strings])


MIN_GENE_LEN = 90


def expect_orfs(orc, strings):
    """Find_Orfs of every probe (linear, no truncated ORFs): int32 [n, 4] frame, stop_position, gene_len, orf_len"""
    prm = orc.mg_params(min_gene_len=MIN_GENE_LEN, allow_truncated=False)
    return [orc.find_orfs_general(text(s), prm) for s in strings]


def orf_regions(orfs_of_probe, lens):
    """Entropy_Filter's region (probe, first, len, strand) of every ORF, in order"""
    return [(j,) + eo.orf_region(int(o[1]), int(o[2]), int(o[0]), lens[j]) for j, rows in enumerate(orfs_of_probe) for o in rows]


def entropy_region_rows():
    """(probe, first, len, strand): codon-aligned and not, across 2^31 / 2^32 and round the read's end, both strands"""
    def rows(j0, x):
        return [(j0, x - 100, 201, 1), (j0, x + 100, 198, -1), (j0, 2950, 120, 1), (j0, 30, 90, -1), (j0, 0, 3000, 1), (j0 + 8, 85, 86, -1),
                (j0 + 12, 1, 1023, 1), (j0 + 13, 4999, 4998, -1), (j0 + 5, 0, 15, 1)]
    return _per_group(rows)


def expect_entropy_counts(strings, regions, aa):
    return np.array([eo.counts(text(strings[j]), f, ln, s, aa) for j, f, ln, s in regions], np.int32).reshape(-1, 20)


def audit_region_rows():
    def rows(j0, x):
        return [(j0, x - 150, 300, 1), (j0, x + 151, 303, -1), (j0, 2900, 210, 1), (j0, 50, 120, -1), (j0, 0, 2997, 1), (j0 + 8, 2, 60, 1),
                (j0 + 13, 4999, 4500, -1), (j0 + 12, 1000, 99, 1), (j0 + 5, 14, 15, -1), (j0 + 4, 0, 2, 1)]
    return _per_group(rows)


def _letters(layout, strings, seen, pairs, other="n"):
    """the probe strings as letters, `other` where the position is read from a listed index"""
    listed = {int(layout.probe_base[j]) + p for j, p in pairs}
    out = []
    for j, s in enumerate(strings):
        t = list(text(s))
        for p, g in enumerate(seen[j]):
            if int(g) in listed:
                t[p] = other
        out.append("".join(t))
    return out


def expect_audit(layout, strings, seen):
    return ao.audit_records(_letters(layout, strings, seen, AMB_PAIRS), audit_region_rows())


WINDOW, SKIP = 1000, 997
N_WINDOW_ROWS = 4_311_155                               # of the whole batch (tests/test_big_batch_host.py adds them up)


def expect_windows(layout, strings, seen):
    """[rows of probe j]: int32 [n, 5]"""
    letters = _letters(layout, strings, seen, AMB_PAIRS)
    return [np.array([c for _, _, c in wo.window_rows(s, WINDOW, SKIP)], np.int32).reshape(-1, 5) for s in letters]


def uncovered_intervals():
    """(probe, lo, hi), any order"""
    def rows(j0, x):
        return [(j0, x - 10, x + 10), (j0, 100, 200), (j0, 150, 400), (j0 + 13, 0, 5000), (j0 + 12, 0, 1), (j0 + 12, 1024, 1025), (j0 + 9, 499, 500),
                (j0 + 9, 250, 250), (j0 + 8, 10, 20)]
    return _per_group(rows)[::-1]


def expect_uncovered(lengths):
    """gaps (probe, first, len, 1) and the gap offsets, for reads of the lengths given (a kernel that took a read's length from
    truncated offsets sees other lengths)"""
    return wo.batch_uncovered(lengths, uncovered_intervals())


def seen_lengths(layout, modulus=None):
    """the probes' lengths as the difference of their two offsets, each taken modulo `modulus` first"""
    a, b = layout.probe_base, layout.probe_base + np.array([GROUP_LENS[j % K] for j in range(N_PROBES)], np.int64)
    return [int(x) for x in ((b - a) if modulus is None else (b % modulus - a % modulus))]


FEATURE_PROBES = [K * g + k for g in (1, 2) for k in (0, 13)]
OPAQUE_PAIRS = [(j, p) for j in FEATURE_PROBES for p in (7, 1300, 2500)]


def feature_lines():
    """gene lines (header, a, b, frame), 1-based as glimmer prints them, on the probes of groups 1 and 2"""
    lines = []
    for j in FEATURE_PROBES:
        L = GROUP_LENS[j % K]
        lines += [("p%d" % j, 10, 300, 1), ("p%d" % j, 700, 401, -2), ("p%d" % j, 900, 1499, 3), ("p%d" % j, L - 500, L + 2, 1)]
    return lines


def feature_inputs(layout, strings, seen):
    """-> (genes, sd) for features_oracle.count, the letters upper-case and 'N' where the position is read from an opaque index"""
    up = [s.upper() for s in _letters(layout, strings, seen, OPAQUE_PAIRS, "N")]
    seqs = [("p%d" % j, up[j]) for j in FEATURE_PROBES]
    return fc.oracle_inputs(seqs, feature_lines())


def feature_rows(genes):
    """the C ABI's gene rows (probe, strand, start, end, start_codon), grouped by read"""
    return [(int(hdr[1:]), g.strand, g.start, g.end, g.start_codon) for hdr, hgenes in genes.items() for g in hgenes]


def expect_features(layout, strings, seen):
    genes, sd = feature_inputs(layout, strings, seen)
    gs, ns = feo.count(genes, sd)
    return fc.table_of(gs, 50), fc.table_of(ns, 50)


# ---------------------------------------------------------------------------------------------------------------------------------
# The same layout in LETTERS (gmg_letters: one byte per base, 4 GiB), for gmg_regions_text and gmg_runs_text: the filler is the text
# ttaa, the probes are random letters over the alphabet of tests/test_gpu_text.py (upper and lower case, IUPAC codes, '*', '-').
# ---------------------------------------------------------------------------------------------------------------------------------

ALPHABET = b"acgtACGTacgtnNrykmRYKMbdhvswBDHVSW*-"
LETTER_SEEDS = (9201, 9202, 9203)
TEXT_HEADS = [b"", b">", b">" + b"h" * 298 + b"\n"]
_probe_letters = None


def probe_letters():
    """the 45 probe reads as uint8 arrays of letters"""
    global _probe_letters
    if _probe_letters is None:
        abc = np.frombuffer(ALPHABET, np.uint8)
        _probe_letters = []
        for seed in LETTER_SEEDS:
            rng = np.random.default_rng(seed)
            _probe_letters += [abc[rng.integers(0, len(abc), size=n)] for n in GROUP_LENS]
    return _probe_letters


class LetterLayout(Layout):
    """Layout over letters: letters_at (g), letter_strings (modulus) -> bytes per probe, letters () -> the 4 GiB array"""

    def __init__(self):
        super().__init__()
        p = probe_letters()
        self.group_letters = [np.concatenate(p[K * g:K * g + K]) for g in range(3)]

    def letters_at(self, g):
        g = np.asarray(g, np.int64)
        assert g.size == 0 or (g.min() >= 0 and g.max() < self.total)
        out = np.frombuffer(b"ttaa", np.uint8)[g % 4]
        for s, start in enumerate(self.slot_start):
            m = (g >= start) & (g < start + GROUP_BASES)
            out[m] = self.group_letters[self.slots[s]][g[m] - start]
        return out

    def letter_strings(self, modulus=None):
        return [self.letters_at(self.index_of(j, modulus)).tobytes() for j in range(N_PROBES)]

    def letters(self):
        assert self.total % 4 == 0
        out = np.full(self.total // 4, 0x61617474, np.uint32).view(np.uint8)          # "ttaa", little endian
        for s, start in enumerate(self.slot_start):
            out[start:start + GROUP_BASES] = self.group_letters[self.slots[s]]
        return out


def text_regions():
    """(probe, first, len, strand) and their heads: gmg_reads_extract's regions of above, and the empty region"""
    regions = extract_regions() + [(K * g, CROSS[g], 0, 1) for g in range(3)]
    return regions, [TEXT_HEADS[k % 3] for k in range(len(regions))]


def expect_regions_text(strings, width):
    """strings: the probes' letters (bytes)"""
    import text_oracle as to
    regions, heads = text_regions()
    return "".join(to.region_record(strings[j].decode("latin-1"), (j, f, n, s), h.decode("latin-1"), width)
                   for (j, f, n, s), h in zip(regions, heads)).encode("latin-1")


def text_runs():
    """-> (runs [n, 4] naming probes, string_run_off, heads, pad_front, pad_behind): splice_strings (runs of every kind, upwards and
    downwards across 2^31 / 2^32) with a letter taken as it is, and pads that shift the codons"""
    strs = [s + [(K * (k % 3), CROSS[k % 3] + k, 2, so.LITERAL_AS_IS + 1)] for k, s in enumerate(splice_strings())]
    runs = np.array([r for s in strs for r in s], np.int64).reshape(-1, 4)
    sro = np.concatenate([[0], np.cumsum([len(s) for s in strs])]).astype(np.uint64)
    heads = [TEXT_HEADS[(k + 1) % 3] for k in range(len(strs))]
    return runs, sro, heads, [k % 4 for k in range(len(strs))], [(2 * k) % 5 for k in range(len(strs))]


def text_runs_big(layout):
    runs = text_runs()[0].copy()
    lit = (runs[:, 3] >= so.LITERAL) & (runs[:, 3] < so.LITERAL_AS_IS)
    runs[~lit, 0] = layout.probe_read[runs[~lit, 0]]
    return runs.astype(np.uint32)


def expect_runs_text(strings, mode, width):
    import runs_text_oracle as rto
    runs, sro, heads, front, behind = text_runs()
    return rto.text(strings, runs, sro, heads, rto.Params(mode, width), front, behind)


# ---- the output side: a text of more than 2^32 bytes from a small batch of letters ---------------------------------------------------

OUT_READ_LEN, OUT_RECORDS, OUT_WIDTH = 20_000, 215_000, 60
OUT_SEED = 9301


def out_letters():
    """two reads: 37 letters, then the one of 20,000 the records are cut from"""
    abc = np.frombuffer(ALPHABET, np.uint8)
    rng = np.random.default_rng(OUT_SEED)
    return [abc[rng.integers(0, len(abc), size=n)].tobytes() for n in (37, OUT_READ_LEN)]


def out_regions():
    """int32 [n, 4]: every record is the whole long read, from another first position, on alternating strands, modulo the read"""
    k = np.arange(OUT_RECORDS, dtype=np.int64)
    return np.stack([np.ones_like(k), (k * 7919) % OUT_READ_LEN, np.full_like(k, OUT_READ_LEN), 1 - 2 * (k % 2)], 1).astype(np.int32)


def out_head(k):
    return b"" if k % 3 == 0 else b">" if k % 3 == 1 else b">rec%d\n" % k


def out_head_lens():
    k = np.arange(OUT_RECORDS, dtype=np.int64)
    digits = np.floor(np.log10(np.maximum(k, 1))).astype(np.int64) + 1
    return np.where(k % 3 == 0, 0, np.where(k % 3 == 1, 1, 5 + digits))


def out_record_offsets(body):
    """text offsets of the records, body = bytes of a record behind its head"""
    off = np.zeros(OUT_RECORDS + 1, np.int64)
    np.cumsum(out_head_lens() + body, out=off[1:])
    return off


def out_slices(total):
    """(offset, bytes): 128 KiB around byte 2^31, 128 KiB around byte 2^32, the last 64 KiB"""
    return [(M31 - (64 << 10), 128 << 10), (M32 - (64 << 10), 128 << 10), (total - (64 << 10), 64 << 10)]


def expect_out_slice(off, record_of, a, n):
    """bytes [a, a + n) of the text whose records begin at off[] and whose record k is record_of (k)"""
    k0, k1 = int(np.searchsorted(off, a, "right")) - 1, int(np.searchsorted(off, a + n, "left"))
    blob = b"".join(record_of(k) for k in range(k0, k1))
    return blob[a - int(off[k0]):a - int(off[k0]) + n]


def out_region_record(k):
    import text_oracle as to
    seq = out_letters()[1].decode("latin-1")
    _, first, n, strand = (int(x) for x in out_regions()[k])
    return to.region_record(seq, (1, first, n, strand), out_head(k).decode("latin-1"), OUT_WIDTH).encode("latin-1")


REGION_BODY = OUT_READ_LEN + (OUT_READ_LEN - 1) // OUT_WIDTH + 1


def out_runs():
    """uint32 [2 n, 4], string_run_off: string k = the long read upwards up to a cut, then downwards from its end to the cut"""
    k = np.arange(OUT_RECORDS, dtype=np.int64)
    cut = OUT_READ_LEN - (k % 977)
    up = np.stack([np.ones_like(k), np.zeros_like(k), cut, np.full_like(k, so.UP)], 1)
    down = np.stack([np.ones_like(k), np.full_like(k, OUT_READ_LEN - 1), OUT_READ_LEN - cut, np.full_like(k, so.DOWN)], 1)
    runs = np.stack([up, down], 1).reshape(-1, 4).astype(np.uint32)
    return runs, (2 * np.arange(OUT_RECORDS + 1)).astype(np.uint64)


def out_runs_record(k):
    import runs_text_oracle as rto
    runs, _ = out_runs()
    return rto.records(out_letters(), runs[2 * k:2 * k + 2], [0, 2], [out_head(k)], rto.Params(rto.DNA, OUT_WIDTH))[0]
