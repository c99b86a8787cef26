"""Python restatement of gmg_runs_text (tests only): the strings a plan of runs describes, printed over the LETTERS of the reads
through the caller's tables, or translated codon by codon, as records of text.  Written from the header comment in include/gmg.h,
not from the kernel.  The line rule is text_oracle.record's; the run kinds are splice_oracle's."""
import splice_oracle as so
import text_oracle as to

DNA, PROTEIN = 0, 1
# extract_aa.py's dictionary, as the standard code is usually written: first base T C A G, then the second, then the third
SCRIPT_CODE = "FFLLSSSSYY**CC*WLLLLPPPPHHQQRRRRIIIMTTTTNNKKSSRRVVVVAAAADDEEGGGG"
_RC = bytes.maketrans(b"ATCGatcg", b"TAGCtagc")


class Params:
    """the fields of gmg_runs_text_params, with the script's rules as defaults (gmg_runs_text_params_script, table 0)"""

    def __init__(self, mode=DNA, width=0, aa=None, **fields):
        ident = bytes(range(256))
        self.up = ident
        self.down = ident.translate(_RC)
        self.sub_up = bytes(ord("G") if c == ord("C") else ord("C") for c in range(256))
        self.sub_down = self.sub_up.translate(_RC)
        self.literal = b"ACGT"
        self.pad, self.unknown = ord(" "), ord("X")
        self.aa = script_aa() if aa is None else bytes(aa)
        self.mode, self.width = mode, width
        for name, value in fields.items():
            assert hasattr(self, name)
            setattr(self, name, value if name not in ("pad", "unknown") or isinstance(value, int) else ord(value))


def script_aa():
    """the script's dictionary in the index of gmg_xlate_table: 16*b0 + 4*b1 + b2 with a=0 c=1 g=2 t=3"""
    order = "TCAG"
    return bytes(ord(SCRIPT_CODE[16 * order.index(a) + 4 * order.index(b) + order.index(c)]) for a in "ACGT" for b in "ACGT" for c in "ACGT")


def run_bytes(seqs, run, prm):
    """the bytes one run prints; seqs: the reads as bytes"""
    read, first, n, kind = (int(x) for x in run)
    if kind >= so.LITERAL_AS_IS:
        return bytes([prm.up[seqs[read][first]]]) * n if n else b""
    if kind >= so.LITERAL:
        return bytes([prm.literal[kind & 3]]) * n
    s = seqs[read]
    table = (prm.up, prm.down, prm.sub_up, prm.sub_down)[kind]
    at = range(first, first + n) if kind in (so.UP, so.SUB_UP) else range(first, first - n, -1)
    return bytes(table[s[p]] for p in at)


def bad_run(lengths, run):
    """True where gmg_runs_text refuses the run: lengths = the reads' lengths"""
    read, first, n, kind = (int(x) for x in run)
    if kind >= so.LITERAL_AS_IS + 4:
        return True
    if so.LITERAL <= kind < so.LITERAL_AS_IS or (kind >= so.LITERAL_AS_IS and n == 0):
        return False
    if read >= len(lengths):
        return True
    L = lengths[read]
    if kind >= so.LITERAL_AS_IS:
        return first >= L
    if kind in (so.UP, so.SUB_UP):
        return first + n > L
    return first > L if n == 0 else (first >= L or n > first + 1)


def printed(seqs, runs, sro, k, front, behind, prm):
    """P_k: the pad bytes in front, the runs of string k, the pad bytes behind"""
    body = b"".join(run_bytes(seqs, r, prm) for r in runs[int(sro[k]):int(sro[k + 1])])
    return bytes([prm.pad]) * front + body + bytes([prm.pad]) * behind


def translate(p, prm):
    """one character per whole codon of P: aa[idx] for upper-case ACGT, lowered A-Z for lower-case acgt, `unknown` otherwise"""
    out = bytearray()
    for t in range(len(p) // 3):
        codon = p[3 * t:3 * t + 3]
        if all(c in b"ACGT" for c in codon):
            out.append(prm.aa[sum(b"ACGT".index(c) << (4 - 2 * i) for i, c in enumerate(codon))])
        elif all(c in b"acgt" for c in codon):
            a = prm.aa[sum(b"acgt".index(c) << (4 - 2 * i) for i, c in enumerate(codon))]
            out.append(a + 32 if ord("A") <= a <= ord("Z") else a)
        else:
            out.append(prm.unknown)
    return bytes(out)


def records(seqs, runs, sro, heads, prm, pad_front=None, pad_behind=None):
    """the records of the text, one bytes object each"""
    out = []
    for k in range(len(sro) - 1):
        p = printed(seqs, runs, sro, k, int(pad_front[k]) if pad_front is not None else 0, int(pad_behind[k]) if pad_behind is not None else 0, prm)
        chars = translate(p, prm) if prm.mode == PROTEIN else p
        out.append(to.record(heads[k].decode("latin-1"), chars.decode("latin-1"), prm.width).encode("latin-1"))
    return out


def text(seqs, runs, sro, heads, prm, pad_front=None, pad_behind=None):
    return b"".join(records(seqs, runs, sro, heads, prm, pad_front, pad_behind))


def case_inputs(gmg, name):
    """a recorded case (splice_oracle.CASES) as gmg_runs_text takes it: (seqs as bytes, runs, string_run_off, heads, pad_front,
    pad_behind) from the two input files and gmg_edits_plan"""
    fasta = so.read_fasta(so.CASES[name][0])
    headers, seqs = [h for h, _ in fasta], [s for _, s in fasta]
    genes = so.parse_predict(so.CASES[name][1], headers)
    runs, sro, rows = gmg.edits_plan(so.offsets(seqs), genes, so.odd_letters(seqs))
    heads = [(">%s_%d,%d_%s\n" % (headers[genes[line][0]], start, end, "+" if strand > 0 else "-")).encode()
             for line, start, end, strand, _, _ in rows]
    return [s.encode() for s in seqs], runs, sro, heads, [r[4] for r in rows], [r[5] for r in rows]
