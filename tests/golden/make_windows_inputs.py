"""Writes the hand-made inputs of tests/golden/windows/ (deterministic; the recorded outputs beside them come from the reference's
window-acgt, uncovered and entropy-fasta, built outside this repository -- g++ -O1 -w -std=gnu++98 -fpermissive -Isrc/Common
-Isrc/Util against delcher.o fasta.o gene.o kelley.o; they are kept in cases.json, the short ones as text, the others as the
SHA-256 digest and the length of the whole output):
  hand.fna            a multi-fasta file with records of 0, 1, 3, 4, 5, 9, 10, 11, 15, 16, 17, 18, 40 and 70 bases -- W - 1, W and W + 1
                      for the window lengths 1, 4, 10, 16, 17 of the recorded runs -- with n / r / w letters and upper case
  circ40.fna          a genome of 40 bases in both cases with an n and a y
  circ40.coords       lines <tag> <start> <end> <dir> on it: overlapping, touching, nested, identical and origin-crossing on both strands,
                      and lines that do not parse; every line is one that no recorded option set sends outside the sequence
  circ40_d.coords     as above plus the lines that give an EMPTY interval (dir > 0 and end = start - 1), which only a run with -d and
                      without -s / --nostop keeps on the sequence
  multi3.fna / .coords  three records and lines <id> <tag> <start> <end> <dir> for uncovered_gpu --multi
  ef.fna              gene strings for entropy-fasta, one of them with nnn and Ryn codons and upper case
  ef_bad.fna          the same with a record of 10 bases in the middle: the status-1 exit
Lines at which the reference leaves its buffers (tests/windows_oracle.py flags them) are not written."""
import os
import random
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import windows_oracle as wo  # noqa: E402

OUT = os.path.join(HERE, "windows")
OPTION_SETS = [{}, dict(use_dir=True), dict(skip_start=True), dict(skip_stop=True), dict(circular=False)]


def unflagged(lengths, line, option_sets, tags=None):
    return all(not wo.coord_intervals(lengths, line, tags=tags, **kw)[2] for kw in option_sets)


def main():
    os.makedirs(OUT, exist_ok=True)
    rng = random.Random(20261020)
    with open(os.path.join(OUT, "hand.fna"), "w") as f:
        for n in (0, 1, 3, 4, 5, 9, 10, 11, 15, 16, 17, 18, 40, 70):
            s = [rng.choice("acgt") for _ in range(n)]
            if n >= 9:
                for p, ch in zip(rng.sample(range(n), 3), "nrw"):
                    s[p] = ch
            if n in (4, 16, 40):
                s = [c.upper() if rng.random() < 0.5 else c for c in s]
            if n == 17:
                s[0], s[-1] = "N", "n"
            s = "".join(s)
            f.write(">len%d  a record of %d bases\n" % (n, n) + "".join(s[i:i + 30] + "\n" for i in range(0, n, 30)))
    L = 40
    seq = [rng.choice("acgt") for _ in range(L)]
    seq[7], seq[33] = "n", "y"
    seq = "".join(c.upper() if rng.random() < 0.3 else c for c in seq)
    with open(os.path.join(OUT, "circ40.fna"), "w") as f:
        f.write(">circ40  a hand-made circular genome\n" + seq[:25] + "\n" + seq[25:] + "\n")
    lines = ["ovl_a 5 8 +1\n", "ovl_b 7 10 +1\n", "touch 11 14 +1\n", "nest_out 25 17 -1\n", "nest_in 22 19 -1\n", "same 7 10 +1\n",
             "\n", "# a comment\n", "short 12\n", "letters 12x 20 +1\n", "tabs\t33\t36\t+2\n",
             "cross_f 38 2 +1\n", "cross_r 3 38 -1\n", "rev 32 29 -1\n"]
    empty = ["empty_gap 27 26 +1\n", "empty_0 1 0 +1\n", "empty_L 41 40 +1\n", "empty_in 12 11 +1\n"]
    assert all(unflagged([L], l, OPTION_SETS) for l in lines)
    keep = [l for l in lines if unflagged([L], l, OPTION_SETS)]
    with open(os.path.join(OUT, "circ40.coords"), "w") as f:
        f.write("".join(keep))
    with open(os.path.join(OUT, "circ40_d.coords"), "w") as f:
        f.write("".join(keep[:6] + [l for l in empty if unflagged([L], l, [dict(use_dir=True)])] + keep[6:]))
    recs = [("m%d" % r, "".join(rng.choice("aacgtttgn") for _ in range(n))) for r, n in enumerate((90, 0, 131))]
    with open(os.path.join(OUT, "multi3.fna"), "w") as f:
        for tag, s in recs:
            f.write(">%s record of %d bases\n" % (tag, len(s)) + "".join(s[i:i + 60] + "\n" for i in range(0, len(s), 60)))
    with open(os.path.join(OUT, "multi3.coords"), "w") as f:
        for r, (tag, s) in enumerate(recs):
            for k in range(8 if s else 0):
                a = rng.randrange(1, len(s) + 1)
                ln = rng.choice([6, 9, 12, 17])
                d = rng.choice([1, -1])
                b = (a - 1 + d * (ln - 1)) % len(s) + 1
                line = "g%d_%02d %s %d %d %+d\n" % (r, k, tag, a, b, d)
                if unflagged([len(x) for _, x in recs], line, OPTION_SETS, tags=[t for t, _ in recs]):
                    f.write(line)
    genes = []
    for k, n in enumerate((30, 63, 96, 150)):
        s = "atg" + "".join(rng.choice("acgt") for _ in range(n - 6)) + "taa"
        if k == 1:
            s = s[:9] + "nnn" + s[12:21] + "Ryn" + s[24:30] + s[30:].upper()
        genes.append(("gene%d  %d bases" % (k, n), s))
    for name, recs in (("ef.fna", genes), ("ef_bad.fna", genes[:2] + [("odd  ten bases", "atgcccgggt")] + genes[2:])):
        with open(os.path.join(OUT, name), "w") as f:
            for hdr, s in recs:
                f.write(">%s\n" % hdr + "".join(s[i:i + 60] + "\n" for i in range(0, len(s), 60)))


if __name__ == "__main__":
    main()
