"""Writes the hand-made inputs of tests/golden/audit/ (deterministic; the recorded outputs beside them come from the reference's
anomaly, start-codon-distrib and entropy-score, built outside this repository with the plain g++ line of oracle/Makefile; they are
kept in cases.json, the short ones as text, the others as the SHA-256 digest and the length of the whole output; the 300 moved genes
of the genome's predict file are made by audit_oracle.moved_genes when a test needs them):
  tiny.fna            a genome of 180 bases in both cases with n / r / y letters
  tiny.coords         genes on it, wrapping the origin on both strands, with a direction column; lines that do not parse
  tiny_acgt.coords    tiny.coords without the lines whose region holds one amino acid only (entropy-score prints a NaN there, whose
                      sign is the platform's)
  multi4.fna / .coords  four records and lines <id> <tag> <start> <end> <dir> for --multi
Lines at which the reference leaves its buffers (tests/audit_oracle.py flags them) are not written."""
import os
import random
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import audit_oracle as ao  # noqa: E402

OUT = os.path.join(HERE, "audit")


def unflagged(records, lines, **kw):
    keep = []
    for line in lines:
        if not ao.anomaly(records, line, **kw)[2] and not ao.start_codon_distrib(records, line, **kw)[2]:
            keep.append(line)
    return keep


def main():
    os.makedirs(OUT, exist_ok=True)
    rng = random.Random(20260105)
    L = 180
    seq = [rng.choice("aaacgtttg") for _ in range(L)]
    for p in rng.sample(range(L), 7):
        seq[p] = rng.choice("nry")
    seq = [c.upper() if rng.random() < 0.4 else c for c in seq]
    seq[171:174] = "AtG"
    seq[6:9] = "tAa"
    seq[2:5] = "caT"                                    # a reverse-strand start codon at bases 5, 4, 3
    tiny = "".join(seq)
    with open(os.path.join(OUT, "tiny.fna"), "w") as f:
        f.write(">tiny  a hand-made circular genome\n" + tiny[:70] + "\n" + tiny[70:140] + "\n" + tiny[140:] + "\n")
    records = [("tiny", tiny)]
    lines = ["g_wrap_f  172  9  +1\n", "g_wrap_r  5  171  -1\n", "g_wrap_f1  172  10  +1\n", "g_wrap_r2  5  169  -1\n", "\n", "# a comment\n",
             "short 12\n", "tabs\t20\t49\t+2\n", "nodir 30 62\n", "letters 12x 40 +1\n"]
    for k in range(60):
        a = rng.randrange(1, L + 1)
        ln = rng.choice([9, 12, 15, 16, 17, 30, 45, 60, 61])
        d = rng.choice([1, -1])
        b = (a - 1 + d * (ln - 1)) % L + 1
        lines.append("orf%05d %d %d %+d\n" % (k, a, b, d))
    with open(os.path.join(OUT, "tiny.coords"), "w") as f:
        f.write("".join(l if ao.scan_fields(l, 2) is None else "".join(unflagged(records, [l])) for l in lines))
    with open(os.path.join(OUT, "tiny_acgt.coords"), "w") as f:
        for l in ao.coord_lines(open(os.path.join(OUT, "tiny.coords")).read()):
            if not any("nan" in ao.entropy_score(records, l, **kw)[0] for kw in ({}, dict(use_dir=True, skip_start=True, skip_stop=True))):
                f.write(l)
    recs = []
    for r in range(4):
        n = rng.choice([90, 151, 64, 240])
        recs.append(("rec%d" % r, "".join(rng.choice("aacgtttg") for _ in range(n))))
    with open(os.path.join(OUT, "multi4.fna"), "w") as f:
        for tag, s in recs:
            f.write(">%s record of %d bases\n" % (tag, len(s)) + "\n".join(s[i:i + 60] for i in range(0, len(s), 60)) + "\n")
    with open(os.path.join(OUT, "multi4.coords"), "w") as f:
        for r, (tag, s) in enumerate(recs):
            for k in range(25):
                a = rng.randrange(1, len(s) + 1)
                ln = rng.choice([9, 12, 16, 17, 30, 45])
                d = rng.choice([1, -1])
                b = (a - 1 + d * (ln - 1)) % len(s) + 1
                line = "g%d_%02d %d %d %+d\n" % (r, k, a, b, d)
                if unflagged([(tag, s)], [line]) and unflagged([(tag, s)], [line], use_dir=True):
                    f.write("g%d_%02d %s %d %d %+d\n" % (r, k, tag, a, b, d))


if __name__ == "__main__":
    main()
