"""Expected outputs of the reference's scripts/extract_aa.py -- the gene strings of a prediction run with its predicted insertions,
deletions and substitutions applied -- for gmg_edits_plan + gmg_reads_splice and extract-aa_gpu (tests/golden/extract_aa/).

    python3 tests/golden/make_extract_aa.py [<reference>/scripts/extract_aa.py]

The script is Python 2.  Its text is read where it lies, converted IN MEMORY (lib2to3, then three textual fixes: the cmp sort, the
integer division of the trim, string.maketrans) and executed; nothing of it is written anywhere.  What is written is data:

  recorded.sha256           the SHA-256 of its two output files, <name>.ffn and <name>.faa, for data/seqs.fa with
                            predict/<name>.predict, for the three recorded runs that cover every read of seqs.fa (glimmer-mg.indel,
                            glimmer-mg.sub, classes.indel): 6 files, 1,041 records, 330 KB of text.  A test that needs such a
                            text (to feed it to the reference's build-icm -r) takes the expansion of the plan once it has this digest
  edges.fa, edges.predict   a synthetic case made here: one read per rule of the script's edit arithmetic (listed below, beside
                            the reads), then a dozen reads with random genes and edit lists
  edges.ffn / edges.faa     the script's output for it

Deterministic: the same script gives the same files byte for byte.  Test infrastructure; data only.
"""
import functools
import hashlib
import io
import os
import random
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "extract_aa")
REAL = ["glimmer-mg.indel", "glimmer-mg.sub", "classes.indel"]


def load_script(path):
    """the script's namespace, converted in memory"""
    from lib2to3 import refactor
    text = open(path).read()
    tool = refactor.RefactoringTool(refactor.get_fixers_from_package("lib2to3.fixes"))
    text = str(tool.refactor_string(text + "\n", "extract_aa.py"))
    for old, new in [(".sort(gene_compare)", ".sort(key=functools.cmp_to_key(gene_compare))"),
                     ("len(gene_seq)/3", "len(gene_seq)//3"),
                     ("string.maketrans", "str.maketrans")]:
        assert text.count(old) == 1, old
        text = text.replace(old, new)
    ns = {"__name__": "extract_aa", "functools": functools}
    exec(compile(text, "extract_aa.py", "exec"), ns)
    return ns


def run_script(ns, seqs, predict, prefix):
    argv = sys.argv
    sys.argv = ["extract_aa.py", "-s", seqs, "-p", predict, "-o", prefix]
    try:
        ns["main"]()
    finally:
        sys.argv = argv


# ---- the synthetic case ---------------------------------------------------------------------------------------------------------

def _seq(rng, n):
    return "".join(rng.choice("ACGT") for _ in range(n))


def _put(seq, at, letters):
    """letters at the 1-based position `at`"""
    return seq[:at - 1] + letters + seq[at - 1 + len(letters):]


def _line(k, a, b, frame, ins=(), dels=(), subs=()):
    return "orf%05d %8d %8d  %+d %8.2f I:%s D:%s S:%s" % (k, a, b, frame, 1.0 + k / 8, ",".join(map(str, ins)), ",".join(map(str, dels)),
                                                          ",".join(map(str, subs)))


def edges():
    """[(header, sequence, [gene lines])]: forward genes are (a, b, +f), reverse genes (b, a, -f) with a < b, 1-based inclusive"""
    rng = random.Random(20260417)
    reads = []

    def add(name, L, genes, letters=()):
        s = _seq(rng, L)
        for at, text in letters:
            s = _put(s, at, text)
        reads.append((name, s, [_line(k + 1, *g) for k, g in enumerate(genes)]))

    # an edit at base 1 and at base L, of every kind
    add("ins_first", 90, [(1, 90, 1, [1])])
    add("ins_last", 90, [(1, 90, 1, [90])])
    add("del_first", 90, [(1, 90, 1, [], [1])])                       # the duplicate of nothing yet: a pad blank at the string's front
    add("del_first_rev", 90, [(90, -2, -1, [], [1])])                  # ... and behind a reverse string
    add("del_last", 90, [(1, 93, 1, [], [90])])
    add("sub_first_last", 91, [(1, 91, 2, [], [], [1, 91]), (91, 2, -3, [], [], [])])
    # neighbours: insertion then deletion (the deletion duplicates a dropped base: nothing), deletion then insertion, two
    # insertions then a deletion, two deletions in a row (the second duplicates the first one's base)
    add("ins_del", 84, [(4, 84, 1, [30], [31])])
    add("del_ins", 84, [(4, 84, 1, [31], [30])])
    add("ins_ins_del", 84, [(84, 4, -2, [30, 31], [32])])
    add("del_del", 84, [(4, 84, 1, [], [30, 31])])
    add("sub_del", 84, [(4, 84, 1, [], [31], [30])])                   # the deletion duplicates the substituted letter
    # the same position in two lists: the list of lower priority is stuck from there on
    add("ins_and_del", 100, [(1, 99, 1, [40], [40, 60])])              # deletion 60 never fires: one pad blank more
    add("del_and_sub", 100, [(1, 99, 1, [], [40], [40, 50])])
    add("ins_and_sub", 100, [(99, 1, -1, [40], [], [40, 50])])
    add("twice_in_a_list", 100, [(1, 99, 1, [], [50, 50, 70])])        # 70 is behind the stuck cursor
    add("listed_by_two_genes", 120, [(1, 60, 1, [], [50]), (120, 61, -1, [], [50, 90], [100])])
    add("stuck_from_the_start", 100, [(1, 99, 1, [0, 20], [10])])      # position 0 is never reached: no insertion is applied
    # positions beyond the read
    add("beyond_L", 90, [(1, 90, 1, [91], [95, 96], [92])])
    # file order against start order, with edits in both (the shifts accumulate in file order)
    add("file_order", 120, [(61, 120, 1, [70], [80, 100]), (1, 57, 1, [], [20], [30]), (117, 58, -3, [65])])
    add("equal_starts", 120, [(1, 60, 1, [], [10]), (2, 31, 2, [15])])       # both adjusted starts are 0: the sort keeps file order
    # partial on the left, on the right, on both, in the three frames of both strands
    for k, (a, b) in enumerate([(0, 60), (-1, 60), (-2, 60), (40, 91), (40, 92), (40, 93), (0, 93), (-1, 92), (-2, 91)]):
        add("partial_fwd_%d" % k, 90, [(a, b, 1 + k % 3, [50] if k % 2 else [], [45] if k % 3 == 0 else [])])
        add("partial_rev_%d" % k, 90, [(b, a, -1 - k % 3, [], [50] if k % 2 else [], [47] if k % 3 == 1 else [])])
    # right-partial genes whose end moves beyond the pads: blanks inside the string (three starts: one survives the trim)
    add("pads_fwd", 90, [(1, 93, 1, [], [95])])
    add("pads_fwd_1", 90, [(2, 96, 2)])
    add("pads_fwd_2", 90, [(3, 97, 3, [], [200, 201])])
    add("pads_rev", 90, [(97, 3, -1, [], [200])])                      # a reverse gene skips the blanks of its start window
    # starts far to the left: the three-character start window never meets the pads at -6 and below
    add("left_of_pads", 90, [(-6, 60, 1), (-5, 61, 2), (-4, 62, 3), (-3, 63, 1)])
    add("left_of_pads_rev", 90, [(60, -6, -1), (61, -5, -2), (62, -4, -3)])
    add("end_inside_start", 90, [(30, 31, 1), (40, 38, -1), (50, 20, 1)])
    # substitutions on C, c, A and N; the same under a reverse gene
    add("sub_letters", 96, [(1, 96, 1, [], [], [10, 20, 30, 40]), ], [(10, "C"), (20, "c"), (30, "A"), (40, "N")])
    add("sub_letters_rev", 96, [(96, 1, -1, [], [], [10, 20, 30, 40, 50]), ], [(10, "C"), (20, "c"), (30, "A"), (40, "N"), (50, "g")])
    # lower case and ambiguity letters under reverse and forward genes
    add("letters_rev", 96, [(96, 1, -1, [33], [60]), (4, 96, 1)], [(10, "acgtn"), (25, "RYKMN"), (44, "SWBDHV"), (70, "x")])
    add("no_genes", 60, [])
    # random genes and edit lists
    for k in range(12):
        L = rng.randrange(60, 121)
        s = _seq(rng, L)
        for _ in range(rng.randrange(0, 4)):
            s = _put(s, rng.randrange(1, L + 1), rng.choice("acgtNRC"))
        lines = []
        for g in range(rng.randrange(1, 4)):
            a, b = sorted((rng.randrange(-5, L + 1), rng.randrange(1, L + 7)))
            lists = [sorted(rng.randrange(1, L + 3) for _ in range(rng.choice((0, 0, 1, 2, 3)))) for _ in range(3)]
            f = rng.randrange(1, 4)
            lines.append(_line(g + 1, *((a, b, f) if rng.random() < 0.5 else (b, a, -f)), *lists))
        reads.append(("random_%d" % k, s, lines))
    return reads


def main():
    script = sys.argv[1] if len(sys.argv) > 1 else "/root/reference/scripts/extract_aa.py"
    ns = load_script(script)
    os.makedirs(OUT, exist_ok=True)
    sizes = {}
    with tempfile.TemporaryDirectory() as tmp, io.open(os.path.join(OUT, "recorded.sha256"), "w", newline="\n") as digests:
        for name in REAL:
            run_script(ns, os.path.join(HERE, "data", "seqs.fa"), os.path.join(HERE, "predict", name + ".predict"), os.path.join(tmp, name))
            for ext in (".ffn", ".faa"):
                data = open(os.path.join(tmp, name + ext), "rb").read()
                digests.write("%s  %s\n" % (hashlib.sha256(data).hexdigest(), name + ext))
            sizes[name] = (data.count(b">"), os.path.getsize(os.path.join(tmp, name + ".ffn")))
    reads = edges()
    with io.open(os.path.join(OUT, "edges.fa"), "w", newline="\n") as fa, io.open(os.path.join(OUT, "edges.predict"), "w", newline="\n") as pr:
        for k, (name, seq, lines) in enumerate(reads):
            fa.write(">%s\n" % name)
            width = 60 if k % 2 else 70                  # (sequence lines of two widths: the reads span two and one lines)
            for i in range(0, len(seq), width):
                fa.write(seq[i:i + width] + "\n")
            pr.write(">%s\n" % name)
            for line in lines:
                pr.write(line + "\n")
    run_script(ns, os.path.join(OUT, "edges.fa"), os.path.join(OUT, "edges.predict"), os.path.join(OUT, "edges"))
    ffn = open(os.path.join(OUT, "edges.ffn")).read().split("\n")
    strings = ffn[1::2]
    assert any(" " in s.strip(" ") or (s != s.strip(" ") and s.strip(" ")) for s in strings), "no blank in any string"
    assert any(s.startswith(" ") for s in strings) and any(s.endswith(" ") for s in strings), "blanks at one side only"
    assert any(s == "" for s in strings), "no empty record"
    sizes["edges"] = (len(strings), os.path.getsize(os.path.join(OUT, "edges.ffn")))
    for name in REAL + ["edges"]:
        print("%-18s %4d genes, %6d bytes of .ffn" % ((name,) + sizes[name]))


if __name__ == "__main__":
    main()
