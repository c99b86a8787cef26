"""Python restatement of what extract / multi-extract PRINT (tests only): Output_Subsequence's record rule on top of
extract_oracle.region_chars and complement, and the two programs' command lines around it.  Written from the semantics in
include/gmg.h (gmg_regions_text), not from the library's code; the skip and length decisions are gmg_extract_plan's, which
tests/test_extract_host.py pins to the recorded runs."""
import extract_oracle as xo

WIDTH = 60


def record(head, letters, width=WIDTH):
    """head, then the letters with a newline in front of a letter whenever `width` letters stand on the line (0: never), and a
    final newline: 61 letters at width 60 are 60, newline, 1, newline; 60 letters are 60, newline; none is a newline"""
    if width:
        letters = "\n".join(letters[i:i + width] for i in range(0, len(letters), width))
    return head + letters + "\n"


def region_record(seq, region, head, width=WIDTH):
    _, first, n, strand = region
    return record(head, xo.region_chars(seq, first, n, strand) if n else "", width)


def two_field_head(tag):
    return "%-10s " % tag


def run(gmg, program, opts, fasta, coords_text):
    """`program` ("extract" or "multi-extract") with the options opts (a list as on the command line, without the two files) ->
    ([(id of the coordinate line, its record)] in the order of the lines (extract) or by record of the file and then by line
    (multi-extract: the reference's order among the lines of one tag is its std::sort's), stderr)"""
    multi = program == "multi-extract"
    fasta_out, flags, min_len, k = True, 0, 0, 0
    while k < len(opts):
        o = opts[k]
        if o == "-2":
            fasta_out = False
        elif o == "-l":
            k += 1
            min_len = int(opts[k])
        else:
            flags |= {"-d": gmg.COORD_USE_DIR, "-s": gmg.COORD_SKIP_START, "-t": gmg.COORD_SKIP_STOP, "-w": gmg.COORD_NOWRAP}[o]
        k += 1
    use_dir = bool(flags & gmg.COORD_USE_DIR)
    recs = [(h.split()[0].decode() if h.split() else "", s) for h, s in xo.records(fasta)]
    if not multi:
        recs = recs[:1]
    err, lines = "", []
    for line in coords_text.splitlines(True):
        f = line.split()
        want = (2 if multi else 1) + 2 + (1 if use_dir else 0)
        if len(f) < want or not all(xo._is_int(x) for x in f[want - 2 - use_dir:want]):
            err += "ERROR:  Skipped following coord line\n" + line
            continue
        nums = [int(x) for x in f[want - 2 - use_dir:want]]
        lines.append((f[0], f[1] if multi else None, nums[0], nums[1], nums[2] if use_dir else 0))
    rows, src = [], []
    if multi:
        for r, (tag, _) in enumerate(recs):
            for ln in lines:
                if ln[1] == tag:
                    rows.append((r, ln[2], ln[3], ln[4]))
                    src.append(ln)
        flags |= gmg.COORD_MULTI
    else:
        rows, src = [(0, ln[2], ln[3], ln[4]) for ln in lines], lines
    off = [0]
    for _, s in recs:
        off.append(off[-1] + len(s))
    regions, line_of = gmg.extract_plan(off, rows, flags, min_len)
    out = []
    for region, ln in zip(regions, line_of):
        name, tag, start, end, _ = src[int(ln)]
        if not fasta_out:
            head = two_field_head(tag if multi else name)
        elif multi:
            head = ">%s  %s  %d %d  len=%d\n" % (name, tag, start, end, region[2])
        else:                                           # (the start moves with the letters under -s; multi-extract's does not)
            if flags & gmg.COORD_SKIP_START:
                start += 3 if region[3] > 0 else -3
            head = ">%s  %d %d  len=%d\n" % (name, start, end, region[2])
        out.append((name, region_record(recs[region[0]][1], region, head, WIDTH if fasta_out else 0)))
    return out, err


def body_lines_ok(text_out):
    """every body line of a multi-fasta text holds 60 letters, except the last of its record (1 .. 60, or none for an empty record)"""
    recs, cur = [], None
    for line in text_out.split("\n")[:-1]:
        if line.startswith(">"):
            cur = []
            recs.append(cur)
        else:
            cur.append(line)
    return all(all(len(x) == WIDTH for x in body[:-1]) and (len(body[-1]) <= WIDTH and (len(body) == 1 or body[-1])) for body in recs)
