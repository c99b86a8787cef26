"""Plain-Python restatement of the reference's window-acgt and uncovered (src/Util/window-acgt.cc, src/Util/uncovered.cc), letter by
letter: the ring buffer itself, the sort-and-merge itself.  The device calls gmg_window_counts / gmg_regions_uncovered
(glimmer-mg_amd/csrc/gmg_windows.hip) and the host planner gmg_uncovered_plan are tested against it; the restatement itself is
pinned to outputs recorded from the reference's programs (tests/golden/windows/cases.json, tests/test_windows_host.py).

Every program function returns (stdout, stderr, flagged): flagged = [(input line, why)] names the lines at which the reference
leaves its buffers or reads the file otherwise than gmg_fasta_ingest does."""

import audit_oracle as ao

MAX_LINE = 300                                           # src/Common/delcher.hh

SUBSCRIPT = {"a": 0, "c": 1, "g": 2, "t": 3}


def subscript(ch):
    """window-acgt.cc:233-252"""
    return SUBSCRIPT.get(ch.lower(), 4)


def percent(a, b):
    """Percent (src/Common/delcher.cc:201-211): 100.0 * (a / b) in that order -- 4085 of 10000 prints as 40.8 -- and 0 for b = 0"""
    return 0.0 if b == 0 else 100.0 * (float(a) / float(b))


def window_rows(seq, window_len, window_skip):
    """the lines window-acgt prints for one record's letters: [(position, size, [a, c, g, t, other])], by the ring buffer of
    window-acgt.cc:58-137"""
    window = [""] * window_len
    rows = []
    win_pos = win_next = 1
    win_sub = win_size = last_pos = 0
    count = [0] * 5
    for ch in seq:
        if win_size == window_len:
            count[subscript(window[win_sub])] -= 1
            win_pos += 1
        else:
            win_size += 1
        count[subscript(ch)] += 1
        window[win_sub] = ch
        win_sub = (win_sub + 1) % window_len
        if win_size == window_len and win_pos == win_next:
            rows.append((win_pos, win_size, list(count)))
            last_pos = win_pos
            win_next += window_skip
    if win_pos != last_pos:                              # Finish
        while win_pos < win_next and win_size > 0:
            count[subscript(window[win_sub])] -= 1
            win_pos += 1
            win_size -= 1
            win_sub = (win_sub + 1) % window_len
        if win_size > 0:
            rows.append((win_pos, win_size, list(count)))
    return rows


def closed_form_windows(L, W, S):
    """[(position, size)] as include/gmg.h states them"""
    if L == 0:
        return []
    if L < W:
        return [(1, L)]
    k = (L - W) // S
    out = [(1 + j * S, W) for j in range(k + 1)]
    if (L - W) % S != 0 and (k + 1) * S < L:
        out.append((1 + (k + 1) * S, L - (k + 1) * S))
    return out


def batch_window_counts(seqs, window_len, window_skip):
    """what gmg_window_counts returns for a batch of strings: (read_window_off, rows [[a, c, g, t, other]])"""
    off, rows = [0], []
    for s in seqs:
        rows += [c for _, _, c in window_rows(s, window_len, window_skip)]
        off.append(len(rows))
    return off, rows


def ambiguous_bases(seqs):
    """job-wide indices of the letters outside acgtACGT (gmg_fasta_ambiguous's numbering)"""
    out, base = [], 0
    for s in seqs:
        out += [base + i for i, ch in enumerate(s) if ch not in "acgtACGT"]
        base += len(s)
    return out


def window_acgt(text, window_len, window_skip, percents=False):
    """window-acgt W S < text: the whole program (window-acgt.cc:58-137), line by line as fgets with MAX_LINE hands them out"""
    out, flagged = [], []
    window = [4] * window_len                            # (the ring buffer holds Subscript of its letters)
    win_pos = win_next = 1
    win_sub = win_size = last_pos = 0
    count = [0] * 5
    sub = [4] * 256
    for ch, k in (("a", 0), ("c", 1), ("g", 2), ("t", 3)):
        sub[ord(ch)] = sub[ord(ch.upper())] = k
    if percents:
        def print_line(pos, size):
            out.append("%8d %7d %6.1f %6.1f %6.1f %6.1f %6.1f %6.1f\n" % ((pos, size) + tuple(percent(c, size) for c in count)
                                                                          + (percent(count[1] + count[2], size),)))
    else:
        def print_line(pos, size):
            out.append("%8d %7d %6d %6d %6d %6d %6d %6.1f\n" % (pos, size, count[0], count[1], count[2], count[3], count[4],
                                                                percent(count[1] + count[2], size)))

    def finish(win_pos, win_size, win_sub):
        while win_pos < win_next and win_size > 0:
            count[window[win_sub]] -= 1
            win_pos += 1
            win_size -= 1
            win_sub = (win_sub + 1) % window_len
        if win_size > 0:
            print_line(win_pos, win_size)

    seen_header = False
    for ln, line in enumerate(text.splitlines(keepends=True)):
        if "\0" in line:
            flagged.append((ln, "NUL byte"))
        if len(line) >= MAX_LINE:
            flagged.append((ln, "line too long"))
        body = line.split()
        if body and body[0][0] == ">":                   # First_Non_Blank (line) == '>'
            seen_header = True
            if win_pos != last_pos:
                finish(win_pos, win_size, win_sub)
            out.append(line)
            out.append("%8s %7s %6s %6s %6s %6s %6s %6s\n" % ("Position", "Length", "As", "Cs", "Gs", "Ts", "Other", "%GC"))
            win_pos = win_next = 1
            win_sub = win_size = last_pos = 0
            count[:] = [0] * 5
            continue
        if not seen_header and body:
            flagged.append((ln, "sequence before the first header"))
        if ">" in line:
            flagged.append((ln, "'>' inside a sequence line"))
        for ch in "".join(body).encode("latin-1"):
            k = sub[ch]
            if win_size == window_len:
                count[window[win_sub]] -= 1
                win_pos += 1
            else:
                win_size += 1
            count[k] += 1
            window[win_sub] = k
            win_sub += 1
            if win_sub == window_len:
                win_sub = 0
            if win_pos == win_next and win_size == window_len:
                print_line(win_pos, win_size)
                last_pos = win_pos
                win_next += window_skip
    if win_pos != last_pos:
        finish(win_pos, win_size, win_sub)
    return "".join(out), "", flagged


# ---- uncovered -----------------------------------------------------------------------------------------------------------------

def too_long(line):
    """a coordinate line that fgets (line, MAX_LINE) hands over in pieces"""
    return len(line) >= MAX_LINE - 1 and not (len(line) == MAX_LINE - 1 and line.endswith("\n"))


def coord_intervals(lengths, coords_text, use_dir=False, circular=True, skip_start=False, skip_stop=False, tags=None):
    """uncovered.cc:81-175: coordinate lines -> ([(record, lo, hi)] in the order of the lines, stderr, flagged).  tags: the records'
    tags, --multi of uncovered_gpu: a line is <id> <tag> <start> <end> [<dir>]; otherwise every line is about record 0"""
    regions, err, flagged = [], [], []
    for ln, line in enumerate(coords_text.splitlines(True)):
        if too_long(line):
            flagged.append((ln, "line too long"))
            continue
        f = ao.scan_fields(line, 3 if use_dir else 2, 2 if tags is not None else 1)
        if f is None:
            err.append("ERROR:  Skipped following coord line\n" + line)
            continue
        rec = 0
        if tags is not None:
            if f[0][1] not in tags:
                flagged.append((ln, "unknown sequence"))
                continue
            rec = tags.index(f[0][1])
        seq_len = lengths[rec]
        start, end = f[1][:2]
        if use_dir:
            d = f[1][2]
        elif (start < end and (not circular or end - start <= seq_len // 2)) or (circular and start - end > seq_len // 2):
            d = 1
        else:
            d = -1
        made = []
        if d > 0:
            extract_len = 1 + end - start
            if extract_len < 0:
                extract_len += seq_len
            i = start - 1
            if skip_start:
                i += 3
                extract_len -= 3
            if skip_stop:
                extract_len -= 3
            j = i + extract_len
            if j <= seq_len:
                made.append((i, j))
            else:
                made += [(i, seq_len), (0, j - seq_len)]
        else:
            extract_len = 1 + start - end
            if extract_len < 0:
                extract_len += seq_len
            i = start
            if skip_start:
                i -= 3
                extract_len -= 3
            if skip_stop:
                extract_len -= 3
            j = i - extract_len
            if j >= 0:
                made.append((j, i))
            else:
                made += [(0, i), (seq_len + j, seq_len)]
        if any(not (0 <= lo <= hi <= seq_len) for lo, hi in made):
            flagged.append((ln, "off the sequence"))
            continue
        regions += [(rec, lo, hi) for lo, hi in made]
    return regions, "".join(err), flagged


def coalesce(regions):
    """Coalesce_Regions, uncovered.cc:186-214 (the order sort gives equal lo does not reach the result)"""
    lst = sorted(list(r) for r in regions)
    if not lst:
        return lst
    j = 0
    for i in range(1, len(lst)):
        if lst[i][0] <= lst[j][1]:
            if lst[j][1] < lst[i][1]:
                lst[j][1] = lst[i][1]
        else:
            j += 1
            lst[j] = lst[i]
    return lst[:j + 1]


def uncovered_gaps(seq_len, regions, min_len=0):
    """Output_Uncovered, uncovered.cc:254-288: [(a, len)] of the gaps it prints"""
    gaps, a = [], 0
    for lo, hi in coalesce(regions):
        ln = lo - a
        if ln > 0 and ln >= min_len:
            gaps.append((a, ln))
        a = hi
    ln = seq_len - a
    if ln > 0 and ln >= min_len:
        gaps.append((a, ln))
    return gaps


def batch_uncovered(lengths, intervals, min_len=0):
    """what gmg_regions_uncovered returns: (gaps [(read, first, len, 1)], read_gap_off); intervals = [(read, lo, hi)] in any order"""
    per = [[] for _ in lengths]
    for r, lo, hi in intervals:
        per[r].append((lo, hi))
    gaps, off = [], [0]
    for r, L in enumerate(lengths):
        gaps += [(r, a, ln, 1) for a, ln in uncovered_gaps(L, per[r], min_len)]
        off.append(len(gaps))
    return gaps, off


def format_gaps(seq, gaps, fasta_format=True, first_tag=1):
    """Output_Subsequence for every gap of one sequence; tags count from first_tag.  -> (text, the last tag's number)"""
    out, ct = [], first_tag - 1
    for a, ln in gaps:
        ct += 1
        tag = "seq%05d" % ct
        piece = seq[a:a + ln]
        if fasta_format:
            out.append(">%s  %d %d  len=%d\n" % (tag, a + 1, a + ln, ln))
            out.append("\n".join(piece[k:k + 60] for k in range(0, ln, 60)) + "\n")
        else:
            out.append("%-10s " % tag + piece + "\n")
    return "".join(out), ct


def uncovered(records, coords_text, min_len=0, fasta_format=True, multi=False, **kw):
    """uncovered [options] SEQ COORDS on the first record of records = [(tag, letters)]; multi: uncovered_gpu --multi, the gaps of all
    records in file order, the tag counter running on"""
    recs = records if multi else records[:1]
    lengths = [len(s) for _, s in recs]
    regions, err, flagged = coord_intervals(lengths, coords_text, tags=[t for t, _ in recs] if multi else None, **kw)
    if flagged:
        return "", err, flagged
    out, ct = [], 0
    for r, (_, seq) in enumerate(recs):
        text, ct = format_gaps(seq, uncovered_gaps(len(seq), [(lo, hi) for rr, lo, hi in regions if rr == r], min_len), fasta_format, ct + 1)
        out.append(text)
    return "".join(out), err, flagged


# ---- entropy-fasta -------------------------------------------------------------------------------------------------------------

def fasta_read(text):
    """[(hdr, letters)] as Fasta_Read (src/Common/fasta.cc:236-283) hands the records over: hdr = the header line behind '>' and its
    leading blanks, letters = every byte up to the next '>' that is no white space"""
    out = []
    for chunk in text.split(">")[1:]:
        hdr, _, body = chunk.partition("\n")
        out.append((hdr.lstrip(" "), "".join(body.split())))
    return out


def entropy_fasta(text):
    """entropy-fasta < text (src/Util/entropy-fasta.cc:48-107) -> (stdout, stderr, flagged, status).  A record whose length is no
    multiple of 3 ends the program with status 1"""
    import entropy_oracle as eo
    aa = eo.tables()[11]
    out, flagged = [], []
    if "\0" in text:
        flagged.append((0, "NUL byte"))
    for hdr, seq in fasta_read(text):
        if len(seq) % 3 != 0:
            return "".join(out), hdr + " not divisible by 3\n", flagged, 1
        count = [0] * 20
        low = seq.lower()
        for c in range(0, len(seq), 3):
            code = ao.codon_code(low[c:c + 3])
            k = eo.AMINO.find(aa[code]) if code >= 0 else -1
            if k >= 0:
                count[k] += 1
        out.append(">%s\t%g\n%s\n" % (hdr, eo.finish(count, eo.POS, eo.NEG)[2], seq))
    return "".join(out), "", flagged, 0
