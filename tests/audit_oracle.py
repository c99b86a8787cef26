"""A plain Python restatement of what gmg_genes_audit promises (include/gmg.h), letter by letter as the reference compares them:
anomaly lower-cases the raw letters, complements them on the reverse strand (Complement, src/Common/gene.cc) and tests codons with
strncmp against lower-case patterns (src/Glimmer/anomaly.cc:254-286), so a codon matches exactly when its three letters are
acgt letters (either case) that spell a pattern.  No numpy in the arithmetic, no sharing with the library."""

COMP = {"a": "t", "c": "g", "g": "c", "t": "a"}
CODE = {"a": 0, "c": 1, "g": 2, "t": 3}


_FWD = "".join(chr(c).lower() if chr(c).lower() in CODE else "n" for c in range(256))
_REV = "".join(COMP.get(chr(c).lower(), "n") for c in range(256))


def region_letters(seq, first, length, strand, count=None, offset=0):
    """letters of region offsets offset .. offset + count - 1 in reading direction, lower-cased and (strand < 0) complemented;
    a letter outside acgt comes out as 'n'"""
    L = len(seq)
    n = length if count is None else count
    if n <= 0:
        return ""
    if n > L or any(ord(ch) > 255 for ch in seq[:1]):   # (more than once round: letter by letter)
        idx = [(first + i) % L if strand > 0 else (first - i) % L for i in range(offset, offset + n)]
        return "".join((_FWD if strand > 0 else _REV)[ord(seq[k]) & 255] for k in idx)
    lo = (first + offset) % L if strand > 0 else (first - offset - (n - 1)) % L      # the lowest position, then upwards with one wrap
    piece = seq[lo:lo + n] + seq[:max(lo + n - L, 0)]
    return piece.translate(_FWD) if strand > 0 else piece[::-1].translate(_REV)


def codon_code(letters):
    if len(letters) != 3 or any(ch not in CODE for ch in letters):
        return -1
    return 16 * CODE[letters[0]] + 4 * CODE[letters[1]] + CODE[letters[2]]


def which(letters, patterns):
    for k, p in enumerate(patterns):
        if letters == p:
            return k
    return -1


def audit_region(seq, first, length, strand, starts, stops, next_stop=True):
    """-> dict of a gmg_gene_audit's fields, `inner` = the list of offsets in place of inner_begin"""
    L = len(seq)
    cod = lambda off: region_letters(seq, first, length, strand, 3, off)
    rec = {"first_codon": -1, "last_codon": -1, "start_which": -1, "stop_which": -1, "last_back_stop": -1, "next_stop": -1}
    if length >= 3:
        rec["first_codon"], rec["last_codon"] = codon_code(cod(0)), codon_code(cod(length - 3))
        rec["start_which"], rec["stop_which"] = which(cod(0), starts), which(cod(length - 3), stops)
    rec["inner"] = [i for i in range(0, max(length - 3, 0), 3) if which(cod(i), stops) >= 0]
    rec["n_inner_stops"] = len(rec["inner"])
    for i in range(length - 6, -1, -3):
        if which(cod(i), stops) >= 0:
            rec["last_back_stop"] = i
            break
    if next_stop and rec["stop_which"] < 0:
        for j in range(length, L, 3):
            if which(cod(j), stops) >= 0:
                rec["next_stop"] = j
                break
    return rec


def audit_records(seqs, regions, starts=("atg", "gtg", "ttg"), stops=("taa", "tag", "tga"), next_stop=True):
    """seqs: the reads' letters; regions: (read, first, len, strand) -> (records [dict], inner [int], hist [65])"""
    recs, inner, hist = [], [], [0] * 65
    for read, first, length, strand in regions:
        r = audit_region(seqs[read], first, length, strand, starts, stops, next_stop)
        r["inner_begin"] = len(inner)
        inner += r["inner"]
        hist[64 if r["first_codon"] < 0 else r["first_codon"]] += 1
        recs.append(r)
    return recs, inner, hist


def ambiguous_bases(seqs):
    """ascending job-wide indices of the letters outside acgtACGT, the reads back to back"""
    out, base = [], 0
    for s in seqs:
        out += [base + i for i, ch in enumerate(s) if ch.lower() not in CODE]
        base += len(s)
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# The two programs, line by line: anomaly (src/Glimmer/anomaly.cc:72-240) and start-codon-distrib
# (src/Util/start-codon-distrib.cc:80-163).  Each returns, beside the text, the input lines at which the reference leaves its
# buffers or its outcome is accidental (what the *_gpu commands refuse).
# ---------------------------------------------------------------------------------------------------------------------------

MAX_LINE = 300                                          # the reference's fgets buffer: a longer line is read in pieces
IUPAC_COMP = dict(zip("acgtrykmbdhvswn", "tgcayrmkvhdbswn"))


def complement(ch):
    """Complement (tolower (letter)): the IUPAC complement; '*', '-', '.' and ' ' stay, anything else is 'n'"""
    return IUPAC_COMP.get(ch, ch if ch in "*-. " else "n")


def fasta_records(text):
    """[(tag, letters)] as Fasta_Read leaves them: everything but white space between two '>'; tag = the header's first token"""
    out = []
    for chunk in text.split(">")[1:]:
        hdr, _, body = chunk.partition("\n")
        out.append(((hdr.split() or [""])[0], "".join(body.split())))
    return out


def scan_fields(line, n_int, skip=1):
    """sscanf (line, "%s ... %ld ...") with `skip` leading %s: -> (strings, ints) when all convert, else None"""
    pos, strs, ints = 0, [], []
    n = len(line)
    for _ in range(skip):
        while pos < n and line[pos].isspace():
            pos += 1
        end = pos
        while end < n and not line[end].isspace():
            end += 1
        if end == pos:
            return None
        strs.append(line[pos:end])
        pos = end
    for _ in range(n_int):
        while pos < n and line[pos].isspace():
            pos += 1
        end = pos
        if end < n and line[end] in "+-":
            end += 1
        digits = end
        while end < n and line[end].isdigit():
            end += 1
        if end == digits:
            return None
        ints.append(int(line[pos:end]))
        pos = end
    return strs, ints


def coord_lines(text):
    """the lines as fgets hands them over (with their newline)"""
    return text.splitlines(True)


def direction(start, end, L, circular=True):
    return 1 if (start < end and (not circular or end - start <= L // 2)) or (circular and start - end > L // 2) else -1


def anomaly(records, coords, starts=("atg", "gtg", "ttg"), stops=("taa", "tag", "tga"), check_start=True, use_dir=False,
            circular=True, multi=False):
    """records: fasta_records(); coords: the coordinate file's text -> (stdout, stderr, flagged [(line number, why)])"""
    by_tag = {}
    for k, (tag, _) in enumerate(records):
        by_tag.setdefault(tag, k)
    out, flagged = [], []
    ok_ct = problem_ct = 0
    for ln, line in enumerate(coord_lines(coords)):
        if len(line) >= MAX_LINE - 1 and not (len(line) == MAX_LINE - 1 and line.endswith("\n")):
            flagged.append((ln, "line too long"))
            continue
        f = scan_fields(line, 3 if use_dir else 2, 2 if multi else 1)
        if f is None:
            out.append("Bad line:  %s\n...Skipping\n" % line)
            continue
        name, (start, end) = f[0][0], f[1][:2]
        if multi and f[0][1] not in by_tag:
            flagged.append((ln, "unknown sequence"))
            continue
        data = records[by_tag[f[0][1]] if multi else 0][1]
        L = len(data)
        d = (1 if f[1][2] > 0 else -1) if use_dir else direction(start, end, L, circular)
        gene_len = 1 + (end - start if d > 0 else start - end)
        if gene_len < 0:
            gene_len += L
        if gene_len < 3 or gene_len > L:
            flagged.append((ln, "gene length"))
            continue
        touched = [L + 1]                               # 1-based indices into Data (0 is its dummy letter)

        def letter(k):                                  # the gene's base k (and beyond: the walk for the next stop)
            p = start + k if d > 0 else start - k
            j = (p if p <= L else p - L) if d > 0 else (p if p >= 1 else p + L)
            if not 1 <= j <= L:
                touched[0] = j
                return "?"
            ch = data[j - 1].lower()
            return ch if d > 0 else complement(ch)

        buf = "".join(letter(k) for k in range(gene_len))
        if touched[0] != L + 1:
            flagged.append((ln, "off the sequence"))
            continue
        problem = False
        msgs = []
        is_stop = lambda s: s[:3] in stops
        if check_start and buf[:3] not in starts:
            msgs.append("%-10s has bad start codon = %.3s\n" % (name, buf))
            problem = True
        if not is_stop(buf[gene_len - 3:]):
            msgs.append("%-10s has bad stop codon = %s\n" % (name, buf[gene_len - 3:]))
            problem = True
            j = gene_len
            while j < L:
                if is_stop("".join(letter(j + i) for i in range(3))):
                    break
                j += 3
            if touched[0] != L + 1:
                flagged.append((ln, "walk off the sequence"))
                continue
            if j >= L:
                flagged.append((ln, "no later stop"))
                continue
            msgs.append("           next stop occurs at offset %d  Gene_Len = %d  diff = %+d\n" % (j, gene_len, j - gene_len + 3))
        counted = True
        if gene_len % 3:
            msgs.append("%-10s %8d %8d has %+d frame shift\n" % (name, start, end, gene_len % 3))
            problem = True
            i = 0
            while i < gene_len - 3 and not is_stop(buf[i:]):
                i += 3
            if i < gene_len - 3:
                stop = start + d * (i - 1)
                if stop < 1:
                    stop += L
                elif stop > L:
                    stop -= L
                msgs.append("   Best prefix is %8d %8d   Len = %d\n" % (start, stop, i))
                i = gene_len - 6
                while i >= 0 and not is_stop(buf[i:]):
                    i -= 3
                i += 3
                begin = start + d * i
                if begin < 1:
                    begin += L
                elif stop > L:
                    begin -= L
                msgs.append("   Best suffix is %8d %8d   Len = %d\n" % (begin, end, gene_len - i - 3))
            else:
                msgs.append("   No stop found in start frame\n")
                counted = False
        else:
            for i in range(0, gene_len - 3, 3):
                if is_stop(buf[i:]):
                    msgs.append("%-10s has stop codon %.3s at offset %d  Gene_Len = %d  diff = %+d\n" % (name, buf[i:], i, gene_len, gene_len - 3 - i))
                    problem = True
        out += msgs
        if counted:
            problem_ct += problem
            ok_ct += not problem
    return "".join(out), "     OK orfs = %7d\nProblem orfs = %7d\n" % (ok_ct, problem_ct), flagged


def start_codon_distrib(records, coords, use_dir=False, circular=True, comma3=False, multi=False):
    """-> (stdout, stderr, flagged [(line number, why)])"""
    by_tag = {}
    for k, (tag, _) in enumerate(records):
        by_tag.setdefault(tag, k)
    count, err, flagged = {}, [], []
    total = 0
    for ln, line in enumerate(coord_lines(coords)):
        if len(line) >= MAX_LINE - 1 and not (len(line) == MAX_LINE - 1 and line.endswith("\n")):
            flagged.append((ln, "line too long"))
            continue
        f = scan_fields(line, 3 if use_dir else 2, 2 if multi else 1)
        if f is None:
            err.append("ERROR:  Skipped following coord line\n" + line)
            continue
        start, end = f[1][:2]
        if multi and f[0][1] not in by_tag:
            flagged.append((ln, "unknown sequence"))
            continue
        seq = records[by_tag[f[0][1]] if multi else 0][1]
        L = len(seq)
        d = f[1][2] if use_dir else direction(start, end, L, circular)
        codon = []
        for i in range(3):
            sub = (start + i if d > 0 else start - i) - 1
            if not -L <= sub < 2 * L:
                flagged.append((ln, "off the sequence"))
                break
            if sub % L == L - 1:                        # Seq_Sub sends it to -1
                flagged.append((ln, "last base"))
                break
            ch = seq[sub % L].lower()
            codon.append(ch if d > 0 else complement(ch))
        else:
            key = "".join(codon)
            count[key] = count.get(key, 0) + 1
            total += 1
    if comma3:
        t = total or 1
        out = "%.3f,%.3f,%.3f\n" % tuple(count.get(c, 0) / t for c in ("atg", "gtg", "ttg"))
    else:
        rows = sorted(count.items(), key=lambda kv: (-kv[1], kv[0]))
        out = "".join(" %s   %6d  %5.1f%%\n" % (c, n, 100.0 * (n / total) if total else 0.0) for c, n in rows) + "Total: %6d\n" % total
    return out, "".join(err), flagged


def entropy_score(records, coords, use_dir=False, circular=True, min_len=0, skip_start=False, skip_stop=False, pos=None, neg=None,
                  multi=False):
    """entropy-score (src/Util/entropy-score.cc:81-160) -> (stdout, stderr, flagged).  A codon with a letter outside acgtACGT counts
    nowhere (Codon_Translation gives 'X'), a trailing partial codon neither"""
    import entropy_oracle as eo
    pos, neg = pos or eo.POS, neg or eo.NEG
    aa = eo.tables()[11]
    by_tag = {}
    for k, (tag, _) in enumerate(records):
        by_tag.setdefault(tag, k)
    out, err, flagged = [], [], []
    for ln, line in enumerate(coord_lines(coords)):
        if len(line) >= MAX_LINE - 1 and not (len(line) == MAX_LINE - 1 and line.endswith("\n")):
            flagged.append((ln, "line too long"))
            continue
        f = scan_fields(line, 3 if use_dir else 2, 2 if multi else 1)
        if f is None:
            err.append("ERROR:  Skipped following coord line\n" + line)
            continue
        start, end = f[1][:2]
        if multi and f[0][1] not in by_tag:
            flagged.append((ln, "unknown sequence"))
            continue
        seq = records[by_tag[f[0][1]] if multi else 0][1]
        L = len(seq)
        d = f[1][2] if use_dir else direction(start, end, L, circular)
        fwd = d > 0
        length = 1 + (end - start if fwd else start - end)
        if length < 0:
            length += L
        i = start - 1
        if skip_start:
            i += 3 if fwd else -3
            length -= 3
        if skip_stop:
            length -= 3
        if length < min_len:
            continue
        if length > L:
            flagged.append((ln, "region length"))
            continue
        if length <= 0:
            length, i = 0, 0
        if not -L <= i < 2 * L:
            flagged.append((ln, "off the sequence"))
            continue
        i %= L
        count = [0] * 20
        letters = region_letters(seq, i, length, 1 if fwd else -1)
        for c in range(0, length - 2, 3):
            code = codon_code(letters[c:c + 3])
            k = eo.AMINO.find(aa[code]) if code >= 0 else -1
            if k >= 0:
                count[k] += 1
        ratio = eo.finish(count, pos, neg)[2]
        out.append("%s \t%5.3f\n" % (line[:-1], ratio))
    return "".join(out), "".join(err), flagged


def moved_genes(predict_text, n=300):
    """the first n gene lines of a .predict file with the end, the start or both moved by +-1, +-2, +-3, +-4, -30 in rotation: the
    coordinate file whose anomaly run shows every kind of message (tests/golden/audit/cases.json, "generated:nc300_moved")"""
    genes = [l.split() for l in predict_text.splitlines() if l and not l.startswith(">")][:n]
    deltas = [1, -1, 2, -2, 3, -3, 4, -4, -30]
    out = []
    for k, g in enumerate(genes):
        start, end, d, what = int(g[1]), int(g[2]), deltas[k % 9], (k // 9) % 3
        if what != 0:
            start += d
        if what != 1:
            end += d
        out.append("%s %8d %8d  %s\n" % (g[0], start, end, g[3]))
    return "".join(out)
