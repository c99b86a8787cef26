"""A sequential Python 3 restatement of the reference's scripts/train_features.py, `--predict P --seq S` path (test
infrastructure: the yardstick of gmg_features_count, gmg_features_format and integration/train-features_gpu).

Written from the script's semantics, line numbers below refer to it:
  parse_predict (163-199), parse_genes (223-280), forward_parse_nongenes (320-467) on the sequence and on its reverse
  complement (497-509), destrand_orientations (544-554), output_stats (562-623), output_featurefile (630-673),
  build_icm's gene strings (731-753), compute_gc (524-533).
One thing is decided here because the script leaves it open: sequences are taken in the order of their first appearance in the
predict file (the script iterates a Python 2 dict).  Only the fractional bins and the order of the gene strings depend on it.
Python 2's `/` on ints is floor division: `//` here.
"""
import hashlib
import os

STARTS = ("ATG", "GTG", "TTG")
ORIENTS = ((1, 1), (1, -1), (-1, 1), (-1, -1))
_RC = str.maketrans("ATCGatcg", "TAGCtagc")

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def rc(seq):
    return seq.translate(_RC)[::-1]


def stops_of(drop_tga=False):
    return ("TAG", "TAA", "XXX" if drop_tga else "TGA")


class Gene:
    __slots__ = ("start", "end", "frame_start", "frame_end", "strand", "start_codon", "stop_codon")

    def __init__(self, start, end, frame_start, frame_end, strand, start_codon, stop_codon):
        self.start, self.end, self.frame_start, self.frame_end = start, end, frame_start, frame_end
        self.strand, self.start_codon, self.stop_codon = strand, start_codon, stop_codon


def parse_seqs(text):
    """-> dict header -> sequence, in file order (a repeated header starts over, as the script's assignment does)"""
    seqs, header = {}, None
    for line in text.splitlines():
        if line[:1] == ">":
            header = line[1:].rstrip()
            seqs[header] = ""
        elif header is not None:
            seqs[header] += line.rstrip()
    return seqs


def gene_of(fields, L):
    """one gene line's fields (id, a, b, frame, ...) on a sequence of L letters"""
    if int(fields[3]) > 0:
        strand, start, end = 1, int(fields[1]) - 1, int(fields[2])
        start_codon, stop_codon = start >= 0, end <= L
        frame_start, frame_end = start + 3 * (1 - int(start_codon)), end - 3 * (1 - int(stop_codon))
    else:
        strand, start, end = -1, int(fields[2]) - 1, int(fields[1])
        stop_codon, start_codon = start >= 0, end <= L
        frame_start, frame_end = start + 3 * (1 - int(stop_codon)), end - 3 * (1 - int(start_codon))
    return Gene(max(0, start), min(end, L), frame_start, frame_end, strand, start_codon, stop_codon)


def parse_predict(predict_text, seqs):
    """-> dict header -> [Gene], headers in the order of their first gene line"""
    genes, header = {}, None
    for line in predict_text.splitlines():
        if line[:1] == ">":
            header = line[1:].rstrip()
        elif line.split():
            genes.setdefault(header, []).append(gene_of(line.split(), len(seqs[header])))
    return genes


def init_stats():
    return {"lengths": {}, "start_codons": dict.fromkeys(STARTS, 0), "adj_orients": dict.fromkeys(ORIENTS, 0),
            "adj_dist": {o: {} for o in ORIENTS}}


def count_genes(stats, genes, seqs, max_overlap):
    for header, hgenes in genes.items():
        hseq = seqs[header]
        last = None
        for g in hgenes:
            n = (g.end - 3 - g.start) // 3
            stats["lengths"][n] = stats["lengths"].get(n, 0) + 1
            s = hseq[g.start:g.end] if g.strand == 1 else rc(hseq[g.start:g.end])
            if g.start_codon and s[:3] in STARTS:
                stats["start_codons"][s[:3]] += 1
            if last is not None:
                o = (last.strand, g.strand)
                stats["adj_orients"][o] += 1
                d = g.start - last.end
                if -d <= max_overlap:
                    stats["adj_dist"][o][d] = stats["adj_dist"][o].get(d, 0) + 1
            last = g


def count_nongenes_pass(stats, pass_strand, genes, seqs, min_length, max_overlap, stops, trace=None):
    lengths, starts, orients, dist = stats["lengths"], stats["start_codons"], stats["adj_orients"], stats["adj_dist"]
    for header, hgenes in genes.items():
        hseq = seqs[header]
        L = len(hseq)
        pre_i = 0
        items = [i for i in range(L) if hseq[i:i + 3] in stops] + [L, L + 1, L + 2]
        for si in items:
            pre_i = max(pre_i, 0)
            while pre_i < len(hgenes) and hgenes[pre_i].end - 3 < si:
                pre_i += 1
            suc_i = pre_i if pre_i < len(hgenes) else -1
            pre_i -= 1
            if suc_i != -1:
                if hgenes[suc_i].end - 3 == si or si - hgenes[suc_i].start + 3 > max_overlap:
                    continue
            # the starts of this item, downwards: (ci, codon or '' for the pseudo-start)
            found = []
            ci = si
            while ci >= 0:
                ci -= 3
                codon = hseq[ci:ci + 3] if ci >= 0 else ""
                if codon in stops:
                    break
                if codon == "" or codon in STARTS:
                    if pre_i != -1 and hgenes[pre_i].end - ci > max_overlap:
                        break
                    found.append((ci, codon))
            num_starts = sum(1 for ci, _ in found if 3 * ((si - ci) // 3) >= min_length)
            for ci, codon in found:
                n = (si - ci) // 3
                lengths[n] = lengths.get(n, 0) + 1
                if 3 * n < min_length:
                    continue
                if codon:
                    starts[codon] += 1
                if pre_i != -1:
                    g = hgenes[pre_i]
                    o = (g.strand, 1) if pass_strand == 1 else (-1, -g.strand)
                    orients[o] += 1.0 / num_starts
                    d = ci - g.end
                    dist[o][d] = dist[o].get(d, 0) + 1.0 / num_starts
                    if trace is not None:
                        trace.append((o, d, num_starts))
                if suc_i != -1:
                    g = hgenes[suc_i]
                    o = (1, g.strand) if pass_strand == 1 else (-g.strand, -1)
                    orients[o] += 1.0 / num_starts
                    d = g.start - (si + 3)
                    dist[o][d] = dist[o].get(d, 0) + 1.0 / num_starts
                    if trace is not None:
                        trace.append((o, d, num_starts))


def mirror(genes, seqs):
    rgenes, rseqs = {}, {}
    for header, hgenes in genes.items():
        rseqs[header] = rc(seqs[header])
        L = len(rseqs[header])
        rgenes[header] = [Gene(L - g.end, L - g.start, L - g.frame_end, L - g.frame_start, -g.strand, g.start_codon, g.stop_codon)
                          for g in hgenes[::-1]]
    return rgenes, rseqs


def destrand(stats):
    o, d = stats["adj_orients"], stats["adj_dist"]
    stats["raw_orients"] = dict(o)
    o[(1, 1)] = (o[(1, 1)] + o[(-1, -1)]) / 2.0
    o[(-1, -1)] = o[(1, 1)]
    for l in list(d[(1, 1)].keys()) + list(d[(-1, -1)].keys()):
        d[(1, 1)][l] = (d[(1, 1)].get(l, 0) + d[(-1, -1)].get(l, 0)) / 2.0
        d[(-1, -1)][l] = d[(1, 1)][l]


def count(genes, seqs, min_length=75, max_overlap=50, drop_tga=False, trace=None):
    """-> (gene stats, non-gene stats) after destrand_orientations; stats['raw_orients'] keeps the four sums before it.
    trace: a list that receives (orientation, distance, num_starts) of every fractional term, in the order they are added"""
    stops = stops_of(drop_tga)
    gs, ns = init_stats(), init_stats()
    count_genes(gs, genes, seqs, max_overlap)
    count_nongenes_pass(ns, 1, genes, seqs, min_length, max_overlap, stops, trace)
    rgenes, rseqs = mirror(genes, seqs)
    count_nongenes_pass(ns, -1, rgenes, rseqs, min_length, max_overlap, stops, trace)
    destrand(gs)
    destrand(ns)
    return gs, ns


# ---- output ------------------------------------------------------------------------------------------------------------------

def _lengths(stats):
    if not stats["lengths"]:
        return ""
    return "".join("%d\t%d\n" % (l, stats["lengths"].get(l, 0)) for l in range(1 + max(stats["lengths"].keys())))


def _starts(stats):
    return "".join("%s\t%d\n" % (sc, stats["start_codons"][sc]) for sc in STARTS)


def _orients(stats):
    return "".join("%d,%d\t%d\n" % (a, b, stats["adj_orients"][(a, b)]) for a, b in ORIENTS)


def _dist(stats, o, max_overlap):
    d = stats["adj_dist"][o]
    if not d:
        return ""
    return "".join("%d\t%.1f\n" % (l, d.get(l, 0)) for l in range(-max_overlap, 1 + max(d.keys())))


def feature_block(stats, orf_type, max_overlap=50):
    out = "DIST LENGTH %s\n%s\n" % (orf_type, _lengths(stats))
    out += "DIST START %s\n%s\n" % (orf_type, _starts(stats))
    out += "DIST ADJACENT_ORIENTATION %s\n%s\n" % (orf_type, _orients(stats))
    for a, b in ORIENTS[:3]:
        out += "DIST ADJACENT_DISTANCE_%d_%d %s\n%s\n" % (a, b, orf_type, _dist(stats, (a, b), max_overlap))
    return out


def feature_file(gs, ns, max_overlap=50):
    return feature_block(gs, "GENE", max_overlap) + feature_block(ns, "NON", max_overlap)


def stat_files(gs, ns, max_overlap=50):
    """-> {file suffix: text} of output_stats for both tables"""
    out = {}
    for stats, tag in ((gs, "genes"), (ns, "non")):
        out["lengths.%s.txt" % tag] = _lengths(stats)
        out["starts.%s.txt" % tag] = _starts(stats)
        out["adj_orients.%s.txt" % tag] = _orients(stats)
        for a, b in ORIENTS[:3]:
            out["adj_dist.%d.%d.%s.txt" % (a, b, tag)] = _dist(stats, (a, b), max_overlap)
    return out


def gc_text(seqs):
    gc = sum(s.count("C") + s.count("G") for s in seqs.values())
    at = sum(s.count("A") + s.count("T") for s in seqs.values())
    return "%f\n" % (float(gc) / (float(at) + float(gc)))


def gene_strings(genes, seqs):
    """build_icm's records: [(header line without '>', string)]"""
    out = []
    for header, hgenes in genes.items():
        hseq = seqs[header]
        for g in hgenes:
            if g.strand == 1:
                s = hseq[g.frame_start:g.frame_end - 3 * int(g.stop_codon)]
            else:
                s = rc(hseq[g.frame_start + 3 * int(g.stop_codon):g.frame_end])
            out.append(("%s_%d-%d_%d%d" % (header, g.start, g.end, int(g.start_codon), int(g.stop_codon)), s))
    return out


def gene_fasta(records):
    return "".join(">%s\n%s\n" % r for r in records)


def sections(text):
    """a feature file's sections: {title line: body}"""
    out = {}
    for block in text.split("\n\n"):
        if block.strip():
            head, _, body = block.partition("\n")
            out[head] = body
    return out


def sha256(text):
    return hashlib.sha256(text.encode("latin-1")).hexdigest()


def load(predict_path, seq_path):
    with open(seq_path, encoding="latin-1") as fp:
        seqs = parse_seqs(fp.read())
    with open(predict_path, encoding="latin-1") as fp:
        genes = parse_predict(fp.read(), seqs)
    return genes, seqs
