//  anomaly_gpu.cc -- the reference's anomaly (src/Glimmer/anomaly.cc) around ONE gmg_genes_audit call (DESIGN.md 4.15,
//  INTEGRATION.md): every gene of a coordinate file checked for a start codon, a stop codon, a frame shift and in-frame stops.
//  The codons are classified on the device; every message of anomaly.cc:76-240 is formatted here from the records and the
//  letters of the file, stdout and the two count lines on stderr byte for byte.  New code, built from this repository alone.
//
//  usage: anomaly_gpu [-A list] [-s] [-Z list] [--multi] [-d] [-w] <sequence-file> <coord-file>
//
//  Kept although odd: a line that does not parse prints "Bad line:" to stdout; "No stop found in start frame" leaves the gene out
//  of both counts; the suffix's wrap test looks at the prefix's Stop (anomaly.cc:214-217).
//  Refused (status 1, one line on stderr that names the coordinate line, nothing on stdout), because the reference's outcome
//  there is an accident of its buffers: see kUsage.

#include "coords_common.h"

#include <getopt.h>
#include <stdarg.h>

using namespace coords;

namespace {

const char *kUsage =
    "USAGE:  anomaly_gpu [options] <sequence-file> <coord-file>\n"
    "\n"
    "Read DNA sequence in <sequence-file> and for each region specified\n"
    "by the coordinates in <coord-file>, check whether the region\n"
    "represents a normal gene, i.e., it begins with a start codon, ends\n"
    "with a stop codon, and has no frame shifts.\n"
    "Output goes to standard output.\n"
    "\n"
    "Options:\n"
    " -A <codon-list>   comma-separated start codons (default atg,gtg,ttg)\n"
    " -s                omit the check that the first codon is a start codon\n"
    " -Z <codon-list>   comma-separated stop codons (default taa,tag,tga)\n"
    " -d, --dir         take the direction from the column behind the coordinates\n"
    " -w, --nowrap      the sequence is not circular: a line is forward when start < end\n"
    " --multi           <sequence-file> holds many records; lines are <id> <sequence tag> <start> <end> [<dir>]\n"
    "\n"
    "Refused with status 1 and one line that names the coordinate line (the reference's outcome is accidental there):\n"
    "  -t altogether (the reference tests a stale letter)\n"
    "  a gene shorter than 3 bases or longer than the sequence\n"
    "  coordinates that one wrap does not bring onto the sequence\n"
    "  a gene without a stop codon whose search for the next one passes the end of the sequence twice, or finds none\n"
    "  a line of 299 characters or more; under --multi a sequence tag that no record has\n"
    "  start or stop codons that are not three letters of acgt, or more than 8 of either\n";

struct Gene {
    size_t line;                 // index into the lines
    std::string name;
    long start, end, len, seq_len;
    int dir;
    uint32_t rec;
};

void CodonList(const char *arg, char dst[8][4], int32_t *n)
{
    std::string s = arg;
    *n = 0;
    for (size_t pos = 0; pos <= s.size();) {
        size_t comma = s.find(',', pos);
        if (comma == std::string::npos) comma = s.size();
        if (comma > pos) {                               // (strtok skips empty fields)
            std::string c = s.substr(pos, comma - pos);
            for (char &ch : c) ch = (char)tolower((unsigned char)ch);
            if (c.size() != 3 || *n >= 8) Die(1, "codon list '%s': up to 8 codons of three letters of acgt", arg);
            memcpy(dst[(*n)++], c.c_str(), 4);
        }
        pos = comma + 1;
    }
}

void Append(std::string &out, const char *fmt, ...) __attribute__((format(printf, 2, 3)));
void Append(std::string &out, const char *fmt, ...)
{
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    const int n = vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    out.append(buf, n < 0 ? 0 : (size_t)n < sizeof buf ? (size_t)n : sizeof buf - 1);
}

}  // namespace

int main(int argc, char **argv)
{
    gmg_audit_params prm;
    memset(&prm, 0, sizeof prm);
    prm.n_start_codons = prm.n_stop_codons = 3;
    memcpy(prm.start_codon, "atg\0gtg\0ttg", 12);
    memcpy(prm.stop_codon, "taa\0tag\0tga", 12);
    prm.flags = GMG_AUDIT_NEXT_STOP;
    bool check_start = true, use_dir = false, circular = true, multi = false;
    static struct option long_options[] = {{"multi", 0, 0, 'm'}, {"dir", 0, 0, 'd'}, {"nowrap", 0, 0, 'w'}, {"help", 0, 0, 'h'}, {0, 0, 0, 0}};
    int ch;
    while ((ch = getopt_long(argc, argv, "A:stZ:dwh", long_options, nullptr)) != EOF) switch (ch) {
        case 'A': CodonList(optarg, prm.start_codon, &prm.n_start_codons); break;
        case 'Z': CodonList(optarg, prm.stop_codon, &prm.n_stop_codons); break;
        case 's': check_start = false; break;
        case 'd': use_dir = true; break;
        case 'w': circular = false; break;
        case 'm': multi = true; break;
        case 'h': printf("%s", kUsage); return 0;
        case 't': Die(1, "-t is refused: the reference fills Codon[3..1] in place of [2..0] and tests a stale letter (anomaly.cc:127-140)");
        default: fprintf(stderr, "%s", kUsage); return 1;
    }
    if (optind > argc - 2) { fprintf(stderr, "%s", kUsage); return 1; }
    const std::vector<Record> recs = ReadFasta(ReadFile(argv[optind]), multi);
    if (recs.empty()) Die(1, "%s holds no sequence", argv[optind]);
    const std::vector<std::string> lines = Lines(ReadFile(argv[optind + 1]));
    std::map<std::string, uint32_t> by_tag;
    for (size_t k = recs.size(); k-- > 0;) by_tag[recs[k].tag] = (uint32_t)k;       // (the first of equal tags)

    // ---- the lines: a gene, or a line that does not parse (printed in its place)
    std::vector<Gene> genes;
    std::vector<long> gene_of_line(lines.size(), -1);
    std::vector<gmg_gene_region> regions;
    for (size_t ln = 0; ln < lines.size(); ln++) {
        const Parsed p = ParseLine(lines[ln], multi, use_dir);
        if (!p.ok) continue;
        Gene g;
        g.line = ln;
        g.name = p.name;
        g.start = p.start;
        g.end = p.end;
        g.rec = 0;
        if (multi) {
            const std::map<std::string, uint32_t>::const_iterator it = by_tag.find(p.tag);
            if (it == by_tag.end()) Refuse(lines[ln], "no record of the sequence file has this tag");
            g.rec = it->second;
        }
        const long L = g.seq_len = (long)recs[g.rec].letters.size();
        if (L < 1) Refuse(lines[ln], "its sequence is empty");
        g.dir = use_dir ? (p.dir > 0 ? +1 : -1) : Direction(g.start, g.end, L, circular);
        g.len = 1 + (g.dir > 0 ? g.end - g.start : g.start - g.end);
        if (g.len < 0) g.len += L;
        if (g.len < 3) Refuse(lines[ln], "a gene shorter than 3 bases (the reference reads in front of its buffer)");
        if (g.len > L) Refuse(lines[ln], "a gene longer than its sequence");
        // the gene's letters sit at start, start +- 1, ...; one wrap must bring every one of them into 1 .. L
        if (g.dir > 0 ? (g.start < 1 || g.start + g.len - 1 > 2 * L) : (g.start > L || g.start - g.len + 1 + L < 1))
            Refuse(lines[ln], "one wrap does not bring the coordinates onto the sequence");
        gmg_gene_region r;
        r.read = g.rec;
        r.first = (int32_t)(((g.start - 1) % L + L) % L);
        r.len = (int32_t)g.len;
        r.strand = g.dir;
        gene_of_line[ln] = (long)genes.size();
        genes.push_back(g);
        regions.push_back(r);
    }

    // ---- one call for all genes of all records
    const char *dev = getenv("GMG_DEVICE");
    Check(gmg_init(dev ? atoi(dev) : 0), "gmg_init");
    Batch batch = Upload(recs);
    gmg_audit *audit = nullptr;
    Check(gmg_genes_audit(batch.reads, regions.data(), regions.size(), &prm, batch.amb.empty() ? nullptr : batch.amb.data(), batch.amb.size(), &audit,
                          nullptr), "gmg_genes_audit");
    uint64_t n_inner = 0;
    Check(gmg_audit_info(audit, nullptr, &n_inner), "gmg_audit_info");
    std::vector<gmg_gene_audit> rec(regions.size() + 1);
    std::vector<int32_t> inner(n_inner + 1);
    Check(gmg_audit_fetch(audit, rec.data(), inner.data(), nullptr), "gmg_audit_fetch");
    gmg_audit_free(audit);
    gmg_reads_free(batch.reads);

    // ---- the messages, in the order of the lines
    std::string out;
    long ok_ct = 0, problem_ct = 0;
    for (size_t ln = 0; ln < lines.size(); ln++) {
        if (gene_of_line[ln] < 0) {
            Append(out, "Bad line:  ");
            out += lines[ln];
            out += "\n...Skipping\n";
            continue;
        }
        const Gene &g = genes[gene_of_line[ln]];
        const gmg_gene_audit &a = rec[gene_of_line[ln]];
        const std::string &data = recs[g.rec].letters;
        const long L = g.seq_len;
        const char *name = g.name.c_str();
        // the gene's base k as the reference holds it in Buffer: lower case, complemented on the reverse strand
        auto letter = [&](long k) -> char {
            long j = g.dir > 0 ? g.start + k : g.start - k;
            if (g.dir > 0 && j > L) j -= L;
            if (g.dir < 0 && j < 1) j += L;
            const char c = (char)tolower((unsigned char)data[j - 1]);
            return g.dir > 0 ? c : Complement(c);
        };
        auto codon = [&](long k) { return std::string({letter(k), letter(k + 1), letter(k + 2)}); };
        bool problem = false;
        if (check_start && a.start_which < 0) {
            Append(out, "%-10s has bad start codon = %.3s\n", name, codon(0).c_str());
            problem = true;
        }
        if (a.stop_which < 0) {
            Append(out, "%-10s has bad stop codon = %s\n", name, codon(g.len - 3).c_str());
            problem = true;
            if (a.next_stop < 0) Refuse(lines[ln], "the gene ends in no stop codon and there is none behind it in its frame (the reference aborts)");
            if (g.dir > 0 ? g.start + a.next_stop + 2 > 2 * L : g.start - a.next_stop - 2 + L < 1)
                Refuse(lines[ln], "the search for the next stop codon passes the end of the sequence twice");
            Append(out, "           next stop occurs at offset %ld  Gene_Len = %ld  diff = %+ld\n", (long)a.next_stop, g.len, (long)a.next_stop - g.len + 3);
        }
        const int frame_shift = (int)(g.len % 3);
        if (frame_shift) {
            Append(out, "%-10s %8ld %8ld has %+d frame shift\n", name, g.start, g.end, frame_shift);
            problem = true;
            if (a.n_inner_stops == 0) {
                out += "   No stop found in start frame\n";
                continue;                               // (counted neither OK nor problem)
            }
            long i = inner[a.inner_begin], stop = g.start + g.dir * (i - 1);
            if (stop < 1) stop += L;
            else if (stop > L) stop -= L;
            Append(out, "   Best prefix is %8ld %8ld   Len = %ld\n", g.start, stop, i);
            i = a.last_back_stop >= 0 ? a.last_back_stop : g.len % 3 - 3;     // (the loop runs out at len - 6 - 3k < 0)
            i += 3;
            long begin = g.start + g.dir * i;
            if (begin < 1) begin += L;
            else if (stop > L) begin -= L;
            Append(out, "   Best suffix is %8ld %8ld   Len = %ld\n", begin, g.end, g.len - i - 3);
        } else {
            for (int32_t k = 0; k < a.n_inner_stops; k++) {
                const long i = inner[a.inner_begin + k];
                Append(out, "%-10s has stop codon %.3s at offset %ld  Gene_Len = %ld  diff = %+ld\n", name, codon(i).c_str(), i, g.len, g.len - 3 - i);
                problem = true;
            }
        }
        if (problem) problem_ct++;
        else ok_ct++;
    }
    fwrite(out.data(), 1, out.size(), stdout);
    fprintf(stderr, "     OK orfs = %7d\n", (int)ok_ct);
    fprintf(stderr, "Problem orfs = %7d\n", (int)problem_ct);
    return 0;
}
