//  start-codon-distrib_gpu.cc -- the reference's start-codon-distrib (src/Util/start-codon-distrib.cc) around ONE
//  gmg_genes_audit call: the distribution of the start codons of a coordinate file, as the table
//  with its Total: line or, with -3, as the atg,gtg,ttg proportions g3-iterated.py hands to glimmer3 -P.  The counts are the
//  call's histogram of first codons; a codon with a letter outside acgt is keyed by its letters here, from the records with the
//  code -1.  New code, built from this repository alone.
//
//  usage: start-codon-distrib_gpu [-d] [-w] [-3] [--multi] <sequence-file> <coords|->
//
//  Refused (status 1, one line on stderr that names the coordinate line, nothing on stdout): see kUsage.

#include "coords_common.h"

#include <getopt.h>

#include <algorithm>

using namespace coords;

namespace {

const char *kUsage =
    "USAGE:  start-codon-distrib_gpu [options] <sequence-file> <coords>\n"
    "\n"
    "Read fasta-format <sequence-file> and count the number of\n"
    "different start codons for the genes specified in <coords>,\n"
    "a file (or - for standard input) of lines\n"
    "  <tag>  <start>  <stop>  [<frame>] ...\n"
    "Coordinates are inclusive counting from 1.  Output goes to stdout.\n"
    "\n"
    "Options:\n"
    " -d, --dir      use the 4th column of each line as the direction (positive is forward)\n"
    " -h             print this message\n"
    " -w, --nowrap   the sequence is not circular: a line is forward when start < stop\n"
    " -3, --3comma   output only the atg,gtg,ttg proportions, comma separated\n"
    " --multi        <sequence-file> holds many records; lines are <id> <sequence tag> <start> <stop> [<dir>]\n"
    "\n"
    "Refused with status 1 and one line that names the coordinate line (the reference's outcome is accidental there):\n"
    "  a start codon that touches the last base of the sequence (the reference indexes in front of its string)\n"
    "  coordinates that one wrap does not bring onto the sequence\n"
    "  a line of 299 characters or more; under --multi a sequence tag that no record has\n";

struct Entry {
    std::string codon;
    long count;
};

bool EntryCmp(const Entry &a, const Entry &b)            // by count, descending; then by codon
{
    if (a.count > b.count) return true;
    return a.count == b.count && a.codon < b.codon;
}

}  // namespace

int main(int argc, char **argv)
{
    bool use_dir = false, circular = true, comma3 = false, multi = false;
    static struct option long_options[] = {{"dir", 0, 0, 'd'}, {"help", 0, 0, 'h'}, {"nowrap", 0, 0, 'w'}, {"3comma", 0, 0, '3'},
                                           {"multi", 0, 0, 'm'}, {0, 0, 0, 0}};
    int ch;
    while ((ch = getopt_long(argc, argv, "dhw3", long_options, nullptr)) != EOF) switch (ch) {
        case 'd': use_dir = true; break;
        case 'w': circular = false; break;
        case '3': comma3 = true; break;
        case 'm': multi = true; break;
        case 'h': fprintf(stderr, "%s", kUsage); return 0;
        default: fprintf(stderr, "%s", kUsage); return 1;
    }
    if (optind > argc - 2) { fprintf(stderr, "%s", kUsage); return 1; }
    const std::vector<Record> recs = ReadFasta(ReadFile(argv[optind]), multi);
    if (recs.empty()) Die(1, "Failed to open file %s", argv[optind]);
    const std::vector<std::string> lines = Lines(ReadFile(argv[optind + 1]));
    std::map<std::string, uint32_t> by_tag;
    for (size_t k = recs.size(); k-- > 0;) by_tag[recs[k].tag] = (uint32_t)k;

    std::vector<gmg_gene_region> regions;
    std::string err;
    for (size_t ln = 0; ln < lines.size(); ln++) {
        const Parsed p = ParseLine(lines[ln], multi, use_dir);
        if (!p.ok) {
            err += "ERROR:  Skipped following coord line\n" + lines[ln];
            continue;
        }
        gmg_gene_region r;
        r.read = 0;
        if (multi) {
            const std::map<std::string, uint32_t>::const_iterator it = by_tag.find(p.tag);
            if (it == by_tag.end()) Refuse(lines[ln], "no record of the sequence file has this tag");
            r.read = it->second;
        }
        const long L = (long)recs[r.read].letters.size();
        if (L < 1) Refuse(lines[ln], "its sequence is empty");
        r.strand = use_dir ? (p.dir > 0 ? +1 : -1) : Direction(p.start, p.end, L, circular);
        r.len = 3;
        for (int i = 0; i < 3; i++) {
            const long sub = (r.strand > 0 ? p.start + i : p.start - i) - 1;
            if (sub < -L || sub >= 2 * L) Refuse(lines[ln], "one wrap does not bring the coordinates onto the sequence");
            if (((sub % L) + L) % L == L - 1) Refuse(lines[ln], "the start codon touches the last base of the sequence (the reference indexes in front of its string)");
        }
        r.first = (int32_t)(((p.start - 1) % L + L) % L);
        regions.push_back(r);
    }

    const char *dev = getenv("GMG_DEVICE");
    Check(gmg_init(dev ? atoi(dev) : 0), "gmg_init");
    Batch batch = Upload(recs);
    gmg_audit_params prm;
    memset(&prm, 0, sizeof prm);                        // no start or stop lists: the codes and their histogram are all that is asked
    gmg_audit *audit = nullptr;
    Check(gmg_genes_audit(batch.reads, regions.data(), regions.size(), &prm, batch.amb.empty() ? nullptr : batch.amb.data(), batch.amb.size(), &audit,
                          nullptr), "gmg_genes_audit");
    std::vector<gmg_gene_audit> rec(regions.size() + 1);
    int64_t hist[65];
    Check(gmg_audit_fetch(audit, rec.data(), nullptr, hist), "gmg_audit_fetch");
    gmg_audit_free(audit);
    gmg_reads_free(batch.reads);

    std::map<std::string, long> odd;                    // the codons with a letter outside acgt, by their letters
    if (hist[64])
        for (size_t k = 0; k < regions.size(); k++) {
            if (rec[k].first_codon >= 0) continue;
            const gmg_gene_region &r = regions[k];
            const std::string &s = recs[r.read].letters;
            const long L = (long)s.size();
            std::string codon;
            for (int i = 0; i < 3; i++) {
                const char c = (char)tolower((unsigned char)s[(size_t)(((r.first + (r.strand > 0 ? i : -i)) % L + L) % L)]);
                codon.push_back(r.strand > 0 ? c : Complement(c));
            }
            odd[codon]++;
        }
    std::vector<Entry> entry;
    long total = 0;
    for (int c = 0; c < 64; c++)
        if (hist[c]) {
            Entry e;
            e.codon = std::string({"acgt"[c >> 4], "acgt"[(c >> 2) & 3], "acgt"[c & 3]});
            e.count = (long)hist[c];
            entry.push_back(e);
            total += e.count;
        }
    for (const std::pair<const std::string, long> &kv : odd) {
        Entry e;
        e.codon = kv.first;
        e.count = kv.second;
        entry.push_back(e);
        total += e.count;
    }
    fputs(err.c_str(), stderr);
    if (comma3) {
        const long t = total ? total : 1;
        const char *want[3] = {"atg", "gtg", "ttg"};
        for (int w = 0; w < 3; w++) {
            double v = 0.0;
            for (const Entry &e : entry)
                if (e.codon == want[w]) v = double(e.count) / t;
            printf(w == 0 ? "%.3f" : w == 1 ? ",%.3f" : ",%.3f\n", v);
        }
    } else {
        std::sort(entry.begin(), entry.end(), EntryCmp);
        for (const Entry &e : entry)
            printf(" %s   %6d  %5.1f%%\n", e.codon.c_str(), (int)e.count, total ? 100.0 * ((double)e.count / (double)total) : 0.0);
        printf("Total: %6d\n", (int)total);
    }
    return 0;
}
