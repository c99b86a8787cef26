//  entropy-score_gpu.cc -- the reference's entropy-score (src/Util/entropy-score.cc) on the device (DESIGN.md 4.15,
//  INTEGRATION.md): the entropy distance ratio appended to every line of a coordinate file.  gmg_extract_plan turns a line into its
//  region (the length test after the cuts, as the reference has it), ONE gmg_entropy_regions call counts the amino acids of all
//  regions, gmg_entropy_from_counts finishes each count vector on the host with the reference's arithmetic, and the line is
//  printed as "%s \t%5.3f\n" -- without its last character, which the reference always drops (:156-158, a stray ';').
//  New code, built from this repository alone.
//
//  usage: entropy-score_gpu [-d] [-E file] [-l N] [-s] [--nostop] [-w] [--multi] <sequence-file> <coords|->
//
//  The options are the reference's, as its getopt string "2dE:hl:sw" and its long-option table accept them: --nostop exists, a
//  short -t does not, and -2 is accepted by getopt and then rejected as the reference rejects it.
//  Refused (status 1, one line on stderr that names the coordinate line, nothing on stdout): see kUsage.

#include "coords_common.h"

#include <getopt.h>

#include <algorithm>
#include <set>

using namespace coords;

namespace {

const char *kUsage =
    "USAGE:  entropy-score_gpu [options] <sequence-file> <coords>\n"
    "\n"
    "Read fasta-format <sequence-file> and for each region specified by the\n"
    "lines  <tag>  <start>  <stop>  [<frame>] ...  of <coords> (a file, or - for\n"
    "standard input) print the line with its entropy distance ratio appended.\n"
    "Output goes to stdout.\n"
    "\n"
    "Options:\n"
    " -d, --dir            use the 4th column of each line as the direction (positive is forward)\n"
    " -E, --entropy <file> read the entropy profiles from <file> (the format long-orfs and glimmer3 read)\n"
    " -h, --help           print this message\n"
    " -l, --minlen <n>     skip regions shorter than <n> (tested after -s / --nostop shortened them)\n"
    " -s, --nostart        omit the first 3 bases of each region\n"
    " --nostop             omit the last 3 bases of each region\n"
    " -w, --nowrap         the sequence is not circular: a line is forward when start < stop\n"
    " --multi              <sequence-file> holds many records; lines are <id> <sequence tag> <start> <stop> [<dir>]\n"
    "\n"
    "Refused with status 1 and one line that names the coordinate line:\n"
    "  coordinates that one wrap does not bring onto the sequence, a region longer than its sequence\n"
    "  a line of 299 characters or more; under --multi a sequence tag that no record has\n";

bool ReadProfiles(const char *path, double pos[20], double neg[20])
{
    FILE *fp = fopen(path, "r");
    if (!fp) Die(1, "Can't open %s for reading.", path);
    char line[4096];
    if (!fgets(line, sizeof line, fp)) { fclose(fp); return false; }    // the header line
    for (int i = 0; i < 20; i++)
        if (fscanf(fp, "%4095s %lf %lf\n", line, pos + i, neg + i) != 3) { fclose(fp); return false; }
    fclose(fp);
    return true;
}

}  // namespace

int main(int argc, char **argv)
{
    bool use_dir = false, circular = true, skip_start = false, skip_stop = false, multi = false, errflg = false;
    long min_len = 0;
    double pos[20], neg[20];
    Check(gmg_entropy_default_profiles(pos, neg), "gmg_entropy_default_profiles");
    static struct option long_options[] = {{"dir", 0, 0, 'd'}, {"entropy", 1, 0, 'E'}, {"help", 0, 0, 'h'}, {"minlen", 1, 0, 'l'},
                                           {"nostart", 0, 0, 's'}, {"nostop", 0, 0, 't'}, {"nowrap", 0, 0, 'w'}, {"multi", 0, 0, 'm'},
                                           {0, 0, 0, 0}};
    int ch;
    while (!errflg && (ch = getopt_long(argc, argv, "2dE:hl:sw", long_options, nullptr)) != EOF) switch (ch) {
        case 'd': use_dir = true; break;
        case 'E': if (!ReadProfiles(optarg, pos, neg)) errflg = true; break;
        case 'h': fprintf(stderr, "%s", kUsage); return 0;
        case 'l': min_len = strtol(optarg, nullptr, 10); break;
        case 's': skip_start = true; break;
        case 't': skip_stop = true; break;
        case 'w': circular = false; break;
        case 'm': multi = true; break;
        default: errflg = true;
    }
    if (errflg || optind > argc - 2) { fprintf(stderr, "%s", kUsage); return 1; }
    const std::vector<Record> recs = ReadFasta(ReadFile(argv[optind]), multi);
    if (recs.empty()) Die(1, "Failed to read file %s", argv[optind]);
    const std::vector<std::string> lines = Lines(ReadFile(argv[optind + 1]));
    std::map<std::string, uint32_t> by_tag;
    for (size_t k = recs.size(); k-- > 0;) by_tag[recs[k].tag] = (uint32_t)k;
    std::vector<uint64_t> off(1, 0), amb;
    for (const Record &r : recs) {
        for (size_t i = 0; i < r.letters.size(); i++)
            if (!r.letters[i] || !strchr("acgtACGT", r.letters[i])) amb.push_back(off.back() + i);
        off.push_back(off.back() + r.letters.size());
    }

    const int flags = (use_dir ? GMG_COORD_USE_DIR : 0) | (circular ? 0 : GMG_COORD_NOWRAP) | (skip_start ? GMG_COORD_SKIP_START : 0) |
                      (skip_stop ? GMG_COORD_SKIP_STOP : 0) | GMG_COORD_MULTI;        // (MULTI: the length test only after the cuts)
    std::vector<gmg_gene_region> regions;
    std::vector<size_t> line_of;
    std::string err;
    for (size_t ln = 0; ln < lines.size(); ln++) {
        const Parsed p = ParseLine(lines[ln], multi, use_dir);
        if (!p.ok) {
            err += "ERROR:  Skipped following coord line\n" + lines[ln];
            continue;
        }
        gmg_coord co;
        co.read = 0;
        if (multi) {
            const std::map<std::string, uint32_t>::const_iterator it = by_tag.find(p.tag);
            if (it == by_tag.end()) Refuse(lines[ln], "no record of the sequence file has this tag");
            co.read = it->second;
        }
        co.dir = p.dir;
        co.start = p.start;
        co.end = p.end;
        gmg_gene_region r;
        uint64_t made = 0;
        if (gmg_extract_plan(off.data(), recs.size(), &co, 1, flags, min_len, &r, nullptr, &made) != GMG_OK)
            Refuse(lines[ln], "one wrap does not bring the coordinates onto the sequence, or the region is longer than its sequence");
        if (!made) continue;                             // shorter than -l
        regions.push_back(r);
        line_of.push_back(ln);
    }

    std::vector<int32_t> counts(regions.size() * 20 + 20);
    if (!regions.empty()) {
        const char *dev = getenv("GMG_DEVICE");
        Check(gmg_init(dev ? atoi(dev) : 0), "gmg_init");
        Batch batch = Upload(recs);
        char aa[64];
        Check(gmg_xlate_table(11, aa), "gmg_xlate_table");       // (Codon_Translation's default table)
        void *d_counts = nullptr;
        Check(gmg_device_malloc(&d_counts, regions.size() * 80), "gmg_device_malloc");
        Check(gmg_entropy_regions(batch.reads, regions.data(), regions.size(), aa, pos, neg, (int32_t *)d_counts, nullptr, nullptr), "gmg_entropy_regions");
        Check(gmg_memcpy_d2h(counts.data(), d_counts, regions.size() * 80, nullptr), "gmg_memcpy_d2h");
        Check(gmg_synchronize(nullptr), "gmg_synchronize");
        gmg_device_free(d_counts);
        gmg_reads_free(batch.reads);
        // A codon with a letter outside acgtACGT counts nowhere in the reference (Codon_Translation gives 'X'); the device counted it
        // under the 2-bit code the letter was packed as: taken out again here, codon by codon (few: the list is short).
        static const char order[] = "ACDEFGHIKLMNPQRSTVWY";
        for (size_t k = 0; k < regions.size() && !amb.empty(); k++) {
            const gmg_gene_region &r = regions[k];
            if (r.len < 3) continue;
            const std::string &s = recs[r.read].letters;
            const uint64_t S = off[r.read], L = off[r.read + 1] - S;
            const bool fwd = r.strand > 0;
            uint64_t lo = fwd ? (uint64_t)r.first : ((uint64_t)r.first + L - ((uint64_t)r.len - 1)) % L;   // the region's lowest position, wrapped
            uint64_t left = (uint64_t)r.len;
            std::set<uint64_t> codons;
            while (left) {
                const uint64_t piece = std::min(left, L - lo);
                for (std::vector<uint64_t>::const_iterator it = std::lower_bound(amb.begin(), amb.end(), S + lo); it != amb.end() && *it < S + lo + piece; ++it) {
                    const uint64_t p = *it - S, offset = fwd ? (p + L - (uint64_t)r.first) % L : ((uint64_t)r.first + L - p) % L;
                    if (offset / 3 * 3 + 2 < (uint64_t)r.len) codons.insert(offset / 3);
                }
                left -= piece;
                lo = 0;
            }
            for (uint64_t c : codons) {
                int idx = 0;
                for (uint64_t t = 0; t < 3; t++) {
                    const uint64_t o = (3 * c + t) % L, p = fwd ? ((uint64_t)r.first + o) % L : ((uint64_t)r.first + L - o) % L;
                    const int code = gmg_base_code((unsigned char)s[p]);
                    idx = 4 * idx + (fwd ? code : 3 - code);
                }
                const char *q = aa[idx] == '*' ? nullptr : strchr(order, aa[idx]);
                if (q) counts[20 * k + (size_t)(q - order)]--;
            }
        }
    }
    fputs(err.c_str(), stderr);
    for (size_t k = 0; k < regions.size(); k++) {
        double ratio = 0.0;
        Check(gmg_entropy_from_counts(&counts[20 * k], pos, neg, nullptr, nullptr, &ratio), "gmg_entropy_from_counts");
        std::string line = lines[line_of[k]];
        line.pop_back();                                 // (the reference drops the last character whatever it is)
        printf("%s \t%5.3f\n", line.c_str(), ratio);
    }
    return 0;
}
