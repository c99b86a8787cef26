//  uncovered_gpu.cc -- the reference's uncovered (src/Util/uncovered.cc) on the device: the
//  stretches of a sequence that none of the regions of a coordinate file covers.  gmg_uncovered_plan turns every line into its one
//  or two intervals, ONE gmg_regions_uncovered call sorts and merges them and returns the gaps, and the letters are printed from the
//  file's own bytes, 60 to a line, under the tags seq00001, seq00002, ...  New code, built from this repository alone.
//
//  usage: uncovered_gpu [-2] [-d] [-l N] [-s] [--nostop] [-w] [--multi] <sequence-file> <coords|->
//
//  The options are the reference's, as its getopt string "2dhl:sw" and its long-option table accept them: --nostop exists, a short
//  -t does not (a usage error with status 1, there and here).
//  --multi: <sequence-file> holds many records and a line is <id> <sequence tag> <start> <end> [<dir>]; the gaps of all records come
//  out in the order of the file, the tag counter running on.
//  Refused (status 1, one line on stderr that names the line, nothing on stdout): see kUsage.

#include "coords_common.h"

#include <getopt.h>

using namespace coords;

namespace {

const char *kUsage =
    "USAGE:  uncovered_gpu [options] <sequence-file> <coords>\n"
    "\n"
    "Read fasta-format <sequence-file> and print the parts of it that none of the regions\n"
    "<tag>  <start>  <stop>  [<dir>] ...  of <coords> (a file, or - for standard input) covers.\n"
    "Coordinates are inclusive and count from 1.  Output goes to stdout in multi-fasta format.\n"
    "\n"
    "Options:\n"
    " -2                   print every part as two fields (tag and letters) on one line\n"
    " -d, --dir            use the 4th column of each line as the direction (positive is forward)\n"
    " -h                   print this message\n"
    " -l, --minlen <n>     do not print parts shorter than <n>\n"
    " -s, --nostart        omit the first 3 bases of each region\n"
    " --nostop             omit the last 3 bases of each region\n"
    " -w, --nowrap         the sequence is not circular: a line is forward when start < stop\n"
    " --multi              <sequence-file> holds many records; lines are <id> <sequence tag> <start> <stop> [<dir>]\n"
    "\n"
    "Refused with status 1 and one line that names the coordinate line:\n"
    "  coordinates whose region, by the reference's own arithmetic, does not lie on the sequence\n"
    "  a line of 299 characters or more; under --multi a sequence tag that no record has\n"
    "  a NUL byte among the letters; a sequence of 2^31 letters or more\n";

}  // namespace

int main(int argc, char **argv)
{
    bool fasta_format = true, use_dir = false, circular = true, skip_start = false, skip_stop = false, multi = false, errflg = false;
    long min_len = 0;
    static struct option long_options[] = {{"dir", 0, 0, 'd'}, {"minlen", 1, 0, 'l'}, {"nostart", 0, 0, 's'}, {"nostop", 0, 0, 't'},
                                           {"nowrap", 0, 0, 'w'}, {"multi", 0, 0, 'm'}, {0, 0, 0, 0}};
    int ch;
    while (!errflg && (ch = getopt_long(argc, argv, "2dhl:sw", long_options, nullptr)) != EOF) switch (ch) {
        case '2': fasta_format = false; break;
        case 'd': use_dir = true; break;
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
    for (const Record &r : recs) {
        if (memchr(r.letters.data(), '\0', r.letters.size())) Die(1, "a NUL byte among the letters of %s", r.tag.c_str());
        if (r.letters.size() >= 0x80000000ull) Die(1, "sequence %s has 2^31 letters or more", r.tag.c_str());
    }
    const std::vector<std::string> lines = Lines(ReadFile(argv[optind + 1]));
    std::map<std::string, uint32_t> by_tag;
    for (size_t k = recs.size(); k-- > 0;) by_tag[recs[k].tag] = (uint32_t)k;
    std::vector<uint64_t> off(1, 0);
    for (const Record &r : recs) off.push_back(off.back() + r.letters.size());

    const int flags = (use_dir ? GMG_COORD_USE_DIR : 0) | (circular ? 0 : GMG_COORD_NOWRAP) | (skip_start ? GMG_COORD_SKIP_START : 0) |
                      (skip_stop ? GMG_COORD_SKIP_STOP : 0);
    std::vector<gmg_interval> intervals;
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
        gmg_interval made[2];
        uint64_t n_made = 0;
        if (gmg_uncovered_plan(off.data(), recs.size(), &co, 1, flags, made, &n_made) != GMG_OK)
            Refuse(lines[ln], "the region does not lie on the sequence (the reference prints from outside its string there)");
        for (uint64_t k = 0; k < n_made; k++) intervals.push_back(made[k]);
    }

    uint64_t n_gaps = 0;
    std::vector<gmg_gene_region> gaps(1);
    if (off.back()) {                                    // (sequences without a letter have no gap)
        const char *dev = getenv("GMG_DEVICE");
        Check(gmg_init(dev ? atoi(dev) : 0), "gmg_init");
        Batch batch = Upload(recs);
        gmg_gaps *res = nullptr;
        Check(gmg_regions_uncovered(batch.reads, intervals.empty() ? nullptr : intervals.data(), intervals.size(), min_len, &res, nullptr),
              "gmg_regions_uncovered");
        Check(gmg_gaps_info(res, &n_gaps), "gmg_gaps_info");
        gaps.resize(n_gaps + 1);
        Check(gmg_gaps_fetch(res, gaps.data(), nullptr), "gmg_gaps_fetch");
        gmg_gaps_free(res);
        gmg_reads_free(batch.reads);
    }

    fputs(err.c_str(), stderr);
    std::string out;
    char buf[128];
    for (uint64_t k = 0; k < n_gaps; k++) {
        const gmg_gene_region &g = gaps[k];
        const std::string &s = recs[g.read].letters;
        snprintf(buf, sizeof buf, "seq%05d", (int)(k + 1));
        const std::string tag = buf;
        if (fasta_format) {
            snprintf(buf, sizeof buf, ">%s  %ld %ld  len=%ld\n", tag.c_str(), (long)g.first + 1, (long)g.first + g.len, (long)g.len);
            out += buf;
            for (int32_t c = 0; c < g.len; c += 60) {
                if (c) out += '\n';
                out.append(s, (size_t)g.first + c, (size_t)(g.len - c < 60 ? g.len - c : 60));
            }
        } else {
            snprintf(buf, sizeof buf, "%-10s ", tag.c_str());
            out += buf;
            out.append(s, (size_t)g.first, (size_t)g.len);
        }
        out += '\n';
        if (out.size() >= (1 << 20)) {
            fwrite(out.data(), 1, out.size(), stdout);
            out.clear();
        }
    }
    fwrite(out.data(), 1, out.size(), stdout);
    return 0;
}
