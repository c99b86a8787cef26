//  multi-extract_gpu.cc -- the reference's multi-extract (src/Util/multi-extract.cc) around ONE gmg_regions_text call (DESIGN.md
//  4.17): the coordinate lines "<id> <tag> <start> <stop> [<dir>]" sorted by tag, and for every record of the
//  multi-fasta file, in the file's order, the regions of the lines that carry its tag, as multi-fasta text or with -2 as
//  "<tag> <letters>" lines.  stdout, the "Skipped following coord line" messages on stderr and the exit status are the
//  reference's.  New code, built from this repository alone.
//
//  usage: multi-extract_gpu [-2] [-d] [-l N] [-s] [-t] [-w] <sequence-file> <coords>|-
//
//  Refused as extract_gpu refuses (status 1, the plan's message and the coordinate line, nothing on stdout).

#include "text_common.h"

#include <algorithm>

using namespace text;

namespace {

const char *kUsage =
    "USAGE:  multi-extract_gpu [options] <sequence-file> <coords>\n"
    "\n"
    "Print the regions of the sequences of multi-fasta <sequence-file> that the lines\n"
    "  <id>  <tag>  <start>  <stop>  [<dir>] ...\n"
    "of <coords> (\"-\": standard input) name, 1-based and inclusive, as multi-fasta\n"
    "text: <tag> is the first word of a sequence's header line, <id> labels the region;\n"
    "a region on the reverse strand is reverse-complemented.\n"
    "\n"
    "Options:\n"
    " -2            each region as two fields, tag and letters, on one line\n"
    " -d, --dir     the direction of a line is its 5th column (positive: forward)\n"
    " -h, --help    this message\n"
    " -l, --minlen <n>   leave out regions shorter than <n> letters\n"
    " -s, --nostart leave out the first 3 letters of each region\n"
    " -t, --nostop  leave out the last 3 letters of each region\n"
    " -w, --nowrap  the sequences are not circular: a line is forward when start < stop\n"
    "\n";

bool ByTag(const Entry &a, const Entry &b) { return a.tag < b.tag; }

}  // namespace

int main(int argc, char **argv)
{
    const Options o = ParseOptions(argc, argv, kUsage);
    const bool use_dir = (o.flags & GMG_COORD_USE_DIR) != 0;
    std::vector<Entry> lines;
    for (const std::string &line : Lines(ReadFile(o.coord_path))) {
        const Parsed p = ParseLine(line, true, use_dir);
        if (!p.ok) { SkippedLine(line); continue; }
        Entry e;
        e.id = p.name;
        e.tag = p.tag;
        e.line = line;
        e.c.read = 0;
        e.c.dir = use_dir ? p.dir : 0;
        e.c.start = p.start;
        e.c.end = p.end;
        lines.push_back(e);
    }
    // the reference's std::sort with the same comparisons on the same input: the same order among equal tags
    std::sort(lines.begin(), lines.end(), ByTag);
    const std::vector<Record> recs = ReadFasta(ReadFile(o.seq_path), true);
    std::vector<Entry> entries;
    for (size_t r = 0; r < recs.size(); r++) {
        const std::pair<std::vector<Entry>::const_iterator, std::vector<Entry>::const_iterator> range =
            std::equal_range(lines.begin(), lines.end(), Entry{"", recs[r].tag, "", gmg_coord()}, ByTag);
        for (std::vector<Entry>::const_iterator it = range.first; it != range.second; ++it) {
            entries.push_back(*it);
            entries.back().c.read = (uint32_t)r;
        }
    }
    Options multi = o;
    multi.flags |= GMG_COORD_MULTI;
    Print(recs, entries, multi, [&](const Entry &e, const gmg_gene_region &r) {
        if (!o.fasta) return TwoFieldHead(e.tag);
        char num[128];
        snprintf(num, sizeof num, "  %ld %ld  len=%ld\n", (long)e.c.start, (long)e.c.end, (long)r.len);
        return ">" + e.id + "  " + e.tag + num;
    });
    return 0;
}
