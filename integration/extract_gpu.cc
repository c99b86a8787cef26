//  extract_gpu.cc -- the reference's extract (src/Util/extract.cc) around ONE gmg_regions_text call (DESIGN.md 4.17,
//  INTEGRATION.md): the regions of a coordinate file as multi-fasta text, or with -2 as "<tag> <letters>" lines, written on the
//  device from the letters of the sequence and copied to stdout.  stdout, the "Skipped following coord line" messages on stderr
//  and the exit status are the reference's.  New code, built from this repository alone.
//
//  usage: extract_gpu [-2] [-d] [-l N] [-s] [-t] [-w] <sequence-file> <coords>|-
//
//  Refused with status 1, the plan's message and the coordinate line on stderr, nothing on stdout: a line that asks for more
//  letters than the sequence holds (the reference laps the circle) or starts where one wrap does not bring it onto the sequence
//  (the reference indexes outside its string); a line of 299 characters or more (the reference reads it in pieces).

#include "text_common.h"

using namespace text;

namespace {

const char *kUsage =
    "USAGE:  extract_gpu [options] <sequence-file> <coords>\n"
    "\n"
    "Print the regions of the first sequence of <sequence-file> that the lines\n"
    "  <tag>  <start>  <stop>  [<dir>] ...\n"
    "of <coords> (\"-\": standard input) name, 1-based and inclusive, as multi-fasta\n"
    "text; a region on the reverse strand is reverse-complemented.\n"
    "\n"
    "Options:\n"
    " -2            each region as two fields, tag and letters, on one line\n"
    " -d, --dir     the direction of a line is its 4th column (positive: forward)\n"
    " -h, --help    this message\n"
    " -l, --minlen <n>   leave out regions shorter than <n> letters\n"
    " -s, --nostart leave out the first 3 letters of each region\n"
    " -t, --nostop  leave out the last 3 letters of each region\n"
    " -w, --nowrap  the sequence is not circular: a line is forward when start < stop\n"
    "\n";

}  // namespace

int main(int argc, char **argv)
{
    const Options o = ParseOptions(argc, argv, kUsage);
    const std::vector<Record> recs = ReadFasta(ReadFile(o.seq_path), false);
    if (recs.empty()) Die(1, "Failed to read file %s", o.seq_path);
    const bool use_dir = (o.flags & GMG_COORD_USE_DIR) != 0, skip_start = (o.flags & GMG_COORD_SKIP_START) != 0;
    std::vector<Entry> entries;
    for (const std::string &line : Lines(ReadFile(o.coord_path))) {
        const Parsed p = ParseLine(line, false, use_dir);
        if (!p.ok) { SkippedLine(line); continue; }
        Entry e;
        e.tag = p.name;
        e.line = line;
        e.c.read = 0;
        e.c.dir = p.dir;
        e.c.start = p.start;
        e.c.end = p.end;
        entries.push_back(e);
    }
    // the header shows the start where the letters begin: 3 further in the region's direction under -s (extract.cc:117-122, 138-143)
    Print(recs, entries, o, [&](const Entry &e, const gmg_gene_region &r) {
        char num[128];
        if (!o.fasta) return TwoFieldHead(e.tag);
        const long start = (long)e.c.start + (skip_start ? (r.strand > 0 ? 3 : -3) : 0);
        snprintf(num, sizeof num, "  %ld %ld  len=%ld\n", start, (long)e.c.end, (long)r.len);
        return ">" + e.tag + num;
    });
    return 0;
}
