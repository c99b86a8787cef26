//  text_common.h -- what extract_gpu and multi-extract_gpu share: the options both programs of the reference take
//  (src/Util/extract.cc:211-288, multi-extract.cc:268-345), the plan of the coordinate lines (gmg_extract_plan: every skip and
//  length decision is the library's) and ONE gmg_regions_text call that writes the whole output on the device.
//  New code, built from this repository alone.
#ifndef GMG_TEXT_COMMON_H
#define GMG_TEXT_COMMON_H

#include "coords_common.h"

#include <getopt.h>

namespace text {

using namespace coords;

struct Options {
    bool fasta = true;           // -2 clears it: "<tag> <letters>" on one line
    int flags = 0;               // GMG_COORD_*
    long min_len = 0;
    const char *seq_path = nullptr, *coord_path = nullptr;
};

inline Options ParseOptions(int argc, char **argv, const char *usage)
{
    // (--2_fields means -d in both programs of the reference: kept)
    static struct option long_options[] = {{"2_fields", 0, 0, 'd'}, {"dir", 0, 0, 'd'}, {"help", 0, 0, 'h'}, {"minlen", 1, 0, 'l'},
                                           {"nostart", 0, 0, 's'}, {"nostop", 0, 0, 't'}, {"nowrap", 0, 0, 'w'}, {0, 0, 0, 0}};
    Options o;
    int ch;
    while ((ch = getopt_long(argc, argv, "2dhl:stw", long_options, nullptr)) != EOF) switch (ch) {
        case '2': o.fasta = false; break;
        case 'd': o.flags |= GMG_COORD_USE_DIR; break;
        case 'h': fprintf(stderr, "%s", usage); exit(EXIT_SUCCESS);
        case 'l': o.min_len = strtol(optarg, nullptr, 10); break;
        case 's': o.flags |= GMG_COORD_SKIP_START; break;
        case 't': o.flags |= GMG_COORD_SKIP_STOP; break;
        case 'w': o.flags |= GMG_COORD_NOWRAP; break;
        default: fprintf(stderr, "%s", usage); exit(EXIT_FAILURE);
    }
    if (optind > argc - 2) { fprintf(stderr, "%s", usage); exit(EXIT_FAILURE); }
    o.seq_path = argv[optind];
    o.coord_path = argv[optind + 1];
    return o;
}

// a coordinate line that took part: its fields as text, and the entry of the plan made from it
struct Entry {
    std::string id, tag, line;   // (id: multi-extract's first column)
    gmg_coord c;
};

inline void SkippedLine(const std::string &line)
{
    fprintf(stderr, "ERROR:  Skipped following coord line\n");
    fputs(line.c_str(), stderr);
}

// printf ("%-10s ", tag): the head of a record under -2
inline std::string TwoFieldHead(const std::string &tag)
{
    std::string h = tag;
    if (h.size() < 10) h.append(10 - h.size(), ' ');
    return h + " ";
}

// The records of `entries`, in their order, to stdout.  head (entry, region) writes a record's first bytes.
template <class Head> void Print(const std::vector<Record> &recs, const std::vector<Entry> &entries, const Options &o, Head head)
{
    std::vector<uint64_t> off(1, 0);
    for (const Record &r : recs) off.push_back(off.back() + r.letters.size());
    std::vector<gmg_coord> coords;
    for (const Entry &e : entries) coords.push_back(e.c);
    std::vector<gmg_gene_region> regions(coords.size() + 1);
    std::vector<uint64_t> entry_of(coords.size() + 1);
    uint64_t n = 0;
    if (gmg_extract_plan(off.data(), recs.size(), coords.data(), coords.size(), o.flags, o.min_len, regions.data(), entry_of.data(), &n) != GMG_OK) {
        // the message names the entry; show the line it came from
        const char *msg = gmg_last_error(), *p = strstr(msg, "line ");
        const unsigned long long k = p ? strtoull(p + 5, nullptr, 10) : 0;
        fprintf(stderr, "ERROR:  %s\n", msg);
        if (k < entries.size()) {
            fprintf(stderr, "coordinate line:  %s", entries[k].line.c_str());
            if (entries[k].line.empty() || entries[k].line.back() != '\n') fputc('\n', stderr);
        }
        exit(EXIT_FAILURE);
    }
    if (n == 0) return;
    std::string heads;
    std::vector<uint64_t> head_off(1, 0);
    for (uint64_t k = 0; k < n; k++) {
        heads += head(entries[entry_of[k]], regions[k]);
        head_off.push_back(heads.size());
    }
    std::string blob;
    for (const Record &r : recs) blob += r.letters;

    const char *dev = getenv("GMG_DEVICE");
    Check(gmg_init(dev ? atoi(dev) : 0), "gmg_init");
    gmg_letters *letters = nullptr;
    Check(gmg_letters_upload(blob.data(), off.data(), recs.size(), &letters), "gmg_letters_upload");
    gmg_text_params prm;
    Check(gmg_text_params_reference(&prm, o.fasta ? 60 : 0), "gmg_text_params_reference");
    size_t bytes = 0;
    Check(gmg_regions_text(letters, regions.data(), n, heads.data(), head_off.data(), &prm, nullptr, &bytes, nullptr), "gmg_regions_text");
    std::vector<char> out(bytes + 1);
    Check(gmg_regions_text(letters, regions.data(), n, heads.data(), head_off.data(), &prm, out.data(), &bytes, nullptr), "gmg_regions_text");
    gmg_letters_free(letters);
    fwrite(out.data(), 1, bytes, stdout);
}

}  // namespace text

#endif
