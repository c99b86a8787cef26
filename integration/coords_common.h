//  coords_common.h -- what anomaly_gpu, start-codon-distrib_gpu and entropy-score_gpu share: the sequence file read as Fasta_Read reads it
//  (src/Common/fasta.cc:236-283), the coordinate file cut into the lines fgets would hand over, the reference's direction rule
//  and the upload of the letters.  New code, built from this repository alone.
#ifndef GMG_COORDS_COMMON_H
#define GMG_COORDS_COMMON_H

#include "../include/gmg.h"

#include <ctype.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <map>
#include <string>
#include <vector>

namespace coords {

const size_t kMaxLine = 300;     // the reference's fgets buffer (gene.hh MAX_LINE): a longer line would be read in pieces

[[noreturn]] inline void Die(int status, const char *fmt, const char *a = "", const char *b = "")
{
    fprintf(stderr, "ERROR:  ");
    fprintf(stderr, fmt, a, b);
    fprintf(stderr, "\n");
    exit(status);
}

inline void Check(int rc, const char *who)
{
    if (rc != GMG_OK) Die(1, "%s: %s", who, gmg_last_error());
}

// a coordinate line the command refuses: one line on stderr that names it, status 1, nothing on stdout
[[noreturn]] inline void Refuse(const std::string &line, const char *why)
{
    std::string shown = line;
    while (!shown.empty() && (shown.back() == '\n' || shown.back() == '\r')) shown.pop_back();
    fprintf(stderr, "ERROR:  coordinate line '%s': %s\n", shown.c_str(), why);
    exit(1);
}

inline std::string ReadFile(const char *path)
{
    FILE *fp = strcmp(path, "-") == 0 ? stdin : fopen(path, "rb");
    if (!fp) Die(1, "Can't open %s for reading.", path);
    std::string s;
    char buf[1 << 16];
    size_t k;
    while ((k = fread(buf, 1, sizeof buf, fp)) > 0) s.append(buf, k);
    if (fp != stdin) fclose(fp);
    return s;
}

struct Record {
    std::string tag, letters;    // the header's first token; every byte of the record that is no white space
};

inline std::vector<Record> ReadFasta(const std::string &text, bool all)
{
    std::vector<Record> out;
    size_t i = text.find('>');
    while (i != std::string::npos && (all || out.empty())) {
        Record r;
        size_t eol = text.find('\n', i);
        if (eol == std::string::npos) eol = text.size();
        size_t b = i + 1;
        while (b < eol && isspace((unsigned char)text[b])) b++;
        size_t e = b;
        while (e < eol && !isspace((unsigned char)text[e])) e++;
        r.tag = text.substr(b, e - b);
        size_t next = text.find('>', eol);
        if (next == std::string::npos) next = text.size();
        for (size_t k = eol; k < next; k++)
            if (!isspace((unsigned char)text[k])) r.letters.push_back(text[k]);
        out.push_back(r);
        i = next < text.size() ? next : std::string::npos;
    }
    return out;
}

inline std::vector<std::string> Lines(const std::string &text)
{
    std::vector<std::string> out;
    for (size_t pos = 0; pos < text.size();) {
        size_t eol = text.find('\n', pos);
        eol = eol == std::string::npos ? text.size() : eol + 1;
        out.push_back(text.substr(pos, eol - pos));
        pos = eol;
    }
    return out;
}

// the reference's rule without -d (anomaly.cc:82, start-codon-distrib.cc:101-105)
inline int Direction(long start, long end, long len, bool circular)
{
    return ((start < end && (!circular || end - start <= len / 2)) || (circular && start - end > len / 2)) ? +1 : -1;
}

// Complement (tolower (letter)) (src/Common/gene.cc:15-19, 1084-1091): the IUPAC complement, 'n' for anything it does not know
inline char Complement(char ch)
{
    static const char from[] = "acgtrykmbdhvswn*-. ", to[] = "tgcayrmkvhdbswn*-. ";
    const char *p = ch ? strchr(from, ch) : nullptr;
    return p ? to[p - from] : 'n';
}

struct Parsed {                  // one line: "<name> [<tag>] <start> <end> [<dir>]"
    bool ok;
    std::string name, tag;
    long start, end;
    int dir;
};

inline Parsed ParseLine(const std::string &line, bool multi, bool use_dir)
{
    Parsed p;
    p.ok = false;
    p.start = p.end = 0;
    p.dir = 0;
    if (line.size() >= kMaxLine - 1 && !(line.size() == kMaxLine - 1 && line.back() == '\n')) Refuse(line, "299 characters or more (the reference reads such a line in pieces)");
    std::vector<char> a(line.size() + 1), b(line.size() + 1);
    a[0] = b[0] = '\0';
    int got;
    if (multi) got = sscanf(line.c_str(), "%s %s %ld %ld %d", a.data(), b.data(), &p.start, &p.end, &p.dir) - 1;
    else got = sscanf(line.c_str(), "%s %ld %ld %d", a.data(), &p.start, &p.end, &p.dir);
    p.ok = got >= (use_dir ? 4 : 3);
    p.name = a.data();
    p.tag = b.data();
    return p;
}

// the letters of the records on the device, back to back, and the job-wide indices of those outside acgtACGT
struct Batch {
    gmg_reads *reads;
    std::vector<uint64_t> off, amb;
};

inline Batch Upload(const std::vector<Record> &recs)
{
    Batch b;
    b.reads = nullptr;
    b.off.push_back(0);
    for (const Record &r : recs) b.off.push_back(b.off.back() + r.letters.size());
    std::string blob;                                   // one packing call from base 0, as the offsets count
    for (const Record &r : recs) blob += r.letters;
    std::vector<uint32_t> packed(gmg_packed_words(blob.size()) + 1);
    if (!blob.empty()) Check(gmg_pack_bases(blob.data(), blob.size(), 0, packed.data()), "gmg_pack_bases");
    for (size_t i = 0; i < blob.size(); i++)
        if (!blob[i] || !strchr("acgtACGT", blob[i])) b.amb.push_back(i);
    Check(gmg_reads_upload(packed.data(), b.off.data(), recs.size(), &b.reads), "gmg_reads_upload");
    return b;
}

}  // namespace coords

#endif
