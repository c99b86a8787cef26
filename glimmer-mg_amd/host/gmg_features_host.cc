// gmg_features_host.cc -- the host side of gmg_features_count (include/gmg.h): which bases of a file are no upper-case ACGT
// (gmg_fasta_not_upper_acgt) and the text of the reference's scripts/train_features.py for a counted table (gmg_features_format:
// output_featurefile, train_features.py:630-673; output_stats, :562-623).  Host only.

#include "../../include/gmg.h"

#include <stdarg.h>
#include <stdint.h>
#include <stddef.h>
#include <stdio.h>
#include <string.h>
#include <string>

extern int gmg_set_error(int code, const char *fmt, ...);

// records as gmg_fasta_ambiguous reads them (gmg_extract_plan.cc), which is how gmg_fasta_ingest numbers the bases
extern "C" int gmg_fasta_not_upper_acgt(const char *bytes, uint64_t n_bytes, uint64_t *base, uint64_t cap, uint64_t *n)
{
    if ((!bytes && n_bytes) || !n || (cap && !base)) return gmg_set_error(GMG_EINVAL, "gmg_fasta_not_upper_acgt: NULL argument");
    enum { PRE, HDR, SEQ } st = PRE;
    uint64_t b = 0, found = 0;
    for (uint64_t i = 0; i < n_bytes; i++) {
        const unsigned char ch = (unsigned char)bytes[i];
        if (ch == '>') { st = HDR; continue; }
        if (st == HDR) { if (ch == '\n') st = SEQ; continue; }
        if (st != SEQ || ch == ' ' || (ch >= 9 && ch <= 13)) continue;
        if (ch != 'A' && ch != 'C' && ch != 'G' && ch != 'T') {
            if (found < cap) base[found] = b;
            found++;
        }
        b++;
    }
    *n = found;
    return GMG_OK;
}

static void put(std::string &s, const char *fmt, ...) __attribute__((format(printf, 2, 3)));
static void put(std::string &s, const char *fmt, ...)
{
    char buf[400];
    va_list ap;
    va_start(ap, fmt);
    const int k = vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (k > 0) s.append(buf, (size_t)k < sizeof buf ? (size_t)k : sizeof buf - 1);
}

static void put_lengths(std::string &s, const gmg_features_table *t)
{
    for (uint64_t l = 0; l < t->n_lengths; l++) put(s, "%llu\t%lld\n", (unsigned long long)l, (long long)t->lengths[l]);
}

static void put_starts(std::string &s, const gmg_features_table *t)
{
    static const char *const name[3] = {"ATG", "GTG", "TTG"};
    for (int k = 0; k < 3; k++) put(s, "%s\t%lld\n", name[k], (long long)t->starts[k]);
}

// Python's '%d' of a float: int(), towards zero
static void put_orients(std::string &s, const gmg_features_table *t)
{
    for (int k = 0; k < 4; k++) put(s, "%d,%d\t%lld\n", k < 2 ? 1 : -1, (k & 1) ? -1 : 1, (long long)t->orient[k]);
}

static void put_dist(std::string &s, const gmg_features_table *t, int k, int max_overlap)
{
    for (uint64_t j = 0; j < t->n_dist[k]; j++) put(s, "%lld\t%.1f\n", (long long)j - max_overlap, t->dist[k][j]);
}

extern "C" int gmg_features_format(const gmg_features_table *t, const char *orf_type, int what, int max_overlap, char *out, size_t *bytes)
{
    if (!t || !bytes || what < GMG_FEATURES_BLOCK || what > GMG_FEATURES_DIST + 2 || (what == GMG_FEATURES_BLOCK && !orf_type) ||
        (t->n_lengths && !t->lengths))
        return gmg_set_error(GMG_EINVAL, "gmg_features_format: bad argument");
    for (int k = 0; k < 3; k++)
        if (t->n_dist[k] && !t->dist[k]) return gmg_set_error(GMG_EINVAL, "gmg_features_format: distance table %d has no values", k);
    std::string s;
    switch (what) {
    case GMG_FEATURES_BLOCK:
        put(s, "DIST LENGTH %s\n", orf_type);
        put_lengths(s, t);
        put(s, "\nDIST START %s\n", orf_type);
        put_starts(s, t);
        put(s, "\nDIST ADJACENT_ORIENTATION %s\n", orf_type);
        put_orients(s, t);
        s += "\n";
        for (int k = 0; k < 3; k++) {
            put(s, "DIST ADJACENT_DISTANCE_%d_%d %s\n", k < 2 ? 1 : -1, (k & 1) ? -1 : 1, orf_type);
            put_dist(s, t, k, max_overlap);
            s += "\n";
        }
        break;
    case GMG_FEATURES_LENGTHS: put_lengths(s, t); break;
    case GMG_FEATURES_STARTS: put_starts(s, t); break;
    case GMG_FEATURES_ORIENTS: put_orients(s, t); break;
    default: put_dist(s, t, what - GMG_FEATURES_DIST, max_overlap); break;
    }
    const size_t room = *bytes;
    *bytes = s.size();
    if (!out) return GMG_OK;
    if (room < s.size()) return gmg_set_error(GMG_ERANGE, "gmg_features_format: %zu bytes of room, the text has %zu", room, s.size());
    memcpy(out, s.data(), s.size());
    return GMG_OK;
}
