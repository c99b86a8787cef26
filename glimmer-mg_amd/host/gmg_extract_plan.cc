// gmg_extract_plan.cc -- the host side of gmg_reads_extract (include/gmg.h): which letters of a file the code complement gets
// wrong (gmg_fasta_ambiguous) and the arithmetic that turns coordinate lines into regions (gmg_extract_plan).  Host only.

#include "../../include/gmg.h"

#include <ctype.h>
#include <stdint.h>
#include <stddef.h>

extern int gmg_set_error(int code, const char *fmt, ...);

// Subscript (Complement (ch)): the reference's complement table (src/Common/gene.cc:15-19) keeps the IUPAC meaning -- r <-> y,
// k <-> m, b <-> v, d <-> h, s, w and n themselves -- and turns everything that is no nucleotide letter into 'n' (or leaves it:
// blank, '*', '-', '.', '_'), all of which Filter sends to 'c'.
static uint8_t rev_code(unsigned char ch)
{
    char comp;
    switch (tolower(ch)) {
    case 'a': comp = 't'; break;
    case 'c': comp = 'g'; break;
    case 'g': comp = 'c'; break;
    case 't': comp = 'a'; break;
    case 'r': comp = 'y'; break;
    case 'y': comp = 'r'; break;
    case 'k': comp = 'm'; break;
    case 'm': comp = 'k'; break;
    case 'b': comp = 'v'; break;
    case 'v': comp = 'b'; break;
    case 'd': comp = 'h'; break;
    case 'h': comp = 'd'; break;
    case 's': comp = 's'; break;
    case 'w': comp = 'w'; break;
    default: comp = 'n'; break;
    }
    return (uint8_t)gmg_base_code(comp);
}

// Fasta_Read's records as gmg_fasta_ingest applies them (gmg_ingest.hip): a '>' outside a header line starts a record, the header
// runs to the end of its line, every byte behind it that is neither '>' nor isspace is a base; bytes in front of the first '>'
// are skipped.
extern "C" int gmg_fasta_ambiguous(const char *bytes, uint64_t n_bytes, uint64_t *base, uint8_t *rev, uint64_t cap, uint64_t *n)
{
    if ((!bytes && n_bytes) || !n || (cap && (!base || !rev))) return gmg_set_error(GMG_EINVAL, "gmg_fasta_ambiguous: NULL argument");
    enum { PRE, HDR, SEQ } st = PRE;
    uint64_t b = 0, found = 0;
    for (uint64_t i = 0; i < n_bytes; i++) {
        const unsigned char ch = (unsigned char)bytes[i];
        if (ch == '>') { st = HDR; continue; }          // ('>' inside a header line is text: the state stays)
        if (st == HDR) { if (ch == '\n') st = SEQ; continue; }
        if (st != SEQ || ch == ' ' || (ch >= 9 && ch <= 13)) continue;
        switch (ch) {
        case 'a': case 'c': case 'g': case 't': case 'A': case 'C': case 'G': case 'T': break;
        default:
            if (found < cap) { base[found] = b; rev[found] = rev_code(ch); }
            found++;
        }
        b++;
    }
    *n = found;
    return GMG_OK;
}

extern "C" int gmg_extract_plan(const uint64_t *base_offsets, uint64_t n_reads, const gmg_coord *coords, uint64_t n, int flags,
                                int64_t min_len, gmg_gene_region *regions, uint64_t *coord_of_region, uint64_t *n_regions)
{
    const int known = GMG_COORD_USE_DIR | GMG_COORD_NOWRAP | GMG_COORD_SKIP_START | GMG_COORD_SKIP_STOP | GMG_COORD_MULTI;
    if (!base_offsets || (!coords && n) || (!regions && n) || !n_regions || (flags & ~known))
        return gmg_set_error(GMG_EINVAL, "gmg_extract_plan: bad argument");
    const bool circular = !(flags & GMG_COORD_NOWRAP), multi = (flags & GMG_COORD_MULTI) != 0;
    uint64_t k = 0;
    *n_regions = 0;
    for (uint64_t c = 0; c < n; c++) {
        const gmg_coord &co = coords[c];
        if (co.read >= n_reads)
            return gmg_set_error(GMG_ERANGE, "gmg_extract_plan: line %llu names sequence %u of %llu", (unsigned long long)c, co.read,
                                 (unsigned long long)n_reads);
        const int64_t L = (int64_t)(base_offsets[co.read + 1] - base_offsets[co.read]);
        const int64_t start = co.start, end = co.end;
        int dir;
        if (flags & GMG_COORD_USE_DIR) dir = co.dir;
        else dir = ((start < end && (!circular || end - start <= L / 2)) || (circular && start - end > L / 2)) ? 1 : -1;
        const bool fwd = dir > 0;
        int64_t len = fwd ? 1 + end - start : 1 + start - end;
        if (len < 0) len += L;
        if (!multi && len < min_len) continue;
        int64_t i = start - 1;
        if (flags & GMG_COORD_SKIP_START) { i += fwd ? 3 : -3; len -= 3; }
        if (flags & GMG_COORD_SKIP_STOP) len -= 3;
        if (len < min_len) continue;
        if (L <= 0)
            return gmg_set_error(GMG_ERANGE, "gmg_extract_plan: line %llu (%lld %lld): sequence %u is empty", (unsigned long long)c,
                                 (long long)start, (long long)end, co.read);
        if (len > L)
            return gmg_set_error(GMG_ERANGE, "gmg_extract_plan: line %llu (%lld %lld): %lld bases from a sequence of %lld", (unsigned long long)c,
                                 (long long)start, (long long)end, (long long)len, (long long)L);
        if (len <= 0) { len = 0; i = 0; }               // an empty record: the reference never looks at the sequence
        if (i < 0) i += L;
        else if (i >= L) i -= L;
        if (i < 0 || i >= L)
            return gmg_set_error(GMG_ERANGE, "gmg_extract_plan: line %llu (%lld %lld) starts outside its sequence of %lld bases",
                                 (unsigned long long)c, (long long)start, (long long)end, (long long)L);
        regions[k].read = co.read;
        regions[k].first = (int32_t)i;
        regions[k].len = (int32_t)len;
        regions[k].strand = fwd ? 1 : -1;
        if (coord_of_region) coord_of_region[k] = c;
        k++;
    }
    *n_regions = k;
    return GMG_OK;
}
