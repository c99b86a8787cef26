// gmg_uncovered_plan.cc -- the host side of gmg_regions_uncovered (include/gmg.h): the arithmetic that turns coordinate lines into
// the intervals uncovered takes off its sequence (src/Util/uncovered.cc:87-174).  Host only.
//
// It is not gmg_extract_plan's: no length test, a region over the sequence's end (the start, on the reverse strand) is cut into
// two intervals and not wrapped, and on the reverse strand i = start (not start - 1) with j = i - extract_len give [j, i).

#include "../../include/gmg.h"

#include <stdint.h>
#include <stddef.h>

extern int gmg_set_error(int code, const char *fmt, ...);

extern "C" int gmg_uncovered_plan(const uint64_t *base_offsets, uint64_t n_reads, const gmg_coord *coords, uint64_t n, int flags,
                                  gmg_interval *intervals, uint64_t *n_intervals)
{
    const int known = GMG_COORD_USE_DIR | GMG_COORD_NOWRAP | GMG_COORD_SKIP_START | GMG_COORD_SKIP_STOP;
    if (!base_offsets || (!coords && n) || (!intervals && n) || !n_intervals || (flags & ~known))
        return gmg_set_error(GMG_EINVAL, "gmg_uncovered_plan: bad argument");
    const bool circular = !(flags & GMG_COORD_NOWRAP);
    uint64_t k = 0;
    *n_intervals = 0;
    for (uint64_t c = 0; c < n; c++) {
        const gmg_coord &co = coords[c];
        if (co.read >= n_reads)
            return gmg_set_error(GMG_ERANGE, "gmg_uncovered_plan: line %llu names sequence %u of %llu", (unsigned long long)c, co.read,
                                 (unsigned long long)n_reads);
        const uint64_t UL = base_offsets[co.read + 1] - base_offsets[co.read];
        if (UL >= 0x80000000ull)
            return gmg_set_error(GMG_ERANGE, "gmg_uncovered_plan: line %llu: sequence %u has %llu bases, 2^31 or more", (unsigned long long)c,
                                 co.read, (unsigned long long)UL);
        const int64_t L = (int64_t)UL, start = co.start, end = co.end;
        // (coordinates that could overflow the sums below are outside every sequence anyway)
        if (start < -0x100000000ll || start > 0x100000000ll || end < -0x100000000ll || end > 0x100000000ll)
            return gmg_set_error(GMG_ERANGE, "gmg_uncovered_plan: line %llu (%lld %lld) lies outside its sequence of %lld bases",
                                 (unsigned long long)c, (long long)start, (long long)end, (long long)L);
        int dir;
        if (flags & GMG_COORD_USE_DIR) dir = co.dir;
        else dir = ((start < end && (!circular || end - start <= L / 2)) || (circular && start - end > L / 2)) ? 1 : -1;
        int64_t lo[2], hi[2];
        int m = 1;
        if (dir > 0) {
            int64_t len = 1 + end - start;
            if (len < 0) len += L;
            int64_t i = start - 1;
            if (flags & GMG_COORD_SKIP_START) { i += 3; len -= 3; }
            if (flags & GMG_COORD_SKIP_STOP) len -= 3;
            const int64_t j = i + len;
            if (j <= L) { lo[0] = i; hi[0] = j; }
            else { lo[0] = i; hi[0] = L; lo[1] = 0; hi[1] = j - L; m = 2; }
        } else {
            int64_t len = 1 + start - end;
            if (len < 0) len += L;
            int64_t i = start;
            if (flags & GMG_COORD_SKIP_START) { i -= 3; len -= 3; }
            if (flags & GMG_COORD_SKIP_STOP) len -= 3;
            const int64_t j = i - len;
            if (j >= 0) { lo[0] = j; hi[0] = i; }
            else { lo[0] = 0; hi[0] = i; lo[1] = L + j; hi[1] = L; m = 2; }
        }
        for (int t = 0; t < m; t++) {
            if (!(0 <= lo[t] && lo[t] <= hi[t] && hi[t] <= L))
                return gmg_set_error(GMG_ERANGE, "gmg_uncovered_plan: line %llu (%lld %lld) gives the region %lld .. %lld of a sequence of %lld bases",
                                     (unsigned long long)c, (long long)start, (long long)end, (long long)lo[t], (long long)hi[t], (long long)L);
            intervals[k].read = co.read;
            intervals[k].lo = (int32_t)lo[t];
            intervals[k].hi = (int32_t)hi[t];
            k++;
        }
    }
    *n_intervals = k;
    return GMG_OK;
}
