// gmg_splice.hip -- gmg_reads_splice (include/gmg.h): a NEW batch on the device whose strings are concatenations of runs -- stretches
// of the reads of a batch read upwards or downwards, with or without the code complement, with or without extract_aa.py's
// substitution on codes, and literal codes: the gene strings of a prediction run with its insertions, deletions and substitutions
// applied, without the text in between.  The sibling of gmg_reads_extract (gmg_extract.hip), with the same shape: lengths and a
// check of every run by one kernel, offsets by a scan, the gather through a tile table.
//
// The gather never sees a string: a string's end is a run's end, so the new batch is the concatenation of ALL runs in output
// order, and the strings' offsets are the runs' offsets at string_run_off[].  k_spl_len leaves every run as 16 bytes {job-wide
// index of the source base that comes out first, length, flags} AT ITS PLACE IN THE OUTPUT: under GMG_EXTRACT_REVERSED the runs of
// a string change places and every run turns round (up <-> down; the complement stays), which reverses the string.
// Substitutions and literals are part of a word's assembly: nothing is patched behind the gather, and no word is written twice.

#include "gmg_internal.h"

#include "gmg_piece.h"
#include "gmg_scan.h"

#include <string.h>
#include <new>

struct SplMeta {
    uint64_t src;                // job-wide index of the source base of the run's base 0
    uint32_t len;
    uint32_t flags;
};
#define SPL_DOWN 1u              // base j of the run is source base src - j (otherwise src + j)
#define SPL_COMP 2u              // 3 - code
#define SPL_SUB 4u               // c -> g, anything else -> c, before the complement
#define SPL_LIT 8u               // the code in bits 4 .. 5, whatever the source holds

// One lane per run.  stats: [0] min string length, [1] max, [2] strings over 512 bases (k_spl_off), [4] first bad run
__global__ __launch_bounds__(256) void k_spl_len(const uint64_t *__restrict__ src_off, uint64_t n_src, const gmg_splice_run *__restrict__ runs,
                                                 uint64_t n_runs, const uint64_t *__restrict__ sro, uint64_t n_strings, int reversed,
                                                 uint32_t *__restrict__ len, SplMeta *__restrict__ meta, unsigned long long *stats)
{
    unsigned long long bad = ~0ull;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i <= n_runs; i += (uint64_t)gridDim.x * blockDim.x) {
        if (i == n_runs) { len[i] = 0; break; }         // (the scan's last output is the total)
        const gmg_splice_run r = runs[i];
        SplMeta m = {0, 0, 0};
        bool ok = r.kind < GMG_RUN_LITERAL_AS_IS + 4 && r.len < 0x80000000u;
        if (ok && r.kind >= GMG_RUN_LITERAL) {
            m.len = r.len;
            m.flags = SPL_LIT | ((r.kind & 3u) << 4);
        } else if (ok) {
            ok = r.read < n_src;
            if (ok) {
                const uint64_t b = src_off[r.read], L = src_off[(uint64_t)r.read + 1] - b;
                const bool down = (r.kind & 1u) != 0;
                if (!down) ok = (uint64_t)r.first + r.len <= L;
                else ok = r.len ? r.first < L && r.len <= r.first + 1u : r.first <= L;
                if (ok) {
                    // the run's first and last source position in its own direction; reversed: it starts at the last and turns
                    const uint64_t p_first = r.first, p_last = r.len ? (down ? p_first - (r.len - 1) : p_first + (r.len - 1)) : p_first;
                    m.src = b + (reversed ? p_last : p_first);
                    m.len = r.len;
                    m.flags = ((down != (reversed != 0)) ? SPL_DOWN : 0u) | (down ? SPL_COMP : 0u) | (r.kind >= GMG_RUN_SUB_UP ? SPL_SUB : 0u);
                }
            }
        }
        if (!ok) { bad = i < bad ? i : bad; m.len = 0; m.flags = SPL_LIT; }
        uint64_t slot = i;
        if (reversed) {                                 // the string of run i: the largest k < n_strings with sro[k] <= i
            uint64_t lo = 0, hi = n_strings - 1;
            while (lo < hi) {
                const uint64_t mid = (lo + hi + 1) >> 1;
                if (sro[mid] <= i) lo = mid; else hi = mid - 1;
            }
            slot = sro[lo] + (sro[lo + 1] - 1 - i);
        }
        meta[slot] = m;
        len[slot] = m.len;
    }
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long c = __shfl_xor(bad, o);
        bad = c < bad ? c : bad;
    }
    if ((threadIdx.x & 63) == 0 && bad != ~0ull) atomicMin(&stats[4], bad);
}

// the strings' offsets out of the runs', and the statistics of their lengths
__global__ __launch_bounds__(256) void k_spl_off(const uint64_t *__restrict__ roff, const uint64_t *__restrict__ sro, uint64_t n_strings,
                                                 uint64_t *__restrict__ new_off, unsigned long long *stats)
{
    unsigned long long mn = ~0ull, mx = 0, over = 0;
    for (uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; k <= n_strings; k += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t b = roff[sro[k]];
        new_off[k] = b;
        if (k < n_strings) {
            const uint64_t l = roff[sro[k + 1]] - b;
            mn = l < mn ? l : mn;
            mx = l > mx ? l : mx;
            over += l > 512;
        }
    }
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long a = __shfl_xor(mn, o), b = __shfl_xor(mx, o);
        mn = a < mn ? a : mn;
        mx = b > mx ? b : mx;
        over += __shfl_xor(over, o);
    }
    if ((threadIdx.x & 63) == 0) {
        if (mn != ~0ull) atomicMin(&stats[0], mn);
        if (mx) atomicMax(&stats[1], mx);
        if (over) atomicAdd(&stats[2], over);
    }
}

// bases j .. j + nb - 1 (nb = 1 .. 16, inside the run) of a run as 2-bit codes from bit 0
__device__ __forceinline__ uint32_t spl_piece(const uint32_t *__restrict__ src, uint64_t run_src, uint32_t flags, uint32_t j, unsigned nb)
{
    const uint32_t mask = nb >= 16 ? 0xffffffffu : ((1u << (2 * nb)) - 1u);
    if (flags & SPL_LIT) return (0x55555555u * ((flags >> 4) & 3u)) & mask;
    const bool down = (flags & SPL_DOWN) != 0;
    uint32_t x = ext_piece(src, down ? run_src - j : run_src + j, 0, down, false, nb);
    if (flags & SPL_SUB) {
        const uint32_t is_c = x & ~(x >> 1) & 0x55555555u;  // code 01
        x = (is_c << 1) | (~is_c & 0x55555555u);            // c -> 10, the rest -> 01
    }
    if (flags & SPL_COMP) x = ~x;
    return x & mask;
}

// One wave per 1,024-base tile of the NEW batch, a lane per 16-base word (k_reads_extract's shape).  The runs that overlap the tile
// -- the first one from the tile table over the runs' offsets -- have their ends and SplMeta fetched once, a lane each, into LDS;
// a lane then assembles its word from pieces, each a 32-base window of the source: a piece ends at the run's end or at the word's
// end.  A tile that more than SPL_R runs overlap (strings of many tiny runs, many tiny strings) takes the words behind the staged
// runs base by base from the tables in memory: slower, the same result.
#define SPL_R 64
__global__ __launch_bounds__(256) void k_reads_splice(const uint32_t *__restrict__ src, const SplMeta *__restrict__ meta,
                                                      const uint64_t *__restrict__ roff, const uint32_t *__restrict__ tile_run, uint64_t n_runs,
                                                      uint64_t total, uint32_t *__restrict__ dst)
{
    __shared__ uint64_t s_end[4][SPL_R], s_beg[4][SPL_R], s_src[4][SPL_R];
    __shared__ uint32_t s_flags[4][SPL_R];
    const uint32_t wv = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    const uint64_t n_tiles = (total + GMG_TILE - 1) / GMG_TILE;
    for (uint64_t t = (uint64_t)blockIdx.x * 4 + wv; t < n_tiles; t += (uint64_t)gridDim.x * 4) {
        const uint64_t r0 = tile_run[t];
        {
            const uint64_t r = r0 + lane < n_runs ? r0 + lane : n_runs - 1;
            const SplMeta m = meta[r];
            s_beg[wv][lane] = roff[r];
            s_end[wv][lane] = r0 + lane < n_runs ? roff[r + 1] : ~0ull;
            s_src[wv][lane] = m.src;
            s_flags[wv][lane] = m.flags;
        }
        __builtin_amdgcn_wave_barrier();
        const uint64_t g0 = t * GMG_TILE + 16 * (uint64_t)lane;
        if (g0 < total) {
            const uint64_t g1 = g0 + 16 < total ? g0 + 16 : total;
            uint32_t k = 0, out = 0;
            uint64_t pos = g0;
            while (pos < g1) {
                while (k < SPL_R && s_end[wv][k] <= pos) k++;          // the run that holds base pos (empty ones are stepped over)
                if (k >= SPL_R) break;
                const uint64_t e = s_end[wv][k] < g1 ? s_end[wv][k] : g1;
                const unsigned nb = (unsigned)(e - pos);                // 1 .. 16
                out |= spl_piece(src, s_src[wv][k], s_flags[wv][k], (uint32_t)(pos - s_beg[wv][k]), nb) << (2u * (unsigned)(pos - g0));
                pos += nb;
            }
            if (pos < g1) {                             // beyond the runs in LDS: base by base
                uint64_t r = r0 + SPL_R - 1;
                for (; pos < g1; pos++) {
                    while (roff[r + 1] <= pos) r++;     // (pos < total = roff[n_runs]: r stays below n_runs)
                    const SplMeta m = meta[r];
                    out |= spl_piece(src, m.src, m.flags, (uint32_t)(pos - roff[r]), 1) << (2u * (unsigned)(pos - g0));
                }
            }
            dst[t * (GMG_TILE / 16) + lane] = out;
        }
        __builtin_amdgcn_wave_barrier();
    }
}

extern "C" int gmg_reads_splice(const gmg_reads *reads, const gmg_splice_run *runs, uint64_t n_runs, const uint64_t *string_run_off,
                                uint64_t n_strings, int flags, gmg_reads **out)
{
    { int rc_enter = gmg_enter("gmg_reads_splice"); if (rc_enter) return rc_enter; }
    if (!reads || (!runs && n_runs) || !string_run_off || !out || n_strings >= 0x7ffffffeull || n_runs >= 0x7ffffffeull ||
        (flags & ~GMG_EXTRACT_REVERSED))
        return gmg_set_error(GMG_EINVAL, "gmg_reads_splice: bad argument");
    if (string_run_off[0] != 0 || string_run_off[n_strings] != n_runs)
        return gmg_set_error(GMG_EINVAL, "gmg_reads_splice: string_run_off must run from 0 to n_runs");
    for (uint64_t k = 0; k < n_strings; k++)
        if (string_run_off[k] > string_run_off[k + 1])
            return gmg_set_error(GMG_EINVAL, "gmg_reads_splice: string_run_off descends at string %llu", (unsigned long long)k);
    const int reversed = (flags & GMG_EXTRACT_REVERSED) != 0;
    const uint64_t n = n_strings;
    hipStream_t s = 0;
    GmgScratch sc(GmgScratch::STREAM, s);               // (kernels already queued may still use the blocks that go back to the cache)
    gmg_splice_run *d_runs = nullptr;
    SplMeta *d_meta = nullptr;
    uint32_t *d_len = nullptr;
    uint64_t *d_sro = nullptr, *d_roff = nullptr, *d_off = nullptr;
    unsigned long long *d_stats = nullptr;
    GMG_HIP(sc.alloc(&d_runs, (n_runs ? n_runs : 1) * sizeof(gmg_splice_run)));
    GMG_HIP(sc.alloc(&d_meta, (n_runs ? n_runs : 1) * sizeof(SplMeta)));
    GMG_HIP(sc.alloc(&d_len, (n_runs + 1) * 4));
    GMG_HIP(sc.alloc(&d_roff, (n_runs + 1) * 8));
    GMG_HIP(sc.alloc(&d_sro, (n + 1) * 8));
    GMG_HIP(sc.alloc(&d_off, (n + 1) * 8));
    GMG_HIP(sc.alloc(&d_stats, 8 * sizeof(unsigned long long)));
    const unsigned long long stats0[6] = {~0ull, 0, 0, 0, ~0ull, 0};
    unsigned long long stats[6];
    GMG_HIP(hipMemcpyAsync(d_stats, stats0, sizeof stats0, hipMemcpyHostToDevice, s));
    if (n_runs) GMG_HIP(hipMemcpyAsync(d_runs, runs, n_runs * sizeof(gmg_splice_run), hipMemcpyHostToDevice, s));
    GMG_HIP(hipMemcpyAsync(d_sro, string_run_off, (n + 1) * 8, hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(k_spl_len, dim3((unsigned)((n_runs + 256) / 256 < 512 ? (n_runs + 256) / 256 : 512)), dim3(256), 0, s, reads->d_off,
                       reads->n_reads, d_runs, n_runs, d_sro, n, reversed, d_len, d_meta, d_stats);
    GMG_HIP((gmg_scan_excl<uint32_t, uint64_t>(d_len, d_roff, n_runs + 1, s)));
    hipLaunchKernelGGL(k_spl_off, dim3((unsigned)((n + 256) / 256 < 512 ? (n + 256) / 256 : 512)), dim3(256), 0, s, d_roff, d_sro, n, d_off, d_stats);
    GMG_HIP(hipGetLastError());
    GMG_HIP(hipMemcpyAsync(&stats[5], d_roff + n_runs, 8, hipMemcpyDeviceToHost, s));
    GMG_HIP(hipMemcpyAsync(stats, d_stats, 5 * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
    GMG_HIP(hipStreamSynchronize(s));
    if (stats[4] != ~0ull) {
        const gmg_splice_run &r = runs[stats[4]];
        return gmg_set_error(GMG_ERANGE, "gmg_reads_splice: run %llu (read %u, first %u, len %u, kind %u) does not fit its read (the batch has %llu)",
                             stats[4], r.read, r.first, r.len, r.kind, (unsigned long long)reads->n_reads);
    }
    // the packed words (guards zeroed; the gather writes every data word), the two tile tables, the gather
    const uint64_t total = stats[5], data_words = (total + 15) / 16;
    uint32_t *alloc = nullptr;
    GMG_HIP(sc.alloc(&alloc, (data_words + 2 * GMG_GUARD_WORDS) * 4));
    GMG_HIP(hipMemsetAsync(alloc, 0, GMG_GUARD_WORDS * 4, s));
    GMG_HIP(hipMemsetAsync(alloc + GMG_GUARD_WORDS + data_words, 0, GMG_GUARD_WORDS * 4, s));
    gmg_reads tmp;                                      // (the batch goes to the heap once nothing can fail any more)
    memset(&tmp, 0, sizeof tmp);
    tmp.n_reads = n;
    tmp.total_bases = total;
    tmp.d_off = d_off;
    tmp.owns_off = 1;
    tmp.n_words = data_words + GMG_GUARD_WORDS;
    tmp.d_packed_alloc = alloc;
    tmp.d_packed = alloc + GMG_GUARD_WORDS;
    { const int rc = gmg_reads_tile_table(&tmp, sc, s); if (rc) return rc; }
    if (data_words) {
        uint32_t *d_tile_run = nullptr;                 // the run that holds the first base of every tile
        GMG_HIP(sc.alloc(&d_tile_run, (tmp.n_tiles + 1) * 4));
        { const int rc = gmg_launch_tile_read(d_roff, n_runs, tmp.n_tiles, d_tile_run, s); if (rc) return rc; }
        const uint64_t blocks = (tmp.n_tiles + 3) / 4;     // one wave per tile
        hipLaunchKernelGGL(k_reads_splice, dim3((unsigned)(blocks < 65536 ? blocks : 65536)), dim3(256), 0, s, reads->d_packed, d_meta, d_roff,
                           d_tile_run, n_runs, total, alloc + GMG_GUARD_WORDS);
        GMG_HIP(hipGetLastError());
    }
    GMG_HIP(hipStreamSynchronize(s));
    gmg_reads_set_lengths(&tmp, stats);
    gmg_reads *r = new (std::nothrow) gmg_reads(tmp);
    if (!r) return gmg_set_error(GMG_ENOMEM, "gmg_reads_splice: out of host memory");
    sc.detach(d_off); sc.detach(alloc); sc.detach(tmp.d_tile_read);
    sc.wait = GmgScratch::NONE;                         // (waited for just now)
    *out = r;
    return GMG_OK;
}
