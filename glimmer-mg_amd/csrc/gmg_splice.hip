// gmg_splice.hip -- gmg_reads_splice (include/gmg.h): a NEW batch on the device whose strings are concatenations of runs -- stretches
// of the reads of a batch read upwards or downwards, with or without the code complement, with or without extract_aa.py's
// substitution on codes, and literal codes: the gene strings of a prediction run with its insertions, deletions and substitutions
// applied, without the text in between.  One of the three batch builders of gmg_gather.h: k_spl_len and k_spl_off are its length
// kernels, SplSource its gather's source.
//
// The gather never sees a string: a string's end is a run's end, so the new batch is the concatenation of ALL runs in output
// order, and the strings' offsets are the runs' offsets at string_run_off[].  k_spl_len leaves every run as 16 bytes {job-wide
// index of the source base that comes out first, length, flags} AT ITS PLACE IN THE OUTPUT: under GMG_EXTRACT_REVERSED the runs of
// a string change places and every run turns round (up <-> down; the complement stays), which reverses the string.
// Substitutions and literals are part of a word's assembly: nothing is patched behind the gather, and no word is written twice.

#include "gmg_internal.h"

#include "gmg_gather.h"
#include "gmg_scan.h"

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
    GmgLenStats st;                                     // (the lengths are the strings': k_spl_off)
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
        if (!ok) { st.bad_item(i); m.len = 0; m.flags = SPL_LIT; }
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
    st.finish(stats);
}

// the strings' offsets out of the runs', and the statistics of their lengths
__global__ __launch_bounds__(256) void k_spl_off(const uint64_t *__restrict__ roff, const uint64_t *__restrict__ sro, uint64_t n_strings,
                                                 uint64_t *__restrict__ new_off, unsigned long long *stats)
{
    GmgLenStats st;
    for (uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; k <= n_strings; k += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t b = roff[sro[k]];
        new_off[k] = b;
        if (k < n_strings) st.length(roff[sro[k + 1]] - b);
    }
    st.finish(stats);
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

// the gather's items are the RUNS: a piece ends at the run's end or at the word's end
struct SplSource {
    static constexpr uint32_t R = 64;
    struct Item { uint64_t beg, src; uint32_t flags; };  // the run's base 0 in the new batch; SplMeta's src and flags
    const uint32_t *__restrict__ src;
    const SplMeta *__restrict__ meta;
    __device__ __forceinline__ Item stage(uint64_t r, uint64_t beg) const
    {
        const SplMeta m = meta[r];
        return Item{beg, m.src, m.flags};
    }
    __device__ __forceinline__ uint32_t piece(const Item &it, uint64_t pos, unsigned &nb) const
    {
        return spl_piece(src, it.src, it.flags, (uint32_t)(pos - it.beg), nb);
    }
};

__global__ __launch_bounds__(256) void k_reads_splice(const uint32_t *__restrict__ src, const SplMeta *__restrict__ meta,
                                                      const uint64_t *__restrict__ roff, const uint32_t *__restrict__ tile_run, uint64_t n_runs,
                                                      uint64_t total, uint32_t *__restrict__ dst)
{
    gmg_gather_tiles(SplSource{src, meta}, roff, tile_run, n_runs, total, dst);
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
    GmgBatchBuilder b(sc, s);
    gmg_splice_run *d_runs = nullptr;
    SplMeta *d_meta = nullptr;
    uint32_t *d_len = nullptr;
    uint64_t *d_sro = nullptr, *d_roff = nullptr, *d_off = nullptr;
    GMG_HIP(sc.alloc(&d_runs, (n_runs ? n_runs : 1) * sizeof(gmg_splice_run)));
    GMG_HIP(sc.alloc(&d_meta, (n_runs ? n_runs : 1) * sizeof(SplMeta)));
    GMG_HIP(sc.alloc(&d_len, (n_runs + 1) * 4));
    GMG_HIP(sc.alloc(&d_roff, (n_runs + 1) * 8));
    GMG_HIP(sc.alloc(&d_sro, (n + 1) * 8));
    GMG_HIP(sc.alloc(&d_off, (n + 1) * 8));
    { const int rc = b.begin(); if (rc) return rc; }
    if (n_runs) GMG_HIP(hipMemcpyAsync(d_runs, runs, n_runs * sizeof(gmg_splice_run), hipMemcpyHostToDevice, s));
    GMG_HIP(hipMemcpyAsync(d_sro, string_run_off, (n + 1) * 8, hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(k_spl_len, dim3(gmg_grid(n_runs + 1, 256, 512)), dim3(256), 0, s, reads->d_off, reads->n_reads, d_runs, n_runs, d_sro, n,
                       reversed, d_len, d_meta, b.d_stats);
    GMG_HIP((gmg_scan_excl<uint32_t, uint64_t>(d_len, d_roff, n_runs + 1, s)));
    hipLaunchKernelGGL(k_spl_off, dim3(gmg_grid(n + 1, 256, 512)), dim3(256), 0, s, d_roff, d_sro, n, d_off, b.d_stats);
    { const int rc = b.lengths(d_roff + n_runs); if (rc) return rc; }
    if (b.stats[4] != ~0ull) {
        const gmg_splice_run &r = runs[b.stats[4]];
        return gmg_set_error(GMG_ERANGE, "gmg_reads_splice: run %llu (read %u, first %u, len %u, kind %u) does not fit its read (the batch has %llu)",
                             b.stats[4], r.read, r.first, r.len, r.kind, (unsigned long long)reads->n_reads);
    }
    { const int rc = b.layout(n, d_off); if (rc) return rc; }
    if (b.data_words) {
        uint32_t *d_tile_run = nullptr;                 // the run that holds the first base of every tile
        GMG_HIP(sc.alloc(&d_tile_run, (b.tmp.n_tiles + 1) * 4));
        { const int rc = gmg_launch_tile_read(d_roff, n_runs, b.tmp.n_tiles, d_tile_run, s); if (rc) return rc; }
        hipLaunchKernelGGL(k_reads_splice, dim3(b.gather_grid()), dim3(256), 0, s, reads->d_packed, d_meta, d_roff, d_tile_run, n_runs, b.total,
                           b.d_words);
    }
    return b.finish("gmg_reads_splice", out);
}
