// gmg_gather.h -- a NEW batch of reads built on the device out of an old one: what gmg_reads_select (gmg_api.hip),
// gmg_reads_extract (gmg_extract.hip) and gmg_reads_splice (gmg_splice.hip) share.  Every one of them is
//     its own length kernel   the length of every item of the output (a read, a region, a run), a check of it, and the
//                             statistics of the lengths through GmgLenStats
//     gmg_scan_excl           the items' offsets in the new batch
//     its own gather kernel   gmg_gather_tiles over its own source policy, through a tile table over those offsets
// between the steps of a GmgBatchBuilder, which owns the counters, the guarded packed words and the gmg_reads that comes out.
#ifndef GMG_GATHER_H
#define GMG_GATHER_H

#include "gmg_internal.h"

#include <string.h>

// ---------------------------------------------------------------------------
// device: the statistics of a batch's lengths
// ---------------------------------------------------------------------------

// stats: [0] shortest, [1] longest, [2] lengths over 512 bases, [3] unused, [4] first bad item.  A lane folds the items of its
// grid-stride loop; finish() -- reached by all 64 lanes of every wave -- sends the four results of a WAVE to the counters with one
// atomic each, and none for a result that changes nothing (every atomic on one address costs ~10 ns at the L2: one per wave of a
// million reads was 0.36 ms).
struct GmgLenStats {
    unsigned long long mn = ~0ull, mx = 0, over = 0, bad = ~0ull;
    __device__ __forceinline__ void length(unsigned long long l)
    {
        mn = l < mn ? l : mn;
        mx = l > mx ? l : mx;
        over += l > 512;
    }
    __device__ __forceinline__ void bad_item(unsigned long long i) { bad = i < bad ? i : bad; }
    __device__ __forceinline__ void finish(unsigned long long *stats)
    {
        for (int o = 32; o > 0; o >>= 1) {
            const unsigned long long a = __shfl_xor(mn, o), b = __shfl_xor(mx, o), c = __shfl_xor(bad, o);
            mn = a < mn ? a : mn;
            mx = b > mx ? b : mx;
            bad = c < bad ? c : bad;
            over += __shfl_xor(over, o);
        }
        if ((threadIdx.x & 63) == 0) {
            if (mn != ~0ull) atomicMin(&stats[0], mn);
            if (mx) atomicMax(&stats[1], mx);
            if (over) atomicAdd(&stats[2], over);
            if (bad != ~0ull) atomicMin(&stats[4], bad);
        }
    }
};

// ---------------------------------------------------------------------------
// device: the gather
// ---------------------------------------------------------------------------

// nb (1 .. 16) bases of a read whose base 0 is job-wide base S, from position p on, as 2-bit codes from bit 0: upwards p, p + 1, ...
// or downwards p, p - 1, ...  The caller keeps the piece inside the read; what the window holds beyond it (the neighbouring
// reads' bases, the guard words) is masked out here.
__device__ __forceinline__ uint32_t ext_piece(const uint32_t *__restrict__ src, uint64_t S, uint32_t p, bool down, bool comp, unsigned nb)
{
    uint32_t x;
    if (!down) {
        const uint64_t sg = S + p;
        const uint64_t w0 = sg >> 4;
        x = (uint32_t)(((uint64_t)src[w0] | ((uint64_t)src[w0 + 1] << 32)) >> (2u * (unsigned)(sg & 15)));
    } else {
        // the 16 bases that END at S + p (word -1 is the guard in front of the batch): base S + p lands in the top two bits;
        // bit reversal turns the order of the bases AND of the two bits of every base, the second of which is undone
        const int64_t lo = (int64_t)(S + p) - 15;
        const int64_t w0 = lo >> 4;
        x = (uint32_t)(((uint64_t)src[w0] | ((uint64_t)src[w0 + 1] << 32)) >> (2u * (unsigned)(lo & 15)));
        x = __brev(x);
        x = ((x >> 1) & 0x55555555u) | ((x & 0x55555555u) << 1);
    }
    if (comp) x ^= 0xffffffffu;
    return x & (nb >= 16 ? 0xffffffffu : ((1u << (2 * nb)) - 1u));
}

// The body of a gather kernel of 256 lanes: one wave per 1,024-base tile of the NEW batch, a lane per 16-base word.  The items that
// overlap the tile -- the first one from the tile table over the items' offsets off[0 .. n] -- have their ends and what the source
// needs of them fetched ONCE by the wave's first lanes into LDS; a lane then assembles its word from pieces, each a 32-base window
// of the source: a piece ends at the item's end, at the word's end, or where the source says so.  No global load depends on
// another one except through LDS.  A tile that more than Source::R items overlap (many tiny or empty items) takes the words behind
// the staged items base by base from the tables in memory: slower, the same result.
//
// Source supplies
//     R                       items staged per tile
//     Item                    what it stages of an item
//     stage (r, beg)          the Item of item r, whose base 0 is base beg of the new batch
//     piece (item, pos, nb)   bases pos .. pos + nb - 1 of the new batch (nb = 1 .. 16, all inside the item) as 2-bit codes from
//                             bit 0, nothing above them; it may lower nb to what it can deliver in one piece
// The guard words on both sides of the data words are the caller's to zero; every data word is written here, once.
template <class Source>
__device__ __forceinline__ void gmg_gather_tiles(const Source &source, const uint64_t *__restrict__ off, const uint32_t *__restrict__ tile_item,
                                                 uint64_t n, uint64_t total, uint32_t *__restrict__ dst)
{
    constexpr uint32_t R = Source::R;
    __shared__ uint64_t s_end[4][R];
    __shared__ typename Source::Item s_item[4][R];
    const uint32_t wv = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    const uint64_t n_tiles = (total + GMG_TILE - 1) / GMG_TILE;
    for (uint64_t t = (uint64_t)blockIdx.x * 4 + wv; t < n_tiles; t += (uint64_t)gridDim.x * 4) {
        const uint64_t r0 = tile_item[t];
        if (lane < R) {
            const uint64_t r = r0 + lane < n ? r0 + lane : n - 1;      // (total > 0: n > 0.  Items beyond the last: a copy of it that never ends)
            s_end[wv][lane] = r0 + lane < n ? off[r + 1] : ~0ull;
            s_item[wv][lane] = source.stage(r, off[r]);
        }
        __builtin_amdgcn_wave_barrier();
        const uint64_t g0 = t * GMG_TILE + 16 * (uint64_t)lane;
        if (g0 < total) {
            const uint64_t g1 = g0 + 16 < total ? g0 + 16 : total;
            uint32_t k = 0, out = 0;
            uint64_t pos = g0;
            while (pos < g1) {
                while (k < R && s_end[wv][k] <= pos) k++;              // the item that holds base pos (empty ones are stepped over)
                if (k >= R) break;
                const uint64_t e = s_end[wv][k] < g1 ? s_end[wv][k] : g1;
                unsigned nb = (unsigned)(e - pos);                      // 1 .. 16
                out |= source.piece(s_item[wv][k], pos, nb) << (2u * (unsigned)(pos - g0));
                pos += nb;
            }
            if (pos < g1) {                             // beyond the items in LDS: base by base
                uint64_t r = r0 + R - 1;
                for (; pos < g1; pos++) {
                    while (off[r + 1] <= pos) r++;      // (pos < total = off[n]: r stays below n)
                    unsigned nb = 1;
                    out |= source.piece(source.stage(r, off[r]), pos, nb) << (2u * (unsigned)(pos - g0));
                }
            }
            dst[t * (GMG_TILE / 16) + lane] = out;
        }
        __builtin_amdgcn_wave_barrier();                // (the next tile's staging overwrites what the slower lanes still read)
    }
}

// ---------------------------------------------------------------------------
// host (gmg_api.hip): the steps around the kernels
// ---------------------------------------------------------------------------

// Scope-owned through the caller's GmgScratch: whatever step fails, the blocks go back to the cache with the caller's holder.
//     begin ()                        the counters, initialised                       -> the caller's length kernel (and scan)
//     lengths (d_total)               total and counters back on the host, after a wait: stats[4] != ~0 is the caller's error
//     layout (n, d_off)               the guarded packed words, both guards zeroed, the gmg_reads, its tile table queued
//                                                                                     -> the caller's gather, on gather_grid () blocks
//     finish (who, out)               wait, the lengths' statistics, the gmg_reads on the heap owning its three blocks
struct __attribute__((visibility("hidden"))) GmgBatchBuilder {
    GmgScratch &sc;
    hipStream_t s;
    unsigned long long *d_stats = nullptr;
    unsigned long long stats[6];                        // GmgLenStats' counters; [5] the new batch's bases
    gmg_reads tmp;                                      // (the batch goes to the heap once nothing can fail any more)
    uint64_t total = 0, data_words = 0;
    uint32_t *d_words = nullptr;                        // the data words: behind the guard in front
    GmgBatchBuilder(GmgScratch &scratch, hipStream_t stream) : sc(scratch), s(stream) { memset(&tmp, 0, sizeof tmp); }
    int begin();
    int lengths(const uint64_t *d_total);
    int layout(uint64_t n, uint64_t *d_off);
    unsigned gather_grid() const                        // one wave per tile
    {
        const uint64_t blocks = (tmp.n_tiles + 3) / 4;
        return (unsigned)(blocks < 65536 ? blocks : 65536);
    }
    int finish(const char *who, gmg_reads **out);
};

#endif
