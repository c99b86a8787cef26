// gmg_extract.hip -- gmg_reads_extract (include/gmg.h): regions of the reads of a batch, any strand, modulo their read, gathered
// into a NEW batch on the device: what `extract` / `multi-extract` print and build-icm parses back, without the text in between
// (src/Util/extract.cc:158-207, Output_Subsequence).  Conceptually the sibling of gmg_reads_select (gmg_api.hip): lengths and a
// check of every region by one kernel, offsets by a scan, the gather through the new batch's tile table.
//
// String k walks its read from position p0 upwards or downwards, modulo the read's length, with or without the code complement:
//     strand > 0            p0 = first              up,   codes as they are
//     strand < 0            p0 = first              down, 3 - code
//     strand > 0, REVERSED  p0 = first + len - 1    down, codes as they are
//     strand < 0, REVERSED  p0 = first - len + 1    up,   3 - code
// (gmg_orient's four cases).  k_ext_len leaves that as 16 bytes per string {source index of the read's base 0, read length, p0,
// the two flags}; k_reads_extract never sees a gmg_gene_region again.
//
// The code complement is not what the reference prints for a letter outside acgt (Complement ('n') = 'n', whose code is c, not
// g): the caller's list of such bases becomes a handful of (output base, code) patches on the host, applied by k_ext_patch
// behind the gather.

#include "gmg_internal.h"

#include "gmg_piece.h"
#include "gmg_scan.h"

#include <string.h>
#include <algorithm>
#include <new>
#include <vector>

struct ExtMeta {
    uint64_t src;                // job-wide index of the source read's base 0
    uint32_t len;                // the read's length (< 2^31); bit 31: complement
    uint32_t p0;                 // position in the read of the string's base 0 (< 2^31); bit 31: walk downwards
};
#define EXT_FLAG 0x80000000u

struct ExtPatch {
    uint64_t base;               // base index in the new batch
    uint64_t code;
};

// stats: [0] min length, [1] max length, [2] strings over 512 bases, [3] unused, [4] first bad region
__global__ __launch_bounds__(256) void k_ext_len(const uint64_t *src_off, const gmg_gene_region *regions, uint64_t n, uint64_t n_src, int reversed,
                                                 uint64_t *len, ExtMeta *meta, unsigned long long *stats)
{
    unsigned long long mn = ~0ull, mx = 0, over = 0, bad = ~0ull;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i <= n; i += (uint64_t)gridDim.x * blockDim.x) {
        uint64_t l = 0;
        if (i < n) {
            const gmg_gene_region r = regions[i];
            ExtMeta m = {0, 0, 0};
            bool ok = r.read < n_src && r.strand != 0 && r.first >= 0 && r.len >= 0;
            if (ok) {
                const uint64_t b = src_off[r.read], L = src_off[(uint64_t)r.read + 1] - b;
                ok = (uint64_t)r.first < L && (uint64_t)r.len <= L;
                if (ok) {
                    l = (uint64_t)r.len;
                    const bool comp = r.strand < 0, down = comp != (reversed != 0);
                    int64_t p0 = r.first;
                    if (reversed && l) p0 += comp ? -(int64_t)(l - 1) : (int64_t)(l - 1);
                    if (p0 < 0) p0 += (int64_t)L;
                    if (p0 >= (int64_t)L) p0 -= (int64_t)L;
                    m.src = b;
                    m.len = (uint32_t)L | (comp ? EXT_FLAG : 0u);
                    m.p0 = (uint32_t)p0 | (down ? EXT_FLAG : 0u);
                }
            }
            if (!ok) bad = i < bad ? i : bad;
            meta[i] = m;
            mn = l < mn ? l : mn;
            mx = l > mx ? l : mx;
            over += l > 512;
        }
        len[i] = l;                                     // len[n] = 0: the scan's last output is the total
    }
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

// One wave per 1,024-base tile of the NEW batch, a lane per 16-base word (k_reads_select's shape).  The strings that overlap the
// tile -- the first one from the tile table -- have their ends and ExtMeta fetched once by the wave's first lanes into LDS; a
// lane then assembles its word from pieces, each a 32-base window of the source: a piece ends at the string's end, at the word's
// end, or where the string wraps around its read.
#define EXT_R 32                                        // strings of a tile handled through LDS; further ones (tiles of many tiny strings) base by base
__global__ __launch_bounds__(256) void k_reads_extract(const uint32_t *__restrict__ src, const ExtMeta *__restrict__ meta,
                                                       const uint64_t *__restrict__ new_off, const uint32_t *__restrict__ tile_read, uint64_t n,
                                                       uint64_t total, uint32_t *__restrict__ dst)
{
    __shared__ uint64_t s_end[4][EXT_R], s_beg[4][EXT_R], s_src[4][EXT_R];
    __shared__ uint32_t s_len[4][EXT_R], s_p0[4][EXT_R];
    const uint32_t wv = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    const uint64_t n_tiles = (total + GMG_TILE - 1) / GMG_TILE;
    for (uint64_t t = (uint64_t)blockIdx.x * 4 + wv; t < n_tiles; t += (uint64_t)gridDim.x * 4) {
        const uint64_t r0 = tile_read[t];
        if (lane < EXT_R) {
            const uint64_t r = r0 + lane < n ? r0 + lane : n - 1;
            const ExtMeta m = meta[r];
            s_beg[wv][lane] = new_off[r];
            s_end[wv][lane] = r0 + lane < n ? new_off[r + 1] : ~0ull;
            s_src[wv][lane] = m.src;
            s_len[wv][lane] = m.len;
            s_p0[wv][lane] = m.p0;
        }
        __builtin_amdgcn_wave_barrier();
        const uint64_t g0 = t * GMG_TILE + 16 * (uint64_t)lane;
        if (g0 < total) {
            const uint64_t g1 = g0 + 16 < total ? g0 + 16 : total;
            uint32_t k = 0, out = 0;
            uint64_t pos = g0;
            while (pos < g1) {
                while (k < EXT_R && s_end[wv][k] <= pos) k++;          // the string that holds base pos (empty ones are stepped over)
                if (k >= EXT_R) break;
                const uint64_t e = s_end[wv][k] < g1 ? s_end[wv][k] : g1;
                const uint32_t L = s_len[wv][k] & ~EXT_FLAG, p0 = s_p0[wv][k] & ~EXT_FLAG;
                const bool comp = (s_len[wv][k] & EXT_FLAG) != 0, down = (s_p0[wv][k] & EXT_FLAG) != 0;
                const uint32_t j = (uint32_t)(pos - s_beg[wv][k]);     // base j of the string: j < its length <= L
                uint32_t p, room;                                       // its position in the read; bases up to the wrap
                if (!down) { p = p0 + j; if (p >= L) p -= L; room = L - p; }
                else { p = p0 >= j ? p0 - j : p0 + L - j; room = p + 1; }
                unsigned nb = (unsigned)(e - pos);                      // 1 .. 16
                nb = nb < room ? nb : room;
                out |= ext_piece(src, s_src[wv][k], p, down, comp, nb) << (2u * (unsigned)(pos - g0));
                pos += nb;
            }
            if (pos < g1) {                             // beyond the strings in LDS: base by base
                uint64_t r = r0 + EXT_R - 1;
                for (; pos < g1; pos++) {
                    while (new_off[r + 1] <= pos) r++;
                    const ExtMeta m = meta[r];
                    const uint32_t L = m.len & ~EXT_FLAG, p0 = m.p0 & ~EXT_FLAG, j = (uint32_t)(pos - new_off[r]);
                    uint32_t p;
                    if (!(m.p0 & EXT_FLAG)) { p = p0 + j; if (p >= L) p -= L; }
                    else p = p0 >= j ? p0 - j : p0 + L - j;
                    const uint64_t sg = m.src + p;
                    uint32_t c = (src[sg >> 4] >> (2u * (unsigned)(sg & 15))) & 3u;
                    if (m.len & EXT_FLAG) c ^= 3u;
                    out |= c << (2u * (unsigned)(pos - g0));
                }
            }
            dst[t * (GMG_TILE / 16) + lane] = out;
        }
        __builtin_amdgcn_wave_barrier();
    }
}

// the exceptions: two bits of a word each (several patches may share a word: atomics on it)
__global__ __launch_bounds__(256) void k_ext_patch(const ExtPatch *__restrict__ patch, uint64_t n, uint32_t *dst)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const ExtPatch p = patch[i];
    const unsigned sh = 2u * (unsigned)(p.base & 15);
    atomicAnd(&dst[p.base >> 4], ~(3u << sh));
    atomicOr(&dst[p.base >> 4], (uint32_t)(p.code & 3) << sh);
}

// The patches of every reverse-strand region that covers a listed base.  src_off, new_off: HOST copies of the two batches' offsets.
static void ext_patches(const gmg_gene_region *regions, uint64_t n, int reversed, const uint64_t *src_off, const uint64_t *new_off,
                        const uint64_t *amb_base, const uint8_t *amb_rev_code, uint64_t n_amb, std::vector<ExtPatch> &out)
{
    for (uint64_t k = 0; k < n; k++) {
        const gmg_gene_region &r = regions[k];
        if (r.strand > 0 || r.len <= 0) continue;
        const uint64_t S = src_off[r.read], L = src_off[(uint64_t)r.read + 1] - S;
        const uint64_t f = (uint64_t)r.first, l = (uint64_t)r.len;
        // region base i sits at position (f - i) mod L: positions [f - l + 1, f], or [0, f] and the read's last l - f - 1
        uint64_t lo[2], hi[2];
        int pieces = 1;
        if (l <= f + 1) { lo[0] = f + 1 - l; hi[0] = f; }
        else { lo[0] = 0; hi[0] = f; lo[1] = L - (l - f - 1); hi[1] = L - 1; pieces = 2; }
        for (int q = 0; q < pieces; q++) {
            const uint64_t *it = std::lower_bound(amb_base, amb_base + n_amb, S + lo[q]);
            for (; it < amb_base + n_amb && *it <= S + hi[q]; ++it) {
                const uint64_t p = *it - S, i = p <= f ? f - p : f + L - p;
                ExtPatch x;
                x.base = new_off[k] + (reversed ? l - 1 - i : i);
                x.code = amb_rev_code[it - amb_base];
                out.push_back(x);
            }
        }
    }
}

extern "C" int gmg_reads_extract(const gmg_reads *reads, const gmg_gene_region *regions, uint64_t n, int flags, const uint64_t *amb_base,
                                 const uint8_t *amb_rev_code, uint64_t n_amb, gmg_reads **out)
{
    { int rc_enter = gmg_enter("gmg_reads_extract"); if (rc_enter) return rc_enter; }
    if (!reads || (!regions && n) || !out || n >= 0x7ffffffeull || (flags & ~GMG_EXTRACT_REVERSED) || (n_amb && (!amb_base || !amb_rev_code)))
        return gmg_set_error(GMG_EINVAL, "gmg_reads_extract: bad argument");
    for (uint64_t i = 0; i < n_amb; i++)
        if (amb_rev_code[i] > 3 || (i && amb_base[i] <= amb_base[i - 1]))
            return gmg_set_error(GMG_EINVAL, "gmg_reads_extract: exception %llu: the list must ascend and hold codes 0 .. 3", (unsigned long long)i);
    const int reversed = (flags & GMG_EXTRACT_REVERSED) != 0;
    hipStream_t s = 0;
    GmgScratch sc(GmgScratch::STREAM, s);               // (kernels already queued may still use the blocks that go back to the cache)
    gmg_gene_region *d_regions = nullptr;
    ExtMeta *d_meta = nullptr;
    uint64_t *d_len = nullptr, *d_off = nullptr;
    unsigned long long *d_stats = nullptr;
    GMG_HIP(sc.alloc(&d_regions, (n ? n : 1) * sizeof(gmg_gene_region)));
    GMG_HIP(sc.alloc(&d_meta, (n ? n : 1) * sizeof(ExtMeta)));
    GMG_HIP(sc.alloc(&d_len, (n + 1) * 8));
    GMG_HIP(sc.alloc(&d_off, (n + 1) * 8));
    GMG_HIP(sc.alloc(&d_stats, 8 * sizeof(unsigned long long)));
    const unsigned long long stats0[6] = {~0ull, 0, 0, 0, ~0ull, 0};
    unsigned long long stats[6];
    GMG_HIP(hipMemcpyAsync(d_stats, stats0, sizeof stats0, hipMemcpyHostToDevice, s));
    if (n) GMG_HIP(hipMemcpyAsync(d_regions, regions, n * sizeof(gmg_gene_region), hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(k_ext_len, dim3((unsigned)((n + 256) / 256 < 512 ? (n + 256) / 256 : 512)), dim3(256), 0, s, reads->d_off, d_regions, n,
                       reads->n_reads, reversed, d_len, d_meta, d_stats);
    GMG_HIP((gmg_scan_excl<uint64_t, uint64_t>(d_len, d_off, n + 1, s)));
    GMG_HIP(hipMemcpyAsync(&stats[5], d_off + n, 8, hipMemcpyDeviceToHost, s));
    GMG_HIP(hipMemcpyAsync(stats, d_stats, 5 * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
    GMG_HIP(hipStreamSynchronize(s));
    if (stats[4] != ~0ull) {
        const gmg_gene_region &r = regions[stats[4]];
        return gmg_set_error(GMG_ERANGE, "gmg_reads_extract: region %llu (read %u, first %d, len %d, strand %d) does not fit its read (the batch has %llu)",
                             stats[4], r.read, r.first, r.len, r.strand, (unsigned long long)reads->n_reads);
    }
    // the exceptions of the reverse-strand regions (few: the offsets of both batches come to the host only when there is a list)
    std::vector<ExtPatch> patches;
    if (n_amb && n) {
        std::vector<uint64_t> src_off(reads->n_reads + 1), new_off(n + 1);
        GMG_HIP(hipMemcpy(src_off.data(), reads->d_off, src_off.size() * 8, hipMemcpyDeviceToHost));
        new_off[0] = 0;
        for (uint64_t k = 0; k < n; k++) new_off[k + 1] = new_off[k] + (uint64_t)regions[k].len;
        ext_patches(regions, n, reversed, src_off.data(), new_off.data(), amb_base, amb_rev_code, n_amb, patches);
    }
    // the packed words (guards zeroed; the gather writes every data word), the tile table, the gather
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
        const uint64_t blocks = (tmp.n_tiles + 3) / 4;     // one wave per tile
        hipLaunchKernelGGL(k_reads_extract, dim3((unsigned)(blocks < 65536 ? blocks : 65536)), dim3(256), 0, s, reads->d_packed, d_meta, d_off,
                           tmp.d_tile_read, n, total, alloc + GMG_GUARD_WORDS);
        GMG_HIP(hipGetLastError());
        if (!patches.empty()) {
            ExtPatch *d_patch = nullptr;
            GMG_HIP(sc.alloc(&d_patch, patches.size() * sizeof(ExtPatch)));
            GMG_HIP(hipMemcpyAsync(d_patch, patches.data(), patches.size() * sizeof(ExtPatch), hipMemcpyHostToDevice, s));
            hipLaunchKernelGGL(k_ext_patch, dim3((unsigned)((patches.size() + 255) / 256)), dim3(256), 0, s, d_patch, (uint64_t)patches.size(),
                               alloc + GMG_GUARD_WORDS);
            GMG_HIP(hipGetLastError());
        }
    }
    GMG_HIP(hipStreamSynchronize(s));
    gmg_reads_set_lengths(&tmp, stats);
    gmg_reads *r = new (std::nothrow) gmg_reads(tmp);
    if (!r) return gmg_set_error(GMG_ENOMEM, "gmg_reads_extract: out of host memory");
    sc.detach(d_off); sc.detach(alloc); sc.detach(tmp.d_tile_read);
    sc.wait = GmgScratch::NONE;                         // (waited for just now)
    *out = r;
    return GMG_OK;
}
