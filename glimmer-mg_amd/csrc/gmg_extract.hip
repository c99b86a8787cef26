// gmg_extract.hip -- gmg_reads_extract (include/gmg.h): regions of the reads of a batch, any strand, modulo their read, gathered
// into a NEW batch on the device: what `extract` / `multi-extract` print and build-icm parses back, without the text in between
// (src/Util/extract.cc:158-207, Output_Subsequence).  One of the three batch builders of gmg_gather.h: k_ext_len is its length
// kernel, ExtSource its gather's source.
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

#include "gmg_device.h"
#include "gmg_gather.h"
#include "gmg_scan.h"

#include <algorithm>
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

__global__ __launch_bounds__(256) void k_ext_len(const uint64_t *src_off, const gmg_gene_region *regions, uint64_t n, uint64_t n_src, int reversed,
                                                 uint64_t *len, ExtMeta *meta, unsigned long long *stats)
{
    GmgLenStats st;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i <= n; i += (uint64_t)gridDim.x * blockDim.x) {
        uint64_t l = 0;
        if (i < n) {
            const gmg_gene_region r = regions[i];
            ExtMeta m = {0, 0, 0};
            uint64_t b, L;
            if (dev_region_fits(r, src_off, n_src, b, L)) {
                l = (uint64_t)r.len;
                const bool comp = r.strand < 0, down = comp != (reversed != 0);
                int64_t p0 = r.first;
                if (reversed && l) p0 += comp ? -(int64_t)(l - 1) : (int64_t)(l - 1);
                if (p0 < 0) p0 += (int64_t)L;
                if (p0 >= (int64_t)L) p0 -= (int64_t)L;
                m.src = b;
                m.len = (uint32_t)L | (comp ? EXT_FLAG : 0u);
                m.p0 = (uint32_t)p0 | (down ? EXT_FLAG : 0u);
            } else st.bad_item(i);
            meta[i] = m;
            st.length(l);
        }
        len[i] = l;                                     // len[n] = 0: the scan's last output is the total
    }
    st.finish(stats);
}

// a string is a walk round its read: a piece also ends where the string wraps around the read
struct ExtSource {
    static constexpr uint32_t R = 32;
    struct Item { uint64_t beg; ExtMeta m; };           // the string's base 0 in the new batch
    const uint32_t *__restrict__ src;
    const ExtMeta *__restrict__ meta;
    __device__ __forceinline__ Item stage(uint64_t r, uint64_t beg) const { return Item{beg, meta[r]}; }
    __device__ __forceinline__ uint32_t piece(const Item &it, uint64_t pos, unsigned &nb) const
    {
        const uint32_t L = it.m.len & ~EXT_FLAG, p0 = it.m.p0 & ~EXT_FLAG;
        const bool comp = (it.m.len & EXT_FLAG) != 0, down = (it.m.p0 & EXT_FLAG) != 0;
        const uint32_t j = (uint32_t)(pos - it.beg);                // base j of the string: j < its length <= L
        uint32_t p, room;                                           // its position in the read; bases up to the wrap
        if (!down) { p = p0 + j; if (p >= L) p -= L; room = L - p; }
        else { p = p0 >= j ? p0 - j : p0 + L - j; room = p + 1; }
        nb = nb < room ? nb : room;
        return ext_piece(src, it.m.src, p, down, comp, nb);
    }
};

__global__ __launch_bounds__(256) void k_reads_extract(const uint32_t *__restrict__ src, const ExtMeta *__restrict__ meta,
                                                       const uint64_t *__restrict__ new_off, const uint32_t *__restrict__ tile_read, uint64_t n,
                                                       uint64_t total, uint32_t *__restrict__ dst)
{
    gmg_gather_tiles(ExtSource{src, meta}, new_off, tile_read, n, total, dst);
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
    GmgBatchBuilder b(sc, s);
    gmg_gene_region *d_regions = nullptr;
    ExtMeta *d_meta = nullptr;
    uint64_t *d_len = nullptr, *d_off = nullptr;
    GMG_HIP(sc.alloc(&d_regions, (n ? n : 1) * sizeof(gmg_gene_region)));
    GMG_HIP(sc.alloc(&d_meta, (n ? n : 1) * sizeof(ExtMeta)));
    GMG_HIP(sc.alloc(&d_len, (n + 1) * 8));
    GMG_HIP(sc.alloc(&d_off, (n + 1) * 8));
    { const int rc = b.begin(); if (rc) return rc; }
    if (n) GMG_HIP(hipMemcpyAsync(d_regions, regions, n * sizeof(gmg_gene_region), hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(k_ext_len, dim3(gmg_grid(n + 1, 256, 512)), dim3(256), 0, s, reads->d_off, d_regions, n, reads->n_reads, reversed, d_len,
                       d_meta, b.d_stats);
    GMG_HIP((gmg_scan_excl<uint64_t, uint64_t>(d_len, d_off, n + 1, s)));
    { const int rc = b.lengths(d_off + n); if (rc) return rc; }
    if (b.stats[4] != ~0ull) {
        const gmg_gene_region &r = regions[b.stats[4]];
        return gmg_set_error(GMG_ERANGE, "gmg_reads_extract: region %llu (read %u, first %d, len %d, strand %d) does not fit its read (the batch has %llu)",
                             b.stats[4], r.read, r.first, r.len, r.strand, (unsigned long long)reads->n_reads);
    }
    // the exceptions of the reverse-strand regions (few: the offsets of both batches come to the host only when there is a list)
    std::vector<ExtPatch> patches;
    if (n_amb && n) {
        std::vector<uint64_t> src_off(reads->n_reads + 1), new_off(n + 1);
        GMG_HIP(gmg_copy_wait(src_off.data(), reads->d_off, src_off.size() * 8, hipMemcpyDeviceToHost, s));
        new_off[0] = 0;
        for (uint64_t k = 0; k < n; k++) new_off[k + 1] = new_off[k] + (uint64_t)regions[k].len;
        ext_patches(regions, n, reversed, src_off.data(), new_off.data(), amb_base, amb_rev_code, n_amb, patches);
    }
    { const int rc = b.layout(n, d_off); if (rc) return rc; }
    if (b.data_words) {
        hipLaunchKernelGGL(k_reads_extract, dim3(b.gather_grid()), dim3(256), 0, s, reads->d_packed, d_meta, d_off, b.tmp.d_tile_read, n, b.total,
                           b.d_words);
        GMG_HIP(hipGetLastError());
        if (!patches.empty()) {
            ExtPatch *d_patch = nullptr;
            GMG_HIP(sc.alloc(&d_patch, patches.size() * sizeof(ExtPatch)));
            GMG_HIP(hipMemcpyAsync(d_patch, patches.data(), patches.size() * sizeof(ExtPatch), hipMemcpyHostToDevice, s));
            hipLaunchKernelGGL(k_ext_patch, dim3((unsigned)((patches.size() + 255) / 256)), dim3(256), 0, s, d_patch, (uint64_t)patches.size(),
                               b.d_words);
        }
    }
    return b.finish("gmg_reads_extract", out);
}
