// gmg_audit.hip -- gmg_genes_audit (include/gmg.h): what anomaly (src/Glimmer/anomaly.cc:76-240) and start-codon-distrib
// (src/Util/start-codon-distrib.cc:84-106) look at in every gene of a coordinate list -- the first and the last codon, every
// in-frame stop codon, the last stop in the frame of the gene's end and, for a gene without a stop codon, the next one round the
// sequence -- for a batch of regions in one call.  Everything it produces is an integer.
//
// A wave per region, as k_entropy (gmg_entropy.hip): a step covers 64 codons, one per lane; the lane reads its three bases from
// the packed read (positions modulo the read's length, the reverse strand downwards and complemented) and tests the codon index
// 16*b0 + 4*b1 + b2 against a 64-bit mask of the stop codons; the wave's ballot of the hits gives their number (population
// count), the first (ffs) and the last one (clz), and in the write pass every hit's place in the list (the population count of the
// ballot's bits below the lane).
//
// The list of offsets has no bound a region at a time short of len / 3 entries, and genes have none at all: count pass -> scan ->
// write pass.  The count pass fills the whole record and the histogram of first codons; the write pass walks only
// the regions that have an inner stop a second time.
//
// Letters outside acgtACGT: the caller's ascending list of their job-wide indices.  The wave finds the part of the list that
// lies in its region's read once (two 64-ary searches, a probe per lane); an empty part -- nearly every read -- costs nothing
// further, otherwise a lane looks each of its three bases up in that part.

#include "gmg_internal.h"

#include "gmg_device.h"
#include "gmg_scan.h"

#include <string.h>
#include <new>
#include <vector>

#define AU_BLOCK 256             // four waves, a region each
#define AU_WAVES (AU_BLOCK / 64)
#define AU_GRID_CAP (256 * 32)   // 8 work-groups of four waves per CU, 4 rounds; the rest loops
#define AU_BINS 65               // the 64 codons, then the regions without a first codon

struct AuditArgs {
    uint64_t start_mask, stop_mask;      // bit c: codon index c is in the list
    int8_t which[128];                   // [c]: index of codon c in the start list, [64 + c]: in the stop list; -1 none
    int next_stop;                       // GMG_AUDIT_NEXT_STOP
};

struct GMG_HIDDEN gmg_audit {
    gmg_gene_audit *d_rec = nullptr;
    int32_t *d_inner = nullptr;
    unsigned long long *d_hist = nullptr;        // AU_BINS
    uint64_t n = 0, n_inner = 0;
    hipStream_t s;
    GmgScratch own;                      // the blocks are free once what is queued on s when the handle goes has run
    explicit gmg_audit(hipStream_t stream) : s(stream), own(GmgScratch::AFTER, stream) {}
};

// stats of a call: [0] first bad region
struct AuRegion {
    DevRegion v;
    const uint64_t *amb;
    uint64_t amb_lo, amb_hi;             // the read's part of the list
};

__device__ __forceinline__ bool au_listed(const uint64_t *__restrict__ amb, uint64_t lo, uint64_t hi, uint64_t g)
{
    const uint64_t l = dev_lower_bound(amb, lo, hi, g);
    return l < hi && amb[l] == g;
}

// codon index of region offsets r, r + 1, r + 2 (0 <= r < n; the three bases wrap one by one), -1 with a listed base
__device__ __forceinline__ int au_codon(const AuRegion &R, int64_t r)
{
    bool listed = false;
    const int idx = R.v.codon(r, [&](uint64_t g) {
        if (R.amb_hi > R.amb_lo) listed |= au_listed(R.amb, R.amb_lo, R.amb_hi, g);
    });
    return listed ? -1 : idx;
}

// the region's read and its part of the list; false: the region does not fit (nothing of it may be read)
__device__ __forceinline__ bool au_region(const gmg_gene_region &r, const uint32_t *packed, const uint64_t *__restrict__ off, uint64_t n_reads,
                                          const uint64_t *__restrict__ amb, uint64_t n_amb, int lane, AuRegion &R)
{
    uint64_t base, L;
    if (!(dev_region_fits(r, off, n_reads, base, L) && L < 0x80000000ull)) return false;
    R.v.packed = packed;
    R.v.base = base;
    R.v.n = (int64_t)L;
    R.v.first = r.first;
    R.v.fwd = r.strand > 0;
    R.amb = amb;
    R.amb_lo = R.amb_hi = 0;
    if (n_amb) {
        R.amb_lo = dev_wave_lower_bound(amb, n_amb, base, lane);
        R.amb_hi = dev_wave_lower_bound(amb, n_amb, base + L, lane);
    }
    return true;
}

// the inner codons: region offsets 3c, c < n_in = the i = 0, 3, ... with i < len - 3 (anomaly.cc:190, 224)
__device__ __forceinline__ int64_t au_n_inner_codons(int32_t len) { return len > 3 ? (int64_t)(len - 1) / 3 : 0; }

__global__ __launch_bounds__(AU_BLOCK) void k_audit_count(AuditArgs a, const uint32_t *__restrict__ packed, const uint64_t *__restrict__ off,
                                                          uint64_t n_reads, const gmg_gene_region *__restrict__ regions, uint64_t n_regions,
                                                          const uint64_t *__restrict__ amb, uint64_t n_amb, gmg_gene_audit *__restrict__ rec,
                                                          uint32_t *__restrict__ cnt, unsigned long long *__restrict__ hist,
                                                          unsigned long long *__restrict__ stats)
{
    __shared__ unsigned s_hist[AU_BINS];
    __shared__ int8_t s_which[128];
    if (threadIdx.x < AU_BINS) s_hist[threadIdx.x] = 0;
    if (threadIdx.x < 128) s_which[threadIdx.x] = a.which[threadIdx.x];
    if (blockIdx.x == 0 && threadIdx.x == 0) cnt[n_regions] = 0;        // (the scan's last output is the total)
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const uint64_t wave0 = (uint64_t)blockIdx.x * AU_WAVES + (threadIdx.x >> 6);
    const uint64_t stride = (uint64_t)gridDim.x * AU_WAVES;
    for (uint64_t k = wave0; k < n_regions; k += stride) {              // (k is the same in every lane of the wave)
        const gmg_gene_region r = regions[k];
        AuRegion R;
        if (!au_region(r, packed, off, n_reads, amb, n_amb, lane, R)) {
            if (lane == 0) { atomicMin(&stats[0], (unsigned long long)k); cnt[k] = 0; }
            continue;
        }
        const int32_t len = r.len;
        // the first and the last codon: lanes 0 and 1
        int c01 = -1;
        if (len >= 3 && lane < 2) c01 = au_codon(R, lane ? (int64_t)len - 3 : 0);
        const int first_codon = __builtin_amdgcn_readlane(c01, 0), last_codon = __builtin_amdgcn_readlane(c01, 1);
        const int start_which = first_codon >= 0 ? s_which[first_codon] : -1;
        const int stop_which = last_codon >= 0 ? s_which[64 + last_codon] : -1;
        // the inner stops: their number and the last one
        const int64_t n_in = au_n_inner_codons(len);
        int n_inner = 0;
        int64_t last_hit = -1;
        for (int64_t c0 = 0; c0 < n_in; c0 += 64) {
            const int64_t c = c0 + lane;
            bool hit = false;
            if (c < n_in) {
                const int code = au_codon(R, 3 * c);
                hit = code >= 0 && ((a.stop_mask >> code) & 1ull);
            }
            const unsigned long long m = __ballot(hit);
            if (m) {
                n_inner += __popcll(m);
                last_hit = 3 * (c0 + 63 - __clzll((long long)m));
            }
        }
        // the last stop among len - 6, len - 9, ...: the inner codons again when len is a multiple of 3, the other frame otherwise --
        // from the top, up to the first step with a hit
        int64_t back = -1;
        if (len % 3 == 0) back = last_hit;
        else if (len >= 6) {
            const int64_t nb = ((int64_t)len - 6) / 3 + 1;
            for (int64_t m0 = 0; m0 < nb; m0 += 64) {
                const int64_t m = m0 + lane;
                bool hit = false;
                if (m < nb) {
                    const int code = au_codon(R, (int64_t)len - 6 - 3 * m);
                    hit = code >= 0 && ((a.stop_mask >> code) & 1ull);
                }
                const unsigned long long mask = __ballot(hit);
                if (mask) { back = (int64_t)len - 6 - 3 * (m0 + __ffsll((unsigned long long)mask) - 1); break; }
            }
        }
        // a gene that ends in no stop codon: on round the read, up to the first step with a hit (anomaly.cc:157-176)
        int64_t next = -1;
        if (a.next_stop && stop_which < 0) {
            for (int64_t j0 = len; j0 < R.v.n; j0 += 3 * 64) {
                const int64_t j = j0 + 3 * lane;
                bool hit = false;
                if (j < R.v.n) {
                    const int code = au_codon(R, j);
                    hit = code >= 0 && ((a.stop_mask >> code) & 1ull);
                }
                const unsigned long long mask = __ballot(hit);
                if (mask) { next = j0 + 3 * (__ffsll((unsigned long long)mask) - 1); break; }
            }
        }
        // the record: eight 32-bit fields, a lane each (inner_begin is the write pass's, or 0 when no region has an inner stop)
        const int32_t v = lane == 0 ? first_codon : lane == 1 ? last_codon : lane == 2 ? start_which : lane == 3 ? stop_which :
                          lane == 4 ? n_inner : lane == 5 ? 0 : lane == 6 ? (int32_t)back : (int32_t)next;
        if (lane < 8) ((int32_t *)(void *)&rec[k])[lane] = v;
        if (lane == 0) {
            cnt[k] = (uint32_t)n_inner;
            atomicAdd(&s_hist[first_codon < 0 ? 64 : first_codon], 1u);
        }
    }
    __syncthreads();
    if (threadIdx.x < AU_BINS && s_hist[threadIdx.x]) atomicAdd(&hist[threadIdx.x], (unsigned long long)s_hist[threadIdx.x]);
}

// the offsets of the inner stops of every region that has one, ascending, at inner[inner_off[k] ..); inner_begin of every record
__global__ __launch_bounds__(AU_BLOCK) void k_audit_write(AuditArgs a, const uint32_t *__restrict__ packed, const uint64_t *__restrict__ off,
                                                          uint64_t n_reads, const gmg_gene_region *__restrict__ regions, uint64_t n_regions,
                                                          const uint64_t *__restrict__ amb, uint64_t n_amb, gmg_gene_audit *__restrict__ rec,
                                                          const uint64_t *__restrict__ inner_off, uint64_t total, int32_t *__restrict__ inner)
{
    const int lane = threadIdx.x & 63;
    const uint64_t wave0 = (uint64_t)blockIdx.x * AU_WAVES + (threadIdx.x >> 6);
    const uint64_t stride = (uint64_t)gridDim.x * AU_WAVES;
    for (uint64_t k = wave0; k < n_regions; k += stride) {
        const uint64_t beg = inner_off[k], end = inner_off[k + 1];
        if (lane == 0) rec[k].inner_begin = (uint32_t)beg;
        if (end == beg) continue;
        const gmg_gene_region r = regions[k];
        AuRegion R;
        if (!au_region(r, packed, off, n_reads, amb, n_amb, lane, R)) continue;
        const int64_t n_in = au_n_inner_codons(r.len);
        uint64_t at = beg;
        for (int64_t c0 = 0; c0 < n_in && at < end; c0 += 64) {
            const int64_t c = c0 + lane;
            bool hit = false;
            if (c < n_in) {
                const int code = au_codon(R, 3 * c);
                hit = code >= 0 && ((a.stop_mask >> code) & 1ull);
            }
            const unsigned long long m = __ballot(hit);
            const uint64_t slot = at + (uint64_t)__popcll(m & ((1ull << lane) - 1ull));
            if (hit && slot < end && slot < total) inner[slot] = (int32_t)(3 * c);
            at += (uint64_t)__popcll(m);
        }
    }
}

// codon index of three lower-case letters of acgt, -1 for anything else
static int au_pattern(const char c[4])
{
    int idx = 0;
    for (int t = 0; t < 3; t++) {
        const char *p = c[t] ? strchr("acgt", c[t]) : nullptr;
        if (!p) return -1;
        idx = 4 * idx + (int)(p - "acgt");
    }
    return c[3] == '\0' ? idx : -1;
}

static int au_args(const gmg_audit_params *p, AuditArgs *a)
{
    memset(a, 0, sizeof *a);
    memset(a->which, -1, sizeof a->which);
    if (p->n_start_codons < 0 || p->n_start_codons > 8 || p->n_stop_codons < 0 || p->n_stop_codons > 8 || (p->flags & ~GMG_AUDIT_NEXT_STOP))
        return gmg_set_error(GMG_EINVAL, "gmg_genes_audit: 0 .. 8 start codons, 0 .. 8 stop codons, flags GMG_AUDIT_NEXT_STOP or 0");
    for (int side = 0; side < 2; side++) {
        const int cnt = side ? p->n_stop_codons : p->n_start_codons;
        for (int i = 0; i < cnt; i++) {
            const char *c = side ? p->stop_codon[i] : p->start_codon[i];
            const int idx = au_pattern(c);
            if (idx < 0)
                return gmg_set_error(GMG_EINVAL, "gmg_genes_audit: %s codon %d is not three lower-case letters of acgt", side ? "stop" : "start", i);
            if (a->which[64 * side + idx] < 0) a->which[64 * side + idx] = (int8_t)i;      // (the first of equal patterns, as the reference's loop)
            (side ? a->stop_mask : a->start_mask) |= 1ull << idx;
        }
    }
    a->next_stop = (p->flags & GMG_AUDIT_NEXT_STOP) != 0;
    return GMG_OK;
}

extern "C" int gmg_genes_audit(const gmg_reads *reads, const gmg_gene_region *regions, uint64_t n, const gmg_audit_params *params,
                               const uint64_t *amb_base, uint64_t n_amb, gmg_audit **out, void *stream)
{
    { int rc_enter = gmg_enter("gmg_genes_audit"); if (rc_enter) return rc_enter; }
    if (!reads || (!regions && n) || !params || !out || (n_amb && !amb_base) || n >= 0x7ffffffeull)
        return gmg_set_error(GMG_EINVAL, "gmg_genes_audit: bad argument");
    AuditArgs a;
    { const int rc = au_args(params, &a); if (rc) return rc; }
    for (uint64_t i = 0; i < n_amb; i++)
        if (amb_base[i] >= reads->total_bases || (i && amb_base[i] <= amb_base[i - 1]))
            return gmg_set_error(GMG_EINVAL, "gmg_genes_audit: ambiguous base %llu: the list must ascend inside the batch", (unsigned long long)i);
    hipStream_t s = (hipStream_t)stream;
    GmgScratch sc(GmgScratch::AFTER, s);
    gmg_gene_audit *d_rec = nullptr;
    unsigned long long *d_hist = nullptr;
    int32_t *d_inner = nullptr;
    GMG_HIP(sc.alloc(&d_rec, (n ? n : 1) * sizeof(gmg_gene_audit)));
    GMG_HIP(sc.alloc(&d_hist, AU_BINS * sizeof(unsigned long long)));
    GMG_HIP(hipMemsetAsync(d_hist, 0, AU_BINS * sizeof(unsigned long long), s));
    uint64_t total = 0;
    if (n) {
        gmg_gene_region *d_regions = nullptr;
        uint64_t *d_amb = nullptr, *d_off = nullptr;
        uint32_t *d_cnt = nullptr;
        unsigned long long *d_stats = nullptr;
        GMG_HIP(sc.alloc(&d_regions, n * sizeof(gmg_gene_region)));
        GMG_HIP(sc.alloc(&d_cnt, (n + 1) * 4));
        GMG_HIP(sc.alloc(&d_off, (n + 1) * 8));
        GMG_HIP(sc.alloc(&d_stats, 8));
        if (n_amb) {
            GMG_HIP(sc.alloc(&d_amb, n_amb * 8));
            GMG_HIP(hipMemcpyAsync(d_amb, amb_base, n_amb * 8, hipMemcpyHostToDevice, s));
        }
        GMG_HIP(hipMemsetAsync(d_stats, 0xff, 8, s));
        GMG_HIP(hipMemcpyAsync(d_regions, regions, n * sizeof(gmg_gene_region), hipMemcpyHostToDevice, s));
        hipLaunchKernelGGL(k_audit_count, dim3(gmg_grid(n, AU_WAVES, AU_GRID_CAP)), dim3(AU_BLOCK), 0, s, a, reads->d_packed, reads->d_off, reads->n_reads, d_regions, n,
                           d_amb, n_amb, d_rec, d_cnt, d_hist, d_stats);
        GMG_HIP(hipGetLastError());
        GMG_HIP((gmg_scan_excl<uint32_t, uint64_t>(d_cnt, d_off, n + 1, s)));
        unsigned long long bad = ~0ull;
        GMG_HIP(hipMemcpyAsync(&total, d_off + n, 8, hipMemcpyDeviceToHost, s));
        GMG_HIP(hipMemcpyAsync(&bad, d_stats, 8, hipMemcpyDeviceToHost, s));
        GMG_HIP(hipStreamSynchronize(s));
        if (bad != ~0ull) {
            const gmg_gene_region &r = regions[bad];
            return gmg_set_error(GMG_ERANGE, "gmg_genes_audit: region %llu (read %u, first %d, len %d, strand %d) does not fit its read (the batch has %llu)",
                                 bad, r.read, r.first, r.len, r.strand, (unsigned long long)reads->n_reads);
        }
        if (total > (uint64_t)gmg_opt(GMG_OPT_MG_MAX_ENTRIES))
            return gmg_set_error(GMG_ETOOBIG, "gmg_genes_audit: %llu inner stop codons, more than mg_max_entries = %lld: audit the regions in smaller batches",
                                 (unsigned long long)total, gmg_opt(GMG_OPT_MG_MAX_ENTRIES));
        if (total) {
            GMG_HIP(sc.alloc(&d_inner, total * 4));
            hipLaunchKernelGGL(k_audit_write, dim3(gmg_grid(n, AU_WAVES, AU_GRID_CAP)), dim3(AU_BLOCK), 0, s, a, reads->d_packed, reads->d_off, reads->n_reads, d_regions, n,
                               d_amb, n_amb, d_rec, d_off, total, d_inner);
            GMG_HIP(hipGetLastError());
        }
    }
    gmg_audit *res = new (std::nothrow) gmg_audit(s);
    if (!res) return gmg_set_error(GMG_ENOMEM, "gmg_genes_audit: out of host memory");
    res->d_rec = res->own.take(sc, d_rec);
    res->d_inner = res->own.take(sc, d_inner);
    res->d_hist = res->own.take(sc, d_hist);
    res->n = n;
    res->n_inner = total;
    *out = res;
    return GMG_OK;
}

extern "C" int gmg_audit_info(const gmg_audit *a, uint64_t *n_regions, uint64_t *n_inner)
{
    if (!a) return gmg_set_error(GMG_EINVAL, "gmg_audit_info: NULL handle");
    if (n_regions) *n_regions = a->n;
    if (n_inner) *n_inner = a->n_inner;
    return GMG_OK;
}

extern "C" int gmg_audit_fetch(const gmg_audit *a, gmg_gene_audit *records, int32_t *inner, int64_t first_codon_hist[65])
{
    if (!a) return gmg_set_error(GMG_EINVAL, "gmg_audit_fetch: NULL handle");
    { int rc_enter = gmg_enter("gmg_audit_fetch"); if (rc_enter) return rc_enter; }
    if (records && a->n) GMG_HIP(hipMemcpyAsync(records, a->d_rec, a->n * sizeof(gmg_gene_audit), hipMemcpyDeviceToHost, a->s));
    if (inner && a->n_inner) GMG_HIP(hipMemcpyAsync(inner, a->d_inner, a->n_inner * 4, hipMemcpyDeviceToHost, a->s));
    if (first_codon_hist) GMG_HIP(hipMemcpyAsync(first_codon_hist, a->d_hist, AU_BINS * 8, hipMemcpyDeviceToHost, a->s));
    GMG_HIP(hipStreamSynchronize(a->s));
    return GMG_OK;
}

extern "C" int gmg_audit_free(gmg_audit *a)
{
    if (!a) return GMG_OK;
    delete a;
    return GMG_OK;
}
