// gmg_features.hip -- gmg_features_count (include/gmg.h): the counting of the reference's scripts/train_features.py
// (`--predict P --seq S`), which retrains the length, start-codon and adjacency distributions between two runs of the pipeline.
//
// The gene side (parse_genes, train_features.py:223-280) needs one codon per gene from the sequence -- k_feat_gene_starts -- and
// is integer arithmetic on the gene list otherwise, done where the list is: on the host.
//
// The non-gene side (forward_parse_nongenes, :320-467, once on every sequence and once on its reverse complement) is the work
// that grows with the bases.  Its work items are the stop codons of all three frames plus the three pseudo-stops L, L + 1, L + 2
// of every sequence that has a gene; an item walks its frame downwards codon by codon to the previous stop, and every start codon
// it meets (and the pseudo-start in front of the sequence) counts once in the length histogram and, when long enough, adds
// 1.0 / num_starts to the orientation and distance bins of the genes on either side.
//
//   k_feat_opaque        one bit per base that is no upper-case ACGT, from the caller's index list: a codon with such a base is
//                        neither start nor stop, on either strand (the script's rc() leaves the letter as it is)
//   k_feat_mark          four bits per base position i, from one pass over the packed words: the codon at i is a stop / a start,
//                        its reverse complement is a stop / a start.  The second pass reads the same table through
//                        i = L - 3 - j: no reverse-complement copy of anything exists.
//   k_feat_items<WRITE>  a lane per UNIT of 32 consecutive slots of one (pass, sequence): slot s <= L - 3 is an item when the
//                        codon there is a stop, slots L .. L + 2 always are.  Units are numbered pass by pass, sequence by
//                        sequence, so unit order followed by slot order is the reference's order of the stops -- a 1.67 Mbp genome
//                        is 52 k units per pass, spread over the device like a batch of reads.  The count pass adds up the integer
//                        histograms (LDS-privatised: integer atomics do not depend on order) and leaves the number of records
//                        per unit; an exclusive scan turns that into offsets; the write pass puts the (bin key, num_starts)
//                        records where the reference would have produced them: starts downwards, preceding gene before
//                        succeeding gene.
//   the fractional bins  every bin is one accumulator that takes its 1.0 / num_starts terms in the reference's order, so a bin's
//                        value is the SEQUENTIAL double sum of its records: a stable radix sort (hipcub) by key keeps the records
//                        of a bin in their order, k_feat_heads / k_feat_head_pos find where the bins begin, and k_feat_sum adds
//                        one bin per wave: 64 coalesced values at a time through LDS, added one after the other.  No atomics on
//                        doubles, no tree.  The four orientation bins are the same thing with the two orientation bits as key.
//
// The preceding / succeeding gene of an item (:345-356) is the first gene whose end - 3 reaches the stop, looking at the genes in
// file order and never going back: a binary search over the PREFIX MAXIMUM of the ends (nested genes and genes out of order make
// the ends themselves non-monotone).  For the mirrored list of the second pass that is L minus the suffix minimum of the starts.

#include "gmg_internal.h"

#include "gmg_scan.h"

#include <hipcub/hipcub.hpp>

#include <string.h>
#include <algorithm>
#include <chrono>
#include <new>
#include <vector>

struct FeatGene {
    int32_t start, end, strand;  // 0-based half-open, clipped to the sequence
    int32_t pmax_end;            // max end of this gene and the ones before it in its sequence
    int32_t smin_start;          // min start of this gene and the ones behind it
    uint32_t group;              // its sequence: index into the groups
};

struct FeatGroup {               // one sequence that has genes
    uint64_t S;                  // job-wide index of its base 0
    int32_t L;
    uint32_t gene_begin, n_genes;
    uint32_t reserved;
};

#define FEAT_UNIT 32             // slots per lane
#define FEAT_LDS_BINS 2048       // length bins counted in LDS; longer ORFs go to HBM one by one

struct FeatArgs {
    const uint32_t *cls;         // 4 bits per base position (k_feat_mark)
    const uint32_t *packed;
    const FeatGroup *groups;
    const FeatGene *genes;
    const uint64_t *unit_off;    // [2 * n_groups + 1]: first unit of (pass, group)
    uint32_t n_groups;
    uint64_t n_units;
    int32_t min_length, max_overlap;
    uint64_t *unit_cnt;          // count pass: records of every unit ([n_units + 1], the last one 0)
    const uint64_t *rec_off;     // write pass
    uint64_t *keys;
    uint32_t *vals;
    unsigned long long *len_hist;        // [n_len_bins]
    unsigned long long *starts;          // [3] ATG GTG TTG
};

__global__ __launch_bounds__(256) void k_feat_opaque(const uint64_t *__restrict__ base, uint64_t n, uint64_t total, uint32_t *opq)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint64_t b = base[i];
    if (b < total) atomicOr(&opq[b >> 5], 1u << (unsigned)(b & 31));
}

// begin and end of the reads that have genes
__global__ __launch_bounds__(256) void k_feat_group_extent(const uint64_t *__restrict__ off, const uint32_t *__restrict__ group_read, uint32_t n,
                                                           uint64_t *__restrict__ ext)
{
    const uint32_t q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= n) return;
    const uint32_t r = group_read[q];
    ext[2 * q] = off[r];
    ext[2 * q + 1] = off[(uint64_t)r + 1];
}

// m_*: bit v set when the codon of packed value v = b0 | b1 << 2 | b2 << 4 is in the set.  A lane makes the word of 8 positions.
__global__ __launch_bounds__(256) void k_feat_mark(const uint32_t *__restrict__ packed, const uint32_t *__restrict__ opq, uint64_t total,
                                                   uint64_t m_fstop, uint64_t m_fstart, uint64_t m_rstop, uint64_t m_rstart, uint32_t *__restrict__ cls)
{
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t g = t * 8;
    if (g >= total) return;
    const uint64_t w = g >> 4, o = g >> 5;
    const uint64_t win = ((uint64_t)packed[w] | ((uint64_t)packed[w + 1] << 32)) >> (2u * (unsigned)(g & 15));
    const uint64_t ow = ((uint64_t)opq[o] | ((uint64_t)opq[o + 1] << 32)) >> (unsigned)(g & 31);
    uint32_t out = 0;
#pragma unroll
    for (int k = 0; k < 8; k++) {
        const unsigned v = (unsigned)(win >> (2 * k)) & 63u;
        if ((ow >> k) & 7u) continue;
        const uint32_t nib = (uint32_t)((m_fstop >> v) & 1u) | ((uint32_t)((m_fstart >> v) & 1u) << 1) | ((uint32_t)((m_rstop >> v) & 1u) << 2) |
                             ((uint32_t)((m_rstart >> v) & 1u) << 3);
        out |= nib << (4 * k);
    }
    cls[t] = out;
}

// bit 0: stop, bit 1: start -- of the codon at position c (c >= 0) of the sequence (pass 0) or of its reverse complement (pass 1)
__device__ __forceinline__ uint32_t feat_codon(const uint32_t *__restrict__ cls, uint64_t S, int32_t L, int pass, int32_t c)
{
    if (c + 3 > L) return 0;
    const uint64_t g = S + (uint64_t)(pass ? L - 3 - c : c);
    const uint32_t nib = (cls[g >> 3] >> (4u * (unsigned)(g & 7))) & 15u;
    return pass ? nib >> 2 : nib & 3u;
}

// which of ATG GTG TTG the start codon at c is: its first letter
__device__ __forceinline__ int feat_which(const uint32_t *__restrict__ packed, uint64_t S, int32_t L, int pass, int32_t c)
{
    const uint64_t g = S + (uint64_t)(pass ? L - 1 - c : c);
    uint32_t b = (packed[g >> 4] >> (2u * (unsigned)(g & 15))) & 3u;
    if (pass) b ^= 3u;
    return b == 0 ? 0 : b == 2 ? 1 : 2;
}

struct FeatView {                // gene k of a sequence as the pass sees it
    const FeatGene *g;
    int32_t n, L;
    int pass;
    __device__ __forceinline__ int32_t reach(int32_t k) const { return pass ? L - g[n - 1 - k].smin_start : g[k].pmax_end; }
    __device__ __forceinline__ void get(int32_t k, int32_t &start, int32_t &end, int32_t &strand) const
    {
        if (!pass) { start = g[k].start; end = g[k].end; strand = g[k].strand; }
        else { const FeatGene x = g[n - 1 - k]; start = L - x.end; end = L - x.start; strand = -x.strand; }
    }
};

__device__ __forceinline__ uint64_t feat_key(int s1, int s2, int32_t dist, int32_t max_overlap)
{
    const uint64_t o = (uint64_t)((s1 > 0 ? 0 : 2) + (s2 > 0 ? 0 : 1));
    return (o << 32) | (uint64_t)(uint32_t)(dist + max_overlap);
}

template <bool WRITE>
__global__ __launch_bounds__(256) void k_feat_items(const FeatArgs a)
{
    __shared__ uint32_t s_hist[WRITE ? 1 : FEAT_LDS_BINS];
    __shared__ uint32_t s_starts[3];
    if (!WRITE) {
        for (uint32_t i = threadIdx.x; i < FEAT_LDS_BINS; i += blockDim.x) s_hist[i] = 0;
        if (threadIdx.x < 3) s_starts[threadIdx.x] = 0;
        __syncthreads();
    }
    const uint64_t u = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (u < a.n_units) {
        // the (pass, sequence) of the unit: the last entry of unit_off that does not exceed u
        uint32_t lo = 0, hi = 2 * a.n_groups;           // unit_off[lo] <= u < unit_off[hi]
        while (hi - lo > 1) {
            const uint32_t mid = lo + (hi - lo) / 2;
            if (a.unit_off[mid] <= u) lo = mid; else hi = mid;
        }
        const int pass = lo >= a.n_groups;
        const FeatGroup grp = a.groups[pass ? lo - a.n_groups : lo];
        const int32_t L = grp.L;
        FeatView view;
        view.g = a.genes + grp.gene_begin;
        view.n = (int32_t)grp.n_genes;
        view.L = L;
        view.pass = pass;
        const int32_t s0 = (int32_t)((u - a.unit_off[lo]) * FEAT_UNIT);
        const int32_t s1 = s0 + FEAT_UNIT - 1 < L + 2 ? s0 + FEAT_UNIT - 1 : L + 2;
        uint64_t n_rec = 0, at = WRITE ? a.rec_off[u] : 0;
        for (int32_t si = s0; si <= s1; si++) {
            if (si < L && !(feat_codon(a.cls, grp.S, L, pass, si) & 1u)) continue;
            // the first gene whose end - 3 reaches the stop, genes taken in order: the succeeding gene; the one before it precedes
            int32_t p = 0, q = view.n;
            while (p < q) {
                const int32_t mid = p + (q - p) / 2;
                if (view.reach(mid) - 3 >= si) q = mid; else p = mid + 1;
            }
            const bool has_suc = p < view.n, has_pre = p > 0;
            int32_t ss = 0, se = 0, sstr = 0, ps = 0, pe = 0, pstr = 0;
            if (has_suc) {
                view.get(p, ss, se, sstr);
                if (se - 3 == si || si - ss + 3 > a.max_overlap) continue;
            }
            if (has_pre) view.get(p - 1, ps, pe, pstr);
            uint32_t ns = 0;
            for (int32_t ci = si - 3;; ci -= 3) {
                const bool pseudo = ci < 0;
                if (!pseudo) {
                    const uint32_t c = feat_codon(a.cls, grp.S, L, pass, ci);
                    if (c & 1u) break;
                    if (!(c & 2u)) continue;
                }
                if (has_pre && pe - ci > a.max_overlap) break;
                const int32_t len = (si - ci) / 3;
                const bool counts = 3 * (int64_t)len >= a.min_length;
                ns += counts;
                if (!WRITE) {
                    if (len < FEAT_LDS_BINS) atomicAdd(&s_hist[len], 1u);
                    else atomicAdd(&a.len_hist[len], 1ull);
                    if (counts && !pseudo) atomicAdd(&s_starts[feat_which(a.packed, grp.S, L, pass, ci)], 1u);
                }
                if (pseudo) break;
            }
            n_rec += (uint64_t)ns * ((has_pre ? 1u : 0u) + (has_suc ? 1u : 0u));
            if (WRITE && ns && (has_pre || has_suc)) {
                // (:442-467; in the second pass pstr / sstr are the mirrored strands, which the script turns back)
                const uint64_t kpre = has_pre ? (pass ? feat_key(-1, -pstr, 0, 0) : feat_key(pstr, 1, 0, 0)) : 0;
                const uint64_t ksuc = has_suc ? (pass ? feat_key(-sstr, -1, ss - (si + 3), a.max_overlap) : feat_key(1, sstr, ss - (si + 3), a.max_overlap)) : 0;
                for (int32_t ci = si - 3;; ci -= 3) {
                    const bool pseudo = ci < 0;
                    if (!pseudo) {
                        const uint32_t c = feat_codon(a.cls, grp.S, L, pass, ci);
                        if (c & 1u) break;
                        if (!(c & 2u)) continue;
                    }
                    if (has_pre && pe - ci > a.max_overlap) break;
                    if (3 * (int64_t)((si - ci) / 3) >= a.min_length) {
                        if (has_pre) { a.keys[at] = kpre | (uint64_t)(uint32_t)(ci - pe + a.max_overlap); a.vals[at] = ns; at++; }
                        if (has_suc) { a.keys[at] = ksuc; a.vals[at] = ns; at++; }
                    }
                    if (pseudo) break;
                }
            }
        }
        if (!WRITE) a.unit_cnt[u] = n_rec;
    }
    if (!WRITE) {
        if (u == a.n_units) a.unit_cnt[u] = 0;          // the scan's last output is the total
        __syncthreads();
        for (uint32_t i = threadIdx.x; i < FEAT_LDS_BINS; i += blockDim.x)
            if (s_hist[i]) atomicAdd(&a.len_hist[i], (unsigned long long)s_hist[i]);
        if (threadIdx.x < 3 && s_starts[threadIdx.x]) atomicAdd(&a.starts[threadIdx.x], (unsigned long long)s_starts[threadIdx.x]);
    }
}

// The start codon of every gene (parse_genes, :248-257): the first three letters of its string, which on the reverse strand are
// the complement of the last three of its range.
__global__ __launch_bounds__(256) void k_feat_gene_starts(const uint32_t *__restrict__ cls, const uint32_t *__restrict__ packed,
                                                          const FeatGroup *__restrict__ groups, const FeatGene *__restrict__ genes, uint64_t n_genes,
                                                          const uint8_t *__restrict__ has_start, unsigned long long *starts)
{
    const uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n_genes) return;
    const FeatGene g = genes[k];
    if (!has_start[k] || g.end - g.start < 3) return;
    const FeatGroup grp = groups[g.group];
    const int pass = g.strand < 0;
    const int32_t c = pass ? grp.L - g.end : g.start;
    if (feat_codon(cls, grp.S, grp.L, pass, c) & 2u) atomicAdd(&starts[feat_which(packed, grp.S, grp.L, pass, c)], 1ull);
}

// flag[i] = record i opens a bin (its key >> shift differs from the one before); flag[n] = 0
__global__ __launch_bounds__(256) void k_feat_heads(const uint64_t *__restrict__ keys, uint64_t n, unsigned shift, uint32_t *__restrict__ flag)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i > n) return;
    flag[i] = i < n && (i == 0 || (keys[i] >> shift) != (keys[i - 1] >> shift));
}

__global__ __launch_bounds__(256) void k_feat_head_pos(const uint32_t *__restrict__ flag, const uint64_t *__restrict__ excl, uint64_t n, uint64_t *__restrict__ pos)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n && flag[i]) pos[excl[i]] = i;
}

// One wave per bin: its records, in their order, 64 at a time -- loaded coalesced, handed round through LDS and added one after
// the other by every lane alike (a slot beyond the bin's end holds 0.0, which changes no sum).
__global__ __launch_bounds__(256) void k_feat_sum(const uint64_t *__restrict__ keys, const uint32_t *__restrict__ vals, uint64_t n,
                                                  const uint64_t *__restrict__ pos, uint64_t n_heads, uint64_t *__restrict__ hkey, double *__restrict__ hsum)
{
    __shared__ double s_v[4][64];
    const uint32_t wv = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    const uint64_t h = (uint64_t)blockIdx.x * 4 + wv;
    if (h >= n_heads) return;
    const uint64_t b = pos[h], e = h + 1 < n_heads ? pos[h + 1] : n;
    double acc = 0.0;
    for (uint64_t i = b; i < e; i += 64) {
        s_v[wv][lane] = i + lane < e ? 1.0 / (double)vals[i + lane] : 0.0;
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int j = 0; j < 64; j++) acc += s_v[wv][j];
        __builtin_amdgcn_wave_barrier();
    }
    if (lane == 0) { hkey[h] = keys[b]; hsum[h] = acc; }
}

// ---- host ---------------------------------------------------------------------------------------------------------------------

struct FeatTable {
    std::vector<int64_t> lengths;
    int64_t starts[3];
    double orient[4], orient_raw[4];
    std::vector<double> dist[4];                        // index = distance + max_overlap; [3] is folded into [0] by finish()
};

struct GMG_HIDDEN gmg_features {
    FeatTable t[2];                                     // GENE, NON
    int32_t max_overlap;
    uint64_t n_records, n_units;
    float stage_ms[GMG_FEATURES_STAGES];
};

static void feat_add(std::vector<double> &v, int64_t idx, double x)
{
    if (idx < 0) return;
    if ((uint64_t)idx >= v.size()) v.resize((size_t)idx + 1, 0.0);
    v[(size_t)idx] += x;
}

// destrand_orientations (:544-554)
static void feat_finish(FeatTable &t)
{
    for (int o = 0; o < 4; o++) t.orient_raw[o] = t.orient[o];
    t.orient[0] = (t.orient[0] + t.orient[3]) / 2.0;
    t.orient[3] = t.orient[0];
    std::vector<double> &a = t.dist[0], &b = t.dist[3];
    if (b.size() > a.size()) a.resize(b.size(), 0.0);
    for (size_t l = 0; l < a.size(); l++) a[l] = (a[l] + (l < b.size() ? b[l] : 0.0)) / 2.0;
    b = a;
}

static inline int64_t floor_div3(int64_t x) { return x >= 0 ? x / 3 : -((-x + 2) / 3); }

// bit v of the result: the codon of packed value v is one of `codons` (upper-case letters), or its reverse complement is
static uint64_t feat_mask(const char *const *codons, int n, bool revcomp)
{
    uint64_t m = 0;
    for (int k = 0; k < n; k++) {
        int c[3];
        for (int i = 0; i < 3; i++) c[i] = gmg_base_code(codons[k][i]);
        if (revcomp) { const int x = 3 - c[2]; c[2] = 3 - c[0]; c[1] = 3 - c[1]; c[0] = x; }
        m |= 1ull << (c[0] | (c[1] << 2) | (c[2] << 4));
    }
    return m;
}

// the bins of one sorted record array: *n_heads bins, their first keys and sums on the host
static int feat_bins(GmgScratch &sc, const uint64_t *d_keys, const uint32_t *d_vals, uint64_t n, unsigned shift, hipStream_t s,
                     std::vector<uint64_t> &hkey, std::vector<double> &hsum)
{
    uint32_t *d_flag = nullptr;
    uint64_t *d_excl = nullptr, *d_pos = nullptr, *d_hkey = nullptr;
    double *d_hsum = nullptr;
    GMG_HIP(sc.alloc(&d_flag, (n + 1) * 4));
    GMG_HIP(sc.alloc(&d_excl, (n + 1) * 8));
    hipLaunchKernelGGL(k_feat_heads, dim3((unsigned)((n + 256) / 256)), dim3(256), 0, s, d_keys, n, shift, d_flag);
    GMG_HIP(hipGetLastError());
    GMG_HIP((gmg_scan_excl<uint32_t, uint64_t>(d_flag, d_excl, n + 1, s)));
    uint64_t n_heads = 0;
    GMG_HIP(hipMemcpyAsync(&n_heads, d_excl + n, 8, hipMemcpyDeviceToHost, s));
    GMG_HIP(hipStreamSynchronize(s));
    hkey.assign(n_heads, 0);
    hsum.assign(n_heads, 0.0);
    if (n_heads) {
        GMG_HIP(sc.alloc(&d_pos, n_heads * 8));
        GMG_HIP(sc.alloc(&d_hkey, n_heads * 8));
        GMG_HIP(sc.alloc(&d_hsum, n_heads * 8));
        hipLaunchKernelGGL(k_feat_head_pos, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, d_flag, d_excl, n, d_pos);
        hipLaunchKernelGGL(k_feat_sum, dim3((unsigned)((n_heads + 3) / 4)), dim3(256), 0, s, d_keys, d_vals, n, d_pos, n_heads, d_hkey, d_hsum);
        GMG_HIP(hipGetLastError());
        GMG_HIP(hipMemcpyAsync(hkey.data(), d_hkey, n_heads * 8, hipMemcpyDeviceToHost, s));
        GMG_HIP(hipMemcpyAsync(hsum.data(), d_hsum, n_heads * 8, hipMemcpyDeviceToHost, s));
        GMG_HIP(hipStreamSynchronize(s));
    }
    sc.release(d_flag); sc.release(d_excl); sc.release(d_pos); sc.release(d_hkey); sc.release(d_hsum);
    return GMG_OK;
}

#define FEAT_DEV_STAGES 5
struct FeatEvents {                                     // the stage clock: events on the call's stream
    hipEvent_t ev[FEAT_DEV_STAGES + 1];
    int n = 0;
    ~FeatEvents() { for (int k = 0; k < n; k++) (void)hipEventDestroy(ev[k]); }
    void mark(hipStream_t s)
    {
        if (n > FEAT_DEV_STAGES) return;
        if (hipEventCreate(&ev[n]) != hipSuccess) return;
        (void)hipEventRecord(ev[n], s);
        n++;
    }
};

extern "C" int gmg_features_count(const gmg_reads *reads, const gmg_feature_gene *genes, uint64_t n_genes, const uint64_t *opaque_base,
                                  uint64_t n_opaque, const gmg_features_params *params, gmg_features **out, void *stream)
{
    { int rc_enter = gmg_enter("gmg_features_count"); if (rc_enter) return rc_enter; }
    if (!reads || !genes || !n_genes || !params || !out || (n_opaque && !opaque_base))
        return gmg_set_error(GMG_EINVAL, "gmg_features_count: bad argument (at least one gene is needed)");
    if (params->max_overlap < 0 || params->max_overlap > (1 << 20) || params->min_length < -(1 << 30) || params->min_length > (1 << 30))
        return gmg_set_error(GMG_EINVAL, "gmg_features_count: max_overlap must be in [0, 2^20], min_length in [-2^30, 2^30]");
    if (n_genes > (uint64_t)gmg_opt(GMG_OPT_MG_MAX_ENTRIES))
        return gmg_set_error(GMG_ETOOBIG, "gmg_features_count: %llu genes, more than mg_max_entries = %lld", (unsigned long long)n_genes,
                             gmg_opt(GMG_OPT_MG_MAX_ENTRIES));
    for (uint64_t i = 0; i < n_opaque; i++)
        if (opaque_base[i] >= reads->total_bases || (i && opaque_base[i] <= opaque_base[i - 1]))
            return gmg_set_error(GMG_EINVAL, "gmg_features_count: opaque base %llu: the list must ascend inside the batch", (unsigned long long)i);
    const int32_t max_overlap = params->max_overlap;
    typedef std::chrono::steady_clock HostClock;
    const HostClock::time_point t_enter = HostClock::now();
    hipStream_t s = (hipStream_t)stream;
    GmgScratch sc(GmgScratch::STREAM, s);

    // ---- the gene list: its groups first (a read per group), then the begin and end of just those reads from the device, through
    // page-locked memory (the whole offset array of a million reads into pageable memory took 30 ms)
    gmg_features *res = new (std::nothrow) gmg_features();
    if (!res) return gmg_set_error(GMG_ENOMEM, "gmg_features_count: out of host memory");
    std::unique_ptr<gmg_features> guard(res);           // until the caller has it
    memset(res->stage_ms, 0, sizeof res->stage_ms);
    res->max_overlap = max_overlap;
    for (int w = 0; w < 2; w++)
        for (int k = 0; k < 4; k++) { res->t[w].orient[k] = 0.0; if (k < 3) res->t[w].starts[k] = 0; }
    std::vector<uint32_t> group_read;
    {
        std::vector<bool> seen(reads->n_reads, false);
        for (uint64_t i = 0; i < n_genes; i++) {
            const uint32_t r = genes[i].read;
            if (i && genes[i - 1].read == r) continue;
            if (r >= reads->n_reads) return gmg_set_error(GMG_ERANGE, "gmg_features_count: gene %llu names read %u of %llu", (unsigned long long)i, r, (unsigned long long)reads->n_reads);
            if (seen[r]) return gmg_set_error(GMG_EINVAL, "gmg_features_count: gene %llu: the genes of read %u are not consecutive", (unsigned long long)i, r);
            seen[r] = true;
            group_read.push_back(r);
        }
    }
    // [2 * groups]: begin, end.  Pageable: hipHostFree of a page-locked buffer waits for the whole device, the null stream included,
    // which a call on a caller's stream must not
    struct Extents { std::vector<uint64_t> v; uint64_t *p = nullptr; } ext;
    {
        ext.v.resize(2 * group_read.size() + 1);
        ext.p = ext.v.data();
        uint32_t *d_group_read = nullptr;
        uint64_t *d_ext = nullptr;
        GMG_HIP(sc.alloc(&d_group_read, group_read.size() * 4));
        GMG_HIP(sc.alloc(&d_ext, group_read.size() * 16));
        GMG_HIP(hipMemcpyAsync(d_group_read, group_read.data(), group_read.size() * 4, hipMemcpyHostToDevice, s));
        hipLaunchKernelGGL(k_feat_group_extent, dim3((unsigned)((group_read.size() + 255) / 256)), dim3(256), 0, s, reads->d_off, d_group_read,
                           (uint32_t)group_read.size(), d_ext);
        GMG_HIP(hipGetLastError());
        GMG_HIP(hipMemcpyAsync(ext.p, d_ext, group_read.size() * 16, hipMemcpyDeviceToHost, s));
        GMG_HIP(hipStreamSynchronize(s));
        sc.release(d_group_read);
        sc.release(d_ext);
    }
    std::vector<FeatGene> fg(n_genes);
    std::vector<uint8_t> has_start(n_genes);
    std::vector<FeatGroup> groups;
    groups.reserve(group_read.size());
    FeatTable &gt = res->t[0];
    int64_t max_L = 0;
    for (uint64_t i = 0; i < n_genes;) {
        const uint32_t r = genes[i].read;
        const uint64_t S = ext.p[2 * groups.size()];
        const int64_t L = (int64_t)(ext.p[2 * groups.size() + 1] - S);
        if (L + 3 + max_overlap > 0x7fffffffll)
            return gmg_set_error(GMG_ETOOBIG, "gmg_features_count: read %u has %lld bases: positions must fit 32 bits", r, (long long)L);
        uint64_t j = i;
        for (; j < n_genes && genes[j].read == r; j++) {
            const gmg_feature_gene &g = genes[j];
            if (g.start < 0 || g.end < 0 || g.start > L || g.end > L || g.strand == 0)
                return gmg_set_error(GMG_ERANGE, "gmg_features_count: gene %llu (read %u, %d .. %d, strand %d) is not clipped to its read of %lld bases",
                                     (unsigned long long)j, r, g.start, g.end, g.strand, (long long)L);
            fg[j].start = g.start; fg[j].end = g.end; fg[j].strand = g.strand > 0 ? 1 : -1; fg[j].group = (uint32_t)groups.size();
            fg[j].pmax_end = j > i && fg[j - 1].pmax_end > g.end ? fg[j - 1].pmax_end : g.end;
            has_start[j] = g.start_codon != 0;
            // parse_genes (:237-280) without the start codon
            const int64_t bin = floor_div3((int64_t)g.end - 3 - g.start);
            if (bin >= 0) {
                if ((uint64_t)bin >= gt.lengths.size()) gt.lengths.resize((size_t)bin + 1, 0);
                gt.lengths[(size_t)bin]++;
            }
            if (j > i) {
                const int o = (fg[j - 1].strand > 0 ? 0 : 2) + (fg[j].strand > 0 ? 0 : 1);
                gt.orient[o] += 1.0;
                const int64_t d = (int64_t)g.start - fg[j - 1].end;
                if (-d <= max_overlap) feat_add(gt.dist[o], d + max_overlap, 1.0);
            }
        }
        for (uint64_t k = j; k-- > i;) fg[k].smin_start = k + 1 < j && fg[k + 1].smin_start < fg[k].start ? fg[k + 1].smin_start : fg[k].start;
        FeatGroup grp;
        grp.S = S; grp.L = (int32_t)L; grp.gene_begin = (uint32_t)i; grp.n_genes = (uint32_t)(j - i); grp.reserved = 0;
        groups.push_back(grp);
        max_L = L > max_L ? L : max_L;
        i = j;
    }
    const uint32_t n_groups = (uint32_t)groups.size();
    std::vector<uint64_t> unit_off(2 * (size_t)n_groups + 1);
    unit_off[0] = 0;
    for (uint32_t k = 0; k < 2 * n_groups; k++)
        unit_off[k + 1] = unit_off[k] + ((uint64_t)groups[k % n_groups].L + 3 + FEAT_UNIT - 1) / FEAT_UNIT;
    const uint64_t n_units = unit_off[2 * n_groups];
    const uint64_t n_len_bins = std::max<uint64_t>((uint64_t)(max_L + 5) / 3 + 2, FEAT_LDS_BINS);

    // ---- device: the opaque bits, the codon classes
    const HostClock::time_point t_device = HostClock::now();
    FeatEvents clock;
    clock.mark(s);
    const uint64_t total = reads->total_bases;
    const uint64_t opq_words = (total + 31) / 32 + 2, cls_words = (total + 7) / 8 + 1;
    uint32_t *d_opq = nullptr, *d_cls = nullptr;
    uint64_t *d_obase = nullptr, *d_unit_off = nullptr, *d_unit_cnt = nullptr, *d_rec_off = nullptr;
    FeatGroup *d_groups = nullptr;
    FeatGene *d_genes = nullptr;
    uint8_t *d_has_start = nullptr;
    unsigned long long *d_hist = nullptr;                 // [n_len_bins] NON lengths, then [3] NON starts, [3] GENE starts
    GMG_HIP(sc.alloc(&d_opq, opq_words * 4));
    GMG_HIP(sc.alloc(&d_cls, cls_words * 4));
    GMG_HIP(sc.alloc(&d_groups, n_groups * sizeof(FeatGroup)));
    GMG_HIP(sc.alloc(&d_genes, n_genes * sizeof(FeatGene)));
    GMG_HIP(sc.alloc(&d_has_start, n_genes));
    GMG_HIP(sc.alloc(&d_unit_off, unit_off.size() * 8));
    GMG_HIP(sc.alloc(&d_unit_cnt, (n_units + 1) * 8));
    GMG_HIP(sc.alloc(&d_rec_off, (n_units + 1) * 8));
    GMG_HIP(sc.alloc(&d_hist, (n_len_bins + 6) * 8));
    GMG_HIP(hipMemsetAsync(d_opq, 0, opq_words * 4, s));
    GMG_HIP(hipMemsetAsync(d_cls, 0, cls_words * 4, s));
    GMG_HIP(hipMemsetAsync(d_hist, 0, (n_len_bins + 6) * 8, s));
    GMG_HIP(hipMemcpyAsync(d_groups, groups.data(), n_groups * sizeof(FeatGroup), hipMemcpyHostToDevice, s));
    GMG_HIP(hipMemcpyAsync(d_genes, fg.data(), n_genes * sizeof(FeatGene), hipMemcpyHostToDevice, s));
    GMG_HIP(hipMemcpyAsync(d_has_start, has_start.data(), n_genes, hipMemcpyHostToDevice, s));
    GMG_HIP(hipMemcpyAsync(d_unit_off, unit_off.data(), unit_off.size() * 8, hipMemcpyHostToDevice, s));
    if (n_opaque) {
        GMG_HIP(sc.alloc(&d_obase, n_opaque * 8));
        GMG_HIP(hipMemcpyAsync(d_obase, opaque_base, n_opaque * 8, hipMemcpyHostToDevice, s));
        hipLaunchKernelGGL(k_feat_opaque, dim3((unsigned)((n_opaque + 255) / 256)), dim3(256), 0, s, d_obase, n_opaque, total, d_opq);
        GMG_HIP(hipGetLastError());
    }
    static const char *const k_starts[3] = {"ATG", "GTG", "TTG"}, *const k_stops[3] = {"TAG", "TAA", "TGA"};
    const int n_stops = params->drop_tga ? 2 : 3;
    if (total) {
        hipLaunchKernelGGL(k_feat_mark, dim3((unsigned)(((total + 7) / 8 + 255) / 256)), dim3(256), 0, s, reads->d_packed, d_opq, total,
                           feat_mask(k_stops, n_stops, false), feat_mask(k_starts, 3, false), feat_mask(k_stops, n_stops, true),
                           feat_mask(k_starts, 3, true), d_cls);
        GMG_HIP(hipGetLastError());
    }
    clock.mark(s);                                      // stage 0: opaque bits + codon classes

    // ---- the items: count, scan, write
    FeatArgs a;
    memset(&a, 0, sizeof a);
    a.cls = d_cls; a.packed = reads->d_packed; a.groups = d_groups; a.genes = d_genes; a.unit_off = d_unit_off;
    a.n_groups = n_groups; a.n_units = n_units; a.min_length = params->min_length; a.max_overlap = max_overlap;
    a.unit_cnt = d_unit_cnt; a.len_hist = d_hist; a.starts = d_hist + n_len_bins;
    if ((n_units + 256) / 256 > 0x7fffffffull)
        return gmg_set_error(GMG_ETOOBIG, "gmg_features_count: %llu units of 32 positions", (unsigned long long)n_units);
    const unsigned item_grid = (unsigned)((n_units + 256) / 256);
    hipLaunchKernelGGL(k_feat_items<false>, dim3(item_grid), dim3(256), 0, s, a);
    hipLaunchKernelGGL(k_feat_gene_starts, dim3((unsigned)((n_genes + 255) / 256)), dim3(256), 0, s, d_cls, reads->d_packed, d_groups, d_genes, n_genes,
                       d_has_start, d_hist + n_len_bins + 3);
    GMG_HIP(hipGetLastError());
    clock.mark(s);                                      // stage 1: count pass
    GMG_HIP((gmg_scan_excl<uint64_t, uint64_t>(d_unit_cnt, d_rec_off, n_units + 1, s)));
    uint64_t n_rec = 0;
    GMG_HIP(hipMemcpyAsync(&n_rec, d_rec_off + n_units, 8, hipMemcpyDeviceToHost, s));
    GMG_HIP(hipStreamSynchronize(s));
    clock.mark(s);                                      // stage 2: scan
    if (n_rec > (uint64_t)gmg_opt(GMG_OPT_MG_MAX_ENTRIES))
        return gmg_set_error(GMG_ETOOBIG, "gmg_features_count: %llu orientation / distance records, more than mg_max_entries = %lld: count the reads in smaller batches",
                             (unsigned long long)n_rec, gmg_opt(GMG_OPT_MG_MAX_ENTRIES));
    FeatTable &nt = res->t[1];
    if (n_rec) {
        uint64_t *d_keys = nullptr, *d_keys2 = nullptr;
        uint32_t *d_vals = nullptr, *d_vals2 = nullptr;
        void *d_tmp = nullptr;
        GMG_HIP(sc.alloc(&d_keys, n_rec * 8));
        GMG_HIP(sc.alloc(&d_keys2, n_rec * 8));
        GMG_HIP(sc.alloc(&d_vals, n_rec * 4));
        GMG_HIP(sc.alloc(&d_vals2, n_rec * 4));
        a.rec_off = d_rec_off; a.keys = d_keys; a.vals = d_vals;
        hipLaunchKernelGGL(k_feat_items<true>, dim3(item_grid), dim3(256), 0, s, a);
        GMG_HIP(hipGetLastError());
        clock.mark(s);                                  // stage 3: write pass
        size_t need = 0, need2 = 0;
        GMG_HIP(hipcub::DeviceRadixSort::SortPairs(nullptr, need, d_keys, d_keys2, d_vals, d_vals2, (int)n_rec, 32, 34, s));
        GMG_HIP(hipcub::DeviceRadixSort::SortPairs(nullptr, need2, d_keys, d_keys2, d_vals, d_vals2, (int)n_rec, 0, 34, s));
        need = need > need2 ? need : need2;
        GMG_HIP(sc.alloc(&d_tmp, need ? need : 16));
        std::vector<uint64_t> hkey;
        std::vector<double> hsum;
        // the four orientation bins: the records in their order, orientation by orientation
        size_t nb = need;
        GMG_HIP(hipcub::DeviceRadixSort::SortPairs(d_tmp, nb, d_keys, d_keys2, d_vals, d_vals2, (int)n_rec, 32, 34, s));
        { const int rc = feat_bins(sc, d_keys2, d_vals2, n_rec, 32, s, hkey, hsum); if (rc) return rc; }
        for (size_t h = 0; h < hkey.size(); h++) nt.orient[(hkey[h] >> 32) & 3] = hsum[h];
        // the distance bins
        nb = need;
        GMG_HIP(hipcub::DeviceRadixSort::SortPairs(d_tmp, nb, d_keys, d_keys2, d_vals, d_vals2, (int)n_rec, 0, 34, s));
        { const int rc = feat_bins(sc, d_keys2, d_vals2, n_rec, 0, s, hkey, hsum); if (rc) return rc; }
        for (size_t h = 0; h < hkey.size(); h++) {
            std::vector<double> &v = nt.dist[(hkey[h] >> 32) & 3];
            const size_t idx = (size_t)(hkey[h] & 0xffffffffull);
            if (idx >= v.size()) v.resize(idx + 1, 0.0);
            v[idx] = hsum[h];
        }
        clock.mark(s);                                  // stage 4: sorts + in-order sums
    }
    const HostClock::time_point t_finish = HostClock::now();
    std::vector<unsigned long long> hist(n_len_bins + 6);
    GMG_HIP(hipMemcpyAsync(hist.data(), d_hist, hist.size() * 8, hipMemcpyDeviceToHost, s));
    GMG_HIP(hipStreamSynchronize(s));
    sc.wait = GmgScratch::NONE;                         // (waited for just now)
    uint64_t top = n_len_bins;
    while (top && !hist[top - 1]) top--;
    nt.lengths.assign(hist.begin(), hist.begin() + top);
    for (int k = 0; k < 3; k++) { nt.starts[k] = (int64_t)hist[n_len_bins + k]; gt.starts[k] = (int64_t)hist[n_len_bins + 3 + k]; }
    feat_finish(gt);
    feat_finish(nt);
    res->n_records = n_rec;
    res->n_units = n_units;
    for (int k = 0; k + 1 < clock.n; k++) (void)hipEventElapsedTime(&res->stage_ms[k], clock.ev[k], clock.ev[k + 1]);
    const HostClock::time_point t_leave = HostClock::now();
    res->stage_ms[FEAT_DEV_STAGES] = std::chrono::duration<float, std::milli>(t_device - t_enter).count();
    res->stage_ms[FEAT_DEV_STAGES + 1] = std::chrono::duration<float, std::milli>(t_finish - t_device).count();
    res->stage_ms[FEAT_DEV_STAGES + 2] = std::chrono::duration<float, std::milli>(t_leave - t_finish).count();
    *out = guard.release();
    return GMG_OK;
}

extern "C" int gmg_features_fetch(const gmg_features *f, int which, gmg_features_table *out)
{
    if (!f || !out || which < 0 || which > 1) return gmg_set_error(GMG_EINVAL, "gmg_features_fetch: bad argument");
    const FeatTable &t = f->t[which];
    out->n_lengths = t.lengths.size();
    out->lengths = t.lengths.empty() ? nullptr : t.lengths.data();
    for (int k = 0; k < 3; k++) {
        out->starts[k] = t.starts[k];
        out->n_dist[k] = t.dist[k].size();
        out->dist[k] = t.dist[k].empty() ? nullptr : t.dist[k].data();
    }
    for (int k = 0; k < 4; k++) { out->orient[k] = t.orient[k]; out->orient_raw[k] = t.orient_raw[k]; }
    return GMG_OK;
}

extern "C" int gmg_features_info(const gmg_features *f, uint64_t *n_units, uint64_t *n_records, float *stage_ms)
{
    if (!f) return gmg_set_error(GMG_EINVAL, "gmg_features_info: NULL handle");
    if (n_units) *n_units = f->n_units;
    if (n_records) *n_records = f->n_records;
    if (stage_ms) memcpy(stage_ms, f->stage_ms, sizeof f->stage_ms);
    return GMG_OK;
}

extern "C" int gmg_features_free(gmg_features *f)
{
    delete f;
    return GMG_OK;
}
