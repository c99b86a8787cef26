// gmg_entropy.hip -- the entropy distance ratio of long-orfs / glimmer3 -E for a batch of regions (include/gmg.h,
// gmg_entropy_*): Entropy_Distance_Ratio (src/Glimmer/long-orfs.cc:301-351, glimmer3.cc:423-473) with
// Forward_Strand_Transfer / Reverse_Strand_Transfer (src/Common/gene.cc:1237-1260, 1533-1556), Codon_Translation
// (gene.cc:1016-1080) and Counts_To_Entropy_Profile (gene.cc:1095-1135).
//
// k_entropy: a wave per region.  A step covers 64 codons, one per lane: the lane reads its three bases from the packed read
// (positions modulo the read's length, the reverse strand downwards and complemented), maps the codon index 16*b0 + 4*b1 + b2
// through a 64-byte class table in LDS (0..19 = the amino acids in the order A C D E F G H I K L M N P Q R S T V W Y, 20 = counts
// nowhere) and the wave counts every class with a ballot and a population count -- no atomics, no per-lane histograms.  The 20
// counts are exact integers: they are what the feature promises bit for bit.
//
// The finish (optional) follows the reference's order of operations: lane j < 20 holds e_j, and S and the two sums of squares are
// 20 sequential additions in j order (every lane adds the same 20 values, read lane by lane).  Against the host finish
// (gmg_entropy_from_counts: libm) it differs only through the device's log and through d * d in place of pow (d, 2).

#include "gmg_internal.h"

#include "gmg_device.h"

#include <math.h>
#include <string.h>
#include <vector>

#define EN_BLOCK 256             // four waves, a region each
#define EN_WAVES (EN_BLOCK / 64)
#define EN_GRID_CAP (256 * 32)   // 8 work-groups of four waves per CU, 4 rounds; the rest loops
#define EN_NONE 20               // class of a codon that counts nowhere

struct EntropyArgs {
    double pos[20], neg[20];
    uint8_t cls[64];             // class of codon index 16*b0 + 4*b1 + b2
};

// the region of ORF o by Entropy_Filter's rule (long-orfs.cc:370-377): 1-based start stop - len (forward) or stop + len + 2
// (reverse), brought onto the sequence as On_Seq_1 does; first = start - 1
__device__ __forceinline__ void en_orf_region(const gmg_mg_orf &o, int64_t n, int64_t &first, int64_t &len, int &strand)
{
    len = o.gene_len > 0 ? o.gene_len : 0;
    strand = o.frame > 0 ? 1 : -1;
    int64_t s = o.frame > 0 ? (int64_t)o.stop_position - o.gene_len - 1 : (int64_t)o.stop_position + o.gene_len + 1;
    if (n > 0) { s %= n; if (s < 0) s += n; } else { s = 0; len = 0; }
    first = s;
}

// lane j's value of x in every lane (j is the same in all lanes: two scalar lane reads, no trip through the LDS crossbar)
__device__ __forceinline__ double en_from_lane(double x, int j)
{
    const int lo = __builtin_amdgcn_readlane(__double2loint(x), j), hi = __builtin_amdgcn_readlane(__double2hiint(x), j);
    return __hiloint2double(hi, lo);
}

template <bool ORFS>
__global__ __launch_bounds__(EN_BLOCK) void k_entropy(EntropyArgs a, const uint32_t *__restrict__ packed,
                                                      const uint64_t *__restrict__ off, const gmg_gene_region *__restrict__ regions,
                                                      const gmg_mg_orf *__restrict__ orfs, uint64_t n_regions,
                                                      int32_t *__restrict__ counts, double *__restrict__ dist)
{
    __shared__ uint8_t s_cls[64];
    if (threadIdx.x < 64) s_cls[threadIdx.x] = a.cls[threadIdx.x];
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const uint64_t wave0 = (uint64_t)blockIdx.x * EN_WAVES + (threadIdx.x >> 6);
    const uint64_t stride = (uint64_t)gridDim.x * EN_WAVES;
    for (uint64_t k = wave0; k < n_regions; k += stride) {              // (k is the same in every lane of the wave)
        uint64_t base;
        int64_t n, first, len;
        int strand;
        if (ORFS) {
            const gmg_mg_orf o = orfs[k];
            base = off[o.read];
            n = (int64_t)(off[o.read + 1] - base);
            en_orf_region(o, n, first, len, strand);
        } else {
            const gmg_gene_region r = regions[k];
            base = off[r.read];
            n = (int64_t)(off[r.read + 1] - base);
            first = r.first;
            len = r.len;
            strand = r.strand;
        }
        const int64_t n_codons = len / 3;                               // a trailing partial codon counts nowhere
        const DevRegion R = {packed, base, n, first, strand > 0};
        int cnt[20];
#pragma unroll
        for (int j = 0; j < 20; j++) cnt[j] = 0;
        for (int64_t c0 = 0; c0 < n_codons; c0 += 64) {
            const int64_t c = c0 + lane;
            int cl = EN_NONE;
            if (c < n_codons) {
                // base i = 3c of the region sits at first + i (forward) or first - i (reverse), modulo n; 0 <= p < n throughout
                // (reads hold fewer than 2^31 bases and len is an int32: 32-bit arithmetic; len <= n needs no division at all)
                uint32_t r = (uint32_t)(3 * c);
                if (r >= (uint32_t)n) r %= (uint32_t)n;
                cl = s_cls[R.codon((int64_t)r)];
            }
#pragma unroll
            for (int j = 0; j < 20; j++) cnt[j] += __popcll(__ballot(cl == j));
        }
        int mine = 0;                                                   // lane j < 20: count j
#pragma unroll
        for (int j = 0; j < 20; j++) mine = lane == j ? cnt[j] : mine;
        if (counts && lane < 20) counts[k * 20 + lane] = mine;
        if (!dist) continue;
        // Counts_To_Entropy_Profile: S0 = the sum of the 20 counts (integers: exact in any order)
        int total = 0;
#pragma unroll
        for (int j = 0; j < 20; j++) total += cnt[j];
        double e = 0.0;
        if (total != 0 && lane < 20) {
            const double pj = (double)mine / (double)total;
            e = pj <= 0.0 ? 0.0 : -1.0 * pj * log(pj);
        }
        double S = 0.0;
#pragma unroll
        for (int j = 0; j < 20; j++) S += en_from_lane(e, j);
        const double ep = total != 0 ? e / S : 0.0;                     // S == 0 (one amino acid): NaN, as in the reference
        const double dp = ep - a.pos[lane < 20 ? lane : 0], dn = ep - a.neg[lane < 20 ? lane : 0];
        const double sp = dp * dp, sn = dn * dn;
        double pos_dist = 0.0, neg_dist = 0.0;
#pragma unroll
        for (int j = 0; j < 20; j++) {
            pos_dist += en_from_lane(sp, j);
            neg_dist += en_from_lane(sn, j);
        }
        pos_dist = sqrt(pos_dist);
        neg_dist = sqrt(neg_dist);
        const double ratio = neg_dist == 0.0 ? (pos_dist == 0.0 ? 1.0 : 1e3) : pos_dist / neg_dist;
        if (lane < 3) dist[k * 3 + lane] = lane == 0 ? pos_dist : lane == 1 ? neg_dist : ratio;
    }
}

static int en_args(const char *who, const char aa[64], const double pos[20], const double neg[20], EntropyArgs *a)
{
    static const char order[] = "ACDEFGHIKLMNPQRSTVWY";
    for (int i = 0; i < 64; i++) {
        const char ch = aa[i];
        if (!((ch >= 'A' && ch <= 'Z') || ch == '*'))
            return gmg_set_error(GMG_EINVAL, "%s: aa[%d] = 0x%02x is neither 'A'..'Z' nor '*'", who, i, (unsigned)(unsigned char)ch);
        const char *p = ch == '*' ? nullptr : strchr(order, ch);
        a->cls[i] = p ? (uint8_t)(p - order) : (uint8_t)EN_NONE;
    }
    memcpy(a->pos, pos, sizeof a->pos);
    memcpy(a->neg, neg, sizeof a->neg);
    return GMG_OK;
}

extern "C" int gmg_entropy_regions(const gmg_reads *reads, const gmg_gene_region *regions, uint64_t n, const char aa[64],
                                   const double pos[20], const double neg[20], int32_t *d_counts, double *d_dist, void *stream)
{
    int rc = gmg_enter("gmg_entropy_regions");
    if (rc) return rc;
    if (!reads || (!regions && n) || !aa || !pos || !neg) return gmg_set_error(GMG_EINVAL, "gmg_entropy_regions: NULL argument");
    EntropyArgs a;
    rc = en_args("gmg_entropy_regions", aa, pos, neg, &a);
    if (rc) return rc;
    if (n == 0 || (!d_counts && !d_dist)) return GMG_OK;
    hipStream_t s = (hipStream_t)stream;
    // read lengths are needed for validation: fetch the offsets once, on the call's stream
    std::vector<uint64_t> off(reads->n_reads + 1);
    GMG_HIP(gmg_copy_wait(off.data(), reads->d_off, off.size() * 8, hipMemcpyDeviceToHost, s));
    for (uint64_t i = 0; i < n; i++) {
        const gmg_gene_region &r = regions[i];
        if (r.read >= reads->n_reads)
            return gmg_set_error(GMG_ERANGE, "gmg_entropy_regions: region %llu: read %u of %llu", (unsigned long long)i, r.read,
                                 (unsigned long long)reads->n_reads);
        const uint64_t L = off[r.read + 1] - off[r.read];
        if (r.first < 0 || (uint64_t)r.first >= L || r.len < 0 || (uint64_t)r.len > L || r.strand == 0)
            return gmg_set_error(GMG_ERANGE, "gmg_entropy_regions: region %llu (first %d, len %d, strand %d) does not fit read %u of length %llu",
                                 (unsigned long long)i, r.first, r.len, r.strand, r.read, (unsigned long long)L);
    }
    GmgScratch sc(GmgScratch::AFTER, s);
    gmg_gene_region *d_regions = nullptr;
    if (sc.alloc(&d_regions, n * sizeof(gmg_gene_region)) != hipSuccess)
        return gmg_set_error(GMG_ENOMEM, "gmg_entropy_regions: no device memory for %llu regions", (unsigned long long)n);
    GMG_HIP(hipMemcpyAsync(d_regions, regions, n * sizeof(gmg_gene_region), hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(k_entropy<false>, dim3(gmg_grid(n, EN_WAVES, EN_GRID_CAP)), dim3(EN_BLOCK), 0, s, a, reads->d_packed, reads->d_off, d_regions,
                       (const gmg_mg_orf *)nullptr, n, d_counts, d_dist);
    GMG_HIP(hipGetLastError());
    return GMG_OK;
}

extern "C" int gmg_entropy_orfs(const gmg_reads *reads, const gmg_mg_result *orfs, const char aa[64], const double pos[20],
                                const double neg[20], int32_t *d_counts, double *d_dist, void *stream)
{
    int rc = gmg_enter("gmg_entropy_orfs");
    if (rc) return rc;
    if (!reads || !orfs || !aa || !pos || !neg) return gmg_set_error(GMG_EINVAL, "gmg_entropy_orfs: NULL argument");
    EntropyArgs a;
    rc = en_args("gmg_entropy_orfs", aa, pos, neg, &a);
    if (rc) return rc;
    uint64_t n = 0;
    rc = gmg_mg_result_info(orfs, &n, nullptr);
    if (rc) return rc;
    if (n != orfs->n_orfs || orfs->n_reads != reads->n_reads)
        return gmg_set_error(GMG_EINVAL, "gmg_entropy_orfs: the result holds %llu ORFs of %llu reads, the batch has %llu reads",
                             (unsigned long long)n, (unsigned long long)orfs->n_reads, (unsigned long long)reads->n_reads);
    if (n == 0 || (!d_counts && !d_dist)) return GMG_OK;
    hipLaunchKernelGGL(k_entropy<true>, dim3(gmg_grid(n, EN_WAVES, EN_GRID_CAP)), dim3(EN_BLOCK), 0, (hipStream_t)stream, a, reads->d_packed, reads->d_off,
                       (const gmg_gene_region *)nullptr, orfs->d_orfs, n, d_counts, d_dist);
    GMG_HIP(hipGetLastError());
    return GMG_OK;
}

// ---------------------------------------------------------------------------
// host: the finish of one count vector with libm, in the reference's order of operations
// ---------------------------------------------------------------------------

extern "C" int gmg_entropy_from_counts(const int32_t counts[20], const double pos[20], const double neg[20], double *pos_dist,
                                       double *neg_dist, double *ratio)
{
    if (!counts || !pos || !neg) return gmg_set_error(GMG_EINVAL, "gmg_entropy_from_counts: NULL argument");
    // pow (x, 2) through libm as the reference calls it, not folded into x * x: the two differ in the last bit now and then
    static volatile double two = 2.0;
    double ep[20], sum = 0.0;
    for (int j = 0; j < 20; j++) sum += counts[j];
    if (sum == 0.0) {
        for (int j = 0; j < 20; j++) ep[j] = 0.0;
    } else {
        for (int j = 0; j < 20; j++) ep[j] = counts[j] / sum;
        sum = 0.0;
        for (int j = 0; j < 20; j++) {
            if (ep[j] <= 0.0) ep[j] = 0.0;
            else ep[j] = -1.0 * ep[j] * log(ep[j]);
            sum += ep[j];
        }
        for (int j = 0; j < 20; j++) ep[j] /= sum;
    }
    double pd = 0.0, nd = 0.0;
    for (int j = 0; j < 20; j++) {
        pd += pow(ep[j] - pos[j], two);
        nd += pow(ep[j] - neg[j], two);
    }
    pd = sqrt(pd);
    nd = sqrt(nd);
    if (pos_dist) *pos_dist = pd;
    if (neg_dist) *neg_dist = nd;
    if (ratio) *ratio = nd == 0.0 ? (pd == 0.0 ? 1.0 : 1e3) : pd / nd;
    return GMG_OK;
}

extern "C" int gmg_entropy_default_profiles(double pos[20], double neg[20])
{
    // the amino-acid entropy profiles of genes and non-genes Glimmer 3 ships as its defaults, order A C D E F G H I K L M N P Q R S T V W Y
    static const double p[20] = {0.08468, 0.01606, 0.05739, 0.05752, 0.04328, 0.07042, 0.02942, 0.05624, 0.04442, 0.05620,
                                 0.03029, 0.03975, 0.05116, 0.04098, 0.05989, 0.08224, 0.05660, 0.06991, 0.02044, 0.03310};
    static const double q[20] = {0.07434, 0.03035, 0.05936, 0.04729, 0.05662, 0.07704, 0.05777, 0.05328, 0.03360, 0.05581,
                                 0.01457, 0.03718, 0.04594, 0.05977, 0.08489, 0.05990, 0.04978, 0.07227, 0.01050, 0.01974};
    if (!pos || !neg) return gmg_set_error(GMG_EINVAL, "gmg_entropy_default_profiles: NULL argument");
    memcpy(pos, p, sizeof p);
    memcpy(neg, q, sizeof q);
    return GMG_OK;
}
