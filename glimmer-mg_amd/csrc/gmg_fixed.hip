// gmg_fixed.hip -- fixed-length ICMs on the device: Fixed_Length_ICM_t::Score_Window / subrange_score
// (src/ICM/icm.cc:1565-1645) for a batch of windows (include/gmg.h, gmg_fixed_*).
//
// A model of length L is L sub-models; sub-model i is an ICM_t (model_len i+1, periodicity 1) that predicts base i of the
// permuted window P from P[0..i-1].  The L trees are flattened into one node array (mip as int8, the four ln-probabilities as a
// float4), sub-model i from node off[i].  A window is at most 32 bases, so its 2-bit codes fit one 64-bit register: it is cut
// from the packed read once (dev_window_bits), turned into the segment's orientation, permuted once, and every context base a
// descent asks for is a shift and a mask.
//
// k_fixed_lane: a lane per window walks sub-models lo..hi-1 in order and adds their values in double -- the reference's loop.  The
// first FL_LANE_NODES nodes (levels 0..3) of every sub-model sit in LDS, deeper nodes are read through L2.  (A position-major layout
// -- a work-group per (sub-model, slice of windows), one float per (window, sub-model), then an in-order summing pass -- was as exact
// and slower: DESIGN.md 4.9.)

#include "gmg_internal.h"

#include "gmg_device.h"

#include <new>
#include <string.h>
#include <vector>

#define FL_LANE_NODES 85         // levels 0..3 of a sub-model: (4^4 - 1) / 3
#define FL_LANE_BLOCK 512

struct FixedArgs {
    int L;
    int identity;                // perm[i] == i for every i: no permutation step
    int perm[GMG_MAX_MODEL_LEN];
    int depth[GMG_MAX_MODEL_LEN];
    uint32_t off[GMG_MAX_MODEL_LEN];       // first node of sub-model i in the flat arrays
    uint32_t nodes[GMG_MAX_MODEL_LEN];     // its node count
};

struct GMG_HIDDEN gmg_fixed_model {
    FixedArgs a;
    int max_depth;
    uint64_t total_nodes;
    int8_t *d_mip;               // [total_nodes]
    float4 *d_prob;              // [total_nodes]
    void *d_blob;
    size_t blob_bytes;
    GmgScratch own{GmgScratch::NONE, nullptr, GmgScratch::DRIVER};
};

// ---------------------------------------------------------------------------
// device helpers
// ---------------------------------------------------------------------------

// codes 0..L-1 of the segment's buffer B (gmg_orient), B[j] at bits 2j
__device__ __forceinline__ uint64_t fl_window(const uint32_t *__restrict__ packed, const uint64_t *__restrict__ off,
                                              const gmg_segment sg, int L)
{
    const bool rev = (sg.orient == GMG_REVERSED || sg.orient == GMG_REVCOMP);
    const bool comp = (sg.orient == GMG_COMPLEMENTED || sg.orient == GMG_REVCOMP);
    const uint64_t base = off[sg.read] + sg.lo;
    // B[0..L) of a reversed buffer is S[lo+len-1] down to S[lo+len-L]: the last L bases of the segment, fields reversed
    uint64_t x = dev_window_bits(packed, (int64_t)(rev ? base + sg.len - (uint64_t)L : base));
    if (rev) {
        x = __brevll(x);
        x = ((x & 0x5555555555555555ull) << 1) | ((x >> 1) & 0x5555555555555555ull);
        x >>= 64 - 2 * L;                                    // (L >= 1: a shift of 0 .. 62)
    }
    if (comp) x = ~x;
    return L == 32 ? x : x & ((1ull << (2 * L)) - 1);
}

// P[i] = B[perm[i]] (Permute_String, src/ICM/icm.cc:1988-2004)
__device__ __forceinline__ uint64_t fl_permute(const FixedArgs &a, uint64_t x)
{
    if (a.identity) return x;
    uint64_t p = 0;
    for (int i = 0; i < a.L; i++) p |= ((x >> (2 * a.perm[i])) & 3ull) << (2 * i);
    return p;
}

// Full_Window_Prob (src/ICM/icm.cc:557-610) of sub-model i on the permuted window p: the descent of ICM_t's full window (pos == -1
// stops, pos < -1 goes back to the parent), its first `ln` nodes read from LDS (s_mip / s_prob from that sub-model's first node),
// the others from the flat arrays
__device__ __forceinline__ float fl_value(const int8_t *__restrict__ mip, const float4 *__restrict__ prob, const int8_t *s_mip,
                                          const float4 *s_prob, int ln, int depth, uint64_t p, int i)
{
    int node = 0;
    for (int l = 0; l < depth; l++) {
        const int pos = node < ln ? s_mip[node] : mip[node];
        if (pos == -1) break;
        if (pos < -1) { node = dev_parent(node); break; }
        node = 4 * node + (int)((p >> (2 * pos)) & 3ull) + 1;
    }
    if ((node < ln ? s_mip[node] : mip[node]) < -1) node = dev_parent(node);
    const float4 row = node < ln ? s_prob[node] : prob[node];
    const int c = (int)((p >> (2 * i)) & 3ull);
    return c == 0 ? row.x : c == 1 ? row.y : c == 2 ? row.z : row.w;
}

__global__ __launch_bounds__(FL_LANE_BLOCK) void k_fixed_lane(FixedArgs a, const int8_t *__restrict__ mip, const float4 *__restrict__ prob,
                                                              const uint32_t *__restrict__ packed, const uint64_t *__restrict__ off,
                                                              const gmg_segment *__restrict__ segs, uint64_t n, int lo, int hi,
                                                              double *__restrict__ out)
{
    __shared__ int8_t s_mip[GMG_MAX_MODEL_LEN * FL_LANE_NODES];
    __shared__ float4 s_prob[GMG_MAX_MODEL_LEN * FL_LANE_NODES];
    for (int i = lo; i < hi; i++) {
        const int ln = a.nodes[i] < FL_LANE_NODES ? (int)a.nodes[i] : FL_LANE_NODES;
        for (int t = threadIdx.x; t < ln; t += blockDim.x) {
            s_mip[i * FL_LANE_NODES + t] = mip[a.off[i] + t];
            s_prob[i * FL_LANE_NODES + t] = prob[a.off[i] + t];
        }
    }
    __syncthreads();
    for (uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; k < n; k += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t p = fl_permute(a, fl_window(packed, off, segs[k], a.L));
        double s = 0.0;
        for (int i = lo; i < hi; i++) {
            const int ln = a.nodes[i] < FL_LANE_NODES ? (int)a.nodes[i] : FL_LANE_NODES;
            s += (double)fl_value(mip + a.off[i], prob + a.off[i], s_mip + i * FL_LANE_NODES, s_prob + i * FL_LANE_NODES, ln,
                                  a.depth[i], p, i);
        }
        out[k] = s;
    }
}

int gmg_launch_fixed(const gmg_fixed_model *m, const gmg_reads *r, const gmg_segments *sg, int lo, int hi, double *d_out,
                     hipStream_t s)
{
    // 46 KB of LDS per work-group: three per CU; a grid of three per CU for all 256 CUs stays resident and loads its tables once
    hipLaunchKernelGGL(k_fixed_lane, dim3(gmg_grid(sg->n, FL_LANE_BLOCK, 3 * 256)), dim3(FL_LANE_BLOCK), 0, s, m->a, m->d_mip, m->d_prob,
                       r->d_packed, r->d_off, sg->d_segs, sg->n, lo, hi, d_out);
    GMG_HIP(hipGetLastError());
    return GMG_OK;
}

// ---------------------------------------------------------------------------
// entry points
// ---------------------------------------------------------------------------

extern "C" int gmg_fixed_model_upload(int L, const int32_t *perm, const int16_t *const *mip, const float *const *prob4,
                                      const int *model_depth, const int *num_nodes, gmg_fixed_model **out)
{
    int rc = gmg_enter("gmg_fixed_model_upload");
    if (rc) return rc;
    if (!perm || !mip || !prob4 || !model_depth || !num_nodes || !out)
        return gmg_set_error(GMG_EINVAL, "gmg_fixed_model_upload: NULL argument");
    if (L < 1 || L > GMG_MAX_MODEL_LEN)
        return gmg_set_error(GMG_EBADMODEL, "gmg_fixed_model_upload: length %d outside [1,%d]", L, GMG_MAX_MODEL_LEN);
    FixedArgs a;
    memset(&a, 0, sizeof a);
    a.L = L;
    a.identity = 1;
    bool seen[GMG_MAX_MODEL_LEN] = {false};
    for (int i = 0; i < L; i++) {
        if (perm[i] < 0 || perm[i] >= L || seen[perm[i]])
            return gmg_set_error(GMG_EBADMODEL, "gmg_fixed_model_upload: the permutation is not a bijection of 0..%d (entry %d = %d)",
                                 L - 1, i, (int)perm[i]);
        seen[perm[i]] = true;
        a.perm[i] = perm[i];
        if (perm[i] != i) a.identity = 0;
    }
    uint64_t total = 0;
    int max_depth = 0;
    for (int i = 0; i < L; i++) {
        const int D = model_depth[i], N = num_nodes[i];
        if (!mip[i] || !prob4[i]) return gmg_set_error(GMG_EINVAL, "gmg_fixed_model_upload: NULL table of sub-model %d", i);
        if (D < 0 || D > i || D > 12)
            return gmg_set_error(GMG_EBADMODEL, "gmg_fixed_model_upload: sub-model %d: depth %d outside [0,%d]", i, D, i < 12 ? i : 12);
        long need = 0, pw = 1;
        for (int l = 0; l <= D; l++) { need += pw; pw *= 4; }
        if (N < need)
            return gmg_set_error(GMG_EBADMODEL, "gmg_fixed_model_upload: sub-model %d: num_nodes=%d < %ld needed for depth %d", i, N, need, D);
        for (int k = 0; k < N; k++)
            if (mip[i][k] < -2 || mip[i][k] > i)        // model_len i+1: context positions 0..i
                return gmg_set_error(GMG_EBADMODEL, "gmg_fixed_model_upload: sub-model %d: mut_info_pos %d at node %d outside [-2,%d]",
                                     i, (int)mip[i][k], k, i);
        a.off[i] = (uint32_t)total;
        a.nodes[i] = (uint32_t)N;
        a.depth[i] = D;
        total += (uint64_t)N;
        if (D > max_depth) max_depth = D;
        if (total > 0x7fffffffull) return gmg_set_error(GMG_EBADMODEL, "gmg_fixed_model_upload: %llu nodes", (unsigned long long)total);
    }
    // one blob: the float4 rows first (16-byte aligned), then the int8 mip column
    const size_t bytes = total * sizeof(float4) + total;
    std::vector<unsigned char> h(bytes);
    float *hp = (float *)h.data();
    int8_t *hm = (int8_t *)(h.data() + total * sizeof(float4));
    for (int i = 0; i < L; i++) {
        memcpy(hp + 4 * (size_t)a.off[i], prob4[i], (size_t)a.nodes[i] * 4 * sizeof(float));
        for (uint32_t k = 0; k < a.nodes[i]; k++) hm[a.off[i] + k] = (int8_t)mip[i][k];
    }
    std::unique_ptr<gmg_fixed_model> m(new (std::nothrow) gmg_fixed_model());
    if (!m) return gmg_set_error(GMG_ENOMEM, "gmg_fixed_model_upload: out of host memory");
    m->a = a;
    m->max_depth = max_depth;
    m->total_nodes = total;
    m->blob_bytes = bytes;
    GMG_HIP(m->own.alloc(&m->d_blob, bytes));
    GMG_HIP(hipMemcpy(m->d_blob, h.data(), bytes, hipMemcpyHostToDevice));
    GMG_HANDLE_READY();
    m->d_prob = (float4 *)m->d_blob;
    m->d_mip = (int8_t *)((unsigned char *)m->d_blob + total * sizeof(float4));
    *out = m.release();
    return GMG_OK;
}

extern "C" int gmg_fixed_model_free(gmg_fixed_model *m)
{
    if (!m) return GMG_OK;
    delete m;
    return GMG_OK;
}

extern "C" int gmg_fixed_model_info(const gmg_fixed_model *m, int *length, int *max_depth, uint64_t *table_bytes)
{
    if (!m) return gmg_set_error(GMG_EINVAL, "gmg_fixed_model_info: NULL model");
    if (length) *length = m->a.L;
    if (max_depth) *max_depth = m->max_depth;
    if (table_bytes) *table_bytes = m->blob_bytes;
    return GMG_OK;
}

extern "C" int gmg_fixed_score(const gmg_fixed_model *m, const gmg_reads *reads, const gmg_segments *segs, int lo, int hi,
                               double *d_out, void *stream)
{
    int rc = gmg_enter("gmg_fixed_score");
    if (rc) return rc;
    if (!m || !reads || !segs || (!d_out && segs->n)) return gmg_set_error(GMG_EINVAL, "gmg_fixed_score: NULL argument");
    if (lo < 0 || hi < lo || hi > m->a.L)
        return gmg_set_error(GMG_EINVAL, "gmg_fixed_score: bad range lo = %d hi = %d for length %d", lo, hi, m->a.L);
    if (segs->n == 0) return GMG_OK;
    if (segs->min_len < (uint64_t)m->a.L)
        return gmg_set_error(GMG_ERANGE, "gmg_fixed_score: a segment of %llu bases is shorter than the model's %d",
                             (unsigned long long)segs->min_len, m->a.L);
    return gmg_launch_fixed(m, reads, segs, lo, hi, d_out, (hipStream_t)stream);
}
