// gmg_models.hip -- a batch of binary .icm files parsed and flattened ON THE DEVICE (gmg_model_set_*, include/gmg.h).
//
// gmg_icm_open + gmg_icm_device_model cost a model three fread calls per node, two copies of its tables, a breadth-first
// expansion on the host, a hipMalloc, a synchronous copy from pageable memory and a hipFree.  Here the raw bytes of many files
// go up on the caller's stream into a scratch block of the library's cache, and three kernels leave in ONE block what
// gmg_model_upload would have built, byte for byte:
//   k_ms_ids      a lane per record: is its id 0 (a sub-model starts), where is the first negative id (the stream ends);
//                 the mut_info_pos table filled with -2 (a slot no record names is a cut node)
//   (gmg_scan_excl over the id-0 flags of the whole batch: the sub-model of every record)
//   k_ms_parse    a lane per record: Try_Input's checks, the record scattered to its slot, the exponent range of its values
//   k_ms_flatten  a lane per output element: completed tree (cshift / crow / chalf) by a walk of at most D steps from the root,
//                 the direct tables of tiny models by the plain descents
// Values are moved as 32-bit words, never computed.  Nothing waits before gmg_model_set_finish.
//
// The binary format (src/ICM/icm.cc:614-726): 150 header bytes, six int32 {200, 150, model_len, depth, periodicity, num_nodes},
// then records {int32 id, float prob[4], int16 mut_info_pos} of 22 bytes -- so nothing behind the header is 4-byte aligned.

#include "gmg_internal.h"
#include "gmg_scan.h"

#include <stdio.h>
#include <string.h>
#include <memory>
#include <new>
#include <string>
#include <vector>

#define MS_HEADER 174                                   // ID_STRING_LEN + six int32
#define MS_RECORD 22
#define MS_BLOCK 256
#define MS_MAX_GRID_X 2048

namespace {

// what the kernels know about member k (one array on the device, indexed by blockIdx.y)
struct MsDesc {
    uint64_t file_off;           // the file's bytes inside the staging area
    uint64_t n_bytes;
    uint64_t blob_off;           // the model's blob inside the block
    uint64_t rec_base;           // its first entry in the flag / prefix arrays of the batch
    uint64_t o_prob, o_cshift, o_crow, o_chalf, o_dense, o_part;     // GmgModelLayout (o_mip is 0)
    uint64_t n_flat;             // output elements of k_ms_flatten
    uint32_t max_rec;            // records whose id lies inside the file
    int32_t W, D, P, N;
    uint32_t fast, dense, cstride, ctot, n_leaves, n_dense, n_part;
};

// per member, written by the kernels and read back at _finish
enum { ST_REC_ERR, ST_MIP_ERR, ST_END, ST_ZEROS, ST_MIN_EXP, ST_MAX_EXP, ST_ODD, ST_WORDS = 8 };
enum { ERR_NODE, ERR_PROB, ERR_MIP_READ, ERR_ORDER };   // ST_REC_ERR = 8 * record + one of these, the lowest wins

__device__ __forceinline__ int32_t ms_i32(const unsigned char *p) { int32_t v; __builtin_memcpy(&v, p, 4); return v; }
__device__ __forceinline__ uint32_t ms_u32(const unsigned char *p) { uint32_t v; __builtin_memcpy(&v, p, 4); return v; }
__device__ __forceinline__ int16_t ms_i16(const unsigned char *p) { int16_t v; __builtin_memcpy(&v, p, 2); return v; }

__device__ __forceinline__ uint32_t ms_wave_min(uint32_t x)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { const uint32_t y = __shfl_xor(x, o); x = y < x ? y : x; }
    return x;
}
__device__ __forceinline__ uint32_t ms_wave_max(uint32_t x)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { const uint32_t y = __shfl_xor(x, o); x = y > x ? y : x; }
    return x;
}

// A lane per record of file blockIdx.y: flag[.] = (id == 0), ST_END = the first record with a negative id.  The same lanes fill
// the model's mut_info_pos table with -2.
__global__ __launch_bounds__(MS_BLOCK) void k_ms_ids(const MsDesc *desc, unsigned char *block, const unsigned char *stage, uint32_t *flag,
                                                     uint32_t *status)
{
    const MsDesc &d = desc[blockIdx.y];
    const unsigned char *file = stage + d.file_off;
    const uint32_t t0 = blockIdx.x * MS_BLOCK + threadIdx.x, step = gridDim.x * MS_BLOCK;
    uint32_t end = 0xffffffffu;
    for (uint32_t r = t0; r < d.max_rec; r += step) {
        const int32_t id = ms_i32(file + MS_HEADER + (uint64_t)MS_RECORD * r);
        flag[d.rec_base + r] = id == 0;
        if (id < 0 && r < end) end = r;
    }
    end = ms_wave_min(end);
    if ((threadIdx.x & 63u) == 0 && end != 0xffffffffu) atomicMin(&status[blockIdx.y * ST_WORDS + ST_END], end);
    const uint64_t PN = (uint64_t)d.P * d.N;
    uint32_t *mip4 = (uint32_t *)(block + d.blob_off);  // (256-byte aligned)
    for (uint64_t i = t0; i < PN / 4; i += step) mip4[i] = 0xfefefefeu;
    if (t0 < (PN & 3)) block[d.blob_off + (PN & ~(uint64_t)3) + t0] = 0xfe;
}

// A lane per record before the end of the stream: Try_Input's checks in its order, then the record goes to slot period * N + id.
__global__ __launch_bounds__(MS_BLOCK) void k_ms_parse(const MsDesc *desc, unsigned char *block, const unsigned char *stage, const uint32_t *flag,
                                                       const uint32_t *pref, uint32_t *status)
{
    const MsDesc &d = desc[blockIdx.y];
    const unsigned char *file = stage + d.file_off;
    uint32_t *st = status + blockIdx.y * ST_WORDS;
    const uint32_t end = st[ST_END];                    // (k_ms_ids has finished)
    const uint32_t zeros_before = pref[d.rec_base];
    int8_t *mip = (int8_t *)(block + d.blob_off);
    uint32_t *prob = (uint32_t *)(block + d.blob_off + d.o_prob);
    uint32_t rec_err = 0xffffffffu, mip_err = 0xffffffffu, min_exp = 255, max_exp = 0, odd = 0;
    for (uint32_t r = blockIdx.x * MS_BLOCK + threadIdx.x; r < end; r += gridDim.x * MS_BLOCK) {
        const uint64_t at = MS_HEADER + (uint64_t)MS_RECORD * r;
        const int32_t id = ms_i32(file + at);           // >= 0: the record lies before the end
        const int64_t period = (int64_t)(pref[d.rec_base + r] + flag[d.rec_base + r] - zeros_before) - 1;
        if (r == end - 1) st[ST_ZEROS] = (uint32_t)(period + 1);
        uint32_t kind = 0xffffffffu;
        if (period < 0 || period >= d.P || id >= d.N) kind = ERR_NODE;
        else if (at + 20 > d.n_bytes) kind = ERR_PROB;
        else if (at + 22 > d.n_bytes) kind = ERR_MIP_READ;
        else if (id != 0 && id <= ms_i32(file + at - MS_RECORD)) kind = ERR_ORDER;     // (id != 0 and period >= 0: r > 0)
        if (kind != 0xffffffffu) {
            const uint32_t key = r * 8 + kind;
            if (key < rec_err) rec_err = key;
            continue;
        }
        const int m = ms_i16(file + at + 20);
        if (m < -2 || m > d.W - 1) {
            if (r < mip_err) mip_err = r;
            continue;
        }
        const uint64_t slot = (uint64_t)period * d.N + (uint32_t)id;
        mip[slot] = (int8_t)m;
        uint4 v;
        v.x = ms_u32(file + at + 4); v.y = ms_u32(file + at + 8); v.z = ms_u32(file + at + 12); v.w = ms_u32(file + at + 16);
        *(uint4 *)(prob + 4 * slot) = v;
        if (m == -2) continue;                          // (a cut node's values are never read: gmg_model_upload leaves them out)
        const uint32_t b4[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const uint32_t b = b4[k], ex = (b >> 23) & 0xffu;
            if ((b << 1) == 0) continue;
            if ((b >> 31) == 0 || ex == 0 || ex == 255) odd = 1;
            min_exp = ex < min_exp ? ex : min_exp;
            max_exp = ex > max_exp ? ex : max_exp;
        }
    }
    // (every lane of a wave works on the same file: one atomic per wave and word, and only where there is something to say)
    rec_err = ms_wave_min(rec_err);
    mip_err = ms_wave_min(mip_err);
    min_exp = ms_wave_min(min_exp);
    max_exp = ms_wave_max(max_exp);
    odd = ms_wave_max(odd);
    if ((threadIdx.x & 63u) == 0) {
        if (rec_err != 0xffffffffu) atomicMin(&st[ST_REC_ERR], rec_err);
        if (mip_err != 0xffffffffu) atomicMin(&st[ST_MIP_ERR], mip_err);
        if (min_exp != 255) atomicMin(&st[ST_MIN_EXP], min_exp);
        if (max_exp != 0) atomicMax(&st[ST_MAX_EXP], max_exp);
        if (odd) atomicOr(&st[ST_ODD], 1u);
    }
}

__device__ __forceinline__ int ms_parent(int x) { return (x - 1) / 4; }     // src/ICM/icm.hh:84, C truncation

// dense_entry / dense_part_entry of gmg_api.hip on the device tables: the row index and the base it predicts
__device__ __forceinline__ uint32_t ms_dense_entry(const int8_t *mip, const uint32_t *prob, int W, int D, uint32_t idx)
{
    int node = 0;
    for (int i = 0; i < D; i++) {
        const int pos = mip[node];
        if (pos == -1) break;
        if (pos < -1) { node = ms_parent(node); break; }
        node = 4 * node + (int)((idx >> (2 * pos)) & 3) + 1;
    }
    if (mip[node] < -1) node = ms_parent(node);
    return prob[4 * (size_t)node + ((idx >> (2 * (W - 1))) & 3)];
}

__device__ __forceinline__ uint32_t ms_dense_part_entry(const int8_t *mip, const uint32_t *prob, int W, int D, int j, uint32_t idx)
{
    int node = 0;
    const int start = j - (W - 1);
    for (int i = 0; i < D; i++) {
        const int q = start + mip[node];
        if (q < 0) break;
        node = 4 * node + (int)((idx >> (2 * q)) & 3) + 1;
    }
    if (mip[node] == -2) node = ms_parent(node);
    return prob[4 * (size_t)node + ((idx >> (2 * j)) & 3)];
}

// A lane per output element of model blockIdx.y: [P][ctot] completed-tree nodes (fast shapes), then [P][4^W] full windows and
// [P][(4^W - 4) / 3] partial windows (tiny shapes).  Node (level l, index i) of the completed tree is reached from the root along
// the l base-4 digits of i, first step = highest digit -- complete_tree of gmg_api.hip without its queue: an original node with a
// position hands on to its child; a node without one (mip -1) or a cut node (-2: its parent's row) stops the walk, everything
// below it repeats that row and has cshift 0.  Every index depends on the digits alone: 4 * node + 1 + b < num_nodes for D steps.
__global__ __launch_bounds__(MS_BLOCK) void k_ms_flatten(const MsDesc *desc, unsigned char *block)
{
    const MsDesc &d = desc[blockIdx.y];
    unsigned char *blob = block + d.blob_off;
    const uint64_t n_tree = d.fast ? (uint64_t)d.P * d.ctot : 0, n_full = (uint64_t)d.P * d.n_dense;
    for (uint64_t e = (uint64_t)blockIdx.x * MS_BLOCK + threadIdx.x; e < d.n_flat; e += (uint64_t)gridDim.x * MS_BLOCK) {
        if (e < n_tree) {
            const uint32_t p = (uint32_t)(e / d.ctot), c = (uint32_t)(e % d.ctot);
            int l = 0;
            uint32_t base = 0, size = 1;
            while (c >= base + size) { base += size; size *= 4; l++; }
            const uint32_t i = c - base;
            const int8_t *mip = (const int8_t *)blob + (size_t)p * d.N;
            const uint4 *prob = (const uint4 *)(blob + d.o_prob) + (size_t)p * d.N;
            int node = 0, row = -1;
            for (int t = 0; t < l && row < 0; t++) {
                const int m = mip[node];
                if (m >= 0) node = 4 * node + 1 + (int)((i >> (2 * (l - 1 - t))) & 3);
                else row = m == -2 ? ms_parent(node) : node;
            }
            uint32_t shift = 0;
            if (row < 0) {                              // the walk arrived on an original node
                const int m = mip[node];
                row = m == -2 ? ms_parent(node) : node;
                if (m >= 0) shift = 2u * (uint32_t)m;
            }
            const uint4 v = prob[row];
            ((uint4 *)(blob + d.o_crow))[(size_t)p * d.ctot + c] = v;
            if (l < d.D) blob[d.o_cshift + (size_t)p * d.cstride + c] = (unsigned char)shift;
            else {                                      // a leaf: its values once more, split in halves (GmgDevModel::chalf)
                uint2 *half = (uint2 *)(blob + d.o_chalf) + (size_t)p * d.n_leaves * 2;
                half[i] = make_uint2(v.x, v.y);
                half[d.n_leaves + i] = make_uint2(v.z, v.w);
            }
        } else if (e - n_tree < n_full) {
            const uint64_t k = e - n_tree;
            const uint32_t p = (uint32_t)(k / d.n_dense), idx = (uint32_t)(k % d.n_dense);
            ((uint32_t *)(blob + d.o_dense))[k] = ms_dense_entry((const int8_t *)blob + (size_t)p * d.N, (const uint32_t *)(blob + d.o_prob) + 4 * (size_t)p * d.N, d.W, d.D, idx);
        } else {
            const uint64_t k = e - n_tree - n_full;
            const uint32_t p = (uint32_t)(k / d.n_part);
            uint32_t idx = (uint32_t)(k % d.n_part);
            int j = 0;
            for (uint32_t cnt = 4; idx >= cnt; cnt *= 4) { idx -= cnt; j++; }         // position j holds 4^(j+1) entries
            ((uint32_t *)(blob + d.o_part))[k] = ms_dense_part_entry((const int8_t *)blob + (size_t)p * d.N, (const uint32_t *)(blob + d.o_prob) + 4 * (size_t)p * d.N, d.W, d.D, j, idx);
        }
    }
}

size_t ms_align(size_t x, size_t a) { return (x + a - 1) / a * a; }

int32_t host_i32(const unsigned char *p) { int32_t v; memcpy(&v, p, 4); return v; }

// the header of a binary .icm as ICM_t::Try_Input reads it (host/icm.cc); the message goes to `msg`
bool header_info(const unsigned char *b, uint64_t n, int param[6], char *msg, size_t msg_len)
{
    if (!b || n < 150) { snprintf(msg, msg_len, "ERROR reading ICM header"); return false; }
    if (n < MS_HEADER) { snprintf(msg, msg_len, "ERROR reading parameters"); return false; }
    for (int k = 0; k < 6; k++) param[k] = host_i32(b + 150 + 4 * k);
    if (param[0] != 200) { snprintf(msg, msg_len, "Bad ICM version = %d  should be %d", param[0], 200); return false; }
    if (param[1] != 150) { snprintf(msg, msg_len, "Bad ID_STRING_LEN = %d  should be %d", param[1], 150); return false; }
    if (param[2] <= 0 || param[3] < 0 || param[4] <= 0 || param[5] <= 0) { snprintf(msg, msg_len, "ERROR:  bad ICM parameters"); return false; }
    return true;
}

// gmg_model_upload's shape checks, with its messages
bool shape_ok(int W, int D, int P, int N, char *msg, size_t msg_len)
{
    if (W < 1 || W > GMG_MAX_MODEL_LEN || D < 0 || D > 12 || P < 1 || N < 1) {
        snprintf(msg, msg_len, "gmg_model_upload: unsupported shape len=%d depth=%d period=%d nodes=%d", W, D, P, N);
        return false;
    }
    long need = 0, pw = 1;
    for (int l = 0; l <= D; l++) { need += pw; pw *= 4; }
    if (N < need) { snprintf(msg, msg_len, "gmg_model_upload: num_nodes=%d < %ld needed for depth %d", N, need, D); return false; }
    return true;
}

}  // namespace

struct GMG_HIDDEN gmg_model_set {
    int n = 0;
    hipStream_t stream;
    unsigned char *d_block = nullptr;    // descriptors, status words, every blob
    size_t status_off = 0;
    std::vector<gmg_model> models;
    std::vector<MsDesc> desc;
    std::vector<const unsigned char *> bytes;           // the caller's buffers: read again for the message of a refusal
    std::vector<unsigned char> h_head;                  // descriptors + initial status words as they went up
    std::vector<uint32_t> h_status;
    bool finished = false;
    int rc = GMG_OK, bad_file = -1;
    std::string message;
    GmgScratch own;              // the block is free once what is queued on the load stream when the set goes has run
    explicit gmg_model_set(hipStream_t s) : stream(s), own(GmgScratch::AFTER, s) {}
};

extern "C" int gmg_icm_bytes_info(const void *bytes, uint64_t n_bytes, int *model_len, int *model_depth, int *periodicity, int *num_nodes,
                                  uint64_t *blob_bytes)
{
    int param[6];
    char msg[200];
    if (!header_info((const unsigned char *)bytes, n_bytes, param, msg, sizeof msg)) return gmg_set_error(GMG_EBADMODEL, "%s", msg);
    if (model_len) *model_len = param[2];
    if (model_depth) *model_depth = param[3];
    if (periodicity) *periodicity = param[4];
    if (num_nodes) *num_nodes = param[5];
    if (blob_bytes) {
        if (!shape_ok(param[2], param[3], param[4], param[5], msg, sizeof msg)) return gmg_set_error(GMG_EBADMODEL, "%s", msg);
        GmgModelLayout lay;
        gmg_model_layout(param[2], param[3], param[4], param[5], &lay);
        *blob_bytes = lay.total;
    }
    return GMG_OK;
}

extern "C" int gmg_model_set_load(const void *const *bytes, const uint64_t *n_bytes, int n_files, gmg_model_set **out, void *stream)
{
    int rc = gmg_enter("gmg_model_set_load");
    if (rc) return rc;
    if (!bytes || !n_bytes || !out || n_files < 1 || n_files > 65535)
        return gmg_set_error(GMG_EINVAL, "gmg_model_set_load: bad argument (1 .. 65535 files per call)");
    hipStream_t s = (hipStream_t)stream;
    gmg_model_set *set = new (std::nothrow) gmg_model_set(s);
    if (!set) return gmg_set_error(GMG_ENOMEM, "gmg_model_set_load: out of host memory");
    std::unique_ptr<gmg_model_set> own(set);            // until the caller has it
    set->n = n_files;
    set->models.resize(n_files);
    set->desc.resize(n_files);
    set->bytes.resize(n_files);

    // ---- host: the 24 header bytes of every file, the layout of the block ----
    const size_t desc_bytes = ms_align((size_t)n_files * sizeof(MsDesc), 256);
    const size_t head_bytes = desc_bytes + ms_align((size_t)n_files * ST_WORDS * 4, 256);
    set->status_off = desc_bytes;
    set->h_head.assign(head_bytes, 0);
    uint32_t *st0 = (uint32_t *)(set->h_head.data() + desc_bytes);
    bool contiguous = true;
    size_t at = head_bytes;
    uint64_t total_rec = 0;
    std::vector<GmgModelLayout> lay(n_files);
    for (int k = 0; k < n_files; k++) {
        int param[6];
        char msg[200];
        const unsigned char *b = (const unsigned char *)bytes[k];
        if (!header_info(b, n_bytes[k], param, msg, sizeof msg) || !shape_ok(param[2], param[3], param[4], param[5], msg, sizeof msg))
            return gmg_set_error(GMG_EBADMODEL, "%s (file %d of the batch)", msg, k);
        if (n_bytes[k] >= (1ull << 31) || (uint64_t)param[4] * param[5] >= (1ull << 31))
            return gmg_set_error(GMG_EBADMODEL, "gmg_model_set_load: file %d of the batch is too large for the device loader (2 GiB, 2^31 slots)", k);
        set->bytes[k] = b;
        if (k && b != (const unsigned char *)bytes[k - 1] + n_bytes[k - 1]) contiguous = false;
        MsDesc &d = set->desc[k];
        memset(&d, 0, sizeof d);
        d.W = param[2]; d.D = param[3]; d.P = param[4]; d.N = param[5];
        gmg_model_layout(d.W, d.D, d.P, d.N, &lay[k]);
        const GmgModelLayout &l = lay[k];
        d.n_bytes = n_bytes[k];
        d.blob_off = at;
        at += l.total;                                  // (a multiple of 256)
        d.o_prob = l.o_prob; d.o_cshift = l.o_cshift; d.o_crow = l.o_crow; d.o_chalf = l.o_chalf; d.o_dense = l.o_dense; d.o_part = l.o_part;
        d.fast = l.fast; d.dense = l.dense; d.cstride = (uint32_t)l.cstride; d.ctot = (uint32_t)l.ctot; d.n_leaves = (uint32_t)l.n_leaves;
        d.n_dense = (uint32_t)l.n_dense; d.n_part = (uint32_t)l.n_part;
        d.n_flat = (l.fast ? (uint64_t)d.P * l.ctot : 0) + (uint64_t)d.P * (l.n_dense + l.n_part);
        d.max_rec = n_bytes[k] >= MS_HEADER + 4 ? (uint32_t)((n_bytes[k] - MS_HEADER - 4) / MS_RECORD + 1) : 0;
        d.rec_base = total_rec;
        total_rec += d.max_rec;
        uint32_t *st = st0 + (size_t)k * ST_WORDS;
        st[ST_REC_ERR] = st[ST_MIP_ERR] = 0xffffffffu;
        st[ST_END] = d.max_rec;
        st[ST_MIN_EXP] = 255;
    }
    // the staged files and the scan's arrays are needed only until the kernels have run: a block of their own, given back below
    const size_t blobs_end = at;
    size_t sat = 0;
    for (int k = 0; k < n_files; k++) {
        MsDesc &d = set->desc[k];
        if (contiguous) d.file_off = (uint64_t)(set->bytes[k] - set->bytes[0]);       // as they lie at the caller's: one copy
        else { d.file_off = sat; sat += ms_align((size_t)d.n_bytes, 16); }
    }
    if (contiguous) sat = ms_align((size_t)(set->desc[n_files - 1].file_off + n_bytes[n_files - 1]), 16);
    const size_t flag_off = sat = ms_align(sat, 256);
    const size_t pref_off = sat = ms_align(sat + (size_t)(total_rec + 4) * 4, 256);
    sat += (size_t)(total_rec + 4) * 4;
    memcpy(set->h_head.data(), set->desc.data(), (size_t)n_files * sizeof(MsDesc));

    // ---- device: everything queued on the caller's stream ----
    // (a failure waits for the stream before the blocks go back; on success the set takes the block and the staging block goes back
    // once the kernels queued here have run)
    GmgScratch sc(GmgScratch::STREAM, s);
    unsigned char *blk = nullptr, *scratch = nullptr;
    if (sc.alloc(&blk, blobs_end) != hipSuccess || sc.alloc(&scratch, sat) != hipSuccess)
        return gmg_set_error(GMG_ENOMEM, "gmg_model_set_load: no device memory for %zu + %zu bytes", blobs_end, sat);
    GMG_HIP(hipMemcpyAsync(blk, set->h_head.data(), head_bytes, hipMemcpyHostToDevice, s));
    GMG_HIP(hipMemsetAsync(blk + head_bytes, 0, blobs_end - head_bytes, s));
    if (contiguous)
        GMG_HIP(hipMemcpyAsync(scratch, set->bytes[0], (size_t)(set->desc[n_files - 1].file_off + n_bytes[n_files - 1]), hipMemcpyHostToDevice, s));
    else
        for (int k = 0; k < n_files; k++)
            GMG_HIP(hipMemcpyAsync(scratch + set->desc[k].file_off, set->bytes[k], (size_t)n_bytes[k], hipMemcpyHostToDevice, s));
    uint32_t max_rec = 0;
    uint64_t max_fill = 0, max_flat = 0;
    for (const MsDesc &d : set->desc) {
        max_rec = d.max_rec > max_rec ? d.max_rec : max_rec;
        const uint64_t fill = ((uint64_t)d.P * d.N + 3) / 4;
        max_fill = fill > max_fill ? fill : max_fill;
        max_flat = d.n_flat > max_flat ? d.n_flat : max_flat;
    }
    auto grid_x = [](uint64_t items) {
        const uint64_t b = (items + MS_BLOCK - 1) / MS_BLOCK;
        return (unsigned)(b < 1 ? 1 : b > MS_MAX_GRID_X ? MS_MAX_GRID_X : b);
    };
    const MsDesc *d_desc = (const MsDesc *)blk;
    uint32_t *d_status = (uint32_t *)(blk + set->status_off), *d_flag = (uint32_t *)(scratch + flag_off), *d_pref = (uint32_t *)(scratch + pref_off);
    hipLaunchKernelGGL(k_ms_ids, dim3(grid_x(max_rec > max_fill ? max_rec : max_fill), n_files), dim3(MS_BLOCK), 0, s, d_desc, blk, scratch, d_flag,
                       d_status);
    GMG_HIP(hipGetLastError());
    // (one entry more than there are records: pref[rec_base] of a last file without records is read too)
    GMG_HIP(hipMemsetAsync(d_flag + total_rec, 0, 16, s));
    GMG_HIP((gmg_scan_excl<uint32_t, uint32_t>(d_flag, d_pref, total_rec + 1, s)));
    hipLaunchKernelGGL(k_ms_parse, dim3(grid_x(max_rec), n_files), dim3(MS_BLOCK), 0, s, d_desc, blk, scratch, (const uint32_t *)d_flag,
                       (const uint32_t *)d_pref, d_status);
    GMG_HIP(hipGetLastError());
    if (max_flat) {
        hipLaunchKernelGGL(k_ms_flatten, dim3(grid_x(max_flat), n_files), dim3(MS_BLOCK), 0, s, d_desc, blk);
        GMG_HIP(hipGetLastError());
    }
    set->d_block = set->own.take(sc, blk);
    sc.wait = GmgScratch::AFTER;
    for (int k = 0; k < n_files; k++) {
        const MsDesc &d = set->desc[k];
        gmg_model &m = set->models[k];
        m.min_exp = 255; m.max_exp = 0; m.odd_values = 0;           // (known at _finish)
        gmg_model_bind(&m, blk + d.blob_off, d.W, d.D, d.P, d.N, lay[k]);
    }
    *out = own.release();
    return GMG_OK;
}

// the message of member k's refusal, from its status words and the caller's bytes (the host reads records only here)
static void refusal_message(const gmg_model_set *set, int k, char *msg, size_t msg_len)
{
    const MsDesc &d = set->desc[k];
    const uint32_t *st = set->h_status.data() + (size_t)k * ST_WORDS;
    const unsigned char *rec0 = set->bytes[k] + MS_HEADER;
    auto period_of = [&](uint32_t r) {
        int period = -1;
        for (uint32_t q = 0; q <= r; q++) period += host_i32(rec0 + (size_t)MS_RECORD * q) == 0;
        return period;
    };
    if (st[ST_REC_ERR] != 0xffffffffu) {
        const uint32_t r = st[ST_REC_ERR] / 8, kind = st[ST_REC_ERR] % 8;
        const int id = host_i32(rec0 + (size_t)MS_RECORD * r), period = period_of(r);
        if (kind == ERR_MIP_READ) snprintf(msg, msg_len, "ERROR reading mut_info_pos for node = %d  period = %d", id, period);
        else if (kind == ERR_ORDER)
            snprintf(msg, msg_len, "gmg_model_set_load: node %d follows node %d in sub-model %d: ids must increase inside a sub-model "
                     "(the device loader scatters records, it has no last writer); load this file with gmg_icm_open",
                     id, host_i32(rec0 + (size_t)MS_RECORD * (r - 1)), period);
        else snprintf(msg, msg_len, "ERROR reading icm node = %d  period = %d", id, period);
    } else if ((int64_t)st[ST_ZEROS] < d.P) snprintf(msg, msg_len, "ERROR:  Too few nodes for periodicity = %d", d.P);
    else {
        const uint32_t r = st[ST_MIP_ERR];
        const unsigned char *rec = rec0 + (size_t)MS_RECORD * r;
        int16_t m;
        memcpy(&m, rec + 20, 2);
        snprintf(msg, msg_len, "gmg_model_upload: mut_info_pos %d at slot %zu outside [-2,%d]", (int)m,
                 (size_t)period_of(r) * d.N + (size_t)host_i32(rec), d.W - 1);
    }
}

extern "C" int gmg_model_set_finish(gmg_model_set *set, int *bad_file)
{
    int rc = gmg_enter("gmg_model_set_finish");
    if (rc) return rc;
    if (!set) return gmg_set_error(GMG_EINVAL, "gmg_model_set_finish: NULL set");
    if (!set->finished) {
        set->h_status.assign((size_t)set->n * ST_WORDS, 0);
        GMG_HIP(hipMemcpyAsync(set->h_status.data(), set->d_block + set->status_off, set->h_status.size() * 4, hipMemcpyDeviceToHost, set->stream));
        GMG_HIP(hipStreamSynchronize(set->stream));
        set->finished = true;
        for (int k = 0; k < set->n; k++) {
            const uint32_t *st = set->h_status.data() + (size_t)k * ST_WORDS;
            if (st[ST_REC_ERR] != 0xffffffffu || (int64_t)st[ST_ZEROS] < set->desc[k].P || st[ST_MIP_ERR] != 0xffffffffu) {
                if (set->rc == GMG_OK) {
                    char msg[400];
                    refusal_message(set, k, msg, sizeof msg);
                    set->rc = GMG_EBADMODEL;
                    set->bad_file = k;
                    set->message = msg;
                }
                continue;
            }
            set->models[k].min_exp = (int)st[ST_MIN_EXP];
            set->models[k].max_exp = (int)st[ST_MAX_EXP];
            set->models[k].odd_values = (int)st[ST_ODD];
        }
    }
    if (bad_file) *bad_file = set->bad_file;
    if (set->rc != GMG_OK) return gmg_set_error(set->rc, "%s", set->message.c_str());
    return GMG_OK;
}

extern "C" const gmg_model *gmg_model_set_model(const gmg_model_set *set, int k)
{
    if (!set || k < 0 || k >= set->n) { gmg_set_error(GMG_EINVAL, "gmg_model_set_model: no member %d", k); return nullptr; }
    if (!set->finished || set->rc != GMG_OK) {
        gmg_set_error(GMG_EINVAL, "gmg_model_set_model: %s", set->finished ? "the set was refused" : "gmg_model_set_finish has not been called");
        return nullptr;
    }
    return &set->models[k];
}

extern "C" int gmg_model_set_free(gmg_model_set *set)
{
    if (!set) return GMG_OK;
    // The block may be handed out again once the load stream reaches this point.  What scores with the models was queued by the
    // caller, by default on the null stream: the load stream is made to wait for that one too, on the device -- the host does not
    // block.  (A set used on further streams is the caller's to wait for, as with gmg_model_free.)
    if (!set->finished) (void)hipStreamSynchronize(set->stream);           // (the status copy of a _finish never made: nothing reads h_status later)
    hipEvent_t ev = nullptr;
    if (set->stream != nullptr) {
        if (hipEventCreateWithFlags(&ev, hipEventDisableTiming) == hipSuccess && hipEventRecord(ev, 0) == hipSuccess &&
            hipStreamWaitEvent(set->stream, ev, 0) == hipSuccess) { /* ordered on the device */ }
        else (void)hipStreamSynchronize(0);
        if (ev) (void)hipEventDestroy(ev);
    }
    delete set;
    return GMG_OK;
}

extern "C" int gmg_model_blob(const gmg_model *m, void *dst, size_t *bytes)
{
    int rc = gmg_enter("gmg_model_blob");
    if (rc) return rc;
    if (!m || !bytes) return gmg_set_error(GMG_EINVAL, "gmg_model_blob: NULL argument");
    if (dst) {
        if (*bytes < m->blob_bytes) return gmg_set_error(GMG_EINVAL, "gmg_model_blob: %zu bytes given, the blob has %zu", *bytes, m->blob_bytes);
        GMG_HIP(hipMemcpy(dst, m->d_blob, m->blob_bytes, hipMemcpyDeviceToHost));
    }
    *bytes = m->blob_bytes;
    return GMG_OK;
}

extern "C" int gmg_model_value_stats(const gmg_model *m, int *min_exp, int *max_exp, int *odd_values)
{
    if (!m) return gmg_set_error(GMG_EINVAL, "gmg_model_value_stats: NULL model");
    if (min_exp) *min_exp = m->min_exp;
    if (max_exp) *max_exp = m->max_exp;
    if (odd_values) *odd_values = m->odd_values;
    return GMG_OK;
}
