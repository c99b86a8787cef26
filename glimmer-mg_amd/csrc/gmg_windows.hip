// gmg_windows.hip -- gmg_window_counts and gmg_regions_uncovered (include/gmg.h): the composition of every sliding
// window of every read (src/Util/window-acgt.cc:63-137) and the stretches of every read that a list of intervals leaves uncovered
// (src/Util/uncovered.cc:186-288).  Everything they produce is an integer.
//
// gmg_window_counts.  A window's c, g and t counts are differences of running counts, so no base is looked at once per window:
//   k_win_blocks   the c / g / t counts of every block of 64 bases (four packed words, three masked population counts a word)
//   gmg_scan_excl  their exclusive sums over the whole batch, 32 bits each: a window is shorter than 2^31 bases, so the difference
//                  of two sums is right although the sums themselves wrap
//   k_win_reads    the number of windows of every read (closed form of the reference's ring buffer), then their exclusive sums:
//                  read_window_off -- the one value the host waits for is its last entry
//   k_win_rows     a lane per row, a work-group per 256 consecutive rows: the group finds the reads of its first and last row once
//                  (two 64-ary searches by wave 0), a lane bisects between them; F (p) = the block's running count + the masked
//                  population count of the block's words in front of p, row = F (end) - F (start).  The rows of a group are
//                  consecutive in the table: they go through LDS and leave as full lines, not as 20-byte pieces.
// Whatever W and S are, a row costs two blocks' words and running counts, and neighbouring rows share them in cache.
// Letters outside acgtACGT: the caller's ascending list of job-wide indices.  k_win_amb looks the packed code of each up, three more
// scans give the running counts per code over the LIST; the group narrows the list to the bases of its rows once, a lane bisects
// in that part for its window's two ends: other = the difference of the places, and what the listed bases added to c / g / t is
// taken off again.  a = length - c - g - t - other.
//
// gmg_regions_uncovered.  A sort by (read, lo) (hipcub radix sort of 64-bit keys, hi as the value); the running maximum of hi per
// read is ONE plain running maximum of read << 32 | hi, since reads ascend; interval i of the sorted list opens a gap when its lo
// exceeds the maximum in front of it, every read one more behind its last interval.  Interval i of read r is item i + r, read r's
// tail the item behind its last interval: flags, scan, write.  Nothing touches the bases.

#include "gmg_internal.h"

#include "gmg_device.h"
#include "gmg_scan.h"

#include <hipcub/hipcub.hpp>
#include <new>

#define WN_BLOCK 256
#define WN_GRID_CAP (256 * 32)

struct GMG_HIDDEN gmg_windows {
    uint64_t *d_off = nullptr;           // n_reads + 1
    int32_t *d_counts = nullptr;         // [n_windows][5]
    uint64_t n_reads = 0, n_windows = 0;
    hipStream_t s;
    GmgScratch own;                      // the blocks are free once what is queued on s when the handle goes has run
    explicit gmg_windows(hipStream_t stream) : s(stream), own(GmgScratch::AFTER, stream) {}
};

struct GMG_HIDDEN gmg_gaps {
    gmg_gene_region *d_gaps = nullptr;
    uint64_t *d_off = nullptr;           // n_reads + 1
    uint64_t n_reads = 0, n_gaps = 0;
    hipStream_t s;
    GmgScratch own;                      // (as gmg_windows)
    explicit gmg_gaps(hipStream_t stream) : s(stream), own(GmgScratch::AFTER, stream) {}
};

// c, g, t among the 2-bit fields of w
__device__ __forceinline__ void wn_word_counts(uint32_t w, uint32_t &c, uint32_t &g, uint32_t &t)
{
    const uint32_t lo = w & 0x55555555u, hi = (w >> 1) & 0x55555555u;
    t += (uint32_t)__popc(lo & hi);
    g += (uint32_t)__popc(hi & ~lo);
    c += (uint32_t)__popc(lo & ~hi);
}

__global__ __launch_bounds__(WN_BLOCK) void k_win_blocks(const uint32_t *__restrict__ packed, uint64_t n_words, uint64_t n_blocks,
                                                        uint32_t *__restrict__ bc, uint32_t *__restrict__ bg, uint32_t *__restrict__ bt)
{
    for (uint64_t b = (uint64_t)blockIdx.x * WN_BLOCK + threadIdx.x; b < n_blocks; b += (uint64_t)gridDim.x * WN_BLOCK) {
        uint32_t c = 0, g = 0, t = 0;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const uint64_t w = 4 * b + k;
            if (w < n_words) wn_word_counts(packed[w], c, g, t);
        }
        bc[b] = c; bg[b] = g; bt[b] = t;
    }
}

// windows of a read of L bases (include/gmg.h)
__device__ __forceinline__ uint32_t wn_n_windows(uint64_t L, uint64_t W, uint64_t S)
{
    if (L == 0) return 0;
    if (L < W) return 1;
    const uint64_t k = (L - W) / S;
    return (uint32_t)(k + 1 + (((L - W) % S != 0 && (k + 1) * S < L) ? 1 : 0));      // (k + 1) S <= L - W + S: no overflow
}

// stats[0]: the first read of 2^31 bases or more
__global__ __launch_bounds__(WN_BLOCK) void k_win_reads(const uint64_t *__restrict__ off, uint64_t n_reads, uint64_t W, uint64_t S,
                                                       uint32_t *__restrict__ cnt, unsigned long long *__restrict__ stats)
{
    for (uint64_t r = (uint64_t)blockIdx.x * WN_BLOCK + threadIdx.x; r <= n_reads; r += (uint64_t)gridDim.x * WN_BLOCK) {
        uint32_t n = 0;
        if (r < n_reads) {
            const uint64_t L = off[r + 1] - off[r];
            if (L >= 0x80000000ull) atomicMin(&stats[0], (unsigned long long)r);
            else n = wn_n_windows(L, W, S);
        }
        cnt[r] = n;                                                     // (cnt[n_reads] = 0: the scan's last output is the total)
    }
}

// the packed code of every listed base, as three flags
__global__ __launch_bounds__(WN_BLOCK) void k_win_amb(const uint32_t *__restrict__ packed, const uint64_t *__restrict__ amb, uint64_t n_amb,
                                                     uint32_t *__restrict__ fc, uint32_t *__restrict__ fg, uint32_t *__restrict__ ft)
{
    for (uint64_t i = (uint64_t)blockIdx.x * WN_BLOCK + threadIdx.x; i <= n_amb; i += (uint64_t)gridDim.x * WN_BLOCK) {
        const int code = i < n_amb ? dev_code(packed, amb[i]) : 0;
        fc[i] = code == 1; fg[i] = code == 2; ft[i] = code == 3;
    }
}

struct WnSums {
    const uint32_t *packed;
    uint64_t n_words;
    const uint32_t *pc, *pg, *pt;        // running counts in front of every block of 64 bases
};

// c, g, t among the job-wide bases [0, p), modulo 2^32
__device__ __forceinline__ void wn_front(const WnSums &q, uint64_t p, uint32_t &c, uint32_t &g, uint32_t &t)
{
    const uint64_t b = p >> 6;
    const unsigned in = (unsigned)(p & 63);
    c = q.pc[b]; g = q.pg[b]; t = q.pt[b];
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const unsigned have = in > 16u * k ? in - 16u * k : 0u;         // bases of word k in front of p
        const uint64_t w = 4 * b + k;
        if (have && w < q.n_words) {
            const uint32_t mask = have >= 16 ? 0xffffffffu : (1u << (2 * have)) - 1u;
            wn_word_counts(q.packed[w] & mask, c, g, t);
        }
    }
}

__global__ __launch_bounds__(WN_BLOCK) void k_win_rows(WnSums q, const uint64_t *__restrict__ off, uint64_t n_reads,
                                                      const uint64_t *__restrict__ row_off, uint64_t n_rows, uint64_t W, uint64_t S,
                                                      const uint64_t *__restrict__ amb, uint64_t n_amb, const uint32_t *__restrict__ ac,
                                                      const uint32_t *__restrict__ ag, const uint32_t *__restrict__ at, int32_t *__restrict__ out)
{
    __shared__ uint64_t s_r[2], s_pos[2], s_amb[2];
    __shared__ int32_t s_out[WN_BLOCK * 5];
    const int tid = threadIdx.x, lane = tid & 63;
    const uint64_t n_groups = (n_rows + WN_BLOCK - 1) / WN_BLOCK;
    for (uint64_t grp = blockIdx.x; grp < n_groups; grp += gridDim.x) {
        const uint64_t j0 = grp * WN_BLOCK, rows = n_rows - j0 < WN_BLOCK ? n_rows - j0 : WN_BLOCK, j = j0 + (uint64_t)tid;
        const bool active = (uint64_t)tid < rows;
        __syncthreads();                                                // (the round before has read s_out, s_r, s_amb)
        if (tid < 64) {
            // the read of row x: the last r with row_off[r] <= x = (the first r with row_off[r] >= x + 1) - 1
            const uint64_t a = dev_wave_lower_bound(row_off, n_reads + 1, j0 + 1, lane) - 1;
            const uint64_t b = dev_wave_lower_bound(row_off, n_reads + 1, j0 + rows, lane) - 1;
            if (lane == 0) { s_r[0] = a; s_r[1] = b; }
        }
        __syncthreads();
        uint64_t s = 0, e = 0;
        if (active) {
            // the last r in [s_r[0], s_r[1]] with row_off[r] <= j
            uint64_t lo = s_r[0], hi = s_r[1];
            while (lo < hi) {
                const uint64_t m = (lo + hi + 1) >> 1;
                if (row_off[m] <= j) lo = m;
                else hi = m - 1;
            }
            const uint64_t base = off[lo], L = off[lo + 1] - base, p = (j - row_off[lo]) * S;
            const uint64_t len = L - p < W ? L - p : W;
            s = base + p;
            e = s + len;
            if (tid == 0) s_pos[0] = s;
            if ((uint64_t)tid == rows - 1) s_pos[1] = e;
        }
        uint32_t other = 0, oc = 0, og = 0, ot = 0;
        if (n_amb) {                                                    // (the same in every lane of the grid)
            __syncthreads();
            if (tid < 64) {
                const uint64_t a = dev_wave_lower_bound(amb, n_amb, s_pos[0], lane);
                const uint64_t b = dev_wave_lower_bound(amb, n_amb, s_pos[1], lane);
                if (lane == 0) { s_amb[0] = a; s_amb[1] = b; }
            }
            __syncthreads();
            if (active && s_amb[1] > s_amb[0]) {
                const uint64_t a = dev_lower_bound(amb, s_amb[0], s_amb[1], s), b = dev_lower_bound(amb, a, s_amb[1], e);
                other = (uint32_t)(b - a);
                if (other) { oc = ac[b] - ac[a]; og = ag[b] - ag[a]; ot = at[b] - at[a]; }
            }
        }
        if (active) {
            uint32_t c0, g0, t0, c1, g1, t1;
            wn_front(q, s, c0, g0, t0);
            wn_front(q, e, c1, g1, t1);
            const uint32_t c = c1 - c0 - oc, g = g1 - g0 - og, t = t1 - t0 - ot;
            int32_t *o = s_out + 5 * tid;                               // (a stride of 5 words: no two lanes on a bank twice)
            o[0] = (int32_t)((uint32_t)(e - s) - c - g - t - other);
            o[1] = (int32_t)c; o[2] = (int32_t)g; o[3] = (int32_t)t; o[4] = (int32_t)other;
        }
        __syncthreads();
        int32_t *dst = out + j0 * 5;
        for (uint64_t x = (uint64_t)tid; x < rows * 5; x += WN_BLOCK) dst[x] = s_out[x];
    }
}

extern "C" int gmg_window_counts(const gmg_reads *reads, int64_t window_len, int64_t window_skip, const uint64_t *amb_base, uint64_t n_amb,
                                 gmg_windows **out, void *stream)
{
    { int rc_enter = gmg_enter("gmg_window_counts"); if (rc_enter) return rc_enter; }
    if (!reads || !out || (n_amb && !amb_base)) return gmg_set_error(GMG_EINVAL, "gmg_window_counts: bad argument");
    if (window_len < 1 || window_skip < 1)
        return gmg_set_error(GMG_EINVAL, "gmg_window_counts: window_len %lld and window_skip %lld must both be 1 or more", (long long)window_len,
                             (long long)window_skip);
    if (n_amb >= 0x7ffffffeull) return gmg_set_error(GMG_EINVAL, "gmg_window_counts: %llu listed bases", (unsigned long long)n_amb);
    for (uint64_t i = 0; i < n_amb; i++)
        if (amb_base[i] >= reads->total_bases || (i && amb_base[i] <= amb_base[i - 1]))
            return gmg_set_error(GMG_EINVAL, "gmg_window_counts: ambiguous base %llu: the list must ascend inside the batch", (unsigned long long)i);
    hipStream_t s = (hipStream_t)stream;
    const uint64_t n_reads = reads->n_reads, W = (uint64_t)window_len, S = (uint64_t)window_skip;
    GmgScratch sc(GmgScratch::AFTER, s);
    uint64_t *d_row_off = nullptr;
    uint32_t *d_cnt = nullptr;
    unsigned long long *d_stats = nullptr;
    GMG_HIP(sc.alloc(&d_row_off, (n_reads + 1) * 8));
    GMG_HIP(sc.alloc(&d_cnt, (n_reads + 1) * 4));
    GMG_HIP(sc.alloc(&d_stats, 8));
    GMG_HIP(hipMemsetAsync(d_stats, 0xff, 8, s));
    hipLaunchKernelGGL(k_win_reads, dim3(gmg_grid(n_reads + 1, WN_BLOCK, WN_GRID_CAP)), dim3(WN_BLOCK), 0, s, reads->d_off, n_reads, W, S, d_cnt, d_stats);
    GMG_HIP(hipGetLastError());
    GMG_HIP((gmg_scan_excl<uint32_t, uint64_t>(d_cnt, d_row_off, n_reads + 1, s)));
    // the running counts do not depend on the number of windows: queued before the wait
    const uint64_t n_blocks = (reads->total_bases >> 6) + 1;
    uint32_t *d_b[3] = {nullptr, nullptr, nullptr}, *d_p[3] = {nullptr, nullptr, nullptr};
    uint32_t *d_f[3] = {nullptr, nullptr, nullptr}, *d_a[3] = {nullptr, nullptr, nullptr};
    uint64_t *d_amb = nullptr;
    for (int k = 0; k < 3; k++) {
        GMG_HIP(sc.alloc(&d_b[k], n_blocks * 4));
        GMG_HIP(sc.alloc(&d_p[k], n_blocks * 4));
    }
    hipLaunchKernelGGL(k_win_blocks, dim3(gmg_grid(n_blocks, WN_BLOCK, WN_GRID_CAP)), dim3(WN_BLOCK), 0, s, reads->d_packed, reads->n_words, n_blocks, d_b[0], d_b[1], d_b[2]);
    GMG_HIP(hipGetLastError());
    for (int k = 0; k < 3; k++) GMG_HIP((gmg_scan_excl<uint32_t, uint32_t>(d_b[k], d_p[k], n_blocks, s)));
    if (n_amb) {
        GMG_HIP(sc.alloc(&d_amb, n_amb * 8));
        GMG_HIP(hipMemcpyAsync(d_amb, amb_base, n_amb * 8, hipMemcpyHostToDevice, s));
        for (int k = 0; k < 3; k++) {
            GMG_HIP(sc.alloc(&d_f[k], (n_amb + 1) * 4));
            GMG_HIP(sc.alloc(&d_a[k], (n_amb + 1) * 4));
        }
        hipLaunchKernelGGL(k_win_amb, dim3(gmg_grid(n_amb + 1, WN_BLOCK, WN_GRID_CAP)), dim3(WN_BLOCK), 0, s, reads->d_packed, d_amb, n_amb, d_f[0], d_f[1], d_f[2]);
        GMG_HIP(hipGetLastError());
        for (int k = 0; k < 3; k++) GMG_HIP((gmg_scan_excl<uint32_t, uint32_t>(d_f[k], d_a[k], n_amb + 1, s)));
    }
    uint64_t total = 0;
    unsigned long long bad = ~0ull;
    GMG_HIP(hipMemcpyAsync(&total, d_row_off + n_reads, 8, hipMemcpyDeviceToHost, s));
    GMG_HIP(hipMemcpyAsync(&bad, d_stats, 8, hipMemcpyDeviceToHost, s));
    GMG_HIP(hipStreamSynchronize(s));
    if (bad != ~0ull)
        return gmg_set_error(GMG_ERANGE, "gmg_window_counts: read %llu has 2^31 bases or more", bad);
    if (total > (uint64_t)gmg_opt(GMG_OPT_MG_MAX_ENTRIES))
        return gmg_set_error(GMG_ETOOBIG, "gmg_window_counts: %llu windows, more than mg_max_entries = %lld: a larger skip, or the reads in smaller batches",
                             (unsigned long long)total, gmg_opt(GMG_OPT_MG_MAX_ENTRIES));
    int32_t *d_counts = nullptr;
    GMG_HIP(sc.alloc(&d_counts, (total ? total : 1) * 5 * sizeof(int32_t)));
    if (total) {
        WnSums q;
        q.packed = reads->d_packed; q.n_words = reads->n_words;
        q.pc = d_p[0]; q.pg = d_p[1]; q.pt = d_p[2];
        hipLaunchKernelGGL(k_win_rows, dim3(gmg_grid(total, WN_BLOCK, WN_GRID_CAP)), dim3(WN_BLOCK), 0, s, q, reads->d_off, n_reads, (const uint64_t *)d_row_off, total, W, S,
                           (const uint64_t *)d_amb, n_amb, (const uint32_t *)d_a[0], (const uint32_t *)d_a[1], (const uint32_t *)d_a[2], d_counts);
        GMG_HIP(hipGetLastError());
    }
    gmg_windows *res = new (std::nothrow) gmg_windows(s);
    if (!res) return gmg_set_error(GMG_ENOMEM, "gmg_window_counts: out of host memory");
    res->d_off = res->own.take(sc, d_row_off);
    res->d_counts = res->own.take(sc, d_counts);
    res->n_reads = n_reads;
    res->n_windows = total;
    *out = res;
    return GMG_OK;
}

extern "C" int gmg_windows_info(const gmg_windows *w, uint64_t *n_reads, uint64_t *n_windows)
{
    if (!w) return gmg_set_error(GMG_EINVAL, "gmg_windows_info: NULL handle");
    if (n_reads) *n_reads = w->n_reads;
    if (n_windows) *n_windows = w->n_windows;
    return GMG_OK;
}

extern "C" int gmg_windows_fetch(const gmg_windows *w, uint64_t *read_window_off, int32_t *counts)
{
    if (!w) return gmg_set_error(GMG_EINVAL, "gmg_windows_fetch: NULL handle");
    { int rc_enter = gmg_enter("gmg_windows_fetch"); if (rc_enter) return rc_enter; }
    if (read_window_off) GMG_HIP(hipMemcpyAsync(read_window_off, w->d_off, (w->n_reads + 1) * 8, hipMemcpyDeviceToHost, w->s));
    if (counts && w->n_windows) GMG_HIP(hipMemcpyAsync(counts, w->d_counts, w->n_windows * 5 * sizeof(int32_t), hipMemcpyDeviceToHost, w->s));
    GMG_HIP(hipStreamSynchronize(w->s));
    return GMG_OK;
}

extern "C" int gmg_windows_device(const gmg_windows *w, const uint64_t **d_read_window_off, const int32_t **d_counts)
{
    if (!w) return gmg_set_error(GMG_EINVAL, "gmg_windows_device: NULL handle");
    if (d_read_window_off) *d_read_window_off = w->d_off;
    if (d_counts) *d_counts = w->d_counts;
    return GMG_OK;
}

extern "C" int gmg_windows_free(gmg_windows *w)
{
    if (!w) return GMG_OK;
    delete w;
    return GMG_OK;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// gmg_regions_uncovered
// ---------------------------------------------------------------------------------------------------------------------------------

// key = read << 32 | lo, value = read << 32 | hi; stats[0]: the first interval that does not fit
__global__ __launch_bounds__(WN_BLOCK) void k_gap_keys(const gmg_interval *__restrict__ iv, uint64_t n, const uint64_t *__restrict__ off, uint64_t n_reads,
                                                      uint64_t *__restrict__ key, uint64_t *__restrict__ val, unsigned long long *__restrict__ stats)
{
    for (uint64_t i = (uint64_t)blockIdx.x * WN_BLOCK + threadIdx.x; i < n; i += (uint64_t)gridDim.x * WN_BLOCK) {
        const gmg_interval v = iv[i];
        bool ok = v.read < n_reads && v.lo >= 0 && v.hi >= v.lo;
        if (ok) {
            const uint64_t L = off[(uint64_t)v.read + 1] - off[v.read];
            ok = L < 0x80000000ull && (uint64_t)v.hi <= L;
        }
        if (!ok) atomicMin(&stats[0], (unsigned long long)i);
        key[i] = ok ? (uint64_t)v.read << 32 | (uint32_t)v.lo : ~0ull;
        val[i] = ok ? (uint64_t)v.read << 32 | (uint32_t)v.hi : ~0ull;
    }
}

// stats[1]: the first read of 2^31 bases or more (its tail gap would not fit a gmg_gene_region)
__global__ __launch_bounds__(WN_BLOCK) void k_gap_reads(const uint64_t *__restrict__ off, uint64_t n_reads, unsigned long long *__restrict__ stats)
{
    for (uint64_t r = (uint64_t)blockIdx.x * WN_BLOCK + threadIdx.x; r < n_reads; r += (uint64_t)gridDim.x * WN_BLOCK)
        if (off[r + 1] - off[r] >= 0x80000000ull) atomicMin(&stats[1], (unsigned long long)r);
}

// item m of the merged order, m < n + n_reads: interval i of read r is item i + r, read r's tail the item e_r + r behind its last
// interval.  -> the gap [a, b) the item stands for (b <= a: none) and its read
struct GapItem { uint32_t read; int64_t a, b; };

__device__ __forceinline__ GapItem gap_of_interval(const uint64_t *__restrict__ key, const uint64_t *__restrict__ run, uint64_t i)
{
    GapItem it;
    const uint64_t k = key[i];
    it.read = (uint32_t)(k >> 32);
    it.b = (int64_t)(uint32_t)k;
    it.a = 0;
    if (i) {
        const uint64_t prev = run[i - 1];                               // the running maximum in front of i
        if ((uint32_t)(prev >> 32) == it.read) it.a = (int64_t)(uint32_t)prev;
    }
    return it;
}

template <bool WRITE>
__global__ __launch_bounds__(WN_BLOCK) void k_gap_items(const uint64_t *__restrict__ key, const uint64_t *__restrict__ run, uint64_t n,
                                                       const uint64_t *__restrict__ off, uint64_t n_reads, int64_t min_len,
                                                       uint32_t *__restrict__ flag, const uint64_t *__restrict__ slot, uint64_t total,
                                                       gmg_gene_region *__restrict__ gaps, uint64_t *__restrict__ read_gap_off)
{
    const uint64_t n_items = n + n_reads;
    for (uint64_t x = (uint64_t)blockIdx.x * WN_BLOCK + threadIdx.x; x <= n_items; x += (uint64_t)gridDim.x * WN_BLOCK) {
        if (x == n_items) {
            if (WRITE) read_gap_off[n_reads] = total;
            else flag[x] = 0;                                           // (the scan's last output is the total)
            continue;
        }
        GapItem it;
        uint64_t m;
        if (x < n) {
            it = gap_of_interval(key, run, x);
            m = x + it.read;
        } else {
            const uint64_t r = x - n;
            const uint64_t e = dev_lower_bound(key, 0, n, (r + 1) << 32);    // behind read r's last interval
            it.read = (uint32_t)r;
            it.a = 0;
            if (e) {
                const uint64_t last = run[e - 1];
                if ((uint32_t)(last >> 32) == it.read) it.a = (int64_t)(uint32_t)last;
            }
            it.b = (int64_t)(off[r + 1] - off[r]);
            m = e + r;
            if (WRITE) {
                // read r's first item: its first interval, or this tail
                const uint64_t b = dev_lower_bound(key, 0, e, r << 32);
                read_gap_off[r] = slot[b + r];
            }
        }
        const int64_t len = it.b - it.a;
        const bool keep = len > 0 && len >= min_len;
        if (!WRITE) flag[m] = keep;
        else if (keep) {
            const uint64_t at = slot[m];
            if (at < total) {
                gmg_gene_region g;
                g.read = it.read; g.first = (int32_t)it.a; g.len = (int32_t)len; g.strand = 1;
                gaps[at] = g;
            }
        }
    }
}

extern "C" int gmg_regions_uncovered(const gmg_reads *reads, const gmg_interval *intervals, uint64_t n, int64_t min_len, gmg_gaps **out,
                                     void *stream)
{
    { int rc_enter = gmg_enter("gmg_regions_uncovered"); if (rc_enter) return rc_enter; }
    if (!reads || (!intervals && n) || !out || n >= 0x7ffffffeull || reads->n_reads >= 0x7ffffffeull - n)
        return gmg_set_error(GMG_EINVAL, "gmg_regions_uncovered: bad argument");
    hipStream_t s = (hipStream_t)stream;
    const uint64_t n_reads = reads->n_reads, n_items = n + n_reads;
    GmgScratch sc(GmgScratch::AFTER, s);
    uint64_t *d_gap_off = nullptr, *d_key = nullptr, *d_val = nullptr, *d_key2 = nullptr, *d_val2 = nullptr, *d_run = nullptr, *d_slot = nullptr;
    gmg_interval *d_iv = nullptr;
    uint32_t *d_flag = nullptr;
    unsigned long long *d_stats = nullptr;
    void *d_tmp = nullptr;
    GMG_HIP(sc.alloc(&d_gap_off, (n_reads + 1) * 8));
    GMG_HIP(sc.alloc(&d_stats, 16));
    GMG_HIP(sc.alloc(&d_flag, (n_items + 1) * 4));
    GMG_HIP(sc.alloc(&d_slot, (n_items + 1) * 8));
    GMG_HIP(hipMemsetAsync(d_stats, 0xff, 16, s));
    if (n_reads) {
        hipLaunchKernelGGL(k_gap_reads, dim3(gmg_grid(n_reads, WN_BLOCK, WN_GRID_CAP)), dim3(WN_BLOCK), 0, s, reads->d_off, n_reads, d_stats);
        GMG_HIP(hipGetLastError());
    }
    if (n) {
        GMG_HIP(sc.alloc(&d_iv, n * sizeof(gmg_interval)));
        GMG_HIP(sc.alloc(&d_key, n * 8));
        GMG_HIP(sc.alloc(&d_val, n * 8));
        GMG_HIP(sc.alloc(&d_key2, n * 8));
        GMG_HIP(sc.alloc(&d_val2, n * 8));
        GMG_HIP(sc.alloc(&d_run, n * 8));
        GMG_HIP(hipMemcpyAsync(d_iv, intervals, n * sizeof(gmg_interval), hipMemcpyHostToDevice, s));
        hipLaunchKernelGGL(k_gap_keys, dim3(gmg_grid(n, WN_BLOCK, WN_GRID_CAP)), dim3(WN_BLOCK), 0, s, d_iv, n, reads->d_off, n_reads, d_key, d_val, d_stats);
        GMG_HIP(hipGetLastError());
        // (read, lo) ascending: the key bits that can be set are the 31 of lo and those of the read index
        int end_bit = 32;
        while (end_bit < 64 && (n_reads >> (end_bit - 32))) end_bit++;
        size_t need = 0, need2 = 0;
        GMG_HIP(hipcub::DeviceRadixSort::SortPairs(nullptr, need, d_key, d_key2, d_val, d_val2, (int)n, 0, end_bit, s));
        GMG_HIP(hipcub::DeviceScan::InclusiveScan(nullptr, need2, d_val2, d_run, hipcub::Max(), (int)n, s));
        if (need2 > need) need = need2;
        GMG_HIP(sc.alloc(&d_tmp, need ? need : 1));
        size_t nb = need;
        GMG_HIP(hipcub::DeviceRadixSort::SortPairs(d_tmp, nb, d_key, d_key2, d_val, d_val2, (int)n, 0, end_bit, s));
        nb = need;
        GMG_HIP(hipcub::DeviceScan::InclusiveScan(d_tmp, nb, d_val2, d_run, hipcub::Max(), (int)n, s));
    }
    // a bad interval has the key ~0: it is not read before the host has seen stats[0]
    unsigned long long bad[2] = {~0ull, ~0ull};
    GMG_HIP(hipMemcpyAsync(bad, d_stats, 16, hipMemcpyDeviceToHost, s));
    GMG_HIP(hipStreamSynchronize(s));
    if (bad[1] != ~0ull)
        return gmg_set_error(GMG_ERANGE, "gmg_regions_uncovered: read %llu has 2^31 bases or more", bad[1]);
    if (bad[0] != ~0ull) {
        const gmg_interval &v = intervals[bad[0]];
        return gmg_set_error(GMG_ERANGE, "gmg_regions_uncovered: interval %llu (read %u, lo %d, hi %d) does not fit its read (the batch has %llu)",
                             bad[0], v.read, v.lo, v.hi, (unsigned long long)n_reads);
    }
    uint64_t total = 0;
    hipLaunchKernelGGL(k_gap_items<false>, dim3(gmg_grid(n_items + 1, WN_BLOCK, WN_GRID_CAP)), dim3(WN_BLOCK), 0, s, (const uint64_t *)d_key2, (const uint64_t *)d_run, n,
                       reads->d_off, n_reads, min_len, d_flag, (const uint64_t *)nullptr, (uint64_t)0, (gmg_gene_region *)nullptr, (uint64_t *)nullptr);
    GMG_HIP(hipGetLastError());
    GMG_HIP((gmg_scan_excl<uint32_t, uint64_t>(d_flag, d_slot, n_items + 1, s)));
    GMG_HIP(hipMemcpyAsync(&total, d_slot + n_items, 8, hipMemcpyDeviceToHost, s));
    GMG_HIP(hipStreamSynchronize(s));
    if (total > (uint64_t)gmg_opt(GMG_OPT_MG_MAX_ENTRIES))
        return gmg_set_error(GMG_ETOOBIG, "gmg_regions_uncovered: %llu gaps, more than mg_max_entries = %lld: the reads in smaller batches",
                             (unsigned long long)total, gmg_opt(GMG_OPT_MG_MAX_ENTRIES));
    gmg_gene_region *d_gaps = nullptr;
    GMG_HIP(sc.alloc(&d_gaps, (total ? total : 1) * sizeof(gmg_gene_region)));
    hipLaunchKernelGGL(k_gap_items<true>, dim3(gmg_grid(n_items + 1, WN_BLOCK, WN_GRID_CAP)), dim3(WN_BLOCK), 0, s, (const uint64_t *)d_key2, (const uint64_t *)d_run, n,
                       reads->d_off, n_reads, min_len, (uint32_t *)nullptr, (const uint64_t *)d_slot, total, d_gaps, d_gap_off);
    GMG_HIP(hipGetLastError());
    gmg_gaps *res = new (std::nothrow) gmg_gaps(s);
    if (!res) return gmg_set_error(GMG_ENOMEM, "gmg_regions_uncovered: out of host memory");
    res->d_gaps = res->own.take(sc, d_gaps);
    res->d_off = res->own.take(sc, d_gap_off);
    res->n_reads = n_reads;
    res->n_gaps = total;
    *out = res;
    return GMG_OK;
}

extern "C" int gmg_gaps_info(const gmg_gaps *g, uint64_t *n_gaps)
{
    if (!g) return gmg_set_error(GMG_EINVAL, "gmg_gaps_info: NULL handle");
    if (n_gaps) *n_gaps = g->n_gaps;
    return GMG_OK;
}

extern "C" int gmg_gaps_fetch(const gmg_gaps *g, gmg_gene_region *gaps, uint64_t *read_gap_off)
{
    if (!g) return gmg_set_error(GMG_EINVAL, "gmg_gaps_fetch: NULL handle");
    { int rc_enter = gmg_enter("gmg_gaps_fetch"); if (rc_enter) return rc_enter; }
    if (gaps && g->n_gaps) GMG_HIP(hipMemcpyAsync(gaps, g->d_gaps, g->n_gaps * sizeof(gmg_gene_region), hipMemcpyDeviceToHost, g->s));
    if (read_gap_off) GMG_HIP(hipMemcpyAsync(read_gap_off, g->d_off, (g->n_reads + 1) * 8, hipMemcpyDeviceToHost, g->s));
    GMG_HIP(hipStreamSynchronize(g->s));
    return GMG_OK;
}

extern "C" int gmg_gaps_free(gmg_gaps *g)
{
    if (!g) return GMG_OK;
    delete g;
    return GMG_OK;
}
