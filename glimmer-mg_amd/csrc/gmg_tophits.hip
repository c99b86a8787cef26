// gmg_tophits.hip -- the classification step of Glimmer-MG's pipeline on the device: every read against a database of ICMs,
// the best `top_hits` models of every read kept in HBM while the database streams through in batches (include/gmg.h,
// gmg_tophits_*), and the raw score matrix written as text.
//
// What is reproduced is the script pair Phymm's scoreReadsGlim.pl (the raw matrix: per read and model the simple-score value
// printed with %.4f, the reverse strand's only when it parses to a strictly greater number) and glimmer-mg.py's parse_phymm
// (per read, score_insert of every informative model in matrix order).  Both compare the PRINTED values, so everything here
// works on the key of a value: the %.4f text as an integer count of 1e-4 units (th_key), which orders exactly as the parsed
// numbers do.
//
// k_th_update: a lane per read, its slots in registers, the batch's models in order -- score_insert with its quirks (the first
//              top_hits models fill the slots unsorted; later ones go in at the first slot they strictly beat).
// k_th_len / k_th_text: the batch's matrix lines in two passes -- the length of every field, an exclusive scan (gmg_scan.h),
//              then every lane writes its field at its offset.

#include "gmg_internal.h"

#include "gmg_scan.h"

#include <math.h>
#include <new>
#include <string.h>
#include <vector>

#define TH_BLOCK 256
#define TH_MAX_HITS 16
// |x| * 1e4 below 2^52: the product's rounding error analysis of th_key holds (ulp <= 1/2), and a key fits an int64 easily
#define TH_LIMIT 4503599627370496.0

struct GMG_HIDDEN gmg_tophits {
    const gmg_reads *reads = nullptr;    // the caller's batch (gmg_tophits_scores scores it; it must outlive the handle)
    uint64_t n_reads = 0;
    int top_hits = 0;
    int64_t *d_keys = nullptr;   // [top_hits][n_reads] slot-major (a lane's loads of one slot are coalesced across the wave)
    int32_t *d_models = nullptr; // [top_hits][n_reads], -1 = empty slot
    uint32_t *d_flag = nullptr;  // set by a kernel that met a value it cannot key (NaN, infinite, |x| >= 2^52 / 1e4)
    uint8_t *d_inf = nullptr;    // [cap_inf] the batch's informative flags
    double *d_sums = nullptr;    // [cap_sums] gmg_tophits_scores' scratch: [B][n_reads][2]
    uint32_t *d_len = nullptr;   // [cap_items] field lengths of gmg_tophits_format_rows
    uint64_t *d_off = nullptr;   // [cap_off] their exclusive sums
    char *d_text = nullptr;      // [cap_text]
    size_t cap_inf = 0, cap_sums = 0, cap_items = 0, cap_off = 0, cap_text = 0;
    hipStream_t last = nullptr;  // the stream of the last update (the null stream before the first): gmg_tophits_fetch copies on it
    GmgScratch own{GmgScratch::NONE, nullptr, GmgScratch::DRIVER};
};

// ---------------------------------------------------------------------------
// the key of a value: round-half-even(|x| * 1e4) on the EXACT product, with the sign of x -- the digits "%.4f" prints (glibc rounds
// the exact binary value, ties to even).  p + e is the exact product (1e4 is exact, fma gives the rounding error of p).  With
// n = rint(p) and d = p - n (exact), |d| < 1/2 leaves n whatever e is (d is a multiple of ulp(p) <= 1/2, and |e| <= ulp(p) / 2);
// only d = +-1/2 is a tie of p that e decides: sums of the form q/32 make exact ties (e = 0), which rint already gave to the even n.
// ---------------------------------------------------------------------------
__device__ __forceinline__ bool th_keyable(double x) { return fabs(x) * 1e4 < TH_LIMIT; }   // (false for NaN and infinities)

__device__ __forceinline__ int64_t th_key(double x)
{
    const double a = fabs(x), p = a * 1e4, e = fma(a, 1e4, -p), n = rint(p), d = p - n;
    int64_t k = (int64_t)n;
    if (d == 0.5 && e > 0.0) k++;
    else if (d == -0.5 && e < 0.0) k--;
    return signbit(x) ? -k : k;
}

// scoreReadsGlim.pl's strand rule: the reverse strand's value only when its printed value is strictly greater.  -> the key, and
// whether the winner prints a minus sign (a negative key, or -0.0000 for a negative value that rounds to zero)
__device__ __forceinline__ int64_t th_pick(const double2 v, const int forward_only, bool &minus, bool &ok)
{
    ok = th_keyable(v.x) && (forward_only || th_keyable(v.y));
    if (!ok) { minus = false; return 0; }
    const int64_t kf = th_key(v.x);
    if (!forward_only) {
        const int64_t kr = th_key(v.y);
        if (kr > kf) { minus = signbit(v.y); return kr; }
    }
    minus = signbit(v.x);
    return kf;
}

__device__ __forceinline__ uint32_t th_digits(uint64_t u)
{
    uint32_t n = 1;
    while (u >= 10) { u /= 10; n++; }
    return n;
}

// ---------------------------------------------------------------------------
// score_insert over one batch: lane r holds read r's slots; models b = 0 .. B-1 (global index first + b) in order
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(TH_BLOCK) void k_th_update(const double2 *__restrict__ sums, const uint64_t nr, const int B, const int first,
                                                        const uint8_t *__restrict__ inf, const int forward_only, const int T,
                                                        int64_t *__restrict__ keys, int32_t *__restrict__ models, uint32_t *__restrict__ flag)
{
    const uint64_t r = (uint64_t)blockIdx.x * TH_BLOCK + threadIdx.x;
    if (r >= nr) return;
    int64_t k[TH_MAX_HITS];
    int32_t m[TH_MAX_HITS];
    int filled = 0;
#pragma unroll
    for (int i = 0; i < TH_MAX_HITS; i++) {
        if (i < T) {
            k[i] = keys[(uint64_t)i * nr + r];
            m[i] = models[(uint64_t)i * nr + r];
            filled += m[i] >= 0;
        } else {
            k[i] = 0;
            m[i] = -1;
        }
    }
    bool bad = false;
    for (int b = 0; b < B; b++) {
        if (inf && !inf[b]) continue;
        bool minus, ok;
        int64_t ck = th_pick(sums[(uint64_t)b * nr + r], forward_only, minus, ok);
        bad |= !ok;
        int32_t cm = first + b;
        if (filled < T) {                               // an empty slot: the first one, in arrival order
#pragma unroll
            for (int i = 0; i < TH_MAX_HITS; i++)
                if (i == filled) { k[i] = ck; m[i] = cm; }
            filled++;
            continue;
        }
        // the first slot the score strictly beats takes it, the later ones move down, the last one drops out
        bool in = false;
#pragma unroll
        for (int i = 0; i < TH_MAX_HITS; i++) {
            if (i < T && (in || ck > k[i])) {
                const int64_t tk = k[i];
                const int32_t tm = m[i];
                k[i] = ck; m[i] = cm;
                ck = tk; cm = tm;
                in = true;
            }
        }
    }
    if (bad) atomicOr(flag, 1u);
#pragma unroll
    for (int i = 0; i < TH_MAX_HITS; i++) {
        if (i < T) {
            keys[(uint64_t)i * nr + r] = k[i];
            models[(uint64_t)i * nr + r] = m[i];
        }
    }
}

// ---------------------------------------------------------------------------
// the matrix lines: field i = b * nr + r is the winning strand's %.4f text and a tab, or a newline after the last read of a line
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(TH_BLOCK) void k_th_len(const double2 *__restrict__ sums, const uint64_t n_items, const int forward_only,
                                                     uint32_t *__restrict__ len, uint32_t *__restrict__ flag)
{
    bool bad = false;
    for (uint64_t i = (uint64_t)blockIdx.x * TH_BLOCK + threadIdx.x; i < n_items; i += (uint64_t)gridDim.x * TH_BLOCK) {
        bool minus, ok;
        const int64_t key = th_pick(sums[i], forward_only, minus, ok);
        bad |= !ok;
        const uint64_t u = key < 0 ? (uint64_t)(-key) : (uint64_t)key;
        len[i] = (uint32_t)minus + th_digits(u / 10000) + 5 + 1;        // [-]digits.dddd + the separator
    }
    if (bad) atomicOr(flag, 1u);
}

__global__ __launch_bounds__(TH_BLOCK) void k_th_text(const double2 *__restrict__ sums, const uint64_t nr, const uint64_t n_items,
                                                      const int forward_only, const uint64_t *__restrict__ off, char *__restrict__ text)
{
    for (uint64_t i = (uint64_t)blockIdx.x * TH_BLOCK + threadIdx.x; i < n_items; i += (uint64_t)gridDim.x * TH_BLOCK) {
        bool minus, ok;
        const int64_t key = th_pick(sums[i], forward_only, minus, ok);
        uint64_t u = key < 0 ? (uint64_t)(-key) : (uint64_t)key;
        char buf[24];                                   // written back to front: separator, 4 decimals, '.', integer digits, sign
        int n = 0;
        buf[n++] = (i % nr == nr - 1) ? '\n' : '\t';
        for (int j = 0; j < 4; j++) { buf[n++] = (char)('0' + u % 10); u /= 10; }
        buf[n++] = '.';
        do { buf[n++] = (char)('0' + u % 10); u /= 10; } while (u);
        if (minus) buf[n++] = '-';
        char *dst = text + off[i];
        for (int j = 0; j < n; j++) dst[j] = buf[n - 1 - j];
    }
}

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------
namespace {

unsigned grid_for(uint64_t items)
{
    const uint64_t b = (items + TH_BLOCK - 1) / TH_BLOCK;
    return (unsigned)(b == 0 ? 1 : (b < 256 * 64 ? b : 256 * 64));
}

// the flag the kernels set for a value without a key: read back (the stream is synchronised) and cleared
int check_flag(gmg_tophits *h, hipStream_t s, const char *who)
{
    uint32_t f = 0;
    GMG_HIP(hipMemcpyAsync(&f, h->d_flag, 4, hipMemcpyDeviceToHost, s));
    GMG_HIP(hipStreamSynchronize(s));
    if (f) {
        GMG_HIP(hipMemsetAsync(h->d_flag, 0, 4, s));
        return gmg_set_error(GMG_ERANGE, "%s: a score is not finite or its magnitude is 2^52 / 10^4 or more (no exact %%.4f key)", who);
    }
    return GMG_OK;
}

}  // namespace

extern "C" int gmg_tophits_create(const gmg_reads *reads, int top_hits, gmg_tophits **out)
{
    { int rc_enter = gmg_enter("gmg_tophits_create"); if (rc_enter) return rc_enter; }
    if (!reads || !out) return gmg_set_error(GMG_EINVAL, "gmg_tophits_create: NULL argument");
    *out = nullptr;
    if (top_hits < 1 || top_hits > TH_MAX_HITS)
        return gmg_set_error(GMG_EINVAL, "gmg_tophits_create: top_hits %d outside 1..%d", top_hits, TH_MAX_HITS);
    std::unique_ptr<gmg_tophits> h(new (std::nothrow) gmg_tophits());
    if (!h) return gmg_set_error(GMG_ENOMEM, "gmg_tophits_create: out of host memory");
    h->reads = reads;
    h->n_reads = reads->n_reads;
    h->top_hits = top_hits;
    const size_t slots = (size_t)top_hits * (h->n_reads ? h->n_reads : 1);
    GMG_HIP(h->own.alloc(&h->d_keys, slots * 8));
    GMG_HIP(h->own.alloc(&h->d_models, slots * 4));
    GMG_HIP(h->own.alloc(&h->d_flag, 4));
    GMG_HIP(hipMemset(h->d_keys, 0, slots * 8));
    GMG_HIP(hipMemset(h->d_models, 0xff, slots * 4));
    GMG_HIP(hipMemset(h->d_flag, 0, 4));
    GMG_HANDLE_READY();                                 // (an update on a caller's non-blocking stream is not ordered behind the three memsets)
    *out = h.release();
    return GMG_OK;
}

extern "C" int gmg_tophits_free(gmg_tophits *h)
{
    if (!h) return GMG_OK;
    delete h;
    return GMG_OK;
}

extern "C" int gmg_tophits_update_sums(gmg_tophits *h, const double *d_sums, int B, int first_model, const uint8_t *informative,
                                       int forward_only, void *stream)
{
    { int rc_enter = gmg_enter("gmg_tophits_update_sums"); if (rc_enter) return rc_enter; }
    if (!h || B < 0 || (!d_sums && B && h->n_reads)) return gmg_set_error(GMG_EINVAL, "gmg_tophits_update_sums: NULL argument");
    if (first_model < 0 || (int64_t)first_model + B > INT32_MAX)
        return gmg_set_error(GMG_EINVAL, "gmg_tophits_update_sums: model indices %d + %d outside int32", first_model, B);
    hipStream_t s = (hipStream_t)stream;
    if (B == 0 || h->n_reads == 0) return GMG_OK;
    h->last = s;
    const uint8_t *d_inf = nullptr;
    if (informative) {
        GMG_HIP(h->own.regrow(h->d_inf, h->cap_inf, (size_t)B));
        GMG_HIP(hipMemcpyAsync(h->d_inf, informative, (size_t)B, hipMemcpyHostToDevice, s));
        d_inf = h->d_inf;
    }
    hipLaunchKernelGGL(k_th_update, dim3((unsigned)((h->n_reads + TH_BLOCK - 1) / TH_BLOCK)), dim3(TH_BLOCK), 0, s,
                       (const double2 *)d_sums, h->n_reads, B, first_model, d_inf, forward_only, h->top_hits, h->d_keys, h->d_models,
                       h->d_flag);
    GMG_HIP(hipGetLastError());
    return check_flag(h, s, "gmg_tophits_update_sums");       // (also: the informative flags' host buffer may be reused)
}

extern "C" int gmg_tophits_scores(gmg_tophits *h, const gmg_model *const *models, int B, int first_model, const uint8_t *informative,
                                  int forward_only, void *stream, const double **d_sums_out)
{
    { int rc_enter = gmg_enter("gmg_tophits_scores"); if (rc_enter) return rc_enter; }
    if (!h || B < 0 || (!models && B)) return gmg_set_error(GMG_EINVAL, "gmg_tophits_scores: NULL argument");
    if (d_sums_out) *d_sums_out = nullptr;
    GMG_HIP(h->own.regrow(h->d_sums, h->cap_sums, (size_t)B * h->n_reads * 2));
    int rc = gmg_score_reads_strings(models, B, h->reads, h->d_sums, stream);
    if (rc) return rc;
    rc = gmg_tophits_update_sums(h, h->d_sums, B, first_model, informative, forward_only, stream);
    if (rc == GMG_OK && d_sums_out) *d_sums_out = h->d_sums;
    return rc;
}

extern "C" int gmg_tophits_fetch(const gmg_tophits *h, int64_t *keys, int32_t *models)
{
    { int rc_enter = gmg_enter("gmg_tophits_fetch"); if (rc_enter) return rc_enter; }
    if (!h || ((!keys || !models) && h->n_reads)) return gmg_set_error(GMG_EINVAL, "gmg_tophits_fetch: NULL argument");
    const uint64_t nr = h->n_reads, T = (uint64_t)h->top_hits;
    if (nr == 0) return GMG_OK;
    std::vector<int64_t> k(T * nr);
    std::vector<int32_t> m(T * nr);
    // on the stream that wrote the slots last (every update waits for its stream, so they are complete): not behind the null stream's work
    GMG_HIP(hipMemcpyAsync(k.data(), h->d_keys, T * nr * 8, hipMemcpyDeviceToHost, h->last));
    GMG_HIP(gmg_copy_wait(m.data(), h->d_models, T * nr * 4, hipMemcpyDeviceToHost, h->last));
    for (uint64_t r = 0; r < nr; r++)                   // slot-major on the device, read-major for the caller
        for (uint64_t i = 0; i < T; i++) {
            keys[r * T + i] = k[i * nr + r];
            models[r * T + i] = m[i * nr + r];
        }
    return GMG_OK;
}

extern "C" int gmg_tophits_format_rows(gmg_tophits *h, const double *d_sums, int B, int forward_only, char *host_out, size_t *bytes,
                                       void *stream)
{
    { int rc_enter = gmg_enter("gmg_tophits_format_rows"); if (rc_enter) return rc_enter; }
    if (!h || B < 0 || !bytes || (!d_sums && B && h->n_reads)) return gmg_set_error(GMG_EINVAL, "gmg_tophits_format_rows: NULL argument");
    hipStream_t s = (hipStream_t)stream;
    const uint64_t nr = h->n_reads, n_items = (uint64_t)B * nr;
    if (n_items == 0) {                                 // (no reads: a line of no fields is its newline)
        const size_t need = nr ? 0 : (size_t)B;
        if (host_out && *bytes < need) { *bytes = need; return gmg_set_error(GMG_ERANGE, "gmg_tophits_format_rows: buffer too small"); }
        if (host_out) memset(host_out, '\n', need);
        *bytes = need;
        return GMG_OK;
    }
    GMG_HIP(h->own.regrow(h->d_len, h->cap_items, n_items));
    GMG_HIP(h->own.regrow(h->d_off, h->cap_off, n_items + 1));
    hipLaunchKernelGGL(k_th_len, dim3(grid_for(n_items)), dim3(TH_BLOCK), 0, s, (const double2 *)d_sums, n_items, forward_only, h->d_len,
                       h->d_flag);
    GMG_HIP(hipGetLastError());
    GMG_HIP((gmg_scan_excl<uint32_t, uint64_t>(h->d_len, h->d_off, n_items, s)));
    uint64_t tail[2] = {0, 0};                          // offset and length of the last field
    GMG_HIP(hipMemcpyAsync(&tail[0], h->d_off + n_items - 1, 8, hipMemcpyDeviceToHost, s));
    uint32_t last = 0;
    GMG_HIP(hipMemcpyAsync(&last, h->d_len + n_items - 1, 4, hipMemcpyDeviceToHost, s));
    int rc = check_flag(h, s, "gmg_tophits_format_rows");   // (synchronises)
    if (rc) return rc;
    tail[1] = last;
    const size_t need = (size_t)(tail[0] + tail[1]);
    if (!host_out) { *bytes = need; return GMG_OK; }
    if (*bytes < need) {
        rc = gmg_set_error(GMG_ERANGE, "gmg_tophits_format_rows: buffer of %zu bytes, the lines need %zu", *bytes, need);
        *bytes = need;
        return rc;
    }
    GMG_HIP(h->own.regrow(h->d_text, h->cap_text, need));
    hipLaunchKernelGGL(k_th_text, dim3(grid_for(n_items)), dim3(TH_BLOCK), 0, s, (const double2 *)d_sums, nr, n_items, forward_only,
                       (const uint64_t *)h->d_off, h->d_text);
    GMG_HIP(hipGetLastError());
    GMG_HIP(hipMemcpyAsync(host_out, h->d_text, need, hipMemcpyDeviceToHost, s));
    GMG_HIP(hipStreamSynchronize(s));
    *bytes = need;
    return GMG_OK;
}
