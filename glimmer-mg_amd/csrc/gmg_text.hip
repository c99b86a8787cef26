// gmg_text.hip -- gmg_letters and gmg_regions_text (include/gmg.h): regions of the reads of a batch as the TEXT extract and
// multi-extract print (src/Util/extract.cc:158-207, multi-extract.cc:215-262, Output_Subsequence): a header the caller made, the
// region's letters -- the sequence's own bytes, through a 256-entry table per strand -- with a newline in front of every
// width + 1st letter of a line, and a final newline.  All integers, no sums: the text is byte-identical by construction.
//
// The length of every record is known on the host (head + letters + newlines), so the host uploads one TxRec per record and
// the records' text offsets, and ONE kernel writes the text, organised by OUTPUT bytes: a work-group owns TX_TILE consecutive
// bytes of the text, a lane 16 consecutive bytes at a time, which it stores with one 16-byte store (the text buffer is 256-byte
// aligned and a lane's bytes start at a multiple of 16; only the last, partial 16 bytes of the buffer are stored byte by byte).
// The records of a tile's first and last byte come from two binary searches over all offsets; a lane then finds the record of
// its first byte between those two and walks on from there: record to record where its 16 bytes span several.  Byte q of a
// record is a head byte (q < hlen), the final newline, a line's newline (r = q - hlen, r % (width + 1) == width) or letter
// r - r / (width + 1): position first + j (forward) or first - j (reverse) of the read, modulo its length.  Every byte of the
// text is written exactly once; no atomics, nothing depends on the order of the work-groups.

#include "gmg_internal.h"

#include <string.h>
#include <vector>

#define TX_BLOCK 256
#define TX_LANE_BYTES 16
#define TX_PASSES 4
#define TX_TILE (TX_BLOCK * TX_LANE_BYTES * TX_PASSES)  // bytes of text per work-group: 16 KiB
#define TX_REV 0x80000000u

struct TxRec {
    uint64_t src;                // job-wide index of the read's base 0
    uint64_t head;               // offset of the record's head in the heads
    uint32_t L;                  // the read's length (< 2^31)
    uint32_t first;              // position in the read of the record's letter 0 (< L)
    uint32_t hlen;               // bytes of the head
    uint32_t nlet;               // letters (< 2^31); TX_REV: reverse strand
};

struct GMG_HIDDEN gmg_letters {
    uint8_t *d_letters = nullptr;
    std::vector<uint64_t> off;   // n_reads + 1 (host)
    uint64_t n_reads = 0;
    char *d_text = nullptr;      // the text of the last call
    size_t cap_text = 0;
    hipEvent_t ev[2] = {nullptr, nullptr};   // around the last call's kernel
    int timed = 0;               // ... which there was
    GmgScratch own{GmgScratch::DEVICE, nullptr};         // (the last call's kernel may still run when the handle goes)
    ~gmg_letters()
    {
        if (ev[0]) (void)hipEventDestroy(ev[0]);
        if (ev[1]) (void)hipEventDestroy(ev[1]);
    }
};

// the largest k in [lo, hi] with off[k] <= g (off[lo] <= g)
__device__ __forceinline__ uint64_t tx_find(const uint64_t *__restrict__ off, uint64_t lo, uint64_t hi, uint64_t g)
{
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo + 1) / 2;
        if (off[mid] <= g) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

// where a lane stands in the text: in record k, at byte q of it
struct TxCursor {
    TxRec m;
    uint64_t end;                // text offset of the next record
    uint64_t q;                  // byte of the record
    uint64_t body;               // bytes behind the head: letters, the lines' newlines, the final newline
    uint32_t j, col;             // next letter; letters already on the line
};

__device__ __forceinline__ void tx_open(TxCursor &c, const TxRec *__restrict__ rec, const uint64_t *__restrict__ toff, uint64_t k, uint64_t g,
                                        uint32_t width)
{
    c.m = rec[k];
    const uint64_t beg = toff[k];
    c.end = toff[k + 1];
    c.q = g - beg;
    c.body = c.end - beg - c.m.hlen;
    c.j = c.col = 0;
    if (c.q > c.m.hlen) {
        const uint64_t r = c.q - c.m.hlen;
        if (width) {
            const uint64_t line = r / ((uint64_t)width + 1);
            c.col = (uint32_t)(r - line * ((uint64_t)width + 1));
            c.j = (uint32_t)(r - line);
        } else c.j = (uint32_t)r;
    }
}

__device__ __forceinline__ uint32_t tx_byte(TxCursor &c, const uint8_t *__restrict__ letters, const uint8_t *__restrict__ heads,
                                            const uint8_t *tab, uint32_t width)
{
    uint32_t ch;
    if (c.q < c.m.hlen) ch = heads[c.m.head + c.q];
    else if (c.q - c.m.hlen == c.body - 1) ch = '\n';
    else if (width && c.col == width) { ch = '\n'; c.col = 0; }
    else {
        const bool rev = (c.m.nlet & TX_REV) != 0;
        uint32_t p;
        if (!rev) { p = c.m.first + c.j; if (p >= c.m.L) p -= c.m.L; }
        else p = c.m.first >= c.j ? c.m.first - c.j : c.m.first + c.m.L - c.j;
        ch = tab[(rev ? 256u : 0u) + letters[c.m.src + p]];
        c.j++;
        c.col++;
    }
    c.q++;
    return ch;
}

__global__ __launch_bounds__(TX_BLOCK) void k_regions_text(const uint8_t *__restrict__ letters, const TxRec *__restrict__ rec,
                                                           const uint64_t *__restrict__ toff, const uint64_t n, const uint8_t *__restrict__ heads,
                                                           const uint8_t *__restrict__ tables, const uint32_t width, const uint64_t total,
                                                           uint8_t *__restrict__ text)
{
    __shared__ uint8_t tab[512];
    tab[threadIdx.x] = tables[threadIdx.x];
    tab[256 + threadIdx.x] = tables[256 + threadIdx.x];
    __syncthreads();
    const uint64_t tile0 = (uint64_t)blockIdx.x * TX_TILE;
    if (tile0 >= total) return;
    const uint64_t tile_last = tile0 + TX_TILE - 1 < total - 1 ? tile0 + TX_TILE - 1 : total - 1;
    // the tile's records: the same for every lane (n >= 1 here: there is text)
    const uint64_t klo = tx_find(toff, 0, n - 1, tile0), khi = tx_find(toff, klo, n - 1, tile_last);
#pragma unroll 1
    for (int pass = 0; pass < TX_PASSES; pass++) {
        const uint64_t g = tile0 + ((uint64_t)pass * TX_BLOCK + threadIdx.x) * TX_LANE_BYTES;
        if (g >= total) return;
        TxCursor c;
        uint64_t k = tx_find(toff, klo, khi, g);
        tx_open(c, rec, toff, k, g, width);
        uint32_t w[4] = {0, 0, 0, 0};
        const uint32_t n_here = total - g < TX_LANE_BYTES ? (uint32_t)(total - g) : TX_LANE_BYTES;
#pragma unroll
        for (uint32_t i = 0; i < TX_LANE_BYTES; i++) {
            if (i < n_here) {
                // (a record holds its final newline at least: the next byte is the next record's; g + i < total, so there is one)
                if (g + i == c.end) tx_open(c, rec, toff, ++k, g + i, width);
                w[i >> 2] |= tx_byte(c, letters, heads, tab, width) << (8 * (i & 3));
            }
        }
        if (n_here == TX_LANE_BYTES) *reinterpret_cast<uint4 *>(text + g) = make_uint4(w[0], w[1], w[2], w[3]);
        else {
#pragma unroll
            for (uint32_t i = 0; i < TX_LANE_BYTES; i++)
                if (i < n_here) text[g + i] = (uint8_t)(w[i >> 2] >> (8 * (i & 3)));
        }
    }
}

extern "C" int gmg_text_params_reference(gmg_text_params *p, uint32_t width)
{
    if (!p) return gmg_set_error(GMG_EINVAL, "gmg_text_params_reference: NULL argument");
    static const char from[] = "acgtrykmbdhvswn", to[] = "tgcayrmkvhdbswn";
    for (int ch = 0; ch < 256; ch++) {
        p->fwd[ch] = (uint8_t)ch;
        uint8_t c = 'n';
        if (ch == ' ' || ch == '*' || ch == '-' || ch == '.' || ch == '_') c = (uint8_t)ch;
        else if (ch >= 'a' && ch <= 'z') { const char *f = strchr(from, ch); if (f) c = (uint8_t)to[f - from]; }
        else if (ch >= 'A' && ch <= 'Z') { const char *f = strchr(from, ch + 32); c = (uint8_t)(f ? to[f - from] - 32 : 'N'); }
        p->rev[ch] = c;
    }
    p->width = width;
    p->reserved = 0;
    return GMG_OK;
}

extern "C" int gmg_letters_upload(const char *letters, const uint64_t *base_offsets, uint64_t n_reads, gmg_letters **out)
{
    { int rc_enter = gmg_enter("gmg_letters_upload"); if (rc_enter) return rc_enter; }
    if (!base_offsets || !out || base_offsets[0] != 0) return gmg_set_error(GMG_EINVAL, "gmg_letters_upload: bad argument");
    for (uint64_t r = 0; r < n_reads; r++)
        if (base_offsets[r + 1] < base_offsets[r]) return gmg_set_error(GMG_EINVAL, "gmg_letters_upload: the offsets descend at read %llu", (unsigned long long)r);
    const uint64_t total = base_offsets[n_reads];
    if (!letters && total) return gmg_set_error(GMG_EINVAL, "gmg_letters_upload: NULL letters");
    std::unique_ptr<gmg_letters> l(new (std::nothrow) gmg_letters());
    if (!l) return gmg_set_error(GMG_ENOMEM, "gmg_letters_upload: out of host memory");
    GMG_HIP(l->own.alloc(&l->d_letters, total ? total : 1));
    if (total) GMG_HIP(hipMemcpy(l->d_letters, letters, total, hipMemcpyHostToDevice));
    GMG_HIP(hipEventCreate(&l->ev[0]));
    GMG_HIP(hipEventCreate(&l->ev[1]));
    l->off.assign(base_offsets, base_offsets + n_reads + 1);
    l->n_reads = n_reads;
    *out = l.release();
    return GMG_OK;
}

extern "C" int gmg_letters_free(gmg_letters *l)
{
    if (!l) return GMG_OK;
    delete l;
    return GMG_OK;
}

extern "C" int gmg_letters_kernel_ms(const gmg_letters *l, float *ms)
{
    { int rc_enter = gmg_enter("gmg_letters_kernel_ms"); if (rc_enter) return rc_enter; }
    if (!l || !ms) return gmg_set_error(GMG_EINVAL, "gmg_letters_kernel_ms: NULL argument");
    *ms = 0.0f;
    if (l->timed) GMG_HIP(hipEventElapsedTime(ms, l->ev[0], l->ev[1]));
    return GMG_OK;
}

// The text on the device (in l->d_text), or with only_size just its length.  Returns with the kernel queued on s, not waited for.
static int text_run(const char *who, gmg_letters *l, const gmg_gene_region *regions, uint64_t n, const char *heads, const uint64_t *head_off,
                    const gmg_text_params *prm, bool only_size, size_t cap, bool check_cap, size_t *bytes, GmgScratch &sc, hipStream_t s)
{
    if (!l || (!regions && n) || (!head_off && n) || !prm || !bytes) return gmg_set_error(GMG_EINVAL, "%s: NULL argument", who);
    if (n && head_off[0] != 0) return gmg_set_error(GMG_EINVAL, "%s: head_off[0] must be 0", who);
    std::vector<TxRec> rec;
    std::vector<uint64_t> toff;
    try {
        rec.resize(n);
        toff.resize(n + 1);
    } catch (const std::bad_alloc &) {
        return gmg_set_error(GMG_ENOMEM, "%s: out of host memory", who);
    }
    const uint64_t width = prm->width;
    uint64_t total = 0;
    for (uint64_t k = 0; k < n; k++) {
        const gmg_gene_region &r = regions[k];
        uint64_t b = 0, L = 0;
        bool fits = r.read < l->n_reads && r.strand != 0 && r.first >= 0 && r.len >= 0;
        if (fits) {
            b = l->off[r.read];
            L = l->off[(uint64_t)r.read + 1] - b;
            fits = (uint64_t)r.first < L && (uint64_t)r.len <= L && L < 0x80000000ull;
        }
        if (!fits)
            return gmg_set_error(GMG_ERANGE, "%s: region %llu (read %u, first %d, len %d, strand %d) does not fit its read (the batch has %llu)", who,
                                 (unsigned long long)k, r.read, r.first, r.len, r.strand, (unsigned long long)l->n_reads);
        if (head_off[k + 1] < head_off[k] || head_off[k + 1] - head_off[k] > 0xffffffffull)
            return gmg_set_error(GMG_EINVAL, "%s: head %llu: the offsets must ascend, a head is shorter than 2^32 bytes", who, (unsigned long long)k);
        const uint64_t hlen = head_off[k + 1] - head_off[k], nlet = (uint64_t)r.len;
        TxRec &m = rec[k];
        m.src = b;
        m.head = head_off[k];
        m.L = (uint32_t)L;
        m.first = (uint32_t)r.first;
        m.hlen = (uint32_t)hlen;
        m.nlet = (uint32_t)nlet | (r.strand < 0 ? TX_REV : 0u);
        toff[k] = total;
        total += hlen + nlet + (width && nlet ? (nlet - 1) / width : 0) + 1;
    }
    toff[n] = total;
    const uint64_t n_heads = n ? head_off[n] : 0;
    if (n_heads && !heads) return gmg_set_error(GMG_EINVAL, "%s: NULL heads", who);
    l->timed = 0;
    if (only_size) { *bytes = (size_t)total; return GMG_OK; }
    if (check_cap && cap < total) {
        const int rc = gmg_set_error(GMG_ERANGE, "%s: buffer of %zu bytes, the text needs %llu", who, cap, (unsigned long long)total);
        *bytes = (size_t)total;
        return rc;
    }
    *bytes = (size_t)total;
    if (total == 0) return GMG_OK;
    // (whole 16-byte pieces: the block cache hands out 256-byte aligned blocks; an earlier text goes back once s has come this far)
    if (l->cap_text < total) GMG_HIP(l->own.regrow(l->d_text, l->cap_text, (size_t)((total + 255) & ~255ull), &s));
    TxRec *d_rec = nullptr;
    uint64_t *d_toff = nullptr;
    uint8_t *d_heads = nullptr, *d_tab = nullptr;
    GMG_HIP(sc.alloc(&d_rec, n * sizeof(TxRec)));
    GMG_HIP(sc.alloc(&d_toff, (n + 1) * 8));
    GMG_HIP(sc.alloc(&d_heads, n_heads ? n_heads : 1));
    GMG_HIP(sc.alloc(&d_tab, 512));
    // (pageable sources: every copy has left the host buffer when the call returns)
    GMG_HIP(hipMemcpyAsync(d_rec, rec.data(), n * sizeof(TxRec), hipMemcpyHostToDevice, s));
    GMG_HIP(hipMemcpyAsync(d_toff, toff.data(), (n + 1) * 8, hipMemcpyHostToDevice, s));
    if (n_heads) GMG_HIP(hipMemcpyAsync(d_heads, heads, n_heads, hipMemcpyHostToDevice, s));
    GMG_HIP(hipMemcpyAsync(d_tab, prm->fwd, 256, hipMemcpyHostToDevice, s));
    GMG_HIP(hipMemcpyAsync(d_tab + 256, prm->rev, 256, hipMemcpyHostToDevice, s));
    const uint64_t n_tiles = (total + TX_TILE - 1) / TX_TILE;
    if (n_tiles > 0x7fffffffull) return gmg_set_error(GMG_ETOOBIG, "%s: a text of %llu bytes", who, (unsigned long long)total);
    GMG_HIP(hipEventRecord(l->ev[0], s));
    hipLaunchKernelGGL(k_regions_text, dim3((unsigned)n_tiles), dim3(TX_BLOCK), 0, s, l->d_letters, d_rec, d_toff, n, d_heads, d_tab,
                       (uint32_t)width, total, (uint8_t *)l->d_text);
    GMG_HIP(hipGetLastError());
    GMG_HIP(hipEventRecord(l->ev[1], s));
    l->timed = 1;
    return GMG_OK;
}

extern "C" int gmg_regions_text(gmg_letters *l, const gmg_gene_region *regions, uint64_t n, const char *heads, const uint64_t *head_off,
                                const gmg_text_params *prm, char *host_out, size_t *bytes, void *stream)
{
    { int rc_enter = gmg_enter("gmg_regions_text"); if (rc_enter) return rc_enter; }
    hipStream_t s = (hipStream_t)stream;
    GmgScratch sc(GmgScratch::STREAM, s);
    const size_t cap = bytes ? *bytes : 0;
    const int rc = text_run("gmg_regions_text", l, regions, n, heads, head_off, prm, host_out == nullptr, cap, true, bytes, sc, s);
    if (rc || !host_out || *bytes == 0) return rc;
    GMG_HIP(hipMemcpyAsync(host_out, l->d_text, *bytes, hipMemcpyDeviceToHost, s));
    GMG_HIP(hipStreamSynchronize(s));
    return GMG_OK;
}

extern "C" int gmg_regions_text_device(gmg_letters *l, const gmg_gene_region *regions, uint64_t n, const char *heads, const uint64_t *head_off,
                                       const gmg_text_params *prm, const char **d_text, size_t *bytes, void *stream)
{
    { int rc_enter = gmg_enter("gmg_regions_text_device"); if (rc_enter) return rc_enter; }
    if (!d_text) return gmg_set_error(GMG_EINVAL, "gmg_regions_text_device: NULL argument");
    hipStream_t s = (hipStream_t)stream;
    GmgScratch sc(GmgScratch::STREAM, s);
    *d_text = nullptr;
    const int rc = text_run("gmg_regions_text_device", l, regions, n, heads, head_off, prm, false, 0, false, bytes, sc, s);
    if (rc) return rc;
    GMG_HIP(hipStreamSynchronize(s));
    *d_text = *bytes ? l->d_text : nullptr;
    return GMG_OK;
}
