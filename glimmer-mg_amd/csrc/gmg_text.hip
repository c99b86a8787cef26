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
//
// gmg_runs_text (further down) writes the strings of extract_aa.py -- runs of the reads, pad blanks around them -- or their
// translations through the same walk (tx_tile): only what character j of a record is differs (RtChars).

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

// ---- the record walk, shared by every text kernel: a record type R holds at least `head` (offset of its head in the heads) and
// `hlen` (the head's bytes); what character j of a record is, is the kernel's own business ----

// where a lane stands in the text: in record k, at byte q of it
template <class R>
struct TxCursor {
    R m;
    uint64_t end;                // text offset of the next record
    uint64_t q;                  // byte of the record
    uint64_t body;               // bytes behind the head: characters, the lines' newlines, the final newline
    uint32_t j, col;             // next character; characters already on the line
};

template <class R>
__device__ __forceinline__ void tx_open(TxCursor<R> &c, const R *__restrict__ rec, const uint64_t *__restrict__ toff, uint64_t k, uint64_t g,
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

// the next byte of the record: a head byte, the final newline, a line's newline, or character j = character (k, c.m, j)
template <class R, class F>
__device__ __forceinline__ uint32_t tx_byte(TxCursor<R> &c, uint64_t k, const uint8_t *__restrict__ heads, uint32_t width, F &character)
{
    uint32_t ch;
    if (c.q < c.m.hlen) ch = heads[c.m.head + c.q];
    else if (c.q - c.m.hlen == c.body - 1) ch = '\n';
    else if (width && c.col == width) { ch = '\n'; c.col = 0; }
    else {
        ch = character(k, c.m, c.j);
        c.j++;
        c.col++;
    }
    c.q++;
    return ch;
}

// A work-group's TX_TILE bytes of the text (there is text: n >= 1): 16 bytes per lane and pass, one 16-byte store each
template <class R, class F>
__device__ __forceinline__ void tx_tile(const R *__restrict__ rec, const uint64_t *__restrict__ toff, const uint64_t n,
                                        const uint8_t *__restrict__ heads, const uint32_t width, const uint64_t total, uint8_t *__restrict__ text,
                                        const F &character)
{
    const uint64_t tile0 = (uint64_t)blockIdx.x * TX_TILE;
    if (tile0 >= total) return;
    const uint64_t tile_last = tile0 + TX_TILE - 1 < total - 1 ? tile0 + TX_TILE - 1 : total - 1;
    // the tile's records: the same for every lane
    const uint64_t klo = tx_find(toff, 0, n - 1, tile0), khi = tx_find(toff, klo, n - 1, tile_last);
#pragma unroll 1
    for (int pass = 0; pass < TX_PASSES; pass++) {
        const uint64_t g = tile0 + ((uint64_t)pass * TX_BLOCK + threadIdx.x) * TX_LANE_BYTES;
        if (g >= total) return;
        TxCursor<R> c;
        F ch = character;                               // (whatever it keeps from character to character starts over with the lane's bytes)
        uint64_t k = tx_find(toff, klo, khi, g);
        tx_open(c, rec, toff, k, g, width);
        uint32_t w[4] = {0, 0, 0, 0};
        const uint32_t n_here = total - g < TX_LANE_BYTES ? (uint32_t)(total - g) : TX_LANE_BYTES;
#pragma unroll
        for (uint32_t i = 0; i < TX_LANE_BYTES; i++) {
            if (i < n_here) {
                // (a record holds its final newline at least: the next byte is the next record's; g + i < total, so there is one)
                if (g + i == c.end) tx_open(c, rec, toff, ++k, g + i, width);
                w[i >> 2] |= tx_byte(c, k, heads, width, ch) << (8 * (i & 3));
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

// letter j of a region: position first + j (forward) or first - j (reverse) of the read, modulo its length, through the strand's table
struct TxRegionLetter {
    const uint8_t *__restrict__ letters;
    const uint8_t *tab;          // LDS: fwd, rev
    __device__ __forceinline__ uint32_t operator()(uint64_t, const TxRec &m, uint32_t j) const
    {
        const bool rev = (m.nlet & TX_REV) != 0;
        uint32_t p;
        if (!rev) { p = m.first + j; if (p >= m.L) p -= m.L; }
        else p = m.first >= j ? m.first - j : m.first + m.L - j;
        return tab[(rev ? 256u : 0u) + letters[m.src + p]];
    }
};

__global__ __launch_bounds__(TX_BLOCK) void k_regions_text(const uint8_t *__restrict__ letters, const TxRec *__restrict__ rec,
                                                           const uint64_t *__restrict__ toff, const uint64_t n, const uint8_t *__restrict__ heads,
                                                           const uint8_t *__restrict__ tables, const uint32_t width, const uint64_t total,
                                                           uint8_t *__restrict__ text)
{
    __shared__ uint8_t tab[512];
    tab[threadIdx.x] = tables[threadIdx.x];
    tab[256 + threadIdx.x] = tables[256 + threadIdx.x];
    __syncthreads();
    TxRegionLetter letter{letters, tab};
    tx_tile(rec, toff, n, heads, width, total, text, letter);
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
    GMG_HANDLE_READY();
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

// What every text call does once the length of its text is known: report it in *bytes, and -- unless only the length was asked
// for, the caller's buffer is too small (GMG_ERANGE) or there is no text -- make room for it in the handle's buffer (*write).
static int text_room(const char *who, gmg_letters *l, uint64_t total, bool only_size, size_t cap, bool check_cap, size_t *bytes, hipStream_t s,
                     bool *write)
{
    *write = false;
    l->timed = 0;
    if (only_size) { *bytes = (size_t)total; return GMG_OK; }
    if (check_cap && cap < total) {
        const int rc = gmg_set_error(GMG_ERANGE, "%s: buffer of %zu bytes, the text needs %llu", who, cap, (unsigned long long)total);
        *bytes = (size_t)total;
        return rc;
    }
    *bytes = (size_t)total;
    if (total == 0) return GMG_OK;
    if ((total + TX_TILE - 1) / TX_TILE > 0x7fffffffull) return gmg_set_error(GMG_ETOOBIG, "%s: a text of %llu bytes", who, (unsigned long long)total);
    // (whole 16-byte pieces: the block cache hands out 256-byte aligned blocks; an earlier text goes back once s has come this far)
    if (l->cap_text < total) GMG_HIP(l->own.regrow(l->d_text, l->cap_text, (size_t)((total + 255) & ~255ull), &s));
    *write = true;
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
    bool write = false;
    { const int rc = text_room(who, l, total, only_size, cap, check_cap, bytes, s, &write); if (rc || !write) return rc; }
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
    GMG_HIP(hipEventRecord(l->ev[0], s));
    hipLaunchKernelGGL(k_regions_text, dim3((unsigned)((total + TX_TILE - 1) / TX_TILE)), dim3(TX_BLOCK), 0, s, l->d_letters, d_rec, d_toff, n, d_heads, d_tab,
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

// ---- gmg_runs_text: the strings of extract_aa.py -- pad bytes, runs of the reads, pad bytes -- or their translations, as text --------
// The same kernel shape; character j of record k is byte j of its printed string P_k (DNA) or the translation of bytes 3j .. 3j + 2
// (protein).  Byte p of P_k is a pad byte in front of pad_front and from pad_end on; in between it lies in the run r of the record
// with at[r] <= p < at[r] + len[r], at = the prefix sum of the runs' lengths inside P_k, pad_front included: a lane finds r by
// binary search over the record's runs when it first needs a byte of the record, and walks on run by run from there (its bytes
// ascend).  The four letter tables, the literals, the amino letters and the codon class of every byte stand in LDS.

struct RtRec {
    uint64_t head;               // offset of the record's head in the heads
    uint64_t run0;               // the record's first run
    uint32_t hlen;               // bytes of the head
    uint32_t n_runs;
    uint32_t pad_front, pad_end; // P = pad bytes [0, pad_front), the runs' bytes [pad_front, pad_end), pad bytes from pad_end on
};

struct RtRun {
    uint64_t src;                // job-wide index of the letter at `first` (bits 0 .. 55), the kind (bits 56 .. 63)
    uint32_t len;
    uint32_t at;                 // offset of the run's byte 0 in P
};
#define RT_KIND_SHIFT 56
#define RT_TABLES 1024           // up, down, sub_up, sub_down: in the order of the kinds GMG_RUN_UP .. GMG_RUN_SUB_DOWN
#define RT_OTHER 8u              // codon class of a byte: 0 .. 3 upper-case A C G T, 4 .. 7 lower-case a c g t, RT_OTHER anything else

__device__ __forceinline__ uint32_t rt_class(uint32_t ch)
{
    const uint32_t lower = (ch & 0x20u) ? 4u : 0u;
    switch (ch & ~0x20u) {
    case 'A': return lower;
    case 'C': return lower + 1;
    case 'G': return lower + 2;
    case 'T': return lower + 3;
    }
    return RT_OTHER;
}

template <int MODE>
struct RtChars {
    const uint8_t *__restrict__ letters;
    const RtRun *__restrict__ runs;
    const uint8_t *tab, *lit, *aa, *cls;     // LDS
    uint32_t pad, unknown;
    uint64_t open_k, r;                      // the record the run cursor stands in (~0: none), its run
    RtRun u;

    __device__ __forceinline__ uint32_t byte(uint64_t k, const RtRec &m, uint32_t p)
    {
        if (p < m.pad_front || p >= m.pad_end) return pad;
        if (open_k != k) {                   // (pad_front <= p < pad_end: the record has runs, and one of them holds p)
            uint64_t lo = m.run0, hi = m.run0 + m.n_runs - 1;
            while (lo < hi) {
                const uint64_t mid = lo + (hi - lo + 1) / 2;
                if (runs[mid].at <= p) lo = mid;
                else hi = mid - 1;
            }
            r = lo;
            u = runs[r];
            open_k = k;
        } else {
            while (p - u.at >= u.len) u = runs[++r];
        }
        const uint32_t kind = (uint32_t)(u.src >> RT_KIND_SHIFT), i = p - u.at;
        const uint64_t b = u.src & ((1ull << RT_KIND_SHIFT) - 1);
        if (kind >= GMG_RUN_LITERAL_AS_IS) return tab[letters[b]];
        if (kind >= GMG_RUN_LITERAL) return lit[kind & 3u];
        return tab[(kind << 8) + letters[(kind & 1u) ? b - i : b + i]];
    }

    __device__ __forceinline__ uint32_t operator()(uint64_t k, const RtRec &m, uint32_t j)
    {
        if (MODE == GMG_RUNS_TEXT_DNA) return byte(k, m, j);
        const uint32_t c0 = cls[byte(k, m, 3 * j)], c1 = cls[byte(k, m, 3 * j + 1)], c2 = cls[byte(k, m, 3 * j + 2)];
        if (((c0 | c1 | c2) & RT_OTHER) || (((c0 ^ c1) | (c0 ^ c2)) & 4u)) return unknown;
        uint32_t a = aa[16 * (c0 & 3u) + 4 * (c1 & 3u) + (c2 & 3u)];
        if ((c0 & 4u) && a >= 'A' && a <= 'Z') a += 'a' - 'A';
        return a;
    }
};

template <int MODE>
__global__ __launch_bounds__(TX_BLOCK) void k_runs_text(const uint8_t *__restrict__ letters, const RtRec *__restrict__ rec,
                                                        const uint64_t *__restrict__ toff, const uint64_t n, const RtRun *__restrict__ runs,
                                                        const uint8_t *__restrict__ heads, const gmg_runs_text_params *__restrict__ prm,
                                                        const uint32_t width, const uint32_t pad, const uint32_t unknown, const uint64_t total,
                                                        uint8_t *__restrict__ text)
{
    __shared__ uint8_t tab[RT_TABLES], cls[256], aa[64], lit[4];
    const uint8_t *tables = reinterpret_cast<const uint8_t *>(prm);                      // (up, down, sub_up, sub_down back to back)
    for (uint32_t i = threadIdx.x; i < RT_TABLES; i += TX_BLOCK) tab[i] = tables[i];
    cls[threadIdx.x] = (uint8_t)rt_class(threadIdx.x);
    if (threadIdx.x < 64) aa[threadIdx.x] = (uint8_t)prm->aa[threadIdx.x];
    if (threadIdx.x < 4) lit[threadIdx.x] = prm->literal[threadIdx.x];
    __syncthreads();
    RtChars<MODE> chars{letters, runs, tab, lit, aa, cls, pad, unknown, ~0ull, 0, RtRun{0, 0, 0}};
    tx_tile(rec, toff, n, heads, width, total, text, chars);
}

static_assert(offsetof(gmg_runs_text_params, down) == 256 && offsetof(gmg_runs_text_params, sub_up) == 512 &&
              offsetof(gmg_runs_text_params, sub_down) == 768 && offsetof(gmg_runs_text_params, literal) == RT_TABLES,
              "the kernel reads the four letter tables as one array");

extern "C" int gmg_runs_text_params_script(gmg_runs_text_params *p, int mode, int transl_table)
{
    if (!p) return gmg_set_error(GMG_EINVAL, "gmg_runs_text_params_script: NULL argument");
    if (mode != GMG_RUNS_TEXT_DNA && mode != GMG_RUNS_TEXT_PROTEIN) return gmg_set_error(GMG_EINVAL, "gmg_runs_text_params_script: mode %d", mode);
    memset(p, 0, sizeof *p);
    static const char from[] = "ATCGatcg", to[] = "TAGCtagc";
    for (int ch = 0; ch < 256; ch++) {
        const char *f = ch ? strchr(from, ch) : nullptr;
        p->up[ch] = (uint8_t)ch;
        p->down[ch] = f ? (uint8_t)to[f - from] : (uint8_t)ch;
        p->sub_up[ch] = ch == 'C' ? 'G' : 'C';
        p->sub_down[ch] = ch == 'C' ? 'C' : 'G';
    }
    memcpy(p->literal, "ACGT", 4);
    p->pad = ' ';
    p->unknown = 'X';
    p->mode = (uint32_t)mode;
    // extract_aa.py's dictionary is the standard code; any other table is Codon_Translation's
    return gmg_xlate_table(transl_table == 0 ? 1 : transl_table, p->aa);
}

// The text on the device (in l->d_text), or with only_size just its length.  Returns with the kernel queued on s, not waited for.
static int runs_run(const char *who, gmg_letters *l, const gmg_splice_run *runs, uint64_t n_runs, const uint64_t *sro, uint64_t n,
                    const uint32_t *pad_front, const uint32_t *pad_behind, const char *heads, const uint64_t *head_off,
                    const gmg_runs_text_params *prm, bool only_size, size_t cap, bool check_cap, size_t *bytes, GmgScratch &sc, hipStream_t s)
{
    if (!l || (!runs && n_runs) || !sro || (!head_off && n) || !prm || !bytes) return gmg_set_error(GMG_EINVAL, "%s: NULL argument", who);
    if (prm->mode > GMG_RUNS_TEXT_PROTEIN || prm->reserved[0] || prm->reserved[1])
        return gmg_set_error(GMG_EINVAL, "%s: mode %u, reserved %u %u", who, prm->mode, prm->reserved[0], prm->reserved[1]);
    if (sro[0] != 0 || sro[n] != n_runs) return gmg_set_error(GMG_EINVAL, "%s: string_run_off must run from 0 to n_runs", who);
    for (uint64_t k = 0; k < n; k++)
        if (sro[k] > sro[k + 1]) return gmg_set_error(GMG_EINVAL, "%s: string_run_off descends at string %llu", who, (unsigned long long)k);
    if (n && head_off[0] != 0) return gmg_set_error(GMG_EINVAL, "%s: head_off[0] must be 0", who);
    std::vector<RtRec> rec;
    std::vector<RtRun> run;
    std::vector<uint64_t> toff;
    try {
        rec.resize(n);
        run.resize(n_runs);
        toff.resize(n + 1);
    } catch (const std::bad_alloc &) {
        return gmg_set_error(GMG_ENOMEM, "%s: out of host memory", who);
    }
    const uint64_t width = prm->width;
    uint64_t total = 0;
    for (uint64_t k = 0; k < n; k++) {
        const uint64_t front = pad_front ? pad_front[k] : 0, behind = pad_behind ? pad_behind[k] : 0;
        uint64_t plen = front;
        for (uint64_t q = sro[k]; q < sro[k + 1]; q++) {
            const gmg_splice_run &r = runs[q];
            const bool literal = r.kind >= GMG_RUN_LITERAL && r.kind < GMG_RUN_LITERAL_AS_IS, as_is = r.kind >= GMG_RUN_LITERAL_AS_IS;
            bool fits = r.kind < GMG_RUN_LITERAL_AS_IS + 4;
            uint64_t b = 0;
            if (fits && !literal && !(as_is && r.len == 0)) {
                fits = r.read < l->n_reads;
                if (fits) {
                    b = l->off[r.read];
                    const uint64_t L = l->off[(uint64_t)r.read + 1] - b;
                    if (as_is) fits = r.first < L;
                    else if (!(r.kind & 1u)) fits = (uint64_t)r.first + r.len <= L;
                    else fits = r.len ? r.first < L && (uint64_t)r.len <= (uint64_t)r.first + 1 : r.first <= L;
                    b += r.first;
                }
            }
            if (!fits)
                return gmg_set_error(GMG_ERANGE, "%s: run %llu (read %u, first %u, len %u, kind %u) does not fit its read (the batch has %llu)", who,
                                     (unsigned long long)q, r.read, r.first, r.len, r.kind, (unsigned long long)l->n_reads);
            if (b >> RT_KIND_SHIFT) return gmg_set_error(GMG_ETOOBIG, "%s: a batch of 2^56 letters or more", who);
            if (plen > 0xffffffffull) break;            // (reported below; `at` would not hold it)
            run[q].src = b | ((uint64_t)r.kind << RT_KIND_SHIFT);
            run[q].len = r.len;
            run[q].at = (uint32_t)plen;
            plen += r.len;
        }
        const uint64_t pad_end = plen;
        plen += behind;
        if (plen > 0xffffffffull || sro[k + 1] - sro[k] > 0xffffffffull)
            return gmg_set_error(GMG_ERANGE, "%s: string %llu has 2^32 characters or runs or more", who, (unsigned long long)k);
        if (head_off[k + 1] < head_off[k] || head_off[k + 1] - head_off[k] > 0xffffffffull)
            return gmg_set_error(GMG_EINVAL, "%s: head %llu: the offsets must ascend, a head is shorter than 2^32 bytes", who, (unsigned long long)k);
        const uint64_t hlen = head_off[k + 1] - head_off[k], nchar = prm->mode == GMG_RUNS_TEXT_PROTEIN ? plen / 3 : plen;
        RtRec &m = rec[k];
        m.head = head_off[k];
        m.run0 = sro[k];
        m.hlen = (uint32_t)hlen;
        m.n_runs = (uint32_t)(sro[k + 1] - sro[k]);
        m.pad_front = (uint32_t)front;
        m.pad_end = (uint32_t)pad_end;
        toff[k] = total;
        total += hlen + nchar + (width && nchar ? (nchar - 1) / width : 0) + 1;
    }
    toff[n] = total;
    const uint64_t n_heads = n ? head_off[n] : 0;
    if (n_heads && !heads) return gmg_set_error(GMG_EINVAL, "%s: NULL heads", who);
    bool write = false;
    { const int rc = text_room(who, l, total, only_size, cap, check_cap, bytes, s, &write); if (rc || !write) return rc; }
    RtRec *d_rec = nullptr;
    RtRun *d_run = nullptr;
    uint64_t *d_toff = nullptr;
    uint8_t *d_heads = nullptr;
    gmg_runs_text_params *d_prm = nullptr;
    GMG_HIP(sc.alloc(&d_rec, n * sizeof(RtRec)));
    GMG_HIP(sc.alloc(&d_run, (n_runs ? n_runs : 1) * sizeof(RtRun)));
    GMG_HIP(sc.alloc(&d_toff, (n + 1) * 8));
    GMG_HIP(sc.alloc(&d_heads, n_heads ? n_heads : 1));
    GMG_HIP(sc.alloc(&d_prm, sizeof *prm));
    // (pageable sources: every copy has left the host buffer when the call returns)
    GMG_HIP(hipMemcpyAsync(d_rec, rec.data(), n * sizeof(RtRec), hipMemcpyHostToDevice, s));
    if (n_runs) GMG_HIP(hipMemcpyAsync(d_run, run.data(), n_runs * sizeof(RtRun), hipMemcpyHostToDevice, s));
    GMG_HIP(hipMemcpyAsync(d_toff, toff.data(), (n + 1) * 8, hipMemcpyHostToDevice, s));
    if (n_heads) GMG_HIP(hipMemcpyAsync(d_heads, heads, n_heads, hipMemcpyHostToDevice, s));
    GMG_HIP(hipMemcpyAsync(d_prm, prm, sizeof *prm, hipMemcpyHostToDevice, s));
    const dim3 grid((unsigned)((total + TX_TILE - 1) / TX_TILE));
    GMG_HIP(hipEventRecord(l->ev[0], s));
    if (prm->mode == GMG_RUNS_TEXT_PROTEIN)
        hipLaunchKernelGGL(k_runs_text<GMG_RUNS_TEXT_PROTEIN>, grid, dim3(TX_BLOCK), 0, s, l->d_letters, d_rec, d_toff, n, d_run, d_heads, d_prm,
                           (uint32_t)width, (uint32_t)prm->pad, (uint32_t)prm->unknown, total, (uint8_t *)l->d_text);
    else
        hipLaunchKernelGGL(k_runs_text<GMG_RUNS_TEXT_DNA>, grid, dim3(TX_BLOCK), 0, s, l->d_letters, d_rec, d_toff, n, d_run, d_heads, d_prm,
                           (uint32_t)width, (uint32_t)prm->pad, (uint32_t)prm->unknown, total, (uint8_t *)l->d_text);
    GMG_HIP(hipGetLastError());
    GMG_HIP(hipEventRecord(l->ev[1], s));
    l->timed = 1;
    return GMG_OK;
}

extern "C" int gmg_runs_text(gmg_letters *l, const gmg_splice_run *runs, uint64_t n_runs, const uint64_t *string_run_off, uint64_t n_strings,
                             const uint32_t *pad_front, const uint32_t *pad_behind, const char *heads, const uint64_t *head_off,
                             const gmg_runs_text_params *prm, char *host_out, size_t *bytes, void *stream)
{
    { int rc_enter = gmg_enter("gmg_runs_text"); if (rc_enter) return rc_enter; }
    hipStream_t s = (hipStream_t)stream;
    GmgScratch sc(GmgScratch::STREAM, s);
    const size_t cap = bytes ? *bytes : 0;
    const int rc = runs_run("gmg_runs_text", l, runs, n_runs, string_run_off, n_strings, pad_front, pad_behind, heads, head_off, prm,
                            host_out == nullptr, cap, true, bytes, sc, s);
    if (rc || !host_out || *bytes == 0) return rc;
    GMG_HIP(hipMemcpyAsync(host_out, l->d_text, *bytes, hipMemcpyDeviceToHost, s));
    GMG_HIP(hipStreamSynchronize(s));
    return GMG_OK;
}

extern "C" int gmg_runs_text_device(gmg_letters *l, const gmg_splice_run *runs, uint64_t n_runs, const uint64_t *string_run_off,
                                    uint64_t n_strings, const uint32_t *pad_front, const uint32_t *pad_behind, const char *heads,
                                    const uint64_t *head_off, const gmg_runs_text_params *prm, const char **d_text, size_t *bytes, void *stream)
{
    { int rc_enter = gmg_enter("gmg_runs_text_device"); if (rc_enter) return rc_enter; }
    if (!d_text) return gmg_set_error(GMG_EINVAL, "gmg_runs_text_device: NULL argument");
    hipStream_t s = (hipStream_t)stream;
    GmgScratch sc(GmgScratch::STREAM, s);
    *d_text = nullptr;
    const int rc = runs_run("gmg_runs_text_device", l, runs, n_runs, string_run_off, n_strings, pad_front, pad_behind, heads, head_off, prm, false,
                            0, false, bytes, sc, s);
    if (rc) return rc;
    GMG_HIP(hipStreamSynchronize(s));
    *d_text = *bytes ? l->d_text : nullptr;
    return GMG_OK;
}
