// gmg_edits_plan.cc -- the host side of gmg_reads_splice (include/gmg.h): the edit arithmetic of scripts/extract_aa.py, from the
// gene lines of a predict file to the runs of their strings.  Host only; the rules are restated beside the declaration.
//
// Per read: the corrected read (predict_msa) as a short list of segments -- stretches of the read, single substituted bases, the
// one blank a deletion at base 1 duplicates -- built by hopping from listed position to listed position, O(edits); per gene the
// intervals of corrected characters its walk collects (print_frag_genes), found by stepping over the at most five stretches
// between the walk's two three-character windows instead of over every character; the intervals cut out of the segments are
// the runs.

#include "../../include/gmg.h"

#include <stdint.h>
#include <stddef.h>

#include <algorithm>
#include <vector>

extern int gmg_set_error(int code, const char *fmt, ...);

namespace {

enum { SEG_COPY, SEG_SUB, SEG_BLANK };
struct Seg { int64_t s0, p, len; int kind; };           // corrected characters s0 .. s0 + len - 1: the read from position p upwards
struct Iv { int64_t a, b; };

struct Corrected {
    std::vector<Seg> segs;
    int64_t len = 0;                                    // characters between the pads
    int64_t pads_behind = 3;
    bool blank0 = false;                                // character 0 is the blank a deletion at base 1 put there
    void put(int kind, int64_t p, int64_t n)
    {
        if (n <= 0) return;
        if (kind == SEG_COPY && !segs.empty() && segs.back().kind == SEG_COPY && segs.back().p + segs.back().len == p) segs.back().len += n;
        else { const Seg s = {len, p, n, kind}; segs.push_back(s); }
        len += n;
    }
    bool blank(int64_t s) const { return s < 0 || s >= len || (s == 0 && blank0); }
};

// predict_msa.  ins, del, sub: the sorted 0-based lists of the read
void correct(int64_t L, const std::vector<int64_t> &ins, const std::vector<int64_t> &del, const std::vector<int64_t> &sub, Corrected &c)
{
    enum { NOTHING, BLANK, BASE, SUBST } prev = BLANK;  // what the step before put out (the front pad before step 0)
    size_t i = 0, d = 0, s = 0;
    int64_t f = 0, fired = 0;
    const int64_t never = INT64_MAX;
    for (;;) {
        // a cursor whose position lies behind f is stuck for good
        const int64_t hi = i < ins.size() && ins[i] >= f ? ins[i] : never, hd = d < del.size() && del[d] >= f ? del[d] : never,
                      hs = s < sub.size() && sub[s] >= f ? sub[s] : never;
        if (hi == never) i = ins.size();
        if (hd == never) d = del.size();
        if (hs == never) s = sub.size();
        const int64_t next = std::min(hi, std::min(hd, hs));
        if (next >= L) { c.put(SEG_COPY, f, L - f); break; }
        if (next > f) { c.put(SEG_COPY, f, next - f); prev = BASE; f = next; }
        if (hi == f) { i++; prev = NOTHING; }
        else if (hd == f) {
            d++; fired++;
            if (prev == BLANK) { c.blank0 = true; c.put(SEG_BLANK, 0, 1); }
            else if (prev == BASE) c.put(SEG_COPY, f - 1, 1);
            else if (prev == SUBST) c.put(SEG_SUB, f - 1, 1);
            c.put(SEG_COPY, f, 1);
            prev = BASE;
        } else { s++; c.put(SEG_SUB, f, 1); prev = SUBST; }
        f++;
    }
    c.pads_behind = 3 + (int64_t)del.size() - fired;
}

// print_frag_genes' walk over s = -3 .. s_end - 1 for one gene: the intervals of s whose characters make the string, ascending
void walk(bool forward, int64_t start, int64_t end, const Corrected &c, std::vector<Iv> &out)
{
    const int64_t s_lo = -3, s_hi = c.len + c.pads_behind;
    int64_t cut[6] = {s_lo, start, start + 3, end - 3, end, s_hi};
    for (int k = 0; k < 6; k++) cut[k] = std::min(std::max(cut[k], s_lo), s_hi);
    std::sort(cut, cut + 6);
    bool begun = false;
    int phase = -1;                                     // off; otherwise the steps since the start window, modulo 3
    auto add = [&](int64_t a, int64_t b) {
        if (a >= b) return;
        if (!out.empty() && out.back().b == a) out.back().b = b;
        else { const Iv v = {a, b}; out.push_back(v); }
        begun = true;
    };
    for (int k = 0; k + 1 < 6; k++) {
        const int64_t a = cut[k], b = cut[k + 1];
        if (a >= b) continue;
        if (start <= a && a < start + 3) {              // the start window (forward) / the stop codon (reverse)
            phase = 0;
            if (forward)
                for (int64_t s = a; s < b; s++)
                    if (begun || (s == start && s >= 0)) add(s, s + 1);
        } else if (end - 3 <= a && a < end) {
            phase = -1;
            if (!forward)
                for (int64_t s = a; s < b; s++)
                    if (!c.blank(s)) add(s, s + 1);
        } else if (phase >= 0) {
            // step j = s - a + 1 of this stretch has phase (phase + j) % 3; a string begins where that is 1 (the first base of a
            // codon) and s >= 0
            if (begun) add(a, b);
            else
                for (int64_t s = std::max<int64_t>(a, 0); s < b && s < std::max<int64_t>(a, 0) + 3; s++)
                    if ((phase + (s - a + 1)) % 3 == 1) { add(s, b); break; }
            phase = (int)((phase + (b - a)) % 3);
        }
    }
}

struct Out {
    gmg_splice_run *runs;
    uint64_t cap, n;
    void put(uint32_t read, int64_t first, int64_t len, uint32_t kind)
    {
        if (len <= 0) return;
        if (n < cap) { const gmg_splice_run r = {read, (uint32_t)first, (uint32_t)len, kind}; runs[n] = r; }
        n++;
    }
};

struct Odd {
    const uint64_t *base;
    const char *letter;
    uint64_t n;
};

// positions [p, p + len) of a read whose base 0 is job-wide base S, upwards or downwards, copied or substituted: one run, cut
// where a listed letter needs a literal
void put_piece(Out &o, const Odd &odd, uint32_t read, uint64_t S, int64_t p, int64_t len, bool down, bool subst)
{
    const uint32_t kind = subst ? (down ? GMG_RUN_SUB_DOWN : GMG_RUN_SUB_UP) : (down ? GMG_RUN_DOWN : GMG_RUN_UP);
    if (!odd.n || kind == GMG_RUN_UP) { o.put(read, down ? p + len - 1 : p, len, kind); return; }
    const uint64_t *lo = std::lower_bound(odd.base, odd.base + odd.n, S + (uint64_t)p), *hi = std::lower_bound(lo, odd.base + odd.n, S + (uint64_t)(p + len));
    std::vector<std::pair<int64_t, uint32_t> > lit;     // (position, literal kind), ascending
    for (const uint64_t *it = lo; it < hi; ++it) {
        const char ch = odd.letter[it - odd.base];
        if (subst) lit.push_back(std::make_pair((int64_t)(*it - S), (uint32_t)(GMG_RUN_LITERAL + (down ? 2 : 1))));
        else if (ch != 'a' && ch != 'c' && ch != 'g' && ch != 't')
            lit.push_back(std::make_pair((int64_t)(*it - S), (uint32_t)(GMG_RUN_LITERAL_AS_IS + (gmg_base_code((unsigned char)ch) & 3))));
    }
    if (!down) {
        int64_t at = p;
        for (size_t k = 0; k < lit.size(); k++) {
            o.put(read, at, lit[k].first - at, kind);
            o.put(read, lit[k].first, 1, lit[k].second);
            at = lit[k].first + 1;
        }
        o.put(read, at, p + len - at, kind);
    } else {
        int64_t at = p + len - 1;                       // the next position to put out, going down
        for (size_t k = lit.size(); k-- > 0;) {
            o.put(read, at, at - lit[k].first, kind);
            o.put(read, lit[k].first, 1, lit[k].second);
            at = lit[k].first - 1;
        }
        o.put(read, at, at - p + 1, kind);
    }
}

struct Line { uint64_t gene; int64_t start, end; bool forward; };

}  // namespace

extern "C" int gmg_edits_plan(const uint64_t *base_offsets, uint64_t n_reads, const gmg_edit_gene *genes, uint64_t n_genes,
                              const int64_t *positions, const uint64_t *odd_base, const char *odd_letter, uint64_t n_odd,
                              gmg_splice_run *runs, uint64_t runs_cap, uint64_t *n_runs, uint64_t *string_run_off, gmg_edit_string *strings)
{
    if (!base_offsets || (!genes && n_genes) || !n_runs || (runs_cap && !runs) || (n_odd && (!odd_base || !odd_letter)) ||
        (n_genes && (!string_run_off || !strings)))
        return gmg_set_error(GMG_EINVAL, "gmg_edits_plan: bad argument");
    // the lines of every read, in file order (a counting sort by read), and where every line's lists begin
    std::vector<uint64_t> pos_off(n_genes + 1, 0), first_of(n_reads + 1, 0), by_read(n_genes);
    for (uint64_t g = 0; g < n_genes; g++) {
        if (genes[g].read >= n_reads)
            return gmg_set_error(GMG_ERANGE, "gmg_edits_plan: line %llu names sequence %u of %llu", (unsigned long long)g, genes[g].read,
                                 (unsigned long long)n_reads);
        if (base_offsets[genes[g].read + 1] - base_offsets[genes[g].read] >= 0x80000000ull)
            return gmg_set_error(GMG_ERANGE, "gmg_edits_plan: line %llu: sequence %u has 2^31 bases or more", (unsigned long long)g, genes[g].read);
        pos_off[g + 1] = pos_off[g] + genes[g].n_ins + genes[g].n_del + genes[g].n_sub;
        first_of[genes[g].read + 1]++;
    }
    if (pos_off[n_genes] && !positions) return gmg_set_error(GMG_EINVAL, "gmg_edits_plan: positions listed, but no array of them");
    for (uint64_t r = 0; r < n_reads; r++) first_of[r + 1] += first_of[r];
    {
        std::vector<uint64_t> at(first_of.begin(), first_of.end() - 1);
        for (uint64_t g = 0; g < n_genes; g++) by_read[at[genes[g].read]++] = g;
    }
    const Odd odd = {odd_base, odd_letter, n_odd};
    Out o = {runs, runs_cap, 0};
    uint64_t k = 0;                                     // records so far
    std::vector<int64_t> ins, del, sub;
    std::vector<Line> lines;
    std::vector<Iv> ivs;
    if (n_genes) string_run_off[0] = 0;
    for (uint64_t r = 0; r < n_reads; r++) {
        if (first_of[r] == first_of[r + 1]) continue;
        const uint64_t S = base_offsets[r];
        const int64_t L = (int64_t)(base_offsets[r + 1] - S);
        // get_preds
        ins.clear(); del.clear(); sub.clear(); lines.clear();
        int64_t shift = 0;
        for (uint64_t q = first_of[r]; q < first_of[r + 1]; q++) {
            const gmg_edit_gene &g = genes[by_read[q]];
            const int64_t *p = positions + pos_off[by_read[q]];
            for (uint32_t x = 0; x < g.n_ins; x++) ins.push_back(*p++ - 1);
            for (uint32_t x = 0; x < g.n_del; x++) del.push_back(*p++ - 1);
            for (uint32_t x = 0; x < g.n_sub; x++) sub.push_back(*p++ - 1);
            Line l;
            l.gene = by_read[q];
            l.forward = g.frame > 0;
            l.start = (l.forward ? g.col2 : g.col3) - 1 + shift;
            shift += (int64_t)g.n_del - (int64_t)g.n_ins;
            l.end = (l.forward ? g.col3 : g.col2) + shift;
            lines.push_back(l);
        }
        std::stable_sort(lines.begin(), lines.end(), [](const Line &x, const Line &y) { return x.start < y.start; });
        std::sort(ins.begin(), ins.end());
        std::sort(del.begin(), del.end());
        std::sort(sub.begin(), sub.end());
        Corrected c;
        correct(L, ins, del, sub, c);
        for (const Line &l : lines) {
            ivs.clear();
            walk(l.forward, l.start, l.end, c, ivs);
            int64_t n = 0;
            for (const Iv &v : ivs) n += v.b - v.a;
            int64_t drop = n % 3;                       // the trim, from the far end of the walk
            while (drop && !ivs.empty()) {
                const int64_t cutn = std::min(drop, ivs.back().b - ivs.back().a);
                ivs.back().b -= cutn;
                drop -= cutn;
                if (ivs.back().a == ivs.back().b) ivs.pop_back();
            }
            // the blanks: character 0 at most at the low end, pads at the high end (the walk never collects s < 0)
            uint32_t blanks_lo = 0, blanks_hi = 0;
            for (Iv &v : ivs) {
                if (c.blank0 && v.a == 0 && v.b > 0) { blanks_lo++; v.a++; }
                if (v.b > c.len) { const int64_t from = std::max(v.a, c.len); blanks_hi += (uint32_t)(v.b - from); v.b = from; }
            }
            // the characters left are bases: the segments under every interval, in the string's direction
            const size_t n_iv = ivs.size();
            for (size_t x = 0; x < n_iv; x++) {
                const Iv &v = ivs[l.forward ? x : n_iv - 1 - x];
                if (v.a >= v.b) continue;
                // segments that overlap [v.a, v.b): from the last one that begins at or before v.a
                size_t lo = 0, hi = c.segs.size();
                while (lo + 1 < hi) { const size_t mid = (lo + hi) / 2; if (c.segs[mid].s0 <= v.a) lo = mid; else hi = mid; }
                size_t last = lo;
                while (last + 1 < c.segs.size() && c.segs[last + 1].s0 < v.b) last++;
                for (size_t y = 0; y <= last - lo; y++) {
                    const Seg &sg = c.segs[l.forward ? lo + y : last - y];
                    const int64_t a = std::max(v.a, sg.s0), b = std::min(v.b, sg.s0 + sg.len);
                    if (a >= b || sg.kind == SEG_BLANK) continue;
                    put_piece(o, odd, (uint32_t)r, S, sg.p + (a - sg.s0), b - a, !l.forward, sg.kind == SEG_SUB);
                }
            }
            gmg_edit_string &e = strings[k];
            e.gene = l.gene;
            e.start = l.start;
            e.end = l.end;
            e.strand = l.forward ? 1 : -1;
            e.pad_front = l.forward ? blanks_lo : blanks_hi;
            e.pad_behind = l.forward ? blanks_hi : blanks_lo;
            e.reserved = 0;
            string_run_off[++k] = o.n;
        }
    }
    *n_runs = o.n;
    return GMG_OK;
}
