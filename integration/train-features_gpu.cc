//  train-features_gpu.cc -- the retraining step between two runs of Glimmer-MG's pipeline: what
//  the reference's scripts/train_features.py --predict P --seq S makes of a prediction run, in one process and without Python:
//    <prefix>.features.txt          under -f: the file the next run reads with -f (output_featurefile), or
//    <prefix>.lengths.genes.txt ... without -f: the per-distribution files of output_stats and <prefix>.gc.txt
//    <prefix>.gicm                  the gene ICM, build-icm -r (12 / 7 / 3) on the gene strings of build_icm
//  <prefix> = P without its extension.  The counting runs on the device (gmg_features_count); the gene strings never become text:
//  they are regions of the ingested sequences (gmg_reads_extract, back to front) and the model is trained from that batch
//  (gmg_icm_train_reads).
//
//  usage: train-features_gpu --predict P --seq S [-f] [-l N] [-o N] [-z] [--icm] [--min_icm N]
//
//  Sequences are taken in the order of their first gene line in P; the script iterates a Python 2 dict there, so the order of
//  its additions -- and with it the last bits of its fractional bins -- is not defined by the reference.
//  Not here: --gbk (needs Biopython), --rbs and the .motif file (need ELPH), --indels (extract_aa.py): each is refused with
//  status 2 (the gene ICM of --indels is extract-aa_gpu --gicm, integration/extract-aa_gpu.cc).  A sequence header that occurs twice, a predict header without a sequence, a gene line with fewer than four fields
//  and an input without any gene line end the run with status 1 and a message that names them.  <prefix>.gene.fasta is not
//  written.

#include "../include/gmg.h"
#include "../include/gmg_icm.h"

#include <ctype.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>

#include <map>
#include <string>
#include <vector>

namespace {

const char *kUsage =
    "usage: train-features_gpu --predict P --seq S [-f] [-l N] [-o N] [-z] [--icm] [--min_icm N]\n"
    "  --predict P        Glimmer predictions to train on\n"
    "  --seq S, --seqs S  the sequence file the predictions were made on\n"
    "  -f                 write one feature file for glimmer's -f instead of a file per distribution\n"
    "  -l, --min_length N shortest ORF (nucleotides) that counts beyond the length histogram (default 75)\n"
    "  -o, --max_overlap N largest overlap of two genes, or a gene and an ORF (default 50)\n"
    "  -z                 TGA is no stop codon\n"
    "  --icm              only retrain the gene ICM\n"
    "  --min_icm N        bases of gene strings needed to train an ICM (default 0)\n";

[[noreturn]] void Die(int status, const char *fmt, const char *a = "", const char *b = "")
{
    fprintf(stderr, "ERROR:  ");
    fprintf(stderr, fmt, a, b);
    fprintf(stderr, "\n");
    exit(status);
}

void Check(int rc, const char *who)
{
    if (rc != GMG_OK) Die(1, "%s: %s", who, gmg_last_error());
}

std::string ReadFile(const std::string &path)
{
    FILE *fp = fopen(path.c_str(), "rb");
    if (!fp) Die(1, "Can't open %s for reading.", path.c_str());
    std::string s;
    char buf[1 << 16];
    size_t k;
    while ((k = fread(buf, 1, sizeof buf, fp)) > 0) s.append(buf, k);
    fclose(fp);
    return s;
}

void WriteFile(const std::string &path, const std::string &text)
{
    FILE *fp = fopen(path.c_str(), "wb");
    if (!fp || fwrite(text.data(), 1, text.size(), fp) != text.size() || fclose(fp) != 0) Die(1, "Can't write %s.", path.c_str());
}

// Python's str.rstrip()
std::string RStrip(std::string s)
{
    while (!s.empty() && isspace((unsigned char)s.back())) s.pop_back();
    return s;
}

// os.path.splitext(path)[0]
std::string StripExtension(const std::string &path)
{
    const size_t slash = path.rfind('/');
    size_t name = slash == std::string::npos ? 0 : slash + 1;
    while (name < path.size() && path[name] == '.') name++;            // leading dots of the file name are no extension
    const size_t dot = path.rfind('.');
    return dot == std::string::npos || dot < name ? path : path.substr(0, dot);
}

// Python's int(): optional sign, digits; anything else ends the run as the script's exception would
long long ParseInt(const std::string &tok, const std::string &line)
{
    char *end = nullptr;
    const long long v = strtoll(tok.c_str(), &end, 10);
    if (tok.empty() || *end) Die(1, "not a number: '%s' in predict line '%s'", tok.c_str(), line.c_str());
    return v;
}

// the bounds of hseq[lo:hi] on a string of L letters
void PySlice(long long &lo, long long &hi, long long L)
{
    if (lo < 0) lo += L;
    if (hi < 0) hi += L;
    lo = lo < 0 ? 0 : lo > L ? L : lo;
    hi = hi < 0 ? 0 : hi > L ? L : hi;
    if (hi < lo) hi = lo;
}

struct Gene {                    // parse_predict's Gene (train_features.py:163-199)
    long long start, end, frame_start, frame_end;
    int strand;
    bool start_codon, stop_codon;
};

struct Table {
    gmg_features_table t;
    std::string Text(const char *orf_type, int what, int max_overlap) const
    {
        size_t n = 0;
        Check(gmg_features_format(&t, orf_type, what, max_overlap, nullptr, &n), "gmg_features_format");
        std::string s(n, '\0');
        Check(gmg_features_format(&t, orf_type, what, max_overlap, n ? &s[0] : nullptr, &n), "gmg_features_format");
        return s;
    }
};

}  // namespace

int main(int argc, char **argv)
{
    std::string predict_file, seq_file;
    bool featurefile = false, drop_tga = false, icm_only = false;
    long long min_length = 75, max_overlap = 50, min_icm = 0;
    for (int i = 1; i < argc; i++) {
        std::string a = argv[i], v;
        bool has_v = false;
        const size_t eq = a.find('=');
        if (a.compare(0, 2, "--") == 0 && eq != std::string::npos) { v = a.substr(eq + 1); a = a.substr(0, eq); has_v = true; }
        auto value = [&]() -> std::string {
            if (has_v) return v;
            if (i + 1 >= argc) { fprintf(stderr, "%s", kUsage); Die(2, "%s needs a value", a.c_str()); }
            return argv[++i];
        };
        auto number = [&]() -> long long {
            const std::string s = value();
            char *end = nullptr;
            const long long x = strtoll(s.c_str(), &end, 10);
            if (s.empty() || *end) Die(2, "option %s: invalid integer value: '%s'", a.c_str(), s.c_str());
            return x;
        };
        if (a == "--predict") predict_file = value();
        else if (a == "--seq" || a == "--seqs") seq_file = value();
        else if (a == "-f") featurefile = true;
        else if (a == "-z") drop_tga = true;
        else if (a == "--icm") icm_only = true;
        else if (a == "-l" || a == "--min_length") min_length = number();
        else if (a == "-o" || a == "--max_overlap") max_overlap = number();
        else if (a == "--min_icm") min_icm = number();
        else if (a == "--gbk") Die(2, "--gbk is not supported: reading GenBank files needs Biopython; give --predict and --seq");
        else if (a == "--rbs") Die(2, "--rbs is not supported: the RBS motif needs ELPH, which is not available; no .motif file is written");
        else if (a == "--indels") Die(2, "--indels is not supported: gene strings with indels come from extract_aa.py");
        else if (a == "-h" || a == "--help") { printf("%s", kUsage); return 0; }
        else { fprintf(stderr, "%s", kUsage); Die(2, "no such option: %s", a.c_str()); }
    }
    if (predict_file.empty() || seq_file.empty()) {
        fprintf(stderr, "%s", kUsage);
        Die(2, "Must provide a Glimmer predict file (--predict) and sequence fasta file (--seq)");
    }
    if (max_overlap < 0 || max_overlap > (1 << 20) || min_length < -(1 << 30) || min_length > (1 << 30))
        Die(2, "-o must be in [0, 2^20], -l in [-2^30, 2^30]");
    const std::string prefix = StripExtension(predict_file);
    fprintf(stderr, "%s\n", prefix.c_str());

    // ---- the sequences: ingested on the device; headers as the script reads them (the line behind '>', right-stripped)
    const std::string seq_bytes = ReadFile(seq_file), predict_bytes = ReadFile(predict_file);
    const char *dev = getenv("GMG_DEVICE");
    Check(gmg_init(dev ? atoi(dev) : 0), "gmg_init");
    gmg_reads *reads = nullptr;
    gmg_fasta *index = nullptr;
    Check(gmg_fasta_ingest(seq_bytes.data(), seq_bytes.size(), &reads, &index), "gmg_fasta_ingest");
    uint64_t n_reads = 0, total = 0;
    Check(gmg_fasta_info(index, &n_reads, &total, nullptr), "gmg_fasta_info");
    std::vector<uint64_t> hb(n_reads + 1), he(n_reads + 1), off(n_reads + 1);
    Check(gmg_fasta_headers(index, hb.data(), he.data()), "gmg_fasta_headers");
    {
        std::vector<uint32_t> packed(gmg_packed_words(total));
        Check(gmg_reads_download(reads, packed.data(), off.data()), "gmg_reads_download");
    }
    std::map<std::string, uint32_t> by_header;
    for (uint64_t r = 0; r < n_reads; r++) {
        uint64_t b = hb[r];
        while (b > 0 && seq_bytes[b - 1] != '>') b--;
        const std::string hdr = RStrip(seq_bytes.substr(b, he[r] - b));
        if (!by_header.insert(std::make_pair(hdr, (uint32_t)r)).second) Die(1, "%s: the header '%s' occurs twice", seq_file.c_str(), hdr.c_str());
    }

    // ---- the genes (parse_predict): sequences in the order of their first gene line, genes in file order
    std::vector<uint32_t> order;                        // reads that have genes
    std::map<uint32_t, std::vector<Gene>> genes_of;
    {
        std::string header;
        bool have_header = false;
        size_t pos = 0;
        while (pos < predict_bytes.size()) {
            size_t eol = predict_bytes.find('\n', pos);
            if (eol == std::string::npos) eol = predict_bytes.size();
            const std::string line = predict_bytes.substr(pos, eol - pos);
            pos = eol + 1;
            if (!line.empty() && line[0] == '>') { header = RStrip(line.substr(1)); have_header = true; continue; }
            std::vector<std::string> f;
            for (size_t i = 0; i < line.size();) {
                while (i < line.size() && isspace((unsigned char)line[i])) i++;
                size_t j = i;
                while (j < line.size() && !isspace((unsigned char)line[j])) j++;
                if (j > i) f.push_back(line.substr(i, j - i));
                i = j;
            }
            if (f.empty()) continue;
            if (f.size() < 4) Die(1, "%s: a gene line needs four fields: '%s'", predict_file.c_str(), line.c_str());
            if (!have_header) Die(1, "%s: gene line '%s' in front of the first header", predict_file.c_str(), line.c_str());
            const std::map<std::string, uint32_t>::const_iterator it = by_header.find(header);
            if (it == by_header.end()) Die(1, "the predict header '%s' has no sequence in %s", header.c_str(), seq_file.c_str());
            const long long L = (long long)(off[it->second + 1] - off[it->second]);
            const long long a = ParseInt(f[1], line), b = ParseInt(f[2], line);
            Gene g;
            if (ParseInt(f[3], line) > 0) {
                g.strand = 1; g.start = a - 1; g.end = b;
                g.start_codon = g.start >= 0; g.stop_codon = g.end <= L;
                g.frame_start = g.start + 3 * (1 - (int)g.start_codon); g.frame_end = g.end - 3 * (1 - (int)g.stop_codon);
            } else {
                g.strand = -1; g.start = b - 1; g.end = a;
                g.stop_codon = g.start >= 0; g.start_codon = g.end <= L;
                g.frame_start = g.start + 3 * (1 - (int)g.stop_codon); g.frame_end = g.end - 3 * (1 - (int)g.start_codon);
            }
            g.start = g.start < 0 ? 0 : g.start;
            g.end = g.end > L ? L : g.end;
            if (g.start > L || g.end < 0) Die(1, "%s: the gene '%s' lies outside its sequence", predict_file.c_str(), line.c_str());
            if (!genes_of.count(it->second)) order.push_back(it->second);
            genes_of[it->second].push_back(g);
        }
    }
    if (order.empty()) Die(1, "%s holds no gene line: nothing to train on", predict_file.c_str());

    // ---- the distributions
    if (!icm_only) {
        std::vector<gmg_feature_gene> rows;
        for (uint32_t r : order)
            for (const Gene &g : genes_of[r]) {
                gmg_feature_gene x;
                x.read = r; x.strand = g.strand; x.start = (int32_t)g.start; x.end = (int32_t)g.end; x.start_codon = g.start_codon;
                rows.push_back(x);
            }
        uint64_t n_opaque = 0;
        Check(gmg_fasta_not_upper_acgt(seq_bytes.data(), seq_bytes.size(), nullptr, 0, &n_opaque), "gmg_fasta_not_upper_acgt");
        std::vector<uint64_t> opaque(n_opaque ? n_opaque : 1);
        Check(gmg_fasta_not_upper_acgt(seq_bytes.data(), seq_bytes.size(), opaque.data(), n_opaque, &n_opaque), "gmg_fasta_not_upper_acgt");
        gmg_features_params prm = {(int32_t)min_length, (int32_t)max_overlap, drop_tga ? 1 : 0, 0};
        gmg_features *feat = nullptr;
        Check(gmg_features_count(reads, rows.data(), rows.size(), n_opaque ? opaque.data() : nullptr, n_opaque, &prm, &feat, nullptr), "gmg_features_count");
        Table gene, non;
        Check(gmg_features_fetch(feat, GMG_FEATURES_GENE, &gene.t), "gmg_features_fetch");
        Check(gmg_features_fetch(feat, GMG_FEATURES_NON, &non.t), "gmg_features_fetch");
        const int mo = (int)max_overlap;
        if (featurefile) {
            if (!gene.t.n_lengths || !non.t.n_lengths)    // (the script dies in max() of an empty list)
                Die(1, "%s: a length distribution is empty: no feature file", predict_file.c_str());
            WriteFile(prefix + ".features.txt", gene.Text("GENE", GMG_FEATURES_BLOCK, mo) + non.Text("NON", GMG_FEATURES_BLOCK, mo));
        } else {
            const Table *tab[2] = {&gene, &non};
            const char *tag[2] = {"genes", "non"};
            for (int w = 0; w < 2; w++) {
                WriteFile(prefix + ".lengths." + tag[w] + ".txt", tab[w]->Text("", GMG_FEATURES_LENGTHS, mo));
                WriteFile(prefix + ".starts." + tag[w] + ".txt", tab[w]->Text("", GMG_FEATURES_STARTS, mo));
                WriteFile(prefix + ".adj_orients." + tag[w] + ".txt", tab[w]->Text("", GMG_FEATURES_ORIENTS, mo));
                static const char *const name[3] = {"1.1", "1.-1", "-1.1"};
                for (int k = 0; k < 3; k++)
                    WriteFile(prefix + ".adj_dist." + name[k] + "." + tag[w] + ".txt", tab[w]->Text("", GMG_FEATURES_DIST + k, mo));
            }
        }
        gmg_features_free(feat);
    }

    // ---- one pass over the sequence letters: compute_gc's counts and the letters rc() does not complement
    uint64_t gc = 0, at = 0;
    std::vector<uint64_t> amb_base;
    std::vector<uint8_t> amb_code;
    {
        enum { PRE, HDR, SEQ } st = PRE;
        uint64_t b = 0;
        for (size_t i = 0; i < seq_bytes.size(); i++) {
            const unsigned char ch = (unsigned char)seq_bytes[i];
            if (ch == '>') { st = HDR; continue; }
            if (st == HDR) { if (ch == '\n') st = SEQ; continue; }
            if (st != SEQ || isspace(ch)) continue;
            if (ch == 'A' || ch == 'T') at++;
            else if (ch == 'C' || ch == 'G') gc++;
            if (!strchr("acgtACGT", ch) || ch == 0) { amb_base.push_back(b); amb_code.push_back((uint8_t)gmg_base_code(ch)); }
            b++;
        }
    }

    // ---- the gene ICM (build_icm, :731-778): frame_start .. frame_end without the stop codon, reverse strand complemented
    std::vector<gmg_gene_region> regions;
    uint64_t bp = 0;
    for (uint32_t r : order) {
        const long long L = (long long)(off[r + 1] - off[r]);
        for (const Gene &g : genes_of[r]) {
            long long lo, hi;
            if (g.strand > 0) { lo = g.frame_start; hi = g.frame_end - 3 * (int)g.stop_codon; }
            else { lo = g.frame_start + 3 * (int)g.stop_codon; hi = g.frame_end; }
            PySlice(lo, hi, L);
            if (hi == lo) continue;
            gmg_gene_region x;
            x.read = r; x.len = (int32_t)(hi - lo); x.strand = g.strand; x.first = (int32_t)(g.strand > 0 ? lo : hi - 1);
            regions.push_back(x);
            bp += (uint64_t)(hi - lo);
        }
    }
    if ((long long)bp >= min_icm) {
        const std::string out = prefix + ".gicm";
        unlink(out.c_str());
        gmg_reads *strings = nullptr;
        Check(gmg_reads_extract(reads, regions.data(), regions.size(), GMG_EXTRACT_REVERSED, amb_base.empty() ? nullptr : amb_base.data(),
                                amb_base.empty() ? nullptr : amb_code.data(), amb_base.size(), &strings), "gmg_reads_extract");
        gmg_icm *icm = nullptr;
        Check(gmg_icm_train_reads(strings, 12, 7, 3, &icm), "gmg_icm_train_reads");
        Check(gmg_icm_write(icm, out.c_str()), "gmg_icm_write");
        gmg_icm_free(icm);
        gmg_reads_free(strings);
    }
    if (!icm_only && !featurefile) {
        if (at + gc == 0) Die(1, "%s holds no A, C, G or T: no GC content", seq_file.c_str());
        char buf[64];
        snprintf(buf, sizeof buf, "%f\n", (double)gc / ((double)at + (double)gc));
        WriteFile(prefix + ".gc.txt", buf);
    }
    gmg_fasta_free(index);
    gmg_reads_free(reads);
    return 0;
}
