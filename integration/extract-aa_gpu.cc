//  extract-aa_gpu.cc -- the gene strings of a prediction run with its predicted insertions, deletions and substitutions applied:
//  what the reference's scripts/extract_aa.py -s S -p P makes, in one process and without Python:
//    <prefix>.ffn         the corrected nucleotide string of every gene line, records named >header_start,end_strand
//    <prefix>.faa         their translations (the script's table: a codon of mixed case or with a foreign letter gives X)
//  and with --gicm what train_features.py --indels (build_icm_indels) makes of them:
//    <prefix>.gene.fasta  the .ffn text under that name (no .faa, no .ffn)
//    <prefix>.gicm        the gene ICM, build-icm -r (12 / 7 / 3), when the strings hold at least --min_icm characters
//  <prefix> = -o, or S without its extension.
//
//  The edit arithmetic runs on the host (gmg_edits_plan); the text of both files is written on the device from the plan's runs
//  and pad counts over the file's letters (gmg_runs_text: one call for the strings, one for their translations).  Only --gicm
//  ingests the sequences and splices the strings as a batch (gmg_reads_splice, back to front) to train the model from it
//  (gmg_icm_train_reads).
//
//  usage: extract-aa_gpu -s SEQS -p PREDICT [-o PREFIX] [-z N] [--gicm [--min_icm N]]
//
//  -z N / --transl_table N translates the .faa with GenBank table N (gmg_xlate_table) instead of the script's dictionary, the
//  standard code: glimmer-mg predicts with table 4 on Mycoplasma classes, where TGA is read through.
//
//  Where the script dies this ends with status 1 and one line that names the offender: a sequence header without a record in P, a
//  gene line without its I: D: S: fields (an empty line is one), a gene line under a header that S does not hold, a number that
//  is none, a sequence header that occurs twice.  Nothing is written then.  Sequence lines with white space inside or a '>'
//  behind their first column are refused as well: the script and the ingest count their letters differently.

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
    "usage: extract-aa_gpu -s SEQS -p PREDICT [-o PREFIX] [-z N] [--gicm [--min_icm N]]\n"
    "  -s SEQS       the sequence file the predictions were made on\n"
    "  -p PREDICT    Glimmer-MG predictions with their I: D: S: fields\n"
    "  -o PREFIX     write PREFIX.ffn and PREFIX.faa (default: SEQS without its extension)\n"
    "  -z, --transl_table N   translate PREFIX.faa with GenBank translation table N (default: the script's table, the standard code)\n"
    "  --gicm        write PREFIX.gene.fasta instead and train PREFIX.gicm from the strings (train_features.py --indels)\n"
    "  --min_icm N   characters of gene strings needed to train the ICM (default 0)\n";

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

// Python's str.rstrip() on [b, e)
size_t RStrip(const std::string &s, size_t b, size_t e)
{
    while (e > b && isspace((unsigned char)s[e - 1])) e--;
    return e;
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
    if (tok.empty() || isspace((unsigned char)tok[0]) || *end) Die(1, "not a number: '%s' in predict line '%s'", tok.c_str(), line.c_str());
    return v;
}

// a[5][2:].split(',') of one of the fields I: D: S:
void ParseList(const std::string &field, const std::string &line, std::vector<int64_t> &out, uint32_t &n)
{
    n = 0;
    if (field.size() <= 2) return;
    size_t b = 2;
    for (;;) {
        const size_t c = field.find(',', b);
        out.push_back(ParseInt(field.substr(b, c == std::string::npos ? std::string::npos : c - b), line));
        n++;
        if (c == std::string::npos) break;
        b = c + 1;
    }
}

bool UpperAcgt(char ch) { return ch == 'A' || ch == 'C' || ch == 'G' || ch == 'T'; }

}  // namespace

int main(int argc, char **argv)
{
    std::string seq_file, predict_file, prefix;
    bool gicm = false;
    long long min_icm = 0;
    int transl_table = 0;
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
        if (a == "-s") seq_file = value();
        else if (a == "-p") predict_file = value();
        else if (a == "-o") prefix = value();
        else if (a == "--gicm") gicm = true;
        else if (a == "--min_icm") {
            const std::string s = value();
            char *end = nullptr;
            min_icm = strtoll(s.c_str(), &end, 10);
            if (s.empty() || *end) Die(2, "option %s: invalid integer value: '%s'", a.c_str(), s.c_str());
        } else if (a == "-z" || a == "--transl_table") {
            const std::string s = value();
            char *end = nullptr;
            const long long n = strtoll(s.c_str(), &end, 10);
            char aa[64];
            if (s.empty() || *end || n < 0 || n > 1000 || gmg_xlate_table((int)n, aa) != GMG_OK)
                Die(2, "option %s: no such translation table: '%s'", a.c_str(), s.c_str());
            transl_table = (int)n;
        } else if (a == "-h" || a == "--help") { printf("%s", kUsage); return 0; }
        else { fprintf(stderr, "%s", kUsage); Die(2, "no such option: %s", a.c_str()); }
    }
    if (seq_file.empty()) { fprintf(stderr, "%s", kUsage); Die(2, "Must provide sequence file with -s"); }
    if (predict_file.empty()) { fprintf(stderr, "%s", kUsage); Die(2, "Must provide prediction file with -p"); }
    if (prefix.empty()) prefix = StripExtension(seq_file);

    // ---- the sequences as the script reads them: a line that begins with '>' is a header, any other line is letters (both
    //      right-stripped); the letters of all reads back to back
    const std::string seq_bytes = ReadFile(seq_file), predict_bytes = ReadFile(predict_file);
    std::vector<std::string> headers;
    std::vector<uint64_t> off(1, 0);
    std::string letters;
    for (size_t pos = 0; pos < seq_bytes.size();) {
        size_t eol = seq_bytes.find('\n', pos);
        if (eol == std::string::npos) eol = seq_bytes.size();
        const size_t e = RStrip(seq_bytes, pos, eol);
        if (seq_bytes[pos] == '>') {
            headers.push_back(seq_bytes.substr(pos + 1, e > pos ? e - pos - 1 : 0));
            off.push_back(off.back());
        } else if (e > pos) {
            if (headers.empty()) Die(1, "%s: letters in front of the first header", seq_file.c_str());
            for (size_t i = pos; i < e; i++)
                if (isspace((unsigned char)seq_bytes[i]) || seq_bytes[i] == '>' || seq_bytes[i] == '-')
                    Die(1, "%s: sequence '%s' holds white space, '>' or '-' inside a line", seq_file.c_str(), headers.back().c_str());
            letters.append(seq_bytes, pos, e - pos);
            off.back() += e - pos;
        }
        pos = eol + 1;
    }
    const uint64_t n_reads = headers.size();
    std::map<std::string, uint32_t> by_header;
    for (uint64_t r = 0; r < n_reads; r++)
        if (!by_header.insert(std::make_pair(headers[r], (uint32_t)r)).second)
            Die(1, "%s: the header '%s' occurs twice", seq_file.c_str(), headers[r].c_str());

    // ---- the gene lines (get_preds): a header that comes again starts its list over, as the script's dictionary does
    std::vector<std::vector<gmg_edit_gene> > genes_of(n_reads);
    std::vector<std::vector<int64_t> > positions_of(n_reads);
    std::vector<char> has_record(n_reads, 0);
    {
        long long cur = -2;                             // -2: no header yet; -1: a header the sequence file does not hold
        std::string cur_header;
        for (size_t pos = 0; pos < predict_bytes.size();) {
            size_t eol = predict_bytes.find('\n', pos);
            if (eol == std::string::npos) eol = predict_bytes.size();
            const std::string line = predict_bytes.substr(pos, eol - pos);
            pos = eol + 1;
            if (!line.empty() && line[0] == '>') {
                cur_header = line.substr(1, RStrip(line, 1, line.size()) - 1);
                const std::map<std::string, uint32_t>::const_iterator it = by_header.find(cur_header);
                cur = it == by_header.end() ? -1 : (long long)it->second;
                if (cur >= 0) { has_record[cur] = 1; genes_of[cur].clear(); positions_of[cur].clear(); }
                continue;
            }
            std::vector<std::string> f;
            for (size_t i = 0; i < line.size();) {
                while (i < line.size() && isspace((unsigned char)line[i])) i++;
                size_t j = i;
                while (j < line.size() && !isspace((unsigned char)line[j])) j++;
                if (j > i) f.push_back(line.substr(i, j - i));
                i = j;
            }
            if (f.size() < 8) Die(1, "%s: a gene line needs its I: D: S: fields: '%s'", predict_file.c_str(), line.c_str());
            if (cur == -2) Die(1, "%s: gene line '%s' in front of the first header", predict_file.c_str(), line.c_str());
            if (cur == -1) Die(1, "the predict header '%s' has no sequence in %s", cur_header.c_str(), seq_file.c_str());
            gmg_edit_gene g;
            memset(&g, 0, sizeof g);
            g.read = (uint32_t)cur;
            ParseList(f[5], line, positions_of[cur], g.n_ins);
            ParseList(f[6], line, positions_of[cur], g.n_del);
            ParseList(f[7], line, positions_of[cur], g.n_sub);
            const long long frame = ParseInt(f[3], line);
            g.frame = frame > 0 ? 1 : -1;
            g.col2 = ParseInt(f[1], line);
            g.col3 = ParseInt(f[2], line);
            genes_of[cur].push_back(g);
        }
    }
    std::vector<gmg_edit_gene> genes;
    std::vector<int64_t> positions;
    for (uint64_t r = 0; r < n_reads; r++) {
        if (!has_record[r]) Die(1, "the sequence '%s' has no record in %s", headers[r].c_str(), predict_file.c_str());
        genes.insert(genes.end(), genes_of[r].begin(), genes_of[r].end());
        positions.insert(positions.end(), positions_of[r].begin(), positions_of[r].end());
    }
    genes_of.clear();
    positions_of.clear();

    // ---- the letters the rules on codes get wrong, and the plan
    std::vector<uint64_t> odd_base;
    std::string odd_letter;
    for (uint64_t b = 0; b < letters.size(); b++)
        if (!UpperAcgt(letters[b])) { odd_base.push_back(b); odd_letter += letters[b]; }
    const uint64_t n_genes = genes.size();
    std::vector<uint64_t> sro(n_genes + 1, 0);
    std::vector<gmg_edit_string> strings(n_genes ? n_genes : 1);
    std::vector<gmg_splice_run> runs;
    uint64_t n_runs = 0;
    for (int pass = 0; pass < 2; pass++) {
        Check(gmg_edits_plan(off.data(), n_reads, genes.data(), n_genes, positions.data(), odd_base.data(), odd_letter.data(), odd_base.size(),
                             runs.data(), runs.size(), &n_runs, sro.data(), strings.data()), "gmg_edits_plan");
        if (n_runs <= runs.size()) break;
        runs.resize(n_runs);
    }

    // ---- what is printed: the record names, the pads, and -- for --min_icm -- the script's count of every string, len(line.rstrip()):
    //      the pad in front counts where a run follows it, the pad behind never does (no run prints white space)
    std::string heads;
    std::vector<uint64_t> head_off(n_genes + 1, 0);
    std::vector<uint32_t> pad_front(n_genes ? n_genes : 1), pad_behind(n_genes ? n_genes : 1);
    unsigned long long printed = 0;
    for (uint64_t k = 0; k < n_genes; k++) {
        const gmg_edit_string &e = strings[k];
        char name[64];
        snprintf(name, sizeof name, "_%lld,%lld_%c\n", (long long)e.start, (long long)e.end, e.strand > 0 ? '+' : '-');
        heads += ">" + headers[genes[e.gene].read] + name;
        head_off[k + 1] = heads.size();
        pad_front[k] = e.pad_front;
        pad_behind[k] = e.pad_behind;
        unsigned long long in_runs = 0;
        for (uint64_t q = sro[k]; q < sro[k + 1]; q++) in_runs += runs[q].len;
        if (in_runs) printed += e.pad_front + in_runs;
    }

    // ---- the device: the letters for the text; the ingested codes only where the gene ICM is trained from them
    const char *dev = getenv("GMG_DEVICE");
    Check(gmg_init(dev ? atoi(dev) : 0), "gmg_init");
    const bool train = gicm && (long long)printed >= min_icm;
    gmg_reads *reads = nullptr;
    if (train) {
        gmg_fasta *index = nullptr;
        Check(gmg_fasta_ingest(seq_bytes.data(), seq_bytes.size(), &reads, &index), "gmg_fasta_ingest");
        uint64_t n = 0, total = 0;
        Check(gmg_fasta_info(index, &n, &total, nullptr), "gmg_fasta_info");
        if (n != n_reads || total != letters.size()) Die(1, "%s: the records of the file are not one header line and lines of letters each", seq_file.c_str());
        std::vector<uint32_t> packed(gmg_packed_words(total));
        std::vector<uint64_t> dev_off(n + 1);
        Check(gmg_reads_download(reads, packed.data(), dev_off.data()), "gmg_reads_download");
        if (dev_off != off) Die(1, "%s: the records of the file are not one header line and lines of letters each", seq_file.c_str());
        gmg_fasta_free(index);
    }

    // ---- the text, written on the device: the strings themselves, and their translations
    gmg_letters *on_device = nullptr;
    Check(gmg_letters_upload(letters.data(), off.data(), n_reads, &on_device), "gmg_letters_upload");
    auto text = [&](int mode) {
        gmg_runs_text_params prm;
        Check(gmg_runs_text_params_script(&prm, mode, transl_table), "gmg_runs_text_params_script");
        std::string out;
        size_t bytes = 0;
        for (int pass = 0; pass < 2; pass++) {          // the length, then the text
            Check(gmg_runs_text(on_device, runs.data(), n_runs, sro.data(), n_genes, pad_front.data(), pad_behind.data(), heads.data(),
                                head_off.data(), &prm, pass ? &out[0] : nullptr, &bytes, nullptr), "gmg_runs_text");
            if (bytes == 0) break;
            out.resize(bytes);
        }
        return out;
    };
    const std::string ffn = text(GMG_RUNS_TEXT_DNA), faa = gicm ? std::string() : text(GMG_RUNS_TEXT_PROTEIN);
    gmg_letters_free(on_device);

    if (!gicm) {
        WriteFile(prefix + ".faa", faa);
        WriteFile(prefix + ".ffn", ffn);
    } else {
        // build_icm_indels: the .faa is removed, the .ffn renamed; build-icm -r on it when it holds enough
        unlink((prefix + ".faa").c_str());
        unlink((prefix + ".ffn").c_str());
        WriteFile(prefix + ".gene.fasta", ffn);
        if (train) {
            gmg_reads *reversed = nullptr;
            Check(gmg_reads_splice(reads, runs.data(), n_runs, sro.data(), n_genes, GMG_EXTRACT_REVERSED, &reversed), "gmg_reads_splice");
            gmg_icm *icm = nullptr;
            Check(gmg_icm_train_reads(reversed, 12, 7, 3, &icm), "gmg_icm_train_reads");
            Check(gmg_icm_write(icm, (prefix + ".gicm").c_str()), "gmg_icm_write");
            gmg_icm_free(icm);
            gmg_reads_free(reversed);
        }
    }
    gmg_reads_free(reads);
    return 0;
}
