//  entropy-fasta_gpu.cc -- the reference's entropy-fasta (src/Util/entropy-fasta.cc) on the device:
//  every record of a multi-fasta file of gene strings printed again with the entropy distance ratio of its translation behind its
//  header.  ONE gmg_fasta_ingest and ONE gmg_entropy_regions call (a region per record, counts only); the codons that hold a letter
//  outside acgtACGT are taken off on the host, gmg_entropy_from_counts finishes each count vector with the reference's arithmetic.
//  A record whose length is no multiple of 3 ends the program with status 1 behind the records in front of it, as the reference's
//  exit () does (their text is flushed, to a file as to a pipe).  New code, built from this repository alone.
//
//  usage: entropy-fasta_gpu < multifasta-file
//
//  Refused (status 1, one line on stderr, nothing on stdout): a NUL byte, a file of 2^31 bytes or more, a record of 2^31 letters or
//  more, a file that Fasta_Read and gmg_fasta_ingest split into different records (a '>' and blanks at the very end of the file).

#include "coords_common.h"

#include <algorithm>
#include <set>

using namespace coords;

namespace {

struct Gene {
    std::string hdr, letters;
};

// Fasta_Read (src/Common/fasta.cc:236-283), record after record
std::vector<Gene> ReadGenes(const std::string &text)
{
    std::vector<Gene> out;
    size_t i = 0;
    const size_t n = text.size();
    for (;;) {
        while (i < n && text[i] != '>') i++;
        if (i >= n) break;
        i++;
        while (i < n && text[i] == ' ') i++;
        if (i >= n) break;                               // (the reference drops a header that the file ends in)
        Gene g;
        while (i < n && text[i] != '\n') g.hdr.push_back(text[i++]);
        if (i < n) i++;
        while (i < n && text[i] != '>') {
            if (!isspace((unsigned char)text[i])) g.letters.push_back(text[i]);
            i++;
        }
        out.push_back(g);
    }
    return out;
}

}  // namespace

int main(int argc, char **argv)
{
    (void)argc; (void)argv;                              // (the reference reads no option either)
    const std::string text = ReadFile("-");
    if (text.size() >= 0x7fffffffull) Die(1, "the input has 2^31 bytes or more");
    if (memchr(text.data(), '\0', text.size())) Die(1, "a NUL byte in the input");
    const std::vector<Gene> genes = ReadGenes(text);
    size_t n_good = 0;                                   // the records in front of the first whose length is no multiple of 3
    while (n_good < genes.size() && genes[n_good].letters.size() % 3 == 0) n_good++;
    for (const Gene &g : genes)
        if (g.letters.size() >= 0x80000000ull) Die(1, "a record of 2^31 letters or more");

    double pos[20], neg[20];
    Check(gmg_entropy_default_profiles(pos, neg), "gmg_entropy_default_profiles");
    std::vector<int32_t> counts(n_good * 20 + 20, 0);
    std::vector<gmg_gene_region> regions;
    std::vector<size_t> gene_of;
    for (size_t k = 0; k < n_good; k++)
        if (!genes[k].letters.empty()) {
            gmg_gene_region r;
            r.read = (uint32_t)k; r.first = 0; r.len = (int32_t)genes[k].letters.size(); r.strand = 1;
            regions.push_back(r);
            gene_of.push_back(k);
        }
    if (!regions.empty()) {
        const char *dev = getenv("GMG_DEVICE");
        Check(gmg_init(dev ? atoi(dev) : 0), "gmg_init");
        gmg_reads *reads = nullptr;
        gmg_fasta *index = nullptr;
        Check(gmg_fasta_ingest(text.data(), text.size(), &reads, &index), "gmg_fasta_ingest");
        uint64_t n_reads = 0, total = 0, sum = 0;
        Check(gmg_fasta_info(index, &n_reads, &total, nullptr), "gmg_fasta_info");
        for (const Gene &g : genes) sum += g.letters.size();
        if (n_reads != genes.size() || total != sum) Die(1, "the device and the host split the file into different records");
        char aa[64];
        Check(gmg_xlate_table(11, aa), "gmg_xlate_table");       // (Codon_Translation's default table)
        void *d_counts = nullptr;
        std::vector<int32_t> rows(regions.size() * 20);
        Check(gmg_device_malloc(&d_counts, regions.size() * 80), "gmg_device_malloc");
        Check(gmg_entropy_regions(reads, regions.data(), regions.size(), aa, pos, neg, (int32_t *)d_counts, nullptr, nullptr), "gmg_entropy_regions");
        Check(gmg_memcpy_d2h(rows.data(), d_counts, regions.size() * 80, nullptr), "gmg_memcpy_d2h");
        Check(gmg_synchronize(nullptr), "gmg_synchronize");
        gmg_device_free(d_counts);
        gmg_fasta_free(index);
        gmg_reads_free(reads);
        // A codon with a letter outside acgtACGT counts nowhere in the reference (Codon_Translation gives 'X'); the device counted it
        // under the 2-bit code the letter was packed as: taken out again here, codon by codon.
        static const char order[] = "ACDEFGHIKLMNPQRSTVWY";
        for (size_t x = 0; x < regions.size(); x++) {
            const std::string &s = genes[gene_of[x]].letters;
            int32_t *row = &rows[20 * x];
            size_t last = (size_t)-1;
            for (size_t p = 0; p < s.size(); p++) {
                if (strchr("acgtACGT", s[p]) || p / 3 == last) continue;
                last = p / 3;
                int idx = 0;
                for (size_t t = 0; t < 3; t++) idx = 4 * idx + gmg_base_code((unsigned char)s[3 * last + t]);
                const char *q = aa[idx] == '*' ? nullptr : strchr(order, aa[idx]);
                if (q) row[q - order]--;
            }
            std::copy(row, row + 20, counts.begin() + 20 * gene_of[x]);
        }
    }
    for (size_t k = 0; k < n_good; k++) {
        double ratio = 0.0;
        Check(gmg_entropy_from_counts(&counts[20 * k], pos, neg, nullptr, nullptr, &ratio), "gmg_entropy_from_counts");
        printf(">%s\t%g\n%s\n", genes[k].hdr.c_str(), ratio, genes[k].letters.c_str());
    }
    if (n_good < genes.size()) {
        fflush(stdout);
        fprintf(stderr, "%s not divisible by 3\n", genes[n_good].hdr.c_str());
        return 1;
    }
    return 0;
}
