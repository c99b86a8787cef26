//  window-acgt_gpu.cc -- the reference's window-acgt (src/Util/window-acgt.cc) on the device: the
//  A / C / G / T / other counts and %GC of every sliding window of every record of a multi-fasta file.  ONE gmg_fasta_ingest, one
//  gmg_fasta_ambiguous and one gmg_window_counts for the whole file; the text is formatted on the host from the integers, the header
//  lines are repeated as they stand.  New code, built from this repository alone.
//
//  usage: window-acgt_gpu [-p] <window-len> <window-skip> < multifasta-file
//
//  Refused (status 1, one line on stderr, nothing on stdout): see kUsage.

#include "coords_common.h"

#include <getopt.h>

using namespace coords;

namespace {

const char *kUsage =
    "USAGE:  window-acgt_gpu [options] <window-len> <window-skip> < multifasta-file\n"
    "\n"
    "For every record of the multi-fasta file on standard input print its header line and, for\n"
    "windows of <window-len> letters that start every <window-skip> letters, the position and\n"
    "length of the window, its numbers of a, c, g, t and other letters and its %GC.\n"
    "Output goes to stdout.\n"
    "\n"
    "Options:\n"
    " -h, --help    print this message\n"
    " -p, --percen  print percentages, not counts\n"
    "\n"
    "Refused with status 1 and one line that names the input line:\n"
    "  letters in front of the first header line; a '>' inside a line of letters\n"
    "  a line of 299 characters or more (without its newline); a NUL byte; a record of 2^31 letters or more\n"
    "  a file of 2^31 bytes or more; a window length or skip below 1\n";

[[noreturn]] void RefuseLine(size_t ln, const char *why)
{
    fprintf(stderr, "ERROR:  input line %zu: %s\n", ln + 1, why);
    exit(1);
}

double Percent(double a, double b) { return b == 0.0 ? 0.0 : 100.0 * (a / b); }      // (the reference's order of operations)

}  // namespace

int main(int argc, char **argv)
{
    bool percents = false, errflg = false;
    static struct option long_options[] = {{"help", 0, 0, 'h'}, {"percen", 0, 0, 'p'}, {0, 0, 0, 0}};
    int ch;
    while (!errflg && (ch = getopt_long(argc, argv, "hp", long_options, nullptr)) != EOF) switch (ch) {
        case 'h': fprintf(stderr, "%s", kUsage); return 0;
        case 'p': percents = true; break;
        default: errflg = true;
    }
    if (errflg || optind > argc - 2) { fprintf(stderr, "%s", kUsage); return 1; }
    const int W = (int)strtol(argv[optind], nullptr, 10), S = (int)strtol(argv[optind + 1], nullptr, 10);
    if (W < 1) { fprintf(stderr, "ERROR:  Bad window length = %d\n", W); return 1; }
    if (S < 1) { fprintf(stderr, "ERROR:  Bad window skip = %d\n", S); return 1; }

    const std::string text = ReadFile("-");
    if (text.size() >= 0x7fffffffull) Die(1, "the input has 2^31 bytes or more");
    // the file as the reference's fgets loop sees it: header lines (first non-blank character '>') and lines of letters
    const std::vector<std::string> lines = Lines(text);
    std::vector<size_t> header_line;
    std::vector<uint64_t> length;                        // letters per record
    for (size_t ln = 0; ln < lines.size(); ln++) {
        const std::string &line = lines[ln];
        if (memchr(line.data(), '\0', line.size())) RefuseLine(ln, "a NUL byte");
        if (line.size() >= kMaxLine) RefuseLine(ln, "299 characters or more (the reference reads such a line in pieces)");
        size_t b = 0;
        while (b < line.size() && isspace((unsigned char)line[b])) b++;
        if (b < line.size() && line[b] == '>') {
            header_line.push_back(ln);
            length.push_back(0);
            continue;
        }
        if (line.find('>') != std::string::npos) RefuseLine(ln, "a '>' inside a line of letters (the reference counts it as a letter)");
        uint64_t letters = 0;
        for (size_t k = b; k < line.size(); k++) letters += !isspace((unsigned char)line[k]);
        if (letters && length.empty()) RefuseLine(ln, "letters in front of the first header line");
        if (letters) length.back() += letters;
    }
    for (size_t r = 0; r < length.size(); r++)
        if (length[r] >= 0x80000000ull) RefuseLine(header_line[r], "a record of 2^31 letters or more");

    std::vector<uint64_t> off(length.size() + 1, 0);
    std::vector<int32_t> counts;
    if (!length.empty()) {
        const char *dev = getenv("GMG_DEVICE");
        Check(gmg_init(dev ? atoi(dev) : 0), "gmg_init");
        gmg_reads *reads = nullptr;
        gmg_fasta *index = nullptr;
        Check(gmg_fasta_ingest(text.data(), text.size(), &reads, &index), "gmg_fasta_ingest");
        uint64_t n_reads = 0, total = 0, sum = 0;
        Check(gmg_fasta_info(index, &n_reads, &total, nullptr), "gmg_fasta_info");
        for (uint64_t n : length) sum += n;
        if (n_reads != length.size() || total != sum) Die(1, "the device and the host split the file into different records");
        uint64_t n_amb = 0;
        Check(gmg_fasta_ambiguous(text.data(), text.size(), nullptr, nullptr, 0, &n_amb), "gmg_fasta_ambiguous");
        std::vector<uint64_t> amb(n_amb + 1);
        std::vector<uint8_t> code(n_amb + 1);
        Check(gmg_fasta_ambiguous(text.data(), text.size(), amb.data(), code.data(), n_amb, &n_amb), "gmg_fasta_ambiguous");
        gmg_windows *win = nullptr;
        Check(gmg_window_counts(reads, W, S, n_amb ? amb.data() : nullptr, n_amb, &win, nullptr), "gmg_window_counts");
        uint64_t n_win = 0;
        Check(gmg_windows_info(win, nullptr, &n_win), "gmg_windows_info");
        counts.resize(n_win * 5 + 5);
        Check(gmg_windows_fetch(win, off.data(), counts.data()), "gmg_windows_fetch");
        gmg_windows_free(win);
        gmg_fasta_free(index);
        gmg_reads_free(reads);
    }

    std::string out;
    out.reserve(1 << 20);
    char buf[256];
    for (size_t r = 0; r < length.size(); r++) {
        out += lines[header_line[r]];
        snprintf(buf, sizeof buf, "%8s %7s %6s %6s %6s %6s %6s %6s\n", "Position", "Length", "As", "Cs", "Gs", "Ts", "Other", "%GC");
        out += buf;
        const uint64_t L = length[r];
        for (uint64_t j = 0; j < off[r + 1] - off[r]; j++) {
            const uint64_t p = j * (uint64_t)S, len = L - p < (uint64_t)W ? L - p : (uint64_t)W;
            const int32_t *c = &counts[(off[r] + j) * 5];
            int k = snprintf(buf, sizeof buf, "%8d %7d", (int)(p + 1), (int)len);
            for (int i = 0; i < 5; i++)
                k += percents ? snprintf(buf + k, sizeof buf - k, " %6.1f", Percent(c[i], (double)len)) : snprintf(buf + k, sizeof buf - k, " %6d", c[i]);
            snprintf(buf + k, sizeof buf - k, " %6.1f\n", Percent(c[1] + c[2], (double)len));
            out += buf;
        }
        if (out.size() >= (1 << 20)) {
            fwrite(out.data(), 1, out.size(), stdout);
            out.clear();
        }
    }
    fwrite(out.data(), 1, out.size(), stdout);
    return 0;
}
