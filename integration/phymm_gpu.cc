//  phymm_gpu.cc -- the classification step of Glimmer-MG's pipeline in one process:
//  every read of a FASTA file and its reverse complement against every ICM of a Phymm database (.genomeData in the working
//  directory), with
//    rawPhymmOutput_<prefix>.txt   the raw score matrix, byte for byte as Phymm's scoreReadsGlim.pl -b writes it (the file
//                                  glimmer-mg.py's parse_phymm reads), and
//    <stem>.class.txt              the class file glimmer-mg -c reads: per read its best top_hits informative genomes, as
//                                  parse_phymm + score_insert choose them (lines in read order).
//  The models stream through the device in batches (gmg_tophits_scores: the scores and the per-read slots stay in HBM); the
//  matrix lines are formatted on the device (gmg_tophits_format_rows).
//
//  The ICM files themselves are parsed on the device too (gmg_model_set_load): a reader thread fills one of two page-locked
//  buffers with the raw bytes of the next batch's files while the device scores the current one, and the load of that next batch
//  is queued on a second stream before the scoring starts.  --host-load reads every model with gmg_icm_open instead (the
//  cross-check; the output files are the same bytes).
//
//  usage: phymm_gpu [-f] [-i ignore_file] [-s suffix] [-t top_hits] [--informative FILE] [--no-matrix] [--batch-models B] [--host-load] <reads.fa>
//
//  Inputs whose outcome in the scripts is unknown or accidental are refused with a message (exit status 1): a record with an
//  empty sequence, two records with one read ID, a header without an ID, fewer informative models than top_hits, an ICM path
//  with white space in it, a suffix that the script would read as a pattern, a score the %.4f key cannot hold.

#include "../include/gmg.h"
#include "../include/gmg_icm.h"

#include <dirent.h>
#include <errno.h>
#include <fcntl.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <set>
#include <string>
#include <thread>
#include <unordered_set>
#include <vector>

namespace {

const char *kUsage =
    "usage: phymm_gpu [-f] [-i ignore_file] [-s suffix] [-t top_hits] [--informative FILE] [--no-matrix] [--batch-models B] "
    "[--host-load] <reads.fa>\n"
    "  run in the directory that holds .genomeData\n"
    "  -f                 score the forward strand only\n"
    "  -i FILE            ICMs to leave out: strain directories or full paths, one per line\n"
    "  -s SUFFIX          ICM file suffix (default icm)\n"
    "  -t N               genomes per read in the class file, 1..16 (default 3)\n"
    "  --informative FILE the genomes (<dir>|<file stem>) that may classify a read (default: all)\n"
    "  --no-matrix        do not write rawPhymmOutput_<prefix>.txt\n"
    "  --batch-models B   models per device batch (default 64)\n"
    "  --host-load        read every ICM on the host (gmg_icm_open) instead of parsing the files on the device\n";

[[noreturn]] void Die(const char *fmt, const char *a = "", const char *b = "")
{
    fprintf(stderr, "ERROR:  ");
    fprintf(stderr, fmt, a, b);
    fprintf(stderr, "\n");
    exit(EXIT_FAILURE);
}

void Check(int rc, const char *who)
{
    if (rc != GMG_OK) Die("%s: %s", who, gmg_last_error());
}

bool IsDir(const std::string &p)
{
    struct stat st;
    return stat(p.c_str(), &st) == 0 && S_ISDIR(st.st_mode);
}

bool EndsWith(const std::string &s, const std::string &t)
{
    return s.size() >= t.size() && s.compare(s.size() - t.size(), t.size(), t) == 0;
}

std::vector<std::string> List(const std::string &dir)
{
    std::vector<std::string> out;
    DIR *d = opendir(dir.c_str());
    if (!d) Die("Can't open %s for scanning.", dir.c_str());
    while (struct dirent *e = readdir(d)) out.push_back(e->d_name);
    closedir(d);
    return out;
}

// scanDir: the files of one strain directory that end in ".<suffix>" and have no ".gene." in their name
void ScanDir(const std::string &dir, const std::string &suffix, std::vector<std::string> &icms)
{
    for (const std::string &f : List(dir))
        if (EndsWith(f, "." + suffix) && f.find(".gene.") == std::string::npos) icms.push_back(dir + "/" + f);
}

std::vector<std::string> ReadLines(const char *path)
{
    FILE *fp = fopen(path, "rb");
    if (!fp) Die("Can't open %s for reading.", path);
    std::vector<std::string> lines;
    std::string cur;
    int c;
    while ((c = getc(fp)) != EOF) {
        if (c == '\n') { lines.push_back(cur); cur.clear(); }
        else cur.push_back((char)c);
    }
    if (!cur.empty()) lines.push_back(cur);
    fclose(fp);
    return lines;
}

bool IsSpace(char c) { return c == ' ' || c == '\t' || c == '\n' || c == '\r' || c == '\f' || c == '\v'; }

// parse_phymm's genome name of an ICM path: <directory>|<file name up to its first '.'>
std::string GenomeName(const std::string &path)
{
    const size_t s = path.rfind('/'), s2 = path.rfind('/', s - 1);
    const std::string file = path.substr(s + 1), dir = path.substr(s2 + 1, s - s2 - 1);
    return dir + "|" + file.substr(0, file.find('.'));
}

// The files of one batch, back to back in a page-locked buffer.  Fill() is all the reader thread runs: open / read / close, no
// call into the library.  While a Fill() runs, the main thread touches nothing of that FileBatch (which models a batch holds is
// computed from the batch's number, not kept here); the thread's join() hands it back.
struct FileBatch {
    unsigned char *buf = nullptr;
    std::vector<const void *> ptr;
    std::vector<uint64_t> size;
    std::string error;                                  // what went wrong in Fill(), for the main thread to die with

    void Fill(const std::vector<std::string> &paths, const std::vector<uint64_t> &sizes, size_t first, int nb)
    {
        ptr.assign(nb, nullptr);
        size.assign(nb, 0);
        error.clear();
        size_t at = 0;
        for (int k = 0; k < nb; k++) {
            const std::string &path = paths[first + k];
            const uint64_t want = sizes[first + k];
            const int fd = open(path.c_str(), O_RDONLY);
            if (fd < 0) { error = "Could not open file  " + path + "  errno = " + std::to_string(errno); return; }
            uint64_t got = 0;
            while (got < want) {
                const ssize_t n = read(fd, buf + at + got, want - got);
                if (n < 0 && errno == EINTR) continue;
                if (n <= 0) break;
                got += (uint64_t)n;
            }
            close(fd);
            ptr[k] = buf + at;
            size[k] = got;                              // (a file that shrank since stat(): the parser sees what is there)
            at += want;
        }
    }
};

}  // namespace

int main(int argc, char *argv[])
{
    bool forward_only = false, no_matrix = false, host_load = false;
    const char *ignore_file = nullptr, *informative_file = nullptr, *reads_file = nullptr;
    std::string suffix = "icm";
    int top_hits = 3, batch = 64;
    for (int i = 1; i < argc; i++) {
        const std::string a = argv[i];
        auto value = [&](void) -> const char * {
            if (i + 1 >= argc) { fputs(kUsage, stderr); exit(EXIT_FAILURE); }
            return argv[++i];
        };
        if (a == "-f") forward_only = true;
        else if (a == "-i") ignore_file = value();
        else if (a == "-s") suffix = value();
        else if (a == "-t") top_hits = atoi(value());
        else if (a == "--informative") informative_file = value();
        else if (a == "--no-matrix") no_matrix = true;
        else if (a == "--batch-models") batch = atoi(value());
        else if (a == "--host-load") host_load = true;
        else if (a == "-h" || a == "--help") { fputs(kUsage, stdout); return 0; }
        else if (a.size() > 1 && a[0] == '-') { fprintf(stderr, "ERROR:  unknown option %s\n%s", a.c_str(), kUsage); return EXIT_FAILURE; }
        else if (!reads_file) reads_file = argv[i];
        else { fputs(kUsage, stderr); return EXIT_FAILURE; }
    }
    if (!reads_file) { fputs(kUsage, stderr); return EXIT_FAILURE; }
    if (top_hits < 1 || top_hits > GMG_TOPHITS_MAX) Die("-t %s: top_hits must be 1..16", std::to_string(top_hits).c_str());
    if (batch < 1) Die("--batch-models %s: must be at least 1", std::to_string(batch).c_str());
    // the script matches "\.<suffix>$" with only the suffix's first '.' escaped: any other pattern character changes the match
    if (suffix.empty() || std::count(suffix.begin(), suffix.end(), '.') > 1 ||
        suffix.find_first_not_of("ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz0123456789_-.") != std::string::npos)
        Die("-s %s: the suffix may hold letters, digits, '_', '-' and one '.'", suffix.c_str());

    // ---- the ICM list: scanDir over .genomeData/<dir> and .genomeData/.userAdded/<dir>, sorted bytewise, minus the ignored ----
    if (!IsDir(".genomeData")) Die("Can't open .genomeData for scanning (run in the directory that holds it).");
    std::vector<std::string> icms;
    for (const std::string &d : List(".genomeData"))
        if (d[0] != '.' && IsDir(".genomeData/" + d)) ScanDir(".genomeData/" + d, suffix, icms);
    const std::string user = ".genomeData/.userAdded";
    struct stat st_user;
    if (stat(user.c_str(), &st_user) == 0)
        for (const std::string &d : List(user))
            if (d[0] != '.' && IsDir(user + "/" + d)) ScanDir(user + "/" + d, suffix, icms);
    std::sort(icms.begin(), icms.end());
    std::set<std::string> ignored;
    if (ignore_file)
        for (const std::string &l : ReadLines(ignore_file)) ignored.insert(l);
    std::vector<std::string> kept;
    for (const std::string &p : icms) {
        if (std::find_if(p.begin(), p.end(), IsSpace) != p.end()) Die("ICM path with white space: %s", p.c_str());
        // the script's /genomeData\/(\S+)\// : everything between ".genomeData/" and the last '/'
        const std::string strain = p.substr(12, p.rfind('/') - 12);
        if (ignored.count(strain) || ignored.count(p)) continue;
        kept.push_back(p);
    }
    std::vector<uint8_t> informative(kept.size(), 1);
    if (informative_file) {
        std::unordered_set<std::string> names;
        for (std::string l : ReadLines(informative_file)) {
            while (!l.empty() && IsSpace(l.back())) l.pop_back();       // (parse_phymm's rstrip)
            names.insert(l);
        }
        for (size_t k = 0; k < kept.size(); k++) informative[k] = names.count(GenomeName(kept[k])) != 0;
    }
    const size_t n_informative = (size_t)std::count(informative.begin(), informative.end(), 1);
    if (n_informative < (size_t)top_hits)
        Die("%s informative ICMs, fewer than top_hits (parse_phymm would meet an empty slot)", std::to_string(n_informative).c_str());

    // ---- the reads: the file parsed on the device; read IDs = the first white-space-free token behind a '>' that starts a line ----
    std::vector<char> bytes;
    {
        FILE *fp = fopen(reads_file, "rb");
        if (!fp) Die("Can't open %s for reading.", reads_file);
        char buf[1 << 16];
        size_t n;
        while ((n = fread(buf, 1, sizeof buf, fp)) > 0) bytes.insert(bytes.end(), buf, buf + n);
        fclose(fp);
    }
    Check(gmg_init(0), "gmg_init");
    gmg_reads *reads = nullptr;
    gmg_fasta *index = nullptr;
    Check(gmg_fasta_ingest(bytes.data(), bytes.size(), &reads, &index), "gmg_fasta_ingest");
    uint64_t n_reads = 0, total = 0, gc = 0;
    Check(gmg_fasta_info(index, &n_reads, &total, &gc), "gmg_fasta_info");
    if (n_reads == 0) Die("%s holds no reads", reads_file);
    std::vector<uint64_t> hb(n_reads), he(n_reads), gt(n_reads + 1);
    Check(gmg_fasta_headers(index, hb.data(), he.data()), "gmg_fasta_headers");
    gmg_fasta_free(index);
    std::vector<std::string> ids(n_reads);
    std::unordered_set<std::string> seen;
    for (uint64_t r = 0; r < n_reads; r++) {
        uint64_t g = hb[r];
        while (g > 0 && bytes[g - 1] != '>') g--;                       // (the blanks Fasta_Read skipped)
        gt[r] = g - 1;
        if (g != hb[r] || hb[r] == he[r] || IsSpace(bytes[hb[r]]))
            Die("record %s: a header without a read ID", std::to_string(r + 1).c_str());
        if (gt[r] > 0 && bytes[gt[r] - 1] != '\n') Die("record %s: a '>' inside a line", std::to_string(r + 1).c_str());
        uint64_t e = hb[r];
        while (e < he[r] && !IsSpace(bytes[e])) e++;
        ids[r].assign(bytes.data() + hb[r], e - hb[r]);
        if (!seen.insert(ids[r]).second) Die("read ID %s appears twice (the script's hashes would merge the records)", ids[r].c_str());
    }
    gt[n_reads] = bytes.size();
    for (uint64_t r = 0; r < n_reads; r++) {
        bool empty = true;
        for (uint64_t i = he[r]; i < gt[r + 1] && empty; i++) empty = IsSpace(bytes[i]);
        if (empty) Die("read %s: an empty sequence", ids[r].c_str());
    }

    // ---- output names: the script's, from the file name ----
    std::string base = reads_file;
    if (base.find('/') != std::string::npos) base = base.substr(base.rfind('/') + 1);
    std::string flat = base;
    std::replace(flat.begin(), flat.end(), '.', '_');
    const std::string raw_name = "rawPhymmOutput_" + flat + ".txt";
    const size_t dot = base.rfind('.');
    const std::string class_name = (dot == std::string::npos || dot == 0 ? base : base.substr(0, dot)) + ".class.txt";

    FILE *raw = nullptr;
    if (!no_matrix) {
        raw = fopen(raw_name.c_str(), "wb");
        if (!raw) Die("Can't open %s for writing.", raw_name.c_str());
        fputs("BEGIN_ICM_LIST\n", raw);
        for (const std::string &p : kept) fprintf(raw, "%s\n", p.c_str());
        fputs("END_ICM_LIST\nBEGIN_READID_LIST\n", raw);
        for (const std::string &id : ids) fprintf(raw, "%s\n", id.c_str());
        fputs("END_READID_LIST\nBEGIN_DATA_MATRIX\n", raw);
    }

    // ---- the models in batches: scores + slots on the device, the matrix lines formatted there ----
    gmg_tophits *th = nullptr;
    Check(gmg_tophits_create(reads, top_hits, &th), "gmg_tophits_create");
    const int B = (int)std::min<size_t>((size_t)batch, kept.size());
    std::vector<char> text;
    if (raw) {
        text.resize((size_t)B * n_reads * GMG_TOPHITS_MAX_FIELD);
        Check(gmg_host_register(text.data(), text.size()), "gmg_host_register");
    }
    // one batch scored and its matrix lines written
    auto score_batch = [&](const std::vector<const gmg_model *> &dev, size_t first) {
        const int nb = (int)dev.size();
        const double *d_sums = nullptr;
        Check(gmg_tophits_scores(th, dev.data(), nb, (int)first, informative.data() + first, forward_only, nullptr, &d_sums),
              "gmg_tophits_scores");
        if (raw) {
            size_t n = text.size();
            Check(gmg_tophits_format_rows(th, d_sums, nb, forward_only, text.data(), &n, nullptr), "gmg_tophits_format_rows");
            if (fwrite(text.data(), 1, n, raw) != n) Die("write error on %s", raw_name.c_str());
        }
    };
    if (host_load) {
        for (size_t first = 0; first < kept.size(); first += (size_t)B) {
            const int nb = (int)std::min<size_t>((size_t)B, kept.size() - first);
            std::vector<gmg_icm *> icm(nb);
            std::vector<const gmg_model *> dev(nb);
            for (int k = 0; k < nb; k++) {
                if (gmg_icm_open(kept[first + k].c_str(), &icm[k]) != GMG_OK) Die("%s: %s", kept[first + k].c_str(), gmg_last_error());
                Check(gmg_icm_device_model(icm[k], &dev[k]), "gmg_icm_device_model");
            }
            score_batch(dev, first);
            for (int k = 0; k < nb; k++) gmg_icm_free(icm[k]);
        }
    } else {
        // batch k scores while the device parses batch k + 1 (second stream) and the reader thread fills the idle buffer with k + 2
        std::vector<uint64_t> sizes(kept.size());
        for (size_t k = 0; k < kept.size(); k++) {
            struct stat st;
            if (stat(kept[k].c_str(), &st) != 0) Die("Could not open file  %s", kept[k].c_str());
            sizes[k] = (uint64_t)st.st_size;
        }
        const size_t n_batches = (kept.size() + (size_t)B - 1) / (size_t)B;
        size_t cap = 1;
        for (size_t b = 0; b < n_batches; b++) {
            size_t sum = 0;
            for (size_t k = b * B; k < std::min(kept.size(), (b + 1) * (size_t)B); k++) sum += sizes[k];
            cap = std::max(cap, sum);
        }
        FileBatch fb[2];
        for (FileBatch &f : fb) {
            f.buf = (unsigned char *)malloc(cap);
            if (!f.buf) Die("out of memory for the ICM files of a batch");
            Check(gmg_host_register(f.buf, cap), "gmg_host_register");
        }
        void *load_stream = nullptr;
        Check(gmg_stream_create(&load_stream), "gmg_stream_create");
        auto first_of = [&](size_t b) { return b * (size_t)B; };
        auto count_of = [&](size_t b) { return (int)std::min<size_t>((size_t)B, kept.size() - first_of(b)); };
        auto fill = [&](size_t b) { fb[b & 1].Fill(kept, sizes, first_of(b), count_of(b)); };
        auto queue_load = [&](size_t b) -> gmg_model_set * {        // (the reader of batch b has been joined)
            FileBatch &f = fb[b & 1];
            const int nb = count_of(b);
            if (!f.error.empty()) Die("%s", f.error.c_str());
            for (int k = 0; k < nb; k++) {              // (the header checks of the load itself, here with the path)
                uint64_t blob = 0;
                if (gmg_icm_bytes_info(f.ptr[k], f.size[k], nullptr, nullptr, nullptr, nullptr, &blob) != GMG_OK)
                    Die("%s: %s", kept[first_of(b) + k].c_str(), gmg_last_error());
            }
            gmg_model_set *set = nullptr;
            Check(gmg_model_set_load(f.ptr.data(), f.size.data(), nb, &set, load_stream), "gmg_model_set_load");
            return set;
        };
        auto finish = [&](gmg_model_set *set, size_t b) {
            int bad = -1;
            if (gmg_model_set_finish(set, &bad) != GMG_OK) {
                if (bad < 0) Check(GMG_EHIP, "gmg_model_set_finish");
                Die("%s: %s", kept[first_of(b) + bad].c_str(), gmg_last_error());
            }
        };
        fill(0);
        gmg_model_set *cur = queue_load(0), *next = nullptr;
        finish(cur, 0);
        std::thread reader;
        if (n_batches > 1) reader = std::thread(fill, (size_t)1);
        for (size_t b = 0; b < n_batches; b++) {
            if (b + 1 < n_batches) {
                reader.join();
                next = queue_load(b + 1);
                // the buffer of batch b is idle (its load finished before this iteration) and nothing below reads fb[b & 1]: until
                // the next join it belongs to the reader, which fills it with batch b + 2 while batch b scores
                if (b + 2 < n_batches) reader = std::thread(fill, b + 2);
            }
            std::vector<const gmg_model *> dev(count_of(b));
            for (size_t k = 0; k < dev.size(); k++) dev[k] = gmg_model_set_model(cur, (int)k);
            score_batch(dev, first_of(b));
            if (b + 1 < n_batches) finish(next, b + 1);
            gmg_model_set_free(cur);
            cur = next;
            next = nullptr;
        }
        Check(gmg_stream_destroy(load_stream), "gmg_stream_destroy");
        for (FileBatch &f : fb) {
            gmg_host_unregister(f.buf);
            free(f.buf);
        }
    }
    if (raw) {
        fputs("END_DATA_MATRIX\n", raw);
        if (fclose(raw) != 0) Die("write error on %s", raw_name.c_str());
        gmg_host_unregister(text.data());
    }

    // ---- the class file: per read its slots' genomes, in slot order ----
    std::vector<int64_t> keys((size_t)n_reads * top_hits);
    std::vector<int32_t> models((size_t)n_reads * top_hits);
    Check(gmg_tophits_fetch(th, keys.data(), models.data()), "gmg_tophits_fetch");
    std::vector<std::string> names(kept.size());
    for (size_t k = 0; k < kept.size(); k++) names[k] = GenomeName(kept[k]);
    FILE *cls = fopen(class_name.c_str(), "wb");
    if (!cls) Die("Can't open %s for writing.", class_name.c_str());
    for (uint64_t r = 0; r < n_reads; r++) {
        fprintf(cls, "%s\t", ids[r].c_str());
        for (int t = 0; t < top_hits; t++) {
            const int32_t m = models[r * top_hits + t];
            if (m < 0) Die("read %s: an empty slot", ids[r].c_str());           // (cannot happen: enough informative models)
            fprintf(cls, t ? " %s" : "%s", names[m].c_str());
        }
        fputc('\n', cls);
    }
    if (fclose(cls) != 0) Die("write error on %s", class_name.c_str());
    gmg_tophits_free(th);
    gmg_reads_free(reads);
    return 0;
}
