// Fuzz harness for strainscan_amd/csrc/ss_extract.hip, built with g++ -fsanitize=address,undefined by
// tests/test_extract_host.py::test_record_walker_fuzz_sanitized.  usage: extract_fuzz scratch_dir iterations
// Every iteration damages a small FASTQ / FASTA text (byte flips, markers and line ends dropped in, truncation, a stretch
// doubled) and walks it with the writer's record walker, with and without the base-quality mask: the records must tile the
// text in order, a flat form never outgrows its text, and ss_extract_write with every digest selected must write exactly the
// records that have bases, byte for byte; the sanitizers watch every access.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <vector>
#include "../strainscan_amd/csrc/ss_extract.hip"

// what ss_extract.hip takes from the rest of the library (no device code is linked here)
static int g_min_qual = 0;
namespace ss {
int min_base_qual() { return g_min_qual; }
int input_kind(const char *) { return 0; }
bool inflate_whole(const char *, uint64_t, char **, uint64_t *, int, unsigned) { return false; }
uint64_t inflate_budget_bytes() { return 1ull << 30; }
}  // namespace ss

static std::string slurp(const std::string &p)
{
    std::string v;
    FILE *f = fopen(p.c_str(), "rb");
    if (!f) { perror(p.c_str()); exit(2); }
    char buf[1 << 16];
    size_t n;
    while ((n = fread(buf, 1, sizeof(buf), f)) > 0) v.append(buf, n);
    fclose(f);
    return v;
}

int main(int argc, char **argv)
{
    if (argc < 3) return 2;
    const std::string dir = argv[1], in_path = dir + "/in.txt", out_path = dir + "/out.txt";
    const int iters = atoi(argv[2]);
    const std::string seeds[] = {
        "@r1\nACGTACGTAC\n+\nIIII#IIII5\n@r2 two lines\nACGTA\nCGTTT\n+r2\nIIIII\n#####\n@r3\n\n+\n\n@r4\r\nacgtn\r\n+\r\n@+>I5\r\n@r5\nGGGG\n+\nII",
        ">s1 wrapped\nACGTACGTAC\nGTACGTACGT\nAC\n>s2\n\n>s3\r\nacgt\r\nNNNN\r\n\n>s4\nTTTT",
        "stray\n@r1\nAC\n+\nII\n\n\n>s1\nACGT\n@r2\nA\n+\nI\n",
    };
    uint64_t rng = 0x9E3779B97F4A7C15ull;
    auto rnd = [&] { rng ^= rng << 13; rng ^= rng >> 7; rng ^= rng << 17; return rng; };
    const char drops[] = {'\n', '@', '+', '>', '\r', 'N', '\0'};
    uint64_t walked = 0, written = 0;
    for (int it = -3; it < iters; it++) {
        std::string t = seeds[it < 0 ? it + 3 : rnd() % 3];
        if (it >= 0) {
            for (int m = 0; m < 1 + (int)(rnd() % 3) && !t.empty(); m++) {
                switch (rnd() % 5) {
                case 0: t[rnd() % t.size()] ^= (char)(1 + rnd() % 255); break;
                case 1: t.insert(rnd() % (t.size() + 1), 1, drops[rnd() % sizeof(drops)]); break;
                case 2: t.resize(rnd() % (t.size() + 1)); break;
                case 3: t.erase(rnd() % t.size(), 1 + rnd() % 4); break;
                default: { const size_t a = rnd() % t.size(), n = 1 + rnd() % 12; t.insert(a, t.substr(a, n)); break; }
                }
            }
        }
        // the walker reads [p, p + n) and not a byte more: an exact heap copy lets the sanitizer say so
        std::vector<char> text(t.begin(), t.end());
        for (int mq = 0; mq <= 20; mq += 20) {
            std::string want, flats;
            uint64_t pos = 0, prev_end = 0, n_with_bases = 0;
            Record rec;
            while (next_record(text.data(), text.size(), &pos, mq ? 33u + (unsigned)mq : 0u, &rec)) {
                if (!(rec.t0 >= prev_end && rec.t0 < rec.t1 && rec.t1 <= text.size() && pos == rec.t1) || rec.flat.size() > rec.t1 - rec.t0) {
                    fprintf(stderr, "iteration %d: a record out of place\n", it);
                    return 1;
                }
                if (text[rec.t0] != (rec.fastq ? '@' : '>')) { fprintf(stderr, "iteration %d: a record without its marker\n", it); return 1; }
                prev_end = rec.t1;
                walked++;
                // (a flat form with '\n' in it cannot come from a line; a '\0' may)
                if (rec.flat.find('\n') != std::string::npos) { fprintf(stderr, "iteration %d: a line end inside a flat form\n", it); return 1; }
                if (!rec.flat.empty()) {
                    want.append(text.data() + rec.t0, rec.t1 - rec.t0);
                    flats += rec.flat + "\n";
                    n_with_bases++;
                }
            }
            if (pos != text.size()) { fprintf(stderr, "iteration %d: the walk stopped early\n", it); return 1; }
            // every digest selected: the writer puts out exactly the records with bases
            g_min_qual = mq;
            uint64_t n_keys = 0;
            std::vector<uint64_t> keys(2 * n_with_bases + 2);
            if (ss_flat_record_keys(flats.data(), flats.size(), keys.data(), n_with_bases, &n_keys) != SS_OK || n_keys != n_with_bases) {
                fprintf(stderr, "iteration %d: %llu digests for %llu records\n", it, (unsigned long long)n_keys, (unsigned long long)n_with_bases);
                return 1;
            }
            FILE *f = fopen(in_path.c_str(), "wb");
            if (!f) { perror(in_path.c_str()); return 2; }
            if (!text.empty()) fwrite(text.data(), 1, text.size(), f);
            fclose(f);
            const char *ins[1] = {in_path.c_str()}, *outs[1] = {out_path.c_str()};
            uint64_t c[4];
            const int rc = ss_extract_write(ins, 1, keys.data(), n_keys, outs, c);
            if (rc != SS_OK) { fprintf(stderr, "iteration %d: ss_extract_write %d\n", it, rc); return 1; }
            if (c[1] != n_with_bases || slurp(out_path) != want) { fprintf(stderr, "iteration %d: WRONG TEXT written\n", it); return 1; }
            written += c[1];
        }
    }
    g_min_qual = 0;
    printf("extract_fuzz ok: %llu records walked, %llu written\n", (unsigned long long)walked, (unsigned long long)written);
    return 0;
}
