// Fuzz harness for ss_extract_write_pairs (strainscan_amd/csrc/ss_extract.hip), built with g++ -fsanitize=address,undefined by
// tests/test_pairs_host.py::test_pair_writer_fuzz_sanitized.  usage: pairs_fuzz scratch_dir iterations
// Every iteration damages two small FASTQ / FASTA texts (as tests/extract_fuzz.cpp does) and hands them to the writer as a pair,
// with and without the base-quality mask.  Files with different numbers of records: SS_EIO and no output file.  Otherwise, with
// every pair's digest selected, each output is its input's records in order, byte for byte -- a FASTQ record without bases with
// the one empty quality line behind its '+' line, where there is one -- and the counters are 2n, 2n, n, 0; with the digest of one
// pair selected, exactly the pairs that join to the same bytes.  The sanitizers watch every access.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <vector>
#include "../strainscan_amd/csrc/ss_extract.hip"

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

static bool exists(const std::string &p)
{
    FILE *f = fopen(p.c_str(), "rb");
    if (f) fclose(f);
    return f != nullptr;
}

struct Walked { std::vector<std::string> text, flat; };

// the records of a text as the pair writer writes them
static Walked walk(const std::vector<char> &text, unsigned thr)
{
    Walked w;
    uint64_t pos = 0;
    Record rec;
    while (next_record(text.data(), text.size(), &pos, thr, &rec)) {
        uint64_t t1 = rec.t1;
        if (rec.fastq && rec.flat.empty() && t1 < text.size() && text[t1] == '\n') pos = ++t1;      // its empty quality line
        w.text.emplace_back(text.data() + rec.t0, t1 - rec.t0);
        w.flat.push_back(rec.flat);
    }
    return w;
}

int main(int argc, char **argv)
{
    if (argc < 3) return 2;
    const std::string dir = argv[1];
    const std::string in_path[2] = {dir + "/in_1.txt", dir + "/in_2.txt"}, out_path[2] = {dir + "/out_1.txt", dir + "/out_2.txt"};
    const int iters = atoi(argv[2]);
    const std::string seeds[] = {
        "@r1\nACGTACGTAC\n+\nIIII#IIII5\n@r2 two lines\nACGTA\nCGTTT\n+r2\nIIIII\n#####\n@r3\n\n+\n\n@r4\r\nacgtn\r\n+\r\n@+>I5\r\n@r5\nGGGG\n+\nII",
        "@m1\n\n+\n\n@m2\nAN\n+\nII\n@m3\r\n\r\n+\r\n\r\n@m4\n\n+\n@m5\nA\n+\nI\n@m6\n\n+\n\n",
        ">s1 wrapped\nACGTACGTAC\nGTACGTACGT\nAC\n>s2\n\n>s3\r\nacgt\r\nNNNN\r\n\n>s4\nTTTT\n>s5\nC",
        "stray\n@r1\nAC\n+\nII\n\n\n>s1\nACGT\n@r2\nNC\n+\nII\n>e\n@r3\nA\n+\nI\n",
    };
    uint64_t rng = 0x9E3779B97F4A7C15ull;
    auto rnd = [&] { rng ^= rng << 13; rng ^= rng >> 7; rng ^= rng << 17; return rng; };
    const char drops[] = {'\n', '@', '+', '>', '\r', 'N', '\0'};
    uint64_t paired = 0, unequal = 0, written = 0;
    for (int it = -4; it < iters; it++) {
        std::vector<char> text[2];
        for (int f = 0; f < 2; f++) {
            std::string t = seeds[it < 0 ? (it + 4 + f) % 4 : rnd() % 4];
            for (int m = 0; it >= 0 && m < (int)(rnd() % 3) && !t.empty(); m++) {
                switch (rnd() % 5) {
                case 0: t[rnd() % t.size()] ^= (char)(1 + rnd() % 255); break;
                case 1: t.insert(rnd() % (t.size() + 1), 1, drops[rnd() % sizeof(drops)]); break;
                case 2: t.resize(rnd() % (t.size() + 1)); break;
                case 3: t.erase(rnd() % t.size(), 1 + rnd() % 4); break;
                default: { const size_t a = rnd() % t.size(), n = 1 + rnd() % 12; t.insert(a, t.substr(a, n)); break; }
                }
            }
            text[f].assign(t.begin(), t.end());
            FILE *fp = fopen(in_path[f].c_str(), "wb");
            if (!fp) { perror(in_path[f].c_str()); return 2; }
            if (!text[f].empty()) fwrite(text[f].data(), 1, text[f].size(), fp);
            fclose(fp);
        }
        const char *ins[2] = {in_path[0].c_str(), in_path[1].c_str()}, *outs[2] = {out_path[0].c_str(), out_path[1].c_str()};
        for (int mq = 0; mq <= 20; mq += 20) {
            g_min_qual = mq;
            const Walked w[2] = {walk(text[0], mq ? 33u + (unsigned)mq : 0u), walk(text[1], mq ? 33u + (unsigned)mq : 0u)};
            const size_t n = std::min(w[0].text.size(), w[1].text.size());
            std::vector<std::string> joined;
            std::string flats;
            for (size_t i = 0; i < n; i++) {
                joined.push_back(w[0].flat[i] + "N" + w[1].flat[i]);
                flats += joined.back() + "\n";
            }
            uint64_t n_keys = 0;
            std::vector<uint64_t> keys(2 * n + 2);
            if (ss_flat_record_keys(flats.data(), flats.size(), keys.data(), n, &n_keys) != SS_OK || n_keys != n) {
                fprintf(stderr, "iteration %d: %llu digests for %llu pairs\n", it, (unsigned long long)n_keys, (unsigned long long)n);
                return 1;
            }
            uint64_t c[4];
            int rc = ss_extract_write_pairs(ins, 2, keys.data(), n_keys, outs, c);
            if (w[0].text.size() != w[1].text.size()) {
                if (rc != SS_EIO || exists(out_path[0]) || exists(out_path[1]) || exists(out_path[0] + ".tmp") || exists(out_path[1] + ".tmp")) {
                    fprintf(stderr, "iteration %d: unequal record counts: %d, or a file left behind\n", it, rc);
                    return 1;
                }
                unequal++;
                continue;
            }
            if (rc != SS_OK || c[0] != 2 * n || c[1] != 2 * n || c[2] != n || c[3] != 0) { fprintf(stderr, "iteration %d: all pairs: %d\n", it, rc); return 1; }
            for (int f = 0; f < 2; f++) {
                std::string want;
                for (const auto &t : w[f].text) want += t;
                if (slurp(out_path[f]) != want) { fprintf(stderr, "iteration %d: WRONG TEXT written to file %d\n", it, f + 1); return 1; }
            }
            paired++;
            written += c[1];
            if (!n) continue;
            const size_t pick = rnd() % n;
            rc = ss_extract_write_pairs(ins, 2, keys.data() + 2 * pick, 1, outs, c);
            std::string want[2];
            uint64_t same = 0;
            for (size_t i = 0; i < n; i++)
                if (joined[i] == joined[pick]) { want[0] += w[0].text[i]; want[1] += w[1].text[i]; same++; }
            if (rc != SS_OK || c[2] != same || c[1] != 2 * same || slurp(out_path[0]) != want[0] || slurp(out_path[1]) != want[1]) {
                fprintf(stderr, "iteration %d: one pair: %d, %llu pairs written for %llu\n", it, rc, (unsigned long long)c[2], (unsigned long long)same);
                return 1;
            }
        }
        remove(out_path[0].c_str());
        remove(out_path[1].c_str());
    }
    g_min_qual = 0;
    printf("pairs_fuzz ok: %llu pairs of texts written, %llu with unequal record counts, %llu records\n", (unsigned long long)paired,
           (unsigned long long)unequal, (unsigned long long)written);
    return 0;
}
