// Fuzz harness for ss_read_calls_write (strainscan_amd/csrc/ss_extract.hip), built with g++ -fsanitize=address,undefined by
// tests/test_read_calls_host.py::test_writer_fuzz_sanitized.  usage: read_calls_fuzz scratch_dir iterations
// Every iteration damages a small FASTQ / FASTA text (byte flips, markers and line ends dropped in, truncation, a stretch doubled),
// counts its records with the writer's own walker and hands the writer arrays that are consistent with that count -- exact-size
// heap copies, so that the sanitizer sees a read one entry too far -- or inconsistent in one way: a record too few or too many,
// an offset that steps back or past the lists' end, a class or a listed node outside the tree, a missing array.  A consistent
// call must succeed with one line per record; every other call must fail, and every failure must leave neither the file nor its
// .tmp behind.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <vector>
#include "../strainscan_amd/csrc/ss_extract.hip"

// what ss_extract.hip takes from the rest of the library (no device code is linked here)
namespace ss {
int min_base_qual() { return 0; }
int input_kind(const char *) { return 0; }
bool inflate_whole(const char *, uint64_t, char **, uint64_t *, int, unsigned) { return false; }
uint64_t inflate_budget_bytes() { return 1ull << 30; }
}  // namespace ss

static bool exists(const std::string &p)
{
    struct stat st;
    return stat(p.c_str(), &st) == 0;
}

static uint64_t lines_of(const std::string &p)
{
    FILE *f = fopen(p.c_str(), "rb");
    if (!f) return ~0ull;
    uint64_t n = 0;
    for (int c; (c = fgetc(f)) != EOF;) n += c == '\n';
    fclose(f);
    return n;
}

static void put_file(const std::string &p, const std::string &t)
{
    FILE *f = fopen(p.c_str(), "wb");
    if (!f) { perror(p.c_str()); exit(2); }
    if (!t.empty()) fwrite(t.data(), 1, t.size(), f);
    fclose(f);
}

int main(int argc, char **argv)
{
    if (argc < 3) return 2;
    const std::string dir = argv[1], in1 = dir + "/in1.txt", in2 = dir + "/in2.txt", out1 = dir + "/out1.tsv", out2 = dir + "/out2.tsv";
    const int iters = atoi(argv[2]);
    const std::string seeds[] = {
        "@r1 first\nACGTACGTAC\n+\nIIII#IIII5\n@r2\ttwo lines\nACGTA\nCGTTT\n+r2\nIIIII\n#####\n@\n\n+\n\n@r4\r\nacgtn\r\n+\r\n@+>I5\r\n@r5\nGGGG\n+\nII",
        ">s1 wrapped\nACGTACGTAC\nGTACGTACGT\nAC\n>s2\n\n>s3\r\nacgt\r\nNNNN\r\n\n>\nTTTT",
        "stray\n@r1\nAC\n+\nII\n\n\n>s1\nACGT\n@r2\nA\n+\nI\n",
    };
    uint64_t rng = 0x9E3779B97F4A7C15ull;
    auto rnd = [&] { rng ^= rng << 13; rng ^= rng >> 7; rng ^= rng << 17; return rng; };
    const char drops[] = {'\n', '@', '+', '>', '\r', 'N', '\t', ' ', '\0'};
    const uint32_t n_nodes = 5;
    const std::vector<int64_t> node_value = {-1, 11, 22, 33, -44, 5000000000ll};
    uint64_t good = 0, refused = 0;
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
        // the records of the text as the writer's walker sees them
        uint64_t pos = 0, n_all = 0, n_seq = 0;
        Record rec;
        while (next_record(t.data(), t.size(), &pos, 0u, &rec)) { n_all++; n_seq += !rec.flat.empty(); }
        put_file(in1, t);
        put_file(in2, t);
        for (int pairs = 0; pairs < 2; pairs++) {
            const uint64_t fit = pairs ? n_all : n_seq;
            // 0: consistent; the others: one thing wrong
            const int kind = it < 0 ? 0 : (int)(rnd() % 8);
            uint64_t n = fit;
            if (kind == 1) n = fit + 1;
            if (kind == 2) { if (!fit) continue; n = fit - 1; }
            std::vector<uint32_t> cls(n), score(n), node, hits;
            std::vector<uint64_t> first(n + 1);
            for (uint64_t i = 0; i < n; i++) {
                first[i] = node.size();
                cls[i] = (uint32_t)(rnd() % (n_nodes + 1));
                score[i] = (uint32_t)rnd();
                uint32_t v = 0;
                for (int e = (int)(rnd() % 4); e > 0 && v < n_nodes; e--) {
                    v += 1 + (uint32_t)(rnd() % 2);
                    if (v > n_nodes) break;
                    node.push_back(v);
                    hits.push_back((uint32_t)rnd());
                }
            }
            first[n] = node.size();
            bool broken = kind == 1 || kind == 2;
            // (first[n] is the lists' length by contract: it stays what the arrays hold)
            if (kind == 3 && n >= 2) { first[1 + rnd() % (n - 1)] = first[n] + 1 + rnd() % 3; broken = true; }      // past the lists' end
            if (kind == 4 && n >= 2) {                                                                              // a step back
                const uint64_t i = 1 + rnd() % (n - 1);
                first[i - 1] = first[i] + 1;
                broken = true;
            }
            if (kind == 5 && n) { cls[rnd() % n] = n_nodes + 1 + (uint32_t)(rnd() % 3); broken = true; }
            if (kind == 6 && !node.empty()) { node[rnd() % node.size()] = rnd() % 2 ? 0u : n_nodes + 1; broken = true; }
            const bool no_lists = kind == 7 && !node.empty();
            broken = broken || no_lists;
            // exact-size copies on the heap: nothing behind an array's end may be read
            std::vector<uint32_t> node_x(node.begin(), node.end()), hits_x(hits.begin(), hits.end());
            const char *ins[2] = {in1.c_str(), in2.c_str()}, *outs[2] = {out1.c_str(), out2.c_str()};
            uint64_t c[4];
            const int rc = ss_read_calls_write(ins, pairs ? 2 : 1, outs, n, n ? cls.data() : nullptr, n ? score.data() : nullptr, first.data(),
                                               no_lists || node_x.empty() ? nullptr : node_x.data(), no_lists || hits_x.empty() ? nullptr : hits_x.data(),
                                               node_value.data(), n_nodes, c);
            if (!broken) {
                if (rc != SS_OK) { fprintf(stderr, "iteration %d: a consistent call failed with %d\n", it, rc); return 1; }
                for (int f = 0; f <= pairs; f++)
                    if (lines_of(outs[f]) != n_all + 1 || exists(std::string(outs[f]) + ".tmp")) {
                        fprintf(stderr, "iteration %d: %llu lines for %llu records\n", it, (unsigned long long)lines_of(outs[f]), (unsigned long long)n_all);
                        return 1;
                    }
                if (c[0] != n_all * (pairs + 1) || c[1] != c[0] || c[3] != (n_all - n_seq) * (pairs + 1)) { fprintf(stderr, "iteration %d: counters\n", it); return 1; }
                good++;
            } else {
                if (rc == SS_OK) { fprintf(stderr, "iteration %d: an inconsistent call (kind %d) succeeded\n", it, kind); return 1; }
                refused++;
            }
            for (int f = 0; f < 2; f++) {
                if (rc != SS_OK && (exists(outs[f]) || exists(std::string(outs[f]) + ".tmp"))) {
                    fprintf(stderr, "iteration %d: a failure (kind %d, %d) left a file\n", it, kind, rc);
                    return 1;
                }
                unlink(outs[f]);
            }
        }
    }
    printf("read_calls_fuzz ok: %llu tables written, %llu calls refused\n", (unsigned long long)good, (unsigned long long)refused);
    return 0;
}
