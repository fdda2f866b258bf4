// ss_extract.hip -- the host half of `--extract_reads`: record digests and the writer (host code only).
//
// ss_reads_select (ss_select.hip) leaves the selected records on the device as a flat block; nothing in a resident set says
// where a record stood in its file (the parse threads place their blocks in arrival order, the binning permutes the records, a
// packed slab keeps nothing but A C G T N).  So the selection travels BY CONTENT: the caller digests the selected flat records
// (ss_flat_record_keys), and ss_extract_write reads the input files once more, forms every record's flat form exactly as the
// loader's host grammar does (ss_fastx_to_flat, ss_host.hip: the base-quality mask included) and writes the record's original
// text when the digest of that form is among the selected ones.
//
// The digest is 128 bits, two independent 64-bit hashes over the record's bytes and its length:
//   h1  FNV-1a (64-bit offset basis and prime) over the bytes, then over the eight bytes of the length;
//   h2  a multiply-rotate hash over little-endian 8-byte words (the tail zero-padded), seeded with the length and closed with
//       the splitmix64 finisher.
// A record that was not selected is written only if both collide with a selected record's: a 128-bit collision.
// ss_read_calls_write (`--read_calls`) shares the record walk and nothing else: its sets are in file order, it goes by position.
// No HIP in this file: tests/extract_fuzz.cpp compiles it with g++ -fsanitize=address,undefined as well.
#include <fcntl.h>
#include <sched.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>
#include <zlib.h>

#include <algorithm>
#include <atomic>
#include <string>
#include <thread>
#include <utility>
#include <vector>

#include "strainscan_hip.h"
#include "ss_input_text.h"

using ss::InputText;

namespace {

typedef std::pair<uint64_t, uint64_t> Digest;

inline uint64_t rotl64(uint64_t x, int r) { return (x << r) | (x >> (64 - r)); }

Digest record_digest(const char *p, uint64_t n)
{
    uint64_t h1 = 0xCBF29CE484222325ull;
    for (uint64_t i = 0; i < n; i++) { h1 ^= (uint8_t)p[i]; h1 *= 0x100000001B3ull; }
    for (int b = 0; b < 8; b++) { h1 ^= (uint8_t)(n >> (8 * b)); h1 *= 0x100000001B3ull; }
    uint64_t h2 = 0x9E3779B97F4A7C15ull ^ (n * 0xD6E8FEB86659FD93ull);
    for (uint64_t i = 0; i < n; i += 8) {
        uint64_t w = 0;
        memcpy(&w, p + i, (size_t)std::min<uint64_t>(8, n - i));
        h2 = rotl64(h2 ^ (w * 0xFF51AFD7ED558CCDull), 27) * 0xC4CEB9FE1A85EC53ull + 0x52DCE729ull;
    }
    h2 ^= n;
    h2 = (h2 ^ (h2 >> 30)) * 0xBF58476D1CE4E5B9ull;
    h2 = (h2 ^ (h2 >> 27)) * 0x94D049BB133111EBull;
    h2 ^= h2 >> 31;
    return Digest(h1, h2);
}

// One record of a FASTA / FASTQ text: its original text [t0, t1) and its flat form (the sequence lines concatenated, the
// base-quality mask applied) -- the grammar of ss_fastx_to_flat, one record at a time.
struct Record {
    uint64_t t0 = 0, t1 = 0;
    std::string flat;
    bool fastq = false;
};

inline uint64_t line_end(const char *t, uint64_t i, uint64_t len, bool *has_nl)
{
    const void *nl = memchr(t + i, '\n', len - i);
    *has_nl = nl != nullptr;
    return nl ? (uint64_t)((const char *)nl - t) : len;
}

// the next record at or behind *pos; false at the end of the text.  thr: 33 + the quality threshold, 0 = no mask
bool next_record(const char *t, uint64_t len, uint64_t *pos, unsigned thr, Record *rec)
{
    uint64_t i = *pos;
    bool nl;
    while (i < len) {
        if (t[i] == '\n') { i++; continue; }
        if (t[i] == '>') {
            rec->t0 = i;
            rec->fastq = false;
            rec->flat.clear();
            uint64_t e = line_end(t, i, len, &nl);
            i = nl ? e + 1 : len;
            while (i < len && t[i] != '>') {
                e = line_end(t, i, len, &nl);
                rec->flat.append(t + i, e - i);
                i = nl ? e + 1 : len;
            }
            rec->t1 = *pos = i;
            return true;
        }
        if (t[i] == '@') {
            rec->t0 = i;
            rec->fastq = true;
            rec->flat.clear();
            uint64_t qlen = 0;
            uint64_t e = line_end(t, i, len, &nl);
            i = nl ? e + 1 : len;
            while (i < len && t[i] != '+') {
                e = line_end(t, i, len, &nl);
                rec->flat.append(t + i, e - i);
                i = nl ? e + 1 : len;
            }
            const uint64_t seqlen = rec->flat.size();
            if (i < len) {                                   // the '+' line
                e = line_end(t, i, len, &nl);
                i = nl ? e + 1 : len;
            }
            while (i < len && qlen < seqlen) {
                e = line_end(t, i, len, &nl);
                if (thr) {
                    const uint64_t m = std::min<uint64_t>(e - i, seqlen - qlen);
                    for (uint64_t q = 0; q < m; q++)
                        if ((unsigned char)t[i + q] < thr) rec->flat[qlen + q] = 'N';
                }
                qlen += e - i;
                i = nl ? e + 1 : len;
            }
            rec->t1 = *pos = i;
            return true;
        }
        const uint64_t e = line_end(t, i, len, &nl);         // a stray line: skipped
        i = nl ? e + 1 : len;
    }
    *pos = len;
    return false;
}

// an output file that exists under its name only once everything went well
struct OutputFile {
    std::string path, tmp;
    FILE *f = nullptr;
    bool ok = true;
    bool open_tmp(const char *to)
    {
        path = to;
        tmp = path + ".tmp";
        f = fopen(tmp.c_str(), "wb");
        if (f) setvbuf(f, nullptr, _IOFBF, 1 << 20);
        return f != nullptr;
    }
    void put(const char *p, uint64_t n)
    {
        if (n && fwrite(p, 1, (size_t)n, f) != (size_t)n) ok = false;
    }
    bool commit()
    {
        if (!f) return false;
        const bool closed = fclose(f) == 0;
        f = nullptr;
        if (!ok || !closed || rename(tmp.c_str(), path.c_str()) != 0) { unlink(tmp.c_str()); return false; }
        tmp.clear();
        return true;
    }
    ~OutputFile()
    {
        if (f) fclose(f);
        if (!tmp.empty()) unlink(tmp.c_str());
    }
};

}  // namespace

extern "C" {

int ss_flat_record_keys(const char *flat, uint64_t len, uint64_t *keys, uint64_t cap, uint64_t *n_records)
{
    if ((len && !flat) || !n_records) return SS_EINVAL;
    uint64_t n = 0, i = 0;
    while (i < len) {
        const void *nl = memchr(flat + i, '\n', len - i);
        const uint64_t e = nl ? (uint64_t)((const char *)nl - flat) : len;
        if (e > i) {
            if (keys && n < cap) {
                const Digest d = record_digest(flat + i, e - i);
                keys[2 * n] = d.first;
                keys[2 * n + 1] = d.second;
            }
            n++;
        }
        i = e + 1;
    }
    *n_records = n;
    return (keys && n > cap) ? SS_ERANGE : SS_OK;
}

// ss_extract_write (fragments = false: a pair goes out when either mate's digest is selected) and ss_extract_write_pairs
// (fragments = true: the pair is ONE record, mate 1 + 'N' + mate 2, the record ss_reads_join_pairs_dev makes of it)
static int extract_write(const char *const *in_paths, int n_in, const uint64_t *keys, uint64_t n_keys, const char *const *out_paths,
                         uint64_t counters[4], bool fragments)
{
    if (!in_paths || !out_paths || !counters || n_in < 1 || n_in > 2 || (n_keys && !keys)) return SS_EINVAL;
    for (int f = 0; f < n_in; f++)
        if (!in_paths[f] || !out_paths[f] || !out_paths[f][0]) return SS_EINVAL;
    for (int c = 0; c < 4; c++) counters[c] = 0;
    std::vector<Digest> sel((size_t)n_keys);
    for (uint64_t i = 0; i < n_keys; i++) sel[(size_t)i] = Digest(keys[2 * i], keys[2 * i + 1]);
    std::sort(sel.begin(), sel.end());
    const int mq = ss::min_base_qual();
    const unsigned thr = mq > 0 ? 33u + (unsigned)mq : 0u;
    InputText in[2];
    for (int f = 0; f < n_in; f++) {
        const int rc = in[f].open_path(in_paths[f]);
        if (rc != SS_OK) return rc;
    }
    OutputFile out[2];
    for (int f = 0; f < n_in; f++)
        if (!out[f].open_tmp(out_paths[f])) return SS_EIO;
    uint64_t pos[2] = {0, 0};
    Record rec[2];
    std::string frag;
    for (;;) {
        bool have[2] = {false, false}, hit[2] = {false, false};
        for (int f = 0; f < n_in; f++) have[f] = next_record(in[f].p, in[f].n, &pos[f], thr, &rec[f]);
        if (n_in == 2 && have[0] != have[1]) return SS_EIO;          // unequal record counts (the outputs' destructors clean up)
        if (!have[0]) break;
        if (fragments) {
            counters[0] += 2;
            // a FASTQ record without bases ends behind its '+' line for next_record; its empty quality line is its text too
            for (int f = 0; f < 2; f++)
                if (rec[f].fastq && rec[f].flat.empty() && pos[f] < in[f].n && in[f].p[pos[f]] == '\n') rec[f].t1 = ++pos[f];
            frag.assign(rec[0].flat);
            frag.push_back('N');
            frag.append(rec[1].flat);
            if (!std::binary_search(sel.begin(), sel.end(), record_digest(frag.data(), frag.size()))) continue;
            for (int f = 0; f < 2; f++) out[f].put(in[f].p + rec[f].t0, rec[f].t1 - rec[f].t0);
            counters[1] += 2;
            counters[2]++;
            continue;
        }
        for (int f = 0; f < n_in; f++) {
            counters[0]++;
            if (!rec[f].flat.empty()) hit[f] = std::binary_search(sel.begin(), sel.end(), record_digest(rec[f].flat.data(), rec[f].flat.size()));
        }
        if (!(hit[0] || hit[1])) continue;
        for (int f = 0; f < n_in; f++) {
            out[f].put(in[f].p + rec[f].t0, rec[f].t1 - rec[f].t0);
            counters[1]++;
        }
        if (n_in == 2 && !hit[1]) counters[2]++;
        if (n_in == 2 && !hit[0]) counters[3]++;
    }
    bool ok = true;
    for (int f = 0; f < n_in; f++) ok = out[f].commit() && ok;
    if (!ok) {
        for (int f = 0; f < n_in; f++) unlink(out_paths[f]);
        return SS_EIO;
    }
    return SS_OK;
}

int ss_extract_write(const char *const *in_paths, int n_in, const uint64_t *keys, uint64_t n_keys, const char *const *out_paths,
                     uint64_t counters[4])
{
    return extract_write(in_paths, n_in, keys, n_keys, out_paths, counters, false);
}

int ss_extract_write_pairs(const char *const *in_paths, int n_in, const uint64_t *keys, uint64_t n_keys, const char *const *out_paths,
                           uint64_t counters[4])
{
    if (n_in != 2) return SS_EINVAL;
    return extract_write(in_paths, n_in, keys, n_keys, out_paths, counters, true);
}

}  // extern "C"

// `--read_calls`: the table of ss_reads_calls' numbers beside the names of the input's records.  Nothing here goes by content:
// the set was loaded in file order (ss_reads_load_ordered, or joined in line order), so the i-th record of the file that has a
// sequence is record i of the set (two files of a joined set: record j of both is fragment j).  The walk is next_record's, the
// cost per record a name, four numbers and the list's items.  One file is shared over host threads by the chunks of
// text_chunk_starts -- the chunks ss_reads_load_ordered parsed it in: a first pass counts every chunk's records with a sequence,
// the prefix sum of the counts is each chunk's first entry, a second pass formats the chunks, and the text goes out in chunk
// order.  Two files are walked in lockstep by one thread (their chunks do not begin at the same records).
namespace ss {
// (ss_ingest.hip; weak: a program that holds this file alone -- the fuzz harnesses under tests/ -- walks every text as one chunk)
__attribute__((weak)) bool text_chunk_starts(const char *t, uint64_t n, std::vector<uint64_t> *starts);
}

namespace {

// the arrays of ss_reads_calls, as ss_read_calls_write was given them (checked before anything is read through them)
struct CallsTable {
    uint64_t n_records;
    const uint32_t *rec_class, *rec_score;
    const uint64_t *rec_first;
    const uint32_t *list_node, *list_hits;
    const int64_t *node_value;
};

// the line of one record; entry: the record of the set it takes, ~0 for a record that has none
void calls_line(const CallsTable &T, const char *text, uint64_t text_n, const Record &r, uint64_t entry, std::string *dst)
{
    char num[64];
    uint64_t h0 = r.t0 + 1, h1 = h0;                                // the name: behind the marker, up to white space or the line's end
    while (h1 < text_n && text[h1] != ' ' && text[h1] != '\t' && text[h1] != '\r' && text[h1] != '\n') h1++;
    dst->append(text + h0, (size_t)(h1 - h0));
    if (entry == ~0ull) {
        dst->append("\t-1\t0\t0\t-\n");
        return;
    }
    const uint64_t length = r.flat.size() - (uint64_t)std::count(r.flat.begin(), r.flat.end(), '\r');
    snprintf(num, sizeof(num), "\t%lld\t%u\t%llu\t", (long long)T.node_value[T.rec_class[entry]], T.rec_score[entry], (unsigned long long)length);
    dst->append(num);
    const uint64_t e0 = T.rec_first[entry], e1 = T.rec_first[entry + 1];
    if (e0 == e1) dst->push_back('-');
    for (uint64_t e = e0; e < e1; e++) {
        snprintf(num, sizeof(num), "%s%lld:%u", e > e0 ? " " : "", (long long)T.node_value[T.list_node[e]], T.list_hits[e]);
        dst->append(num);
    }
    dst->push_back('\n');
}

// host threads of the writer: SS_HOST_THREADS, else the CPUs this process may run on; at most 16
unsigned calls_threads()
{
    long n = 0;
    if (const char *e = getenv("SS_HOST_THREADS")) n = atol(e);
    if (n <= 0) {
        cpu_set_t set;
        n = sched_getaffinity(0, sizeof(set), &set) == 0 ? CPU_COUNT(&set) : 1;
    }
    return (unsigned)std::min<long>(std::max<long>(n, 1), 16);
}

// fn(c) for every c < n on up to `threads` threads
template <class F>
void over_chunks(size_t n, unsigned threads, F fn)
{
    std::atomic<size_t> next(0);
    auto worker = [&] {
        for (size_t c; (c = next.fetch_add(1)) < n;) fn(c);
    };
    threads = (unsigned)std::min<size_t>(threads, n);
    if (threads <= 1) return worker();
    std::vector<std::thread> pool;
    for (unsigned w = 0; w < threads; w++) pool.emplace_back(worker);
    for (auto &th : pool) th.join();
}

// one file: SS_OK with the table in `out` (not yet committed), SS_EIO where the file's records are not the table's
int calls_one_file(const CallsTable &T, const InputText &in, unsigned thr, OutputFile &out, uint64_t counters[4])
{
    std::vector<uint64_t> starts;
    if (!ss::text_chunk_starts || !ss::text_chunk_starts(in.p, in.n, &starts)) { starts.assign(1, 0); starts.push_back(in.n); }
    const size_t n_chunks = starts.size() - 1;
    const unsigned threads = calls_threads();
    // the records with a sequence of every chunk (whether a record has one does not depend on the quality mask)
    std::vector<uint64_t> first(n_chunks + 1, 0);
    over_chunks(n_chunks, threads, [&](size_t c) {
        const char *t = in.p + starts[c];
        const uint64_t len = starts[c + 1] - starts[c];
        uint64_t pos = 0, n = 0;
        Record rec;
        while (next_record(t, len, &pos, 0u, &rec)) n += !rec.flat.empty();
        first[c + 1] = n;
    });
    for (size_t c = 0; c < n_chunks; c++) first[c + 1] += first[c];
    if (first[n_chunks] != T.n_records) return SS_EIO;              // the file is not the one the set was loaded from
    // the text, `threads` chunks at a time, written in chunk order
    std::vector<std::string> text(n_chunks);
    std::vector<uint64_t> n_read(n_chunks, 0), n_class(n_chunks, 0), n_empty(n_chunks, 0);
    std::atomic<bool> bad(false);
    for (size_t c0 = 0; c0 < n_chunks; c0 += threads) {
        const size_t c1 = std::min<size_t>(n_chunks, c0 + threads);
        over_chunks(c1 - c0, threads, [&](size_t k) {
            const size_t c = c0 + k;
            const char *t = in.p + starts[c];
            const uint64_t len = starts[c + 1] - starts[c];
            uint64_t pos = 0, entry = first[c];
            Record rec;
            std::string &dst = text[c];
            dst.reserve((size_t)(len / 4));
            while (next_record(t, len, &pos, thr, &rec)) {
                n_read[c]++;
                if (rec.flat.empty()) {
                    n_empty[c]++;
                    calls_line(T, t, len, rec, ~0ull, &dst);
                    continue;
                }
                if (entry >= first[c + 1]) { bad = true; return; }      // (never: the first pass counted this chunk)
                n_class[c] += T.rec_class[entry] != 0u;
                calls_line(T, t, len, rec, entry++, &dst);
            }
            if (entry != first[c + 1]) bad = true;
        });
        if (bad) return SS_EIO;
        for (size_t c = c0; c < c1; c++) {
            out.put(text[c].data(), text[c].size());
            std::string().swap(text[c]);
            counters[0] += n_read[c];
            counters[1] += n_read[c];
            counters[2] += n_class[c];
            counters[3] += n_empty[c];
        }
    }
    return SS_OK;
}

// two files of a joined set, in lockstep: record j of both takes entry j
int calls_two_files(const CallsTable &T, const InputText in[2], unsigned thr, OutputFile out[2], uint64_t counters[4])
{
    uint64_t pos[2] = {0, 0}, next = 0;
    Record rec[2];
    std::string line;
    for (;;) {
        bool have[2];
        for (int f = 0; f < 2; f++) have[f] = next_record(in[f].p, in[f].n, &pos[f], thr, &rec[f]);
        if (have[0] != have[1]) return SS_EIO;                       // unequal record counts
        if (!have[0]) break;
        if (next >= T.n_records) return SS_EIO;
        for (int f = 0; f < 2; f++) {
            line.clear();
            calls_line(T, in[f].p, in[f].n, rec[f], next, &line);
            out[f].put(line.data(), line.size());
            counters[0]++;
            counters[1]++;
            counters[2] += T.rec_class[next] != 0u;
            counters[3] += rec[f].flat.empty();
        }
        next++;
    }
    return next == T.n_records ? SS_OK : SS_EIO;
}

}  // namespace

extern "C" {

int ss_read_calls_write(const char *const *in_paths, int n_in, const char *const *out_paths, uint64_t n_records, const uint32_t *rec_class,
                        const uint32_t *rec_score, const uint64_t *rec_first, const uint32_t *list_node, const uint32_t *list_hits,
                        const int64_t *node_value, uint32_t n_nodes, uint64_t counters[4])
{
    if (!in_paths || !out_paths || !counters || n_in < 1 || n_in > 2 || !rec_first || !node_value) return SS_EINVAL;
    if (n_records && (!rec_class || !rec_score)) return SS_EINVAL;
    for (int f = 0; f < n_in; f++)
        if (!in_paths[f] || !out_paths[f] || !out_paths[f][0]) return SS_EINVAL;
    for (int c = 0; c < 4; c++) counters[c] = 0;
    // the arrays are read as they say they lie: ascending offsets, classes and nodes of this tree
    const uint64_t n_list = rec_first[n_records];
    if (n_list && (!list_node || !list_hits)) return SS_EINVAL;
    for (uint64_t i = 0; i < n_records; i++)
        if (rec_first[i] > rec_first[i + 1] || rec_first[i + 1] > n_list || rec_class[i] > n_nodes) return SS_EINVAL;
    for (uint64_t e = 0; e < n_list; e++)
        if (list_node[e] < 1 || list_node[e] > n_nodes) return SS_EINVAL;
    const CallsTable T{n_records, rec_class, rec_score, rec_first, list_node, list_hits, node_value};
    const int mq = ss::min_base_qual();
    const unsigned thr = mq > 0 ? 33u + (unsigned)mq : 0u;
    InputText in[2];
    for (int f = 0; f < n_in; f++) {
        const int rc = in[f].open_path(in_paths[f]);
        if (rc != SS_OK) return rc;
    }
    OutputFile out[2];
    for (int f = 0; f < n_in; f++) {
        if (!out[f].open_tmp(out_paths[f])) return SS_EIO;
        static const char header[] = "name\tnode\tscore\tlength\thits\n";
        out[f].put(header, sizeof(header) - 1);
    }
    const int rc = n_in == 1 ? calls_one_file(T, in[0], thr, out[0], counters) : calls_two_files(T, in, thr, out, counters);
    if (rc != SS_OK) return rc;                                      // (the outputs' destructors clean up)
    bool ok = true;
    for (int f = 0; f < n_in; f++) ok = out[f].commit() && ok;
    if (!ok) {
        for (int f = 0; f < n_in; f++) unlink(out_paths[f]);
        return SS_EIO;
    }
    return SS_OK;
}

}  // extern "C"
