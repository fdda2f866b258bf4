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
// No HIP in this file: tests/extract_fuzz.cpp compiles it with g++ -fsanitize=address,undefined as well.
#include <fcntl.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>
#include <zlib.h>

#include <algorithm>
#include <string>
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
