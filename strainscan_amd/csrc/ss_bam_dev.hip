// ss_bam_dev.hip -- a BAM sample from its inflated stream to the flat base block.
//
// A BAM is BGZF (gzip members of at most 64 KB) around one stream: "BAM\1", l_text and the header text, n_ref and the
// reference entries, then length-prefixed records.  The reads a BAM contributes are those of a default `samtools fastq`:
// secondary (0x100) and supplementary (0x800) records and records without bases are skipped, a 0x10 record is
// reverse-complemented back to the read as sequenced, every 4-bit code becomes its letter of "=ACMGRSVTWYHKDBN".  The flat
// block is each kept record's letters and a '\n': the flat block of the FASTQ made from the BAM, byte for byte.
//
// Device path (the stream already lies on the device, gpu_gunzip of ss_ginflate.hip):
//   1  walk: one wave per segment of the stream (a BGZF member's text, or 64 KB); its 64 lanes test 64 candidate entries at a
//      time for the guessed entry -- the first position at which a chain of well-formed records starts; htslib writers usually
//      begin a member with a record, so that is the first candidate -- and lane 0 walks from there to the exit, the first record
//      start behind the segment
//   2  on the host: segment 0's entry (the end of the header) is exact; a segment whose entry differs from the exit of the
//      one before is walked again from that exit, until every entry equals the exit in front of it.  By induction that is
//      the sequential walk; a segment that a record spans entirely owns no record start and is not walked
//   3  the record starts, kept flags -> exclusive sum (blocks of 4096 KEPT records go round the ranks of a sharded run)
//      -> each kept record's length + 1 -> exclusive sum -> 16 lanes per record decode the nibbles
// Host path (bam_decode): the same rules in one sequential walk; it serves what the device declines and is the cross-check.
#include "ss_bam.h"

#include <hipcub/hipcub.hpp>
#include <zlib.h>

#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <vector>

namespace ss {
std::atomic<uint64_t> g_bam_dev_files{0}, g_bam_host_files{0}, g_bam_kept{0}, g_bam_skipped{0};
std::atomic<long long> g_hook_bam_walk_decline{0};      // ss_test_hook 7: the device walk declines (as after MAX_ROUNDS)
}

namespace {

constexpr int SHARD_LOG2 = 12;                   // as ss_fastq_dev.hip: blocks of 4096 records go round the ranks
constexpr uint64_t SEG = 64ull << 10;            // segment of a stream that is not BGZF (or a member's text, at most 64 KB)
constexpr uint64_t NONE = ~0ull;                 // no entry found in the segment
constexpr uint64_t FAIL = ~0ull - 1;             // the walk met a record that is not well formed
constexpr int MAX_ROUNDS = 64;                   // re-walk rounds before the device declines (the host walks it)

__host__ __device__ __forceinline__ uint32_t ld32(const uint8_t *s, uint64_t p)
{
    return (uint32_t)s[p] | (uint32_t)s[p + 1] << 8 | (uint32_t)s[p + 2] << 16 | (uint32_t)s[p + 3] << 24;
}
__host__ __device__ __forceinline__ uint32_t ld16(const uint8_t *s, uint64_t p) { return (uint32_t)s[p] | (uint32_t)s[p + 1] << 8; }

// The record at p: 4 + block_size when it is well formed (block_size >= 32 and large enough for its fields, a read name of
// at least one byte that ends with NUL, all of it inside the stream), else 0.  The one rule of both paths.
__host__ __device__ __forceinline__ uint64_t rec_len(const uint8_t *s, uint64_t n, uint64_t p)
{
    if (p > n || n - p < 36) return 0;
    const int32_t bs = (int32_t)ld32(s, p);
    if (bs < 32 || (uint64_t)bs > n - p - 4) return 0;
    const uint64_t lrn = s[p + 12], ncig = ld16(s, p + 16), lseq = ld32(s, p + 20);
    if (lrn == 0 || 32 + lrn + 4 * ncig + (lseq + 1) / 2 + lseq > (uint64_t)bs || s[p + 36 + lrn - 1] != 0) return 0;
    return 4 + (uint64_t)bs;
}

// a candidate entry of the guess only: the reference ids lie in [-1, n_ref), the positions are >= -1
__device__ __forceinline__ bool plausible(const uint8_t *s, uint64_t p, int32_t n_ref)
{
    const int32_t ref = (int32_t)ld32(s, p + 4), pos = (int32_t)ld32(s, p + 8);
    const int32_t nref = (int32_t)ld32(s, p + 24), npos = (int32_t)ld32(s, p + 28);
    return ref >= -1 && ref < n_ref && nref >= -1 && nref < n_ref && pos >= -1 && npos >= -1;
}

// q may be a record start: four plausible, well-formed records follow one another from q (or fewer that end exactly at the end
// of the stream)
__device__ __forceinline__ bool chain_at(const uint8_t *s, uint64_t n, uint64_t q, int32_t n_ref)
{
    uint64_t p = q;
    int ok = 0;
    for (; ok < 4 && p < n; ok++) {
        const uint64_t l = rec_len(s, n, p);
        if (!l || !plausible(s, p, n_ref)) break;
        p += l;
    }
    return ok == 4 || (ok > 0 && p == n);
}

// one wave per listed segment m: entry (guessed first when `search`: the first q in [lo[m], lo[m+1]) where chain_at holds, the
// wave testing 64 consecutive candidates at a time -- a segment inside a long read has none and is searched to its end), then
// lane 0 walks to the exit and counts the record starts in [lo[m], lo[m+1])
__global__ __launch_bounds__(64) void bam_walk_kernel(const uint8_t *__restrict__ s, uint64_t n, const uint64_t *__restrict__ lo,
                                                      const uint32_t *__restrict__ which, uint32_t n_which, int32_t n_ref, int search,
                                                      uint64_t *__restrict__ entry, uint64_t *__restrict__ exit_, uint32_t *__restrict__ count)
{
    const uint32_t i = blockIdx.x;
    if (i >= n_which) return;
    const uint32_t m = which ? which[i] : i;
    const uint64_t b0 = lo[m], b1 = lo[m + 1];
    const int lane = (int)threadIdx.x;
    uint64_t p = entry[m];
    if (search && m > 0) {
        p = NONE;
        for (uint64_t q0 = b0; q0 < b1; q0 += 64) {              // (uniform across the wave: the ballot decides for all lanes)
            const uint64_t q = q0 + (uint64_t)lane;
            const unsigned long long hit = __ballot(q < b1 && chain_at(s, n, q, n_ref));
            if (hit) { p = q0 + (uint64_t)(__ffsll(hit) - 1); break; }
        }
        if (lane == 0) entry[m] = p;
    }
    if (lane != 0) return;
    uint32_t c = 0;
    if (p != NONE) {
        while (p < b1) {                           // every record is >= 36 bytes: at most (b1 - b0) / 36 + 1 rounds
            const uint64_t l = rec_len(s, n, p);
            if (!l) { p = FAIL; c = 0; break; }
            p += l;
            c++;
        }
    }
    exit_[m] = p;
    count[m] = c;
}

// the record starts of segment m from its (settled) entry -> rec[base[m] ...]
__global__ __launch_bounds__(64) void bam_list_kernel(const uint8_t *__restrict__ s, uint64_t n, const uint64_t *__restrict__ entry,
                                                      const uint32_t *__restrict__ count, const uint64_t *__restrict__ base, uint32_t n_seg,
                                                      uint64_t *__restrict__ rec)
{
    const uint32_t m = blockIdx.x * blockDim.x + threadIdx.x;
    if (m >= n_seg) return;
    uint64_t p = entry[m], o = base[m];
    for (uint32_t c = 0; c < count[m]; c++) {
        rec[o + c] = p;
        p += rec_len(s, n, p);                      // (checked by the walk)
    }
}

__global__ void bam_keep_kernel(const uint8_t *__restrict__ s, const uint64_t *__restrict__ rec, uint64_t n_rec, uint32_t *__restrict__ keep)
{
    const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r > n_rec) return;
    if (r == n_rec) { keep[r] = 0; return; }
    const uint64_t p = rec[r];
    keep[r] = (ld16(s, p + 18) & 0x900u) == 0 && ld32(s, p + 20) != 0 ? 1u : 0u;
}

// len1[r] = the kept record's bases + its '\n' when record r belongs to this rank, else 0
__global__ void bam_len_kernel(const uint8_t *__restrict__ s, const uint64_t *__restrict__ rec, const uint32_t *__restrict__ keep,
                               const uint32_t *__restrict__ kidx, uint64_t n_rec, uint32_t shard_rank, uint32_t shard_world,
                               uint64_t *__restrict__ len1)
{
    const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r > n_rec) return;
    if (r == n_rec) { len1[r] = 0; return; }
    len1[r] = keep[r] && (kidx[r] >> SHARD_LOG2) % shard_world == shard_rank ? (uint64_t)ld32(s, rec[r] + 20) + 1 : 0;
}

__device__ __forceinline__ char bam_letter(const uint8_t *seq, uint64_t i, bool rev)
{
    const uint32_t b = seq[i >> 1];
    uint32_t c = (i & 1) ? (b & 15u) : (b >> 4);
    if (rev) c = (c & 1u) << 3 | (c & 2u) << 1 | (c & 4u) >> 1 | (c & 8u) >> 3;      // complement = the four bits reversed
    return "=ACMGRSVTWYHKDBN"[c];
}

// ... and under the base-quality mask 'N' where qual[i] < thr -- qual: the l_seq Phred values behind the packed bases, in the
// same stored order (rec_len has checked that they lie inside the record); *n += 1 then
template <bool MASK>
__device__ __forceinline__ char bam_letter_q(const uint8_t *seq, const uint8_t *qual, uint64_t i, bool rev, uint32_t thr, uint32_t *n)
{
    if (MASK && qual[i] < thr) { *n += 1; return 'N'; }
    return bam_letter(seq, i, rev);
}

// kept record r -> dst + off[r]: its letters (reverse-complemented for 0x10) and '\n'; 16 lanes per record, 16 letters per lane
// and round.  MASK (ss_set_min_base_qual): thr = the lowest quality kept; a record without qualities (qual[0] == 0xFF) is
// not masked and counted; masked[0] += bases masked, masked[1] += such records
template <bool MASK>
__global__ __launch_bounds__(256) void bam_decode_kernel(const uint8_t *__restrict__ s, const uint64_t *__restrict__ rec,
                                                         const uint64_t *__restrict__ len1, const uint64_t *__restrict__ off,
                                                         uint64_t n_rec, char *__restrict__ dst, uint32_t thr,
                                                         unsigned long long *__restrict__ masked)
{
    const uint64_t r = (uint64_t)blockIdx.x * 16 + (threadIdx.x >> 4);
    uint32_t cnt = 0, noq = 0;
    if (r < n_rec && len1[r]) {
        const uint64_t p = rec[r], lseq = len1[r] - 1, o = off[r];
        const uint8_t *seq = s + p + 36 + s[p + 12] + 4 * (uint64_t)ld16(s, p + 16);
        const uint8_t *qual = seq + (lseq + 1) / 2;
        const bool rev = (ld16(s, p + 18) & 0x10u) != 0;
        // (a record without qualities: 0xFF in every place by the format, but only qual[0] is what says so)
        const uint32_t t = MASK && qual[0] != 0xFF ? thr : 0u;
        for (uint64_t c = (uint64_t)(threadIdx.x & 15) * 16; c < lseq; c += 256) {
            if (c + 16 <= lseq) {
                char v[16];
#pragma unroll
                for (int k = 0; k < 16; k++) v[k] = bam_letter_q<MASK>(seq, qual, rev ? lseq - 1 - (c + k) : c + k, rev, t, &cnt);
                __builtin_memcpy(dst + o + c, v, 16);
            } else {
                for (uint64_t k = c; k < lseq; k++) dst[o + k] = bam_letter_q<MASK>(seq, qual, rev ? lseq - 1 - k : k, rev, t, &cnt);
            }
        }
        if ((threadIdx.x & 15) == 0) {
            dst[o + lseq] = '\n';
            if (MASK && qual[0] == 0xFF) noq = 1;
        }
    }
    if (MASK) {
        for (int d = 32; d; d >>= 1) {
            cnt += (uint32_t)__shfl_xor((int)cnt, d, 64);
            noq += (uint32_t)__shfl_xor((int)noq, d, 64);
        }
        if ((threadIdx.x & 63) == 0) {
            if (cnt) atomicAdd(&masked[0], (unsigned long long)cnt);
            if (noq) atomicAdd(&masked[1], (unsigned long long)noq);
        }
    }
}

__global__ void bam_pad_kernel(char *dst, uint64_t from, uint64_t to)
{
    const uint64_t i = from + (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < to) dst[i] = '\n';
}

}  // namespace

namespace ss {

// The header of a BAM stream: 1 = *end is the first record's offset, 0 = more than `avail` bytes are needed, -1 = not a BAM
// stream or a damaged header.
int bam_header(const uint8_t *h, uint64_t avail, uint64_t n, uint64_t *end, int32_t *n_ref)
{
    auto need = [&](uint64_t q) { return q <= avail ? 1 : (q <= n ? 0 : -1); };
    int r = need(12);
    if (r <= 0) return r;
    if (memcmp(h, "BAM\1", 4) != 0) return -1;
    const int32_t l_text = (int32_t)ld32(h, 4);
    if (l_text < 0) return -1;
    uint64_t p = 8 + (uint64_t)l_text;
    if ((r = need(p + 4)) <= 0) return r;
    const int32_t nr = (int32_t)ld32(h, p);
    if (nr < 0) return -1;
    p += 4;
    for (int32_t i = 0; i < nr; i++) {
        if ((r = need(p + 4)) <= 0) return r;
        const int32_t l_name = (int32_t)ld32(h, p);
        if (l_name < 0) return -1;
        p += 4 + (uint64_t)l_name + 4;
        if ((r = need(p)) <= 0) return r;
    }
    *end = p;
    *n_ref = nr;
    return 1;
}

// The host path: the flat block of this rank's kept records -> out (NULL: lengths only; else *out_len bytes are written).
// SS_EIO when the stream is damaged (nothing is to be used then).
int bam_decode(const uint8_t *s, uint64_t n, int shard_rank, int shard_world, char *out, uint64_t *out_len, uint64_t *n_own,
               uint64_t *n_kept, uint64_t *n_skipped)
{
    uint64_t p = 0;
    int32_t n_ref = 0;
    if (bam_header(s, n, n, &p, &n_ref) != 1) return SS_EIO;
    static const char letters[] = "=ACMGRSVTWYHKDBN";
    uint64_t o = 0, kept = 0, skipped = 0, own = 0, masked = 0, noqual = 0;
    const uint32_t min_qual = (uint32_t)min_base_qual();
    while (p < n) {
        const uint64_t l = rec_len(s, n, p);
        if (!l) return SS_EIO;
        const uint32_t flag = ld16(s, p + 18);
        const uint64_t lseq = ld32(s, p + 20);
        if ((flag & 0x900u) || lseq == 0) {
            skipped++;
        } else {
            if ((int)((kept >> SHARD_LOG2) % (uint64_t)shard_world) == shard_rank) {
                if (out) {
                    const uint8_t *seq = s + p + 36 + s[p + 12] + 4 * (uint64_t)ld16(s, p + 16);
                    if (flag & 0x10u) {
                        for (uint64_t j = 0; j < lseq; j++) {
                            const uint64_t i = lseq - 1 - j;
                            uint32_t c = (i & 1) ? (seq[i >> 1] & 15u) : (seq[i >> 1] >> 4);
                            c = (c & 1u) << 3 | (c & 2u) << 1 | (c & 4u) >> 1 | (c & 8u) >> 3;
                            out[o + j] = letters[c];
                        }
                    } else {
                        for (uint64_t j = 0; j < lseq; j++) out[o + j] = letters[(j & 1) ? (seq[j >> 1] & 15u) : (seq[j >> 1] >> 4)];
                    }
                    out[o + lseq] = '\n';
                    // base-quality mask: qual[i] < Q -> 'N', in the stored order; a record without qualities is left as it is
                    const uint8_t *qual = seq + (lseq + 1) / 2;
                    if (min_qual && qual[0] == 0xFF) noqual++;
                    else if (min_qual) {
                        for (uint64_t j = 0; j < lseq; j++)
                            if (qual[(flag & 0x10u) ? lseq - 1 - j : j] < min_qual) { out[o + j] = 'N'; masked++; }
                    }
                }
                o += lseq + 1;
                own++;
            }
            kept++;
        }
        p += l;
    }
    if (out) mask_count(masked, noqual);
    *out_len = o;
    if (n_own) *n_own = own;
    if (n_kept) *n_kept = kept;
    if (n_skipped) *n_skipped = skipped;
    return SS_OK;
}

// The segments of the inflated stream: the text of every BGZF member (ISIZE of each trailer), cut to 64 KB pieces where a
// member is larger (a plain gzip BAM is one member).  -> starts, ascending, the first 0
std::vector<uint64_t> bam_segments(const uint8_t *in, uint64_t in_n, uint64_t n)
{
    std::vector<uint64_t> seg;
    uint64_t pos = 0, o = 0;
    bool bgzf = true;
    while (pos < in_n && bgzf) {
        if (pos + 18 > in_n || in[pos] != 0x1f || in[pos + 1] != 0x8b || !(in[pos + 3] & 4)) { bgzf = false; break; }
        const uint64_t xlen = ld16(in, pos + 10);
        uint64_t bsize = 0;
        for (uint64_t q = pos + 12; q + 4 <= pos + 12 + xlen && q + 4 <= in_n;) {
            const uint64_t slen = ld16(in, q + 2);
            if (in[q] == 'B' && in[q + 1] == 'C' && slen == 2 && q + 6 <= in_n) bsize = ld16(in, q + 4) + 1;
            q += 4 + slen;
        }
        if (bsize < 26 || pos + bsize > in_n) { bgzf = false; break; }
        const uint64_t isize = ld32(in, pos + bsize - 4);
        for (uint64_t c = 0; c < isize; c += SEG) seg.push_back(o + c);
        o += isize;
        pos += bsize;
    }
    if (!bgzf || o != n) {
        seg.clear();
        for (uint64_t c = 0; c < n; c += SEG) seg.push_back(c);
    }
    if (seg.empty()) seg.push_back(0);
    return seg;
}

// The inflated stream on the device -> a new device buffer (big_malloc, padded like a block of ss_reads) with the flat block of
// this rank's kept records.  0 = done, 1 = declined (too many re-walk rounds, too many records: the host decodes it), SS_EIO =
// damaged, other < 0 = SS_E*.  `seg` are the segment starts of bam_segments.
// `recs` (ss_bam_extract.hip): the record starts, kept flags and kept ordinals stay with the caller when the call returns 0; with
// recs->host_rec the starts are the caller's (the host walk: nothing is walked here, and nothing declines but too many records).
int bam_to_flat_dev(const char *d_stream, uint64_t n, const std::vector<uint64_t> &seg_in, int shard_rank, int shard_world,
                    char **d_flat, uint64_t *flat_len, uint64_t *flat_cap, uint64_t *n_records, BamRecords *recs)
{
    hipStream_t st = call_stream_get();
    if (!st) return SS_EHIP;
    const uint8_t *s = reinterpret_cast<const uint8_t *>(d_stream);
    uint64_t *d_lo = nullptr, *d_entry = nullptr, *d_exit = nullptr, *d_base = nullptr, *d_rec = nullptr, *d_len1 = nullptr, *d_off = nullptr;
    uint32_t *d_count = nullptr, *d_which = nullptr, *d_keep = nullptr, *d_kidx = nullptr;
    unsigned long long *d_masked = nullptr;
    void *d_tmp = nullptr;
    char *flat = nullptr;
    const int min_qual = min_base_qual();
    auto done = [&](int r) {
        void *scratch[] = {d_lo, d_entry, d_exit, d_base, d_rec, d_len1, d_off, d_count, d_which, d_keep, d_kidx, d_masked, d_tmp};
        for (void *q : scratch) {
            if (r == 0 && recs && q && (q == d_rec || q == d_keep || q == d_kidx)) continue;      // the caller's from here on
            if (r == 0 && recs && recs->want_off && q && q == d_off) continue;
            if (q) hipFreeAsync(q, st);
        }
        hipStreamSynchronize(st);
        call_stream_put(st);
        if (r != 0 && flat) big_put(flat, *flat_cap);
        return r;
    };
#define BM(call) do { if ((call) != hipSuccess) return done(SS_EHIP); } while (0)
    // the header, from the first bytes of the stream (more of them while the reference entries go on)
    uint64_t hdr_end = 0;
    int32_t n_ref = 0;
    {
        std::vector<uint8_t> h;
        for (uint64_t want = std::min<uint64_t>(n, 1ull << 20);; want = std::min<uint64_t>(n, want * 4)) {
            h.resize(want);
            BM(hipMemcpyAsync(h.data(), s, want, hipMemcpyDeviceToHost, st));
            BM(hipStreamSynchronize(st));
            const int r = bam_header(h.data(), want, n, &hdr_end, &n_ref);
            if (r < 0) return done(SS_EIO);
            if (r > 0) break;
        }
    }
    // segments behind the header; the first one starts at the first record (its entry is exact)
    std::vector<uint64_t> lo{hdr_end};
    for (uint64_t b : seg_in) if (b > hdr_end && b < n) lo.push_back(b);
    const uint32_t n_seg = (uint32_t)lo.size();
    lo.push_back(n);
    std::vector<uint64_t> entry(n_seg, 0), exit_(n_seg, 0);
    std::vector<uint32_t> count(n_seg, 0);
    uint64_t n_rec = 0;
    const bool given = recs && recs->host_rec;
    if (given) {
        n_rec = recs->host_n_rec;
        if (n_rec >= 0x7FFFFFF0ull) return done(1);
    } else if (hdr_end < n) {
        if (g_hook_bam_walk_decline.load()) return done(1);
        entry[0] = hdr_end;
        BM(hipMallocAsync((void **)&d_lo, (n_seg + 1) * 8, st));
        BM(hipMallocAsync((void **)&d_entry, n_seg * 8, st));
        BM(hipMallocAsync((void **)&d_exit, n_seg * 8, st));
        BM(hipMallocAsync((void **)&d_count, n_seg * 4, st));
        BM(hipMallocAsync((void **)&d_which, n_seg * 4, st));
        BM(hipMemcpyAsync(d_lo, lo.data(), (n_seg + 1) * 8, hipMemcpyHostToDevice, st));
        BM(hipMemcpyAsync(d_entry, entry.data(), 8, hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(bam_walk_kernel, dim3(n_seg), dim3(64), 0, st, s, n, (const uint64_t *)d_lo, (const uint32_t *)nullptr,
                           n_seg, n_ref, 1, d_entry, d_exit, d_count);
        BM(hipGetLastError());
        BM(hipMemcpyAsync(entry.data(), d_entry, n_seg * 8, hipMemcpyDeviceToHost, st));
        BM(hipMemcpyAsync(exit_.data(), d_exit, n_seg * 8, hipMemcpyDeviceToHost, st));
        BM(hipMemcpyAsync(count.data(), d_count, n_seg * 4, hipMemcpyDeviceToHost, st));
        BM(hipStreamSynchronize(st));
        // settle the entries: segment m's true entry is the exit of m - 1 once that one walked from ITS true entry
        for (int round = 0;; round++) {
            std::vector<uint32_t> dirty;
            uint64_t e = hdr_end;
            bool exact = true;                                                 // e is the true entry (no dirty segment before it)
            for (uint32_t m = 0; m < n_seg; m++) {
                if (e >= lo[m + 1]) { entry[m] = exit_[m] = e; count[m] = 0; continue; }       // a record spans the segment
                if (entry[m] != e) {
                    entry[m] = e;
                    dirty.push_back(m);
                    exact = false;
                    if (exit_[m] == NONE || exit_[m] == FAIL) break;          // nothing to go on behind it this round
                    e = exit_[m];                                              // (a guess: confirmed or corrected next round)
                    continue;
                }
                if (exit_[m] == FAIL || exit_[m] == NONE) {
                    if (exact) return done(SS_EIO);                            // walked from its true entry: damaged
                    break;
                }
                e = exit_[m];
            }
            if (dirty.empty()) break;
            if (round >= MAX_ROUNDS) return done(1);
            const uint32_t nw = (uint32_t)dirty.size();
            BM(hipMemcpyAsync(d_entry, entry.data(), n_seg * 8, hipMemcpyHostToDevice, st));
            BM(hipMemcpyAsync(d_which, dirty.data(), nw * 4, hipMemcpyHostToDevice, st));
            hipLaunchKernelGGL(bam_walk_kernel, dim3(nw), dim3(64), 0, st, s, n, (const uint64_t *)d_lo, (const uint32_t *)d_which, nw,
                               n_ref, 0, d_entry, d_exit, d_count);
            BM(hipGetLastError());
            std::vector<uint64_t> ex(n_seg);
            std::vector<uint32_t> ct(n_seg);
            BM(hipMemcpyAsync(ex.data(), d_exit, n_seg * 8, hipMemcpyDeviceToHost, st));
            BM(hipMemcpyAsync(ct.data(), d_count, n_seg * 4, hipMemcpyDeviceToHost, st));
            BM(hipStreamSynchronize(st));
            for (uint32_t m : dirty) { exit_[m] = ex[m]; count[m] = ct[m]; }
        }
        for (uint32_t m = 0; m < n_seg; m++) n_rec += count[m];
        if (n_rec >= 0x7FFFFFF0ull) return done(1);
    }
    uint64_t total = 0, kept = 0;
    if (n_rec) {
        BM(hipMallocAsync((void **)&d_rec, n_rec * 8, st));
        BM(hipMallocAsync((void **)&d_keep, (n_rec + 1) * 4, st));
        BM(hipMallocAsync((void **)&d_kidx, (n_rec + 1) * 4, st));
        BM(hipMallocAsync((void **)&d_len1, (n_rec + 1) * 8, st));
        BM(hipMallocAsync((void **)&d_off, (n_rec + 1) * 8, st));
        if (given) {
            BM(hipMemcpyAsync(d_rec, recs->host_rec, n_rec * 8, hipMemcpyHostToDevice, st));
            BM(hipStreamSynchronize(st));
        } else {
            BM(hipMallocAsync((void **)&d_base, n_seg * 8, st));
            std::vector<uint64_t> base(n_seg);
            uint64_t b = 0;
            for (uint32_t m = 0; m < n_seg; m++) { base[m] = b; b += count[m]; }
            BM(hipMemcpyAsync(d_base, base.data(), n_seg * 8, hipMemcpyHostToDevice, st));
            BM(hipMemcpyAsync(d_entry, entry.data(), n_seg * 8, hipMemcpyHostToDevice, st));
            BM(hipMemcpyAsync(d_count, count.data(), n_seg * 4, hipMemcpyHostToDevice, st));
            BM(hipStreamSynchronize(st));                 // (the host vectors go out of scope)
            hipLaunchKernelGGL(bam_list_kernel, dim3((n_seg + 63) / 64), dim3(64), 0, st, s, n, (const uint64_t *)d_entry, (const uint32_t *)d_count,
                               (const uint64_t *)d_base, n_seg, d_rec);
        }
        const unsigned g = (unsigned)((n_rec + 1 + 255) / 256);
        hipLaunchKernelGGL(bam_keep_kernel, dim3(g), dim3(256), 0, st, s, (const uint64_t *)d_rec, n_rec, d_keep);
        BM(hipGetLastError());
        size_t tmp_bytes = 0, tmp2 = 0;
        BM(hipcub::DeviceScan::ExclusiveSum(nullptr, tmp_bytes, d_keep, d_kidx, (int)(n_rec + 1), st));
        BM(hipcub::DeviceScan::ExclusiveSum(nullptr, tmp2, d_len1, d_off, (int)(n_rec + 1), st));
        tmp_bytes = std::max<size_t>(std::max(tmp_bytes, tmp2), 16);
        BM(hipMallocAsync(&d_tmp, tmp_bytes, st));
        size_t t1 = tmp_bytes;
        BM(hipcub::DeviceScan::ExclusiveSum(d_tmp, t1, d_keep, d_kidx, (int)(n_rec + 1), st));
        hipLaunchKernelGGL(bam_len_kernel, dim3(g), dim3(256), 0, st, s, (const uint64_t *)d_rec, (const uint32_t *)d_keep, (const uint32_t *)d_kidx,
                           n_rec, (uint32_t)shard_rank, (uint32_t)shard_world, d_len1);
        BM(hipGetLastError());
        size_t t2 = tmp_bytes;
        BM(hipcub::DeviceScan::ExclusiveSum(d_tmp, t2, d_len1, d_off, (int)(n_rec + 1), st));
        uint32_t k32 = 0;
        BM(hipMemcpyAsync(&k32, d_kidx + n_rec, 4, hipMemcpyDeviceToHost, st));
        BM(hipMemcpyAsync(&total, d_off + n_rec, 8, hipMemcpyDeviceToHost, st));
        BM(hipStreamSynchronize(st));
        kept = k32;
    }
    const uint64_t cap = ss_reads::padded(total);
    *flat_cap = cap;
    if (ss::big_malloc((void **)&flat, cap, flat_cap) != hipSuccess) { flat = nullptr; return done(SS_ENOMEM); }
    unsigned long long masked[2] = {0, 0};
    if (n_rec && min_qual > 0) {
        BM(hipMallocAsync((void **)&d_masked, 16, st));
        BM(hipMemsetAsync(d_masked, 0, 16, st));
        hipLaunchKernelGGL(bam_decode_kernel<true>, dim3((unsigned)((n_rec + 15) / 16)), dim3(256), 0, st, s, (const uint64_t *)d_rec,
                           (const uint64_t *)d_len1, (const uint64_t *)d_off, n_rec, flat, (uint32_t)min_qual, d_masked);
        BM(hipMemcpyAsync(masked, d_masked, 16, hipMemcpyDeviceToHost, st));
    } else if (n_rec) {
        hipLaunchKernelGGL(bam_decode_kernel<false>, dim3((unsigned)((n_rec + 15) / 16)), dim3(256), 0, st, s, (const uint64_t *)d_rec,
                           (const uint64_t *)d_len1, (const uint64_t *)d_off, n_rec, flat, 0u, (unsigned long long *)nullptr);
    }
    hipLaunchKernelGGL(bam_pad_kernel, dim3(1), dim3(64), 0, st, flat, total, cap);
    BM(hipGetLastError());
    BM(hipStreamSynchronize(st));
    mask_count(masked[0], masked[1]);
#undef BM
    *d_flat = flat;
    *flat_len = total;
    uint64_t own = 0;
    const uint64_t blk = 1ull << SHARD_LOG2, n_blk = (kept + blk - 1) / blk;
    for (uint64_t b = (uint64_t)shard_rank; b < n_blk; b += (uint64_t)shard_world) own += std::min<uint64_t>(blk, kept - b * blk);
    *n_records = own;
    g_bam_kept += kept;
    g_bam_skipped += n_rec - kept;
    if (recs) { recs->d_rec = d_rec; recs->d_keep = d_keep; recs->d_kidx = d_kidx; recs->n_rec = n_rec; recs->kept = kept; recs->hdr_end = hdr_end; }
    if (recs && recs->want_off) recs->d_off = d_off;
    return done(0);
}

void BamRecords::release()
{
    bool any = false;
    for (void *q : {(void *)d_rec, (void *)d_keep, (void *)d_kidx, (void *)d_off})
        if (q) { (void)hipFreeAsync(q, ss::l2s::stream()); any = true; }
    if (any) (void)ss::l2s::sync();
    d_rec = nullptr;
    d_keep = d_kidx = nullptr;
    d_off = nullptr;
}

int bam_records_flat_dev(const char *d_stream, uint64_t n, const uint8_t *h_stream, const std::vector<uint64_t> &seg, char **d_flat,
                         uint64_t *flat_len, uint64_t *flat_cap, BamRecords *recs)
{
    uint64_t n_own = 0;
    int rc = bam_to_flat_dev(d_stream, n, seg, 0, 1, d_flat, flat_len, flat_cap, &n_own, recs);
    if (rc != 1) return rc;
    // the device walk declined: the host walks
    std::vector<uint8_t> copy;
    if (!h_stream) {
        copy.resize(n);
        SS_HIP(hipMemcpy(copy.data(), d_stream, n, hipMemcpyDeviceToHost));
        h_stream = copy.data();
    }
    std::vector<uint64_t> host_rec;
    uint64_t hdr_end = 0;
    rc = bam_host_records(h_stream, n, &host_rec, &hdr_end);
    if (rc) return rc;
    recs->host_rec = host_rec.data();
    recs->host_n_rec = host_rec.size();
    rc = bam_to_flat_dev(d_stream, n, seg, 0, 1, d_flat, flat_len, flat_cap, &n_own, recs);
    recs->host_rec = nullptr;
    recs->host_n_rec = 0;
    return rc == 1 ? SS_ERANGE : rc;                                    // (1: more records than hipcub's int item count holds)
}

// One BAM file on the device: inflated there (ss_ginflate.hip), decoded there.  0 = done, 1 = declined (small file, not
// inflated on the device, no room, ...: nothing returned), SS_EIO = the stream is damaged, other < 0 = SS_E*.
int gz_bam_to_flat_dev(const char *path, int shard_rank, int shard_world, char **d_flat, uint64_t *flat_len, uint64_t *flat_cap,
                       uint64_t *n_records)
{
    static const bool trace = getenv("SS_INGEST_TRACE") != nullptr;
    const auto t0 = std::chrono::steady_clock::now();
    auto since = [&] { return std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count(); };
    if (!gz_on_gpu() || g_hook_decline.load()) return 1;
    const int fd = open(path, O_RDONLY);
    if (fd < 0) return 1;
    struct stat sb;
    if (fstat(fd, &sb) != 0 || !S_ISREG(sb.st_mode) || sb.st_size < (1 << 20)) { close(fd); return 1; }
    const uint64_t in_n = (uint64_t)sb.st_size;
    const uint8_t *in = (const uint8_t *)mmap(nullptr, in_n, PROT_READ, MAP_PRIVATE, fd, 0);
    if (in == MAP_FAILED) { close(fd); return 1; }
    char *d_text = nullptr;
    uint64_t n = 0;
    void *lease = nullptr;
    const bool ok = in[0] == 0x1f && in[1] == 0x8b && gpu_gunzip(in, in_n, &d_text, &n, &lease, fd);
    close(fd);
    std::vector<uint64_t> seg;
    if (ok) seg = bam_segments(in, in_n, n);
    munmap((void *)in, in_n);
    if (!ok) return 1;
    if (trace) fprintf(stderr, "[ingest] %s: %.1f MB of BAM stream on the device at %.4f s\n", path, n / 1e6, since());
    const int rc = bam_to_flat_dev(d_text, n, seg, shard_rank, shard_world, d_flat, flat_len, flat_cap, n_records);
    gpu_gunzip_done(lease);
    if (trace) fprintf(stderr, "[ingest] %s: %zu segments decoded (rc %d) at %.4f s\n", path, seg.size(), rc, since());
    if (rc == 0) g_bam_dev_files++;
    return rc;
}

// The inflated stream of one BAM file on the host (INPUT_BAM_GZ: the host inflaters; INPUT_BAM_RAW: the file mapped).  SS_OK,
// SS_EIO (unreadable, a member's CRC or length), SS_ENOMEM.
BamHostStream::~BamHostStream()
{
    if (map) munmap(map, map_n);
    free(text);
}

int bam_host_stream(const char *path, int kind, BamHostStream *out)
{
    char *&text = out->text;
    uint64_t &n = out->n;
    if (kind == INPUT_BAM_RAW) {
        const int fd = open(path, O_RDONLY);
        if (fd < 0) return SS_EIO;
        struct stat sb;
        if (fstat(fd, &sb) != 0 || !S_ISREG(sb.st_mode)) { close(fd); return SS_EIO; }
        out->map_n = (uint64_t)sb.st_size;
        out->map = out->map_n ? mmap(nullptr, out->map_n, PROT_READ, MAP_PRIVATE, fd, 0) : nullptr;
        close(fd);
        if (out->map == MAP_FAILED) { out->map = nullptr; return SS_EIO; }
        out->s = (const uint8_t *)out->map;
        n = out->map_n;
    } else if (inflate_whole(path, inflate_budget_bytes(), &text, &n, 0, 0)) {
        out->s = (const uint8_t *)text;
    } else {
        // zlib: every member in turn, each checked against its CRC-32 and length (a missing BGZF EOF block is no error).  The whole
        // stream is held, within the same budget as the other host inflaters (SS_INFLATE_MAX_GB): a BAM whose stream is larger
        // than that fails with SS_ENOMEM rather than taking the host's memory (the host path does not stream)
        const uint64_t budget = inflate_budget_bytes();
        gzFile g = gzopen(path, "rb");
        if (!g) return SS_EIO;
        gzbuffer(g, 1 << 20);
        uint64_t cap = std::min<uint64_t>(1ull << 24, std::max<uint64_t>(budget, 1));
        text = (char *)malloc(cap);
        int err = text ? Z_OK : Z_MEM_ERROR;
        while (err == Z_OK) {
            if (n == cap) {
                if (cap >= budget) { err = Z_MEM_ERROR; break; }
                char *t2 = (char *)realloc(text, cap = std::min(cap * 2, budget));
                if (!t2) { err = Z_MEM_ERROR; break; }
                text = t2;
            }
            const int got = gzread(g, text + n, (unsigned)std::min<uint64_t>(cap - n, 1u << 30));
            if (got < 0) { err = Z_DATA_ERROR; break; }
            if (got == 0) { gzerror(g, &err); if (err == Z_OK && !gzeof(g)) err = Z_DATA_ERROR; break; }
            n += (uint64_t)got;
        }
        int zerr = Z_OK;
        gzerror(g, &zerr);
        gzclose(g);
        if (err != Z_OK || (zerr != Z_OK && zerr != Z_STREAM_END)) { free(text); text = nullptr; n = 0; return err == Z_MEM_ERROR ? SS_ENOMEM : SS_EIO; }
        out->s = (const uint8_t *)text;
    }
    return SS_OK;
}

int BamDeviceStream::upload(const void *stream, uint64_t n_bytes)
{
    if (big_malloc((void **)&copy, ss_reads::padded(n_bytes), &copy_cap) != hipSuccess) { copy = nullptr; return SS_ENOMEM; }
    if (n_bytes) SS_HIP(hipMemcpy(copy, stream, n_bytes, hipMemcpyHostToDevice));
    d = copy;
    n = n_bytes;
    h = (const uint8_t *)stream;
    seg = bam_segments(nullptr, 0, n);
    return SS_OK;
}

int BamDeviceStream::open_file(const char *path, int kind)
{
    if (kind == INPUT_BAM_GZ && gz_on_gpu() && !g_hook_decline.load()) {
        const int fd = open(path, O_RDONLY);
        struct stat sb;
        if (fd >= 0 && fstat(fd, &sb) == 0 && S_ISREG(sb.st_mode) && sb.st_size >= (1 << 20)) {
            const uint64_t in_n = (uint64_t)sb.st_size;
            const uint8_t *in = (const uint8_t *)mmap(nullptr, in_n, PROT_READ, MAP_PRIVATE, fd, 0);
            if (in != MAP_FAILED) {
                if (in[0] == 0x1f && in[1] == 0x8b && gpu_gunzip(in, in_n, &d, &n, &lease, fd)) seg = bam_segments(in, in_n, n);
                else d = nullptr;
                munmap((void *)in, in_n);
            }
        }
        if (fd >= 0) close(fd);
    }
    if (d) { inflated_on_device = true; return SS_OK; }
    const int rc = bam_host_stream(path, kind, &hs);
    return rc ? rc : upload(hs.s, hs.n);
}

void BamDeviceStream::release()
{
    if (lease) gpu_gunzip_done(lease);
    if (copy) big_put(copy, copy_cap);
    lease = nullptr;
    copy = d = nullptr;
}

// The record starts of a stream in one sequential walk (what the device walk settles on); *hdr_end = the first record's offset.
// SS_EIO: damaged.
int bam_host_records(const uint8_t *s, uint64_t n, std::vector<uint64_t> *rec, uint64_t *hdr_end)
{
    uint64_t p = 0;
    int32_t n_ref = 0;
    if (bam_header(s, n, n, &p, &n_ref) != 1) return SS_EIO;
    *hdr_end = p;
    while (p < n) {
        const uint64_t l = rec_len(s, n, p);
        if (!l) return SS_EIO;
        rec->push_back(p);
        p += l;
    }
    return SS_OK;
}

// The host path for one BAM file (INPUT_BAM_GZ or INPUT_BAM_RAW): the stream inflated on the host, decoded -> *flat (malloc, padded like a
// block of ss_reads).  SS_OK, SS_EIO (damaged: a member's CRC or length, a record, the header), SS_ENOMEM.
int bam_host_flat(const char *path, int kind, int shard_rank, int shard_world, char **flat, uint64_t *flat_len, uint64_t *n_records)
{
    BamHostStream hs;
    const int src = bam_host_stream(path, kind, &hs);
    if (src != SS_OK) return src;
    const uint8_t *s = hs.s;
    const uint64_t n = hs.n;
    uint64_t len = 0, own = 0, kept = 0, skipped = 0;
    int rc = bam_decode(s, n, shard_rank, shard_world, nullptr, &len, &own, &kept, &skipped);
    char *out = nullptr;
    if (rc == SS_OK) {
        out = (char *)malloc(ss_reads::padded(len));
        if (!out) rc = SS_ENOMEM;
        else rc = bam_decode(s, n, shard_rank, shard_world, out, &len, &own, &kept, &skipped);
    }
    if (rc != SS_OK) { free(out); return rc; }
    memset(out + len, '\n', ss_reads::padded(len) - len);
    *flat = out;
    *flat_len = len;
    *n_records = own;
    g_bam_host_files++;
    g_bam_kept += kept;
    g_bam_skipped += skipped;
    return SS_OK;
}

// One BAM input of a load or a scan: the device first (policy 0 and 1), the host for what it declines (policy 0 and 2).
// `on_dev(d_flat, len, cap, n_records)` takes over a device block (big_malloc'ed), `on_host(flat, len, n_records)` a host block
// (malloc'ed, padded; the callee frees it).  SS_EAGAIN: strict policy and the device declined.
int bam_input(const char *path, int kind, int shard_rank, int shard_world, const std::function<int(char *, uint64_t, uint64_t, uint64_t)> &on_dev,
              const std::function<int(char *, uint64_t, uint64_t)> &on_host)
{
    if (kind == INPUT_BAM_GZ && gz_on_gpu()) {
        char *d = nullptr;
        uint64_t len = 0, cap = 0, nrec = 0;
        const int r = gz_bam_to_flat_dev(path, shard_rank, shard_world, &d, &len, &cap, &nrec);
        if (r == 0) return on_dev(d, len, cap, nrec);
        if (r == SS_EIO) return r;                        // damaged: the same on every rank and on the host
        if (gz_policy() == 1) return SS_EAGAIN;           // declined (or this rank's own trouble): the ranks settle it
    }
    char *h = nullptr;
    uint64_t len = 0, nrec = 0;
    const int r = bam_host_flat(path, kind, shard_rank, shard_world, &h, &len, &nrec);
    if (r != SS_OK) return r;
    return on_host(h, len, nrec);
}

}  // namespace ss

extern "C" {

int ss_bam_decode(const void *stream, uint64_t n, int shard_rank, int shard_world, char *out, uint64_t cap, uint64_t *out_len,
                  uint64_t *n_records)
{
    if ((!stream && n) || !out_len || shard_world < 1 || shard_rank < 0 || shard_rank >= shard_world) return SS_EINVAL;
    uint64_t len = 0, own = 0;
    int rc = ss::bam_decode((const uint8_t *)stream, n, shard_rank, shard_world, nullptr, &len, &own, nullptr, nullptr);
    if (rc != SS_OK) return rc;
    *out_len = len;
    if (n_records) *n_records = own;
    if (!out) return SS_OK;
    if (cap < len) return SS_ERANGE;
    return ss::bam_decode((const uint8_t *)stream, n, shard_rank, shard_world, out, &len, &own, nullptr, nullptr);
}

int ss_bam_counters(uint64_t out[4])
{
    if (!out) return SS_EINVAL;
    out[0] = ss::g_bam_dev_files.load();
    out[1] = ss::g_bam_host_files.load();
    out[2] = ss::g_bam_kept.load();
    out[3] = ss::g_bam_skipped.load();
    return SS_OK;
}

int ss_input_kind(const char *path, int *kind)
{
    if (!path || !kind) return SS_EINVAL;
    const int k = ss::input_kind(path);
    *kind = k <= ss::INPUT_CRAM ? k : 0;            // (gzip or no file at all: "anything else")
    return SS_OK;
}

}  // extern "C"
