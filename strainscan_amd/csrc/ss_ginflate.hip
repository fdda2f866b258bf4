// ss_ginflate.hip -- a gzip file inflated by thousands of waves on the GPU.
//
// The reference pipes `zcat` into jellyfish (library/identify.py:81-84).  ss_pgz.hip restates the two-pass scheme of
// Kerbiriou & Chikhi (pugz, 2019) on host threads; on a box whose cgroup grants 16 CPUs that is 11-14 M reads/s, twenty
// times slower than plain text reaches HBM.  The same scheme on the device:
//   A  sync     the deflate data is cut into chunks of SS_GZ_CHUNK bytes.  Every wave searches its chunk for a block
//               entry: the 64 lanes test 64 consecutive bit positions at a time with a register-only header check
//               (non-final dynamic block, complete code-length code); a survivor's header is parsed by the whole wave
//               (code lengths decoded lane-parallel, canonical codes built with ballots: the Kraft sums reject it
//               before a table is written) and 512 symbols are decoded.
//   A2 subsync  a block is entered every SS_GZ_SPLIT_KB (12 KB) of deflate data as well: Huffman-coded data synchronises
//               itself, so a wave that decodes from any bit inside a block with the block's tables -- all 64 bit offsets of
//               a window as hypotheses -- is left with ONE offset after a few windows: an item's first bit, an entry.
//   B  inflate  every wave decodes from its entry to the next chunk's entry.  The 64 lanes decode whole items (literal,
//               or length + distance with their extra bits) SPECULATIVELY at 64 consecutive bit positions of the
//               LDS-staged input; the wave follows the chain of item lengths (readlane), a prefix sum places the items.
//               What lies in the 32 KB in front of the chunk is unknown: the output is 16-bit symbols, a byte or "byte
//               w of the window" (a copy of a copy keeps the index).  The last 2048 symbols are mirrored in an LDS
//               ring; matches that reach further back read the wave's own output from global memory, all such
//               matches of a window together (one lane per symbol) and while the next window is decoded.
//   C  windows  the last 32 KB of every chunk as a map "my window -> the next chunk's window", composed in two levels;
//   D  bytes    all symbols -> bytes in parallel; CRC-32 of the text by segments (combined on the host).
// B-D run SEGMENT by segment (128 MB of deflate data): a segment's text is complete before the next one starts, so the
// window in front of a segment is the end of the text so far, and the scratch (a reusable arena, ~6 GB) does not grow
// with the file.
// Accepted only if every chunk ended exactly on the next one's entry, the stream ended at the file's last trailer and
// CRC-32 and ISIZE of EVERY member match (lanes joined with `cat` are found member by member: the chunk that meets a
// final block finds trailer and header behind it).  A wrong entry (a position inside a block that passed A) shows as the
// chunk before it running past it and is dropped.  A bgzip file (BGZF: every member names its size) needs no search: its
// members are the chunks.  Anything else (a chunk that expands more than 12 times, more than 8 MB of deflate data without a dynamic
// block's start -- stored blocks only --, a damaged file) returns "not handled" and the caller inflates on the host
// (ss_pgz.hip, libdeflate, zlib), so a wrong text cannot get through.
// This file is the driver: one call as the steps of `Gunzip`.  The device code it launches is ss_ginflate_dev.h; what the process
// keeps between calls (scratch arenas, pinned upload buffers, streams) is ss_gz_scratch.hip; range mode's chain between ranks is
// ss_gz_range.hip; ss_ginflate.h declares what the three share.
#include "ss_ginflate_dev.h"

#include <fcntl.h>
#include <sys/stat.h>
#include <unistd.h>
#include <zlib.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <future>
#include <vector>

namespace {

void gf2_square(uint32_t *sq, const uint32_t *mat) { for (int i = 0; i < 32; i++) sq[i] = gf2_times(mat, mat[i]); }
void crc_zero_operator(uint32_t *op /*[32]*/, int log2_bytes)
{
    uint32_t a[32], b[32];
    a[0] = 0xEDB88320u;                                   // one zero BIT
    for (int i = 1; i < 32; i++) a[i] = 1u << (i - 1);
    gf2_square(b, a); gf2_square(a, b); gf2_square(b, a);  // 2, 4, 8 bits = one byte (in b)
    uint32_t *cur = b, *oth = a;
    for (int k = 0; k < log2_bytes; k++) { gf2_square(oth, cur); std::swap(cur, oth); }
    for (int i = 0; i < 32; i++) op[i] = cur[i];
}

// bgzip (BGZF): every member carries its size in an extra field ("BC", 2 bytes: BSIZE = size - 1), so the members -- at most
// 64 KB of text each, nothing in front of any -- are found without decoding.  -> (first data byte, trailer byte) of every
// member, or nothing when the file is not BGZF throughout
struct Bgzf { uint64_t data, trailer; };
std::vector<Bgzf> bgzf_members(const uint8_t *p, uint64_t n)
{
    std::vector<Bgzf> out;
    uint64_t pos = 0;
    while (pos < n) {
        if (pos + 18 > n || p[pos] != 0x1f || p[pos + 1] != 0x8b || p[pos + 2] != 8 || p[pos + 3] != 4) return {};
        const uint64_t xlen = (uint64_t)p[pos + 10] | (uint64_t)p[pos + 11] << 8;
        if (xlen < 6 || pos + 12 + xlen > n) return {};
        uint64_t bsize = 0;
        for (uint64_t q = pos + 12; q + 4 <= pos + 12 + xlen;) {
            const uint64_t slen = (uint64_t)p[q + 2] | (uint64_t)p[q + 3] << 8;
            if (p[q] == 'B' && p[q + 1] == 'C' && slen == 2 && q + 6 <= pos + 12 + xlen) bsize = ((uint64_t)p[q + 4] | (uint64_t)p[q + 5] << 8) + 1;
            q += 4 + slen;
        }
        if (bsize < 12 + xlen + 2 + 8 || pos + bsize > n) return {};
        out.push_back(Bgzf{pos + 12 + xlen, pos + bsize - 8});
        pos += bsize;
    }
    return out;
}

}  // namespace

namespace ss {

// The file image `in` (host) inflated on the device.  true: *text_dev holds *len bytes, every member verified against its
// trailer; the buffer belongs to the scratch arena of the call and is lent until gpu_gunzip_done(*lease).  false: not
// handled here (the caller inflates on the host).
static std::atomic<uint64_t> g_handled{0}, g_declined{0}, g_range_files{0}, g_range_pieces{0};
// ss_test_hook 1 and 2: nothing in the environment can switch these on
std::atomic<long long> g_hook_entry{0}, g_hook_decline{0};

bool gpu_gunzip(const uint8_t *in, uint64_t in_n, char **text_dev, uint64_t *len, void **lease, int fd)
{
    return gpu_gunzip_impl(in, in_n, text_dev, len, lease, fd, nullptr);
}

namespace {

// ---- one call of the device gunzip: its state, and its stages as member functions ------------------------------------------------
// The file's chunks: one per entry (a chunk of the search without one belongs to its predecessor).  `fresh`: the first
// chunk of a gzip member (nothing in front of it); `last`: it ends with the member's final block, the trailer follows
// at `trailer`.
// `hdr`: ~0, or -- an entry INSIDE a block (subsync_kernel) -- where that block's header is.
struct Chunk { uint64_t start; bool fresh, last; uint64_t trailer; uint64_t hdr = ~0ull; };
// range mode: one segment per slice of this rank, its look-ahead entries [gj, gj + n_ph) behind it
struct Seg { size_t gi, gj, n_ph; uint32_t slice; uint64_t hdr_bit; };
struct Member { uint64_t at, len; uint32_t crc, isize; bool open; uint32_t crc0; uint64_t len0; };      // crc0, len0: range mode -- the member's part in the slices before
// A chunk while its segment is inflated: its symbol region [off, off + cap) and what inflate_kernel reported for it
struct Rec : Chunk { uint64_t off = 0, cap = 0, len = 0, end = 0; int status = 0; };
// One segment on its way from chunks to text.  `ph`: up to two look-ahead entries behind the chunks (what a chunk may run over)
struct Segment {
    size_t gi = 0, gj = 0;                // G[gi, gj)
    std::vector<Rec> ch;
    std::vector<Chunk> ph;
    uint32_t consumed_ph = 0;             // look-ahead entries that turned out to lie inside a block of this segment
    std::vector<uint64_t> text_off;       // where every chunk's text begins
    size_t m_first = 0;                   // members[m_first, ...) have text in this segment
};
// the host's side of the per-chunk device arrays (lives until the stream has been synchronised)
struct Staging { std::vector<uint64_t> start, stop, off, cap, hdr, len, end; std::vector<int> status; };
// range mode: what came down the chain in front of a slice
struct ChainIn { uint64_t nl = 0, len = 0; uint32_t crc = (uint32_t)crc32(0L, Z_NULL, 0); std::vector<uint8_t> carry; };

constexpr size_t SEG_CHUNKS = 16384;      // chunks of a segment at most
constexpr uint32_t LOOK = 64;             // search chunks behind a slice in which its last chunk's stop is looked for
constexpr uint64_t SYM_RATIO = 12;        // symbols reserved per byte of deflate data

// What the environment sets, read on EVERY call (the tests change it between the calls of one process)
struct Tunables {
    // SS_GZ_SPLIT_KB: blocks are entered every so many KB of deflate data (subsync_kernel; 0 = at their starts only)
    uint64_t split_bytes = 12 << 10, chunk_bytes = 0, seg_bytes = 128ull << 20, slice_bytes = 0;      // (slice_bytes 0: not set here)
    const bool run_over = getenv("SS_GZ_NO_RUNOVER") == nullptr;      // (test hook: wrong entries are then handled by the host only)
    Tunables()
    {
        if (const char *e = getenv("SS_GZ_SPLIT_KB")) split_bytes = (uint64_t)std::max<long long>(0, atoll(e)) << 10;
        chunk_bytes = split_bytes ? 16 << 10 : 32 << 10;      // (split: every block's start should be found)
        if (const char *e = getenv("SS_GZ_CHUNK")) chunk_bytes = std::max<uint64_t>(4096, (uint64_t)atoll(e));
        if (const char *e = getenv("SS_GZ_SEG_KB")) seg_bytes = std::max<uint64_t>(64, (uint64_t)atoll(e)) << 10;      // (tests: many segments)
        seg_bytes = std::max(seg_bytes, 8 * chunk_bytes);
        if (const char *e = getenv("SS_GZ_SLICE_KB")) slice_bytes = std::max<uint64_t>(64, (uint64_t)atoll(e)) << 10;      // (tests: many slices)
    }
};

// symbols of a segment whose chunks need `need`: + what run-over and further members add
static uint64_t sym_room(uint64_t need) { return need + need / 4 + 64 * (4096 + 64 * SYM_RATIO); }

#define GI(call) do { if ((call) != hipSuccess) return no(#call); } while (0)
#define GB(call) do { if (!(call)) return no(#call); } while (0)

struct Gunzip {
    const uint8_t *const in;
    const uint64_t in_n;
    const int fd;
    RangeRun *const rr;
    const bool trace;
    const Tunables tn;
    // own stream: the two mates of a paired sample are inflated by two host threads, and the legacy default stream would
    // serialise them
    hipStream_t st = call_stream_get();                       // (null: checked once the slices are known -- a rank that fails here still serves the chain)
    const std::chrono::steady_clock::time_point t_begin = std::chrono::steady_clock::now();
    Why why;                                                  // why the call declines

    uint64_t data_off = 0, data_n = 0;                        // the first member's deflate data
    uint32_t n_chunks0 = 0;                                   // chunks of the search
    uint8_t *d_in = nullptr, *d_text = nullptr;
    uint64_t *d_entry = nullptr;
    uint32_t *d_crc = nullptr;
    CrcMember *d_tab = nullptr;
    uint32_t c_searched = 0;                                  // search chunks [0, c_searched) have been launched
    std::vector<Bgzf> bgzf;                                   // a bgzip file: its members ARE the chunks, no search

    std::vector<Chunk> G;
    std::vector<Seg> segs;
    uint32_t n_sub = 0;                                       // entries inside blocks

    Arena *A = nullptr;
    std::future<Arena *> ahead;                               // (a large file: the arena allocated while the image travels)
    uint64_t cap_chunks = 0, text_cap = 0;
    uint64_t *d_start = nullptr, *d_stop = nullptr, *d_off = nullptr, *d_cap = nullptr, *d_len = nullptr, *d_end = nullptr, *d_toff = nullptr, *d_hdr = nullptr;

    std::vector<Member> members;
    uint64_t total = 0, last_end_bit = 0;                     // the text so far
    bool have_prev = false, ended = false;
    uint32_t n_segments = 0;

    Gunzip(const uint8_t *in_, uint64_t in_n_, int fd_, RangeRun *rr_) : in(in_), in_n(in_n_), fd(fd_), rr(rr_), trace(tracing()) {}
    static bool tracing() { static const bool t = getenv("SS_INGEST_TRACE") != nullptr; return t; }

    double since() const { return std::chrono::duration<double>(std::chrono::steady_clock::now() - t_begin).count(); }
    void lap(const char *what)
    {
        if (!trace) return;
        hipStreamSynchronize(st);
        fprintf(stderr, "[ginflate] %-18s at %.4f s\n", what, since());
    }
    bool h2d(void *dst, const void *src, uint64_t bytes) { return hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, st) == hipSuccess; }
    bool d2h(void *dst, const void *src, uint64_t bytes)
    {
        return hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, st) == hipSuccess && hipStreamSynchronize(st) == hipSuccess;
    }

    // ---- the two ways out ------------------------------------------------------------------------------------------------------
    // A stage that cannot go on says why and returns false; nothing else happens there.
    bool no(const char *what, long long arg = 0) { why = Why{what, arg}; return false; }
    void cleanup(bool keep_text)
    {
        if (ahead.valid()) arena_put(ahead.get());            // (a call that leaves before it took the arena over)
        const double c0 = since();
        void *scratch[] = {d_in, d_entry, d_crc, d_tab};
        for (int q = 0; q < 4; q++) {
            if (!scratch[q]) continue;
            if (keep_text && A) A->late_free[q] = scratch[q];      // (freed by gpu_gunzip_done)
            else hipFreeAsync(scratch[q], st);
        }
        const double c1 = since();
        hipStreamSynchronize(st);
        const double c2 = since();
        call_stream_put(st);
        if (trace) fprintf(stderr, "[ginflate] cleanup: free %.4f, sync %.4f, stream back %.4f s\n", c1 - c0, c2 - c1, since() - c2);
        if (!keep_text) { arena_put(A); A = nullptr; }            // (else the caller holds it, with the text, until gpu_gunzip_done)
    }
    // EVERY call that declines leaves through here: a rank that leaves must still serve the chain
    bool declined()
    {
        if (trace) fprintf(stderr, "[ginflate] not handled: %s (%lld)\n", why.what ? why.what : "?", why.arg);
        if (rr) rr->abort_chain();                            // (the other ranks' chain goes on through this one)
        g_declined++;
        cleanup(false);
        return false;
    }
    void hand_out(char **text_dev, uint64_t *len, void **lease)
    {
        cleanup(true);
        g_handled++;
        if (rr) { g_range_files++; g_range_pieces += rr->pieces->size(); }
        *text_dev = (char *)d_text;
        *len = total;
        *lease = A;
    }

    // ---- the header, the search chunks and -- range mode -- the slices -----------------------------------------------------------
    bool plan()
    {
        // (a rank that only serves the chain may hold no more than the first 70 KB of the file: ss_fastq_dev.hip)
        data_off = gzip_header_len(in, rr && rr->inject_decline ? std::min<uint64_t>(in_n, 70u << 10) : in_n);
        if (!data_off) return no("header");
        data_n = in_n - 8 - data_off;
        const uint64_t n_chunks0_ = std::max<uint64_t>(1, (data_n + tn.chunk_bytes - 1) / tn.chunk_bytes);
        if (n_chunks0_ > 0x7FFFFFF0ull) return no("size");
        n_chunks0 = (uint32_t)n_chunks0_;
        if (rr) {
            // the slices, before anything can fail: every rank derives the same ones from the file's size
            const uint64_t slice_bytes = tn.slice_bytes ? tn.slice_bytes : rr->slice_bytes ? rr->slice_bytes
                                         : std::min<uint64_t>(128ull << 20, std::max<uint64_t>(4ull << 20, data_n / (2ull * rr->world)));
            rr->slice_chunks = (uint32_t)std::max<uint64_t>(2 * LOOK, slice_bytes / tn.chunk_bytes);
            rr->n_slices = (n_chunks0 + rr->slice_chunks - 1) / rr->slice_chunks;
            rr->slice_chunks = (n_chunks0 + rr->n_slices - 1) / rr->n_slices;      // equal slices (no sliver at the end)
            rr->n_slices = (n_chunks0 + rr->slice_chunks - 1) / rr->slice_chunks;
            for (uint32_t sl = rr->rank; sl < rr->n_slices; sl += rr->world) rr->mine.push_back(sl);
            if (rr->n_slices < 2) return no("one slice");         // nothing to share out: the whole-file path
            if (rr->inject_decline) return no("declined on request (test hook, or the file could not be mapped)");
            if (trace) fprintf(stderr, "[ginflate] range mode: rank %u of %u, %u slices of %u chunks, %zu mine\n", rr->rank, rr->world, rr->n_slices,
                               rr->slice_chunks, rr->mine.size());
        }
        return st ? true : no("hipStreamCreateWithFlags");
    }
    uint64_t text_guess() const
    {
        const uint8_t *t8 = in + in_n - 8;
        uint64_t guess = (uint64_t)t8[4] | (uint64_t)t8[5] << 8 | (uint64_t)t8[6] << 16 | (uint64_t)t8[7] << 24;      // ISIZE of the last member
        while (guess < in_n) guess += 1ull << 32;
        return (guess <= 16 * in_n ? guess : 3 * in_n) + 64;
    }

    // ---- a LARGE file: its scratch arena and text buffer are allocated on a thread of their own WHILE the image travels --
    // sized by what a segment can need at most (SEG_CHUNKS chunks, seg_bytes of data) instead of what this file's largest one
    // does, which is known only after the search.  A fresh process is handed new device memory at ~25 GB/s: for a 3.4 GB file
    // (4 GB of symbols + 7.7 GB of text) that was 0.14-0.38 s of waiting between the search and the first segment.
    void scratch_ahead()
    {
        if (fd < 0 || rr || in_n < (256ull << 20)) return;
        int device = 0;
        hipGetDevice(&device);
        const uint64_t ub_chunks = SEG_CHUNKS + 80, stage = in_n;
        const uint64_t ub_sym = sym_room((tn.seg_bytes + tn.chunk_bytes + SEG_CHUNKS) * SYM_RATIO + SEG_CHUNKS * 4096), ub_text = text_guess();
        ahead = std::async(std::launch::async, [=]() -> Arena * {
            Why w;                                            // (null: decided in take_scratch, with the real sizes)
            return hipSetDevice(device) == hipSuccess ? acquire_scratch(nullptr, ub_chunks, ub_sym, ub_text, stage, &w) : nullptr;
        });
    }

    // ---- the image on the device, and the search for block starts in it -------------------------------------------------------------
    void search_to(uint32_t c_hi)
    {
        // (the search in pieces, each started on the prefix of the image that had arrived.  Measured (26 loads of each setting
        // interleaved in one process, a pair of 66 MB files): 1 piece -- upload, then search -- 26.0 ms, 2 pieces 26.3, 4 pieces
        // 27.0, 8 pieces 28.4: the search is bound by the chip's throughput (4.5 ms for the pair), a piece takes as long as its
        // slowest chunk, and the pieces of a stream run one after another.  So: one piece, when all of it is there.)
        if (c_hi > c_searched)
            hipLaunchKernelGGL(sync_kernel, dim3(c_hi - c_searched), dim3(64), 0, st, d_in, in_n - 8, data_off, tn.chunk_bytes, n_chunks0, d_entry, (uint64_t)512,
                               trace ? 1 : 0, rr ? rr->slice_chunks : 0u, rr ? rr->rank : 0u, rr ? rr->world : 1u, LOOK, c_searched);
        c_searched = std::max(c_searched, c_hi);
    }
    bool stage_image()
    {
        GI(hipMallocAsync((void **)&d_in, in_n + 8192, st));                 // the stage is filled 1 KB at a time, up to 2 KB ahead
        bool uploaded = false;
        // (pinned buffers cost ~40 ms to make: a file of less than 256 MB takes that way only when a set is there already --
        //  ss_gz_warm_up, or an earlier call -- and then arrives in 8 ms instead of 12-30)
        const uint64_t pread_from = pin_waiting() ? 32ull << 20 : 256ull << 20;
        const uint64_t margin = 64 << 10;
        if (fd >= 0 && in_n >= pread_from && !rr) {               // (`fd`: the same file; smaller ones are there before the buffers are)
            GI(hipMemsetAsync(d_in + in_n, 0, 8192, st));
            GI(hipMallocAsync((void **)&d_entry, (uint64_t)n_chunks0 * 8, st));
            GI(hipStreamSynchronize(st));                         // the allocations are stream-ordered
            lap("stage allocated");
            // the sync search runs on the prefix of the image that has arrived (a candidate's probe reads a few KB beyond its chunk)
            uploaded = upload_file(fd, in_n, d_in, [&](uint64_t ready) {
                // (runs on an upload thread, which has set the device; calls are serialised by upload_file)
                if (!bgzf.empty()) return;
                const uint64_t usable = ready >= in_n ? in_n : (ready > margin + data_off ? ready - margin - data_off : 0);
                const uint32_t c_hi = ready >= in_n ? n_chunks0 : (uint32_t)std::min<uint64_t>(n_chunks0, usable / tn.chunk_bytes);
                if (c_hi == n_chunks0 || c_hi >= c_searched + n_chunks0) {
                    if (trace) fprintf(stderr, "[ginflate] search to chunk %u of %u at %.4f s\n", c_hi, n_chunks0, since());
                    search_to(c_hi);
                }
            });
            if (!uploaded) c_searched = 0;                         // (the image is copied again below: search everything)
        }
        if (!uploaded && rr) {
            // range mode: only this rank's slices travel (+ the search chunks behind each in which its last chunk stops, + the
            // header and the trailer); the rest of the image is never read
            auto part = [&](uint64_t lo, uint64_t hi) { hi = std::min(hi, in_n); return lo >= hi || h2d(d_in + lo, in + lo, hi - lo); };
            GB(part(0, data_off + margin));
            GB(part(in_n > margin ? in_n - margin : 0, in_n));
            for (uint32_t sl : rr->mine) {
                const uint64_t lo = data_off + (uint64_t)sl * rr->slice_chunks * tn.chunk_bytes, hi = lo + ((uint64_t)rr->slice_chunks + LOOK + 8) * tn.chunk_bytes;
                GB(part(lo > margin ? lo - margin : 0, hi + margin));
            }
            uploaded = true;
        }
        if (!uploaded) GB(h2d(d_in, in, in_n));
        GI(hipMemsetAsync(d_in + in_n, 0, 8192, st));
        if (!d_entry) GI(hipMallocAsync((void **)&d_entry, (uint64_t)n_chunks0 * 8, st));
        lap("input on device");
        return true;
    }
    // entry[c]: the bit of the first block start in search chunk c, or ~0
    bool search(std::vector<uint64_t> &entry)
    {
        entry.assign(n_chunks0, 0);
        if (bgzf.empty()) {
            search_to(n_chunks0);
            GB(d2h(entry.data(), d_entry, (uint64_t)n_chunks0 * 8));
        }
        if (trace && bgzf.empty()) {
            unsigned tries = 0;
            hipMemcpyFromSymbol(&tries, HIP_SYMBOL(g_sync_tries), 4);
            fprintf(stderr, "[ginflate] %u chunks, %u candidate blocks decoded\n", n_chunks0, tries);
            tries = 0;
            hipMemcpyToSymbol(HIP_SYMBOL(g_sync_tries), &tries, 4);
        }
        lap("sync");
        if (g_hook_entry.load() > 0) {                           // test hook (ss_test_hook): a wrong entry (a position inside a block) in chunk <n>
            const uint64_t c = (uint64_t)g_hook_entry.load();
            if (c > 0 && c < n_chunks0) entry[c] = (data_off + c * tn.chunk_bytes) * 8 + 12345 % (tn.chunk_bytes * 8);
        }
        return true;
    }

    // ---- the chunk list G (range mode: and this rank's segments), from the search's entries or the members of a bgzip file: host only
    bool chunk_list(const std::vector<uint64_t> &entry)
    {
        if (rr && !bgzf.empty()) {
            // bgzip in range mode: a slice's chunks are the members whose deflate data begins in its byte range -- complete in
            // themselves (no search, no look-ahead, nothing unknown in front of any); the chain still carries the newline count,
            // the record that straddles the cut and the position the slice must begin at (hdr_bit: where its first member's header starts)
            size_t mi = 0;
            for (uint32_t sl : rr->mine) {
                const uint64_t lo = sl == 0 ? 0 : data_off + (uint64_t)sl * rr->slice_chunks * tn.chunk_bytes;
                const uint64_t hi = sl + 1 == rr->n_slices ? ~0ull : data_off + (uint64_t)(sl + 1) * rr->slice_chunks * tn.chunk_bytes;
                while (mi < bgzf.size() && bgzf[mi].data < lo) mi++;
                Seg sg{G.size(), 0, 0, sl, mi ? (bgzf[mi - 1].trailer + 8) * 8 : 0};
                for (; mi < bgzf.size() && bgzf[mi].data < hi; mi++) G.push_back(Chunk{bgzf[mi].data * 8, true, true, bgzf[mi].trailer});
                sg.gj = G.size();
                if (sg.gj == sg.gi) return no("slice without a member", sl);
                segs.push_back(sg);
            }
            if (trace) fprintf(stderr, "[ginflate] bgzip: %zu members, %zu in this rank's slices\n", bgzf.size(), G.size());
        } else if (rr) {
            for (uint32_t sl : rr->mine) {
                const uint32_t c_lo = sl * rr->slice_chunks, c_hi = std::min<uint32_t>(n_chunks0, c_lo + rr->slice_chunks);
                Seg sg{G.size(), 0, 0, sl, 0};
                for (uint32_t c = c_lo; c < c_hi; c++)
                    if (entry[c] != ~0ull) G.push_back(Chunk{entry[c], c == 0, false, 0});
                sg.gj = G.size();
                if (sg.gj == sg.gi) return no("slice without a block start", sl);
                if (sl + 1 < rr->n_slices) {
                    for (uint32_t c = c_hi; c < std::min<uint32_t>(n_chunks0, c_hi + LOOK) && sg.n_ph < 2; c++)
                        if (entry[c] != ~0ull) { G.push_back(Chunk{entry[c], false, false, 0}); sg.n_ph++; }
                    if (!sg.n_ph) return no("no block start behind the slice", sl);
                } else {
                    G[sg.gj - 1].last = true;
                    G[sg.gj - 1].trailer = in_n - 8;
                }
                segs.push_back(sg);
            }
        } else if (bgzf.empty()) {
            for (uint32_t c = 0; c < n_chunks0; c++)
                if (entry[c] != ~0ull) G.push_back(Chunk{entry[c], c == 0, false, 0});
            G.back().last = true;
            G.back().trailer = in_n - 8;
        } else {
            for (const Bgzf &m : bgzf) G.push_back(Chunk{m.data * 8, true, true, m.trailer});
            if (trace) fprintf(stderr, "[ginflate] bgzip: %zu members\n", bgzf.size());
        }
        return true;
    }

    // ---- entries inside the blocks: a block [its start, the next entry) of more than 2 x split_bytes is entered at
    //      equidistant places as well (at most eight pieces; range mode: the look-ahead entries stay whole)
    bool enter_blocks()
    {
        if (!tn.split_bytes || !bgzf.empty() || G.empty()) return true;
        std::vector<uint64_t> b_hdr, s_from, s_lim;
        std::vector<uint32_t> b_first, s_of;                   // positions of a block: [b_first[b], b_first[b + 1]); s_of: which chunk of G
        auto want = [&](size_t i, uint64_t endb) {
            const uint64_t len = endb - G[i].start, pieces = std::min<uint64_t>(8, len / (tn.split_bytes * 8));
            if (pieces < 2) return;
            b_hdr.push_back(G[i].start);
            b_first.push_back((uint32_t)s_of.size());
            for (uint64_t j = 1; j < pieces; j++) { s_from.push_back(G[i].start + len * j / pieces); s_lim.push_back(endb); s_of.push_back((uint32_t)i); }
        };
        if (rr) {
            for (const Seg &sg : segs)
                for (size_t i = sg.gi; i < sg.gj; i++) {
                    if (i + 1 < sg.gj + sg.n_ph) want(i, G[i + 1].start);
                    else if (G[i].last) want(i, G[i].trailer * 8);
                }
        } else {
            for (size_t i = 0; i < G.size(); i++) want(i, i + 1 < G.size() ? G[i + 1].start : (in_n - 8) * 8);
        }
        const size_t ns = s_of.size(), nb = b_hdr.size();
        b_first.push_back((uint32_t)ns);
        if (ns) {
            uint64_t *d_sub = nullptr;                         // block headers | from | limit | entries | first (u32)
            GI(hipMallocAsync((void **)&d_sub, nb * 8 + ns * 8 * 3 + (nb + 1) * 4, st));
            uint64_t *d_bh = d_sub, *d_from = d_sub + nb, *d_lim = d_from + ns, *d_ent = d_lim + ns;
            uint32_t *d_first = reinterpret_cast<uint32_t *>(d_ent + ns);
            std::vector<uint64_t> got(ns);
            const bool ok = h2d(d_bh, b_hdr.data(), nb * 8) && h2d(d_from, s_from.data(), ns * 8) && h2d(d_lim, s_lim.data(), ns * 8) &&
                            h2d(d_first, b_first.data(), (nb + 1) * 4);
            if (ok) hipLaunchKernelGGL(subsync_kernel, dim3((unsigned)nb), dim3(64), 0, st, d_in, in_n - 8, d_bh, d_first, d_from, d_lim, (uint32_t)nb, d_ent);
            const bool ok2 = ok && d2h(got.data(), d_ent, ns * 8);
            hipFreeAsync(d_sub, st);
            if (!ok2) return no("sub-entries");
            std::vector<Chunk> G2;
            std::vector<size_t> at(G.size() + 1);
            size_t k = 0;
            for (size_t i = 0; i < G.size(); i++) {
                at[i] = G2.size();
                G2.push_back(G[i]);
                uint64_t prev = G[i].start;
                for (; k < ns && s_of[k] == i; k++) {
                    if (got[k] == ~0ull || got[k] <= prev || got[k] + 256 >= s_lim[k]) continue;      // (none found, or two searches met in one place)
                    Chunk sub{got[k], false, G[i].last, G[i].trailer, G[i].start};
                    G2.back().last = false;                    // the member's final block ends the LAST piece
                    G2.back().trailer = 0;
                    G2.push_back(sub);
                    prev = got[k];
                    n_sub++;
                }
            }
            at[G.size()] = G2.size();
            for (Seg &sg : segs) { sg.gi = at[sg.gi]; sg.gj = at[sg.gj]; }
            G.swap(G2);
        }
        if (trace) fprintf(stderr, "[ginflate] %zu entries inside blocks wanted, %u found: %zu chunks\n", ns, n_sub, G.size());
        lap("sub-entries");
        return true;
    }
    // What a wave decodes alone is the stretch from its entry to the next.  Entries are dynamic blocks' starts (and places inside
    // them): zlib, pigz and libdeflate begin one every 16-300 KB, but a stream of stored or fixed-Huffman blocks only (level 0,
    // Z_FIXED, some hardware compressors) has none, and ONE wave would then decode the whole file -- minutes of a kernel that looks
    // like a hang.  Such a file goes to the host inflaters, which read it at memory speed.
    bool no_lonely_stretch()
    {
        if (rr || !bgzf.empty()) return true;
        constexpr uint64_t LONELY_BYTES = 8ull << 20;
        uint64_t longest = 0;
        for (size_t i = 0; i < G.size(); i++)
            longest = std::max(longest, ((i + 1 < G.size() ? G[i + 1].start : (in_n - 8) * 8) - G[i].start) / 8);
        return longest <= LONELY_BYTES ? true : no("a stretch of deflate data without a dynamic block's start (MB)", (long long)(longest >> 20));
    }

    // ---- scratch.  The chunks are inflated SEGMENT by segment (seg_bytes of deflate data, 128 MB): the scratch stays a few GB
    // whatever the file's size, and the text of one segment is complete -- bytes -- before the next one starts, so the 32 KB in
    // front of a segment's first chunk are simply the end of the text so far.
    size_t segment_end(size_t gi) const
    {
        size_t gj = gi + 1;
        while (gj < G.size() && (G[gj].start - G[gi].start) / 8 < tn.seg_bytes && gj - gi < SEG_CHUNKS) gj++;
        return gj;
    }
    bool take_scratch()
    {
        uint64_t need_sym = 0, need_chunks = 0;                   // the largest segment decides the scratch
        for (size_t gi = 0, si = 0; gi < G.size(); si++) {
            const size_t gj = rr ? segs[si].gj : segment_end(gi);
            const bool more = rr ? segs[si].n_ph > 0 : gj < G.size();
            const uint64_t bytes = ((more ? G[gj].start : G[gj - 1].last ? G[gj - 1].trailer * 8 : (in_n - 8) * 8) - G[gi].start) / 8;
            need_sym = std::max<uint64_t>(need_sym, (bytes + (gj - gi)) * SYM_RATIO + (gj - gi) * 4096);
            need_chunks = std::max<uint64_t>(need_chunks, gj - gi);
            gi = rr ? (si + 1 < segs.size() ? segs[si + 1].gi : G.size()) : gj;
        }
        cap_chunks = need_chunks + 80;
        const uint64_t sym_elems = sym_room(need_sym);
        if (sym_elems * 2 > (24ull << 30)) return no("segment", (long long)(sym_elems >> 20));      // (GBs without a single block start)
        if (ahead.valid()) {
            A = ahead.get();
            if (A && (A->cap_chunks < cap_chunks || A->sym_elems < sym_elems)) { arena_put(A); A = nullptr; }      // (cannot happen: the bounds are bounds)
        }
        text_cap = text_guess();
        if (rr) text_cap = text_cap / rr->n_slices * rr->mine.size() * 13 / 10 + (1ull << 20);      // this rank's share (it grows when short)
        Why w;
        A = acquire_scratch(A, cap_chunks, sym_elems, text_cap, 0, &w);
        if (!A) return no(w.what, w.arg);
        text_cap = A->text_cap;
        d_text = A->text;
        lap("buffers");
        d_start = A->meta; d_stop = A->meta + cap_chunks; d_off = A->meta + 2ull * cap_chunks; d_cap = A->meta + 3ull * cap_chunks;
        d_len = A->meta + 4ull * cap_chunks; d_end = A->meta + 5ull * cap_chunks; d_toff = A->meta + 6ull * cap_chunks; d_hdr = A->meta + 7ull * cap_chunks;
        return true;
    }

    // ---- one segment: lay out, inflate, repair ------------------------------------------------------------------------------------------
    uint64_t bit_behind(const Segment &s, uint32_t c) const      // where chunk c's input ends at the latest
    {
        if (s.ch[c].last) return s.ch[c].trailer * 8;
        if (c + 1 < s.ch.size()) return s.ch[c + 1].start;
        if (!s.ph.empty()) return s.ph[0].start;
        return (in_n - 8) * 8;
    }
    // every chunk a symbol region of its own, by the length of its input, and nothing in it yet.  false: more than the arena has
    bool lay_out(Segment &s) const
    {
        uint64_t sym_total = 0;
        for (uint32_t c = 0; c < s.ch.size(); c++) {
            Rec &r = s.ch[c];
            r.off = sym_total;
            r.cap = ((bit_behind(s, c) - r.start) / 8 + 1) * SYM_RATIO + 4096;
            r.len = r.end = 0;
            r.status = 0;
            sym_total += r.cap;
        }
        return sym_total <= A->sym_elems;
    }
    // the device arrays of the segment's chunks and look-ahead entries, from the records (`todo` not empty: only those are
    // inflated, what the other chunks produced stays as it is)
    bool chunks_to_device(const Segment &s, const std::vector<uint32_t> &todo, Staging &h)
    {
        const uint32_t nc = (uint32_t)s.ch.size();
        for (uint32_t c = 0; c < nc; c++) {
            const Rec &r = s.ch[c];
            h.start.push_back(r.start | (r.fresh ? 1ull << 63 : 0ull));
            h.stop.push_back(r.last ? ~0ull : bit_behind(s, c));
            h.off.push_back(r.off); h.cap.push_back(r.cap); h.hdr.push_back(r.hdr);
            h.len.push_back(r.len); h.end.push_back(r.end); h.status.push_back(r.status);
        }
        for (size_t k = 0; k < s.ph.size(); k++) {              // look-ahead: only their stops are read
            h.start.push_back(s.ph[k].start);
            h.hdr.push_back(s.ph[k].hdr);
            // (range mode: what follows the look-ahead entries in G is another slice: a chunk that runs over both of them is
            //  stopped a few search chunks further on and declined)
            h.stop.push_back(s.ph[k].last ? ~0ull : (k + 1 < s.ph.size() ? s.ph[k + 1].start
                                                      : rr ? s.ph[k].start + 4 * tn.chunk_bytes * 8 : (s.gj + k + 1 < G.size() ? G[s.gj + k + 1].start : ~0ull)));
            h.off.push_back(0);
            h.cap.push_back(0);
        }
        const uint64_t n_all = nc + s.ph.size();
        GB(h2d(d_start, h.start.data(), n_all * 8));
        GB(h2d(d_stop, h.stop.data(), n_all * 8));
        GB(h2d(d_off, h.off.data(), n_all * 8));
        GB(h2d(d_cap, h.cap.data(), n_all * 8));
        GB(h2d(d_hdr, h.hdr.data(), n_all * 8));
        if (!todo.empty()) {
            GB(h2d(A->status, h.status.data(), (uint64_t)nc * 4));
            GB(h2d(d_len, h.len.data(), (uint64_t)nc * 8));
            GB(h2d(d_end, h.end.data(), (uint64_t)nc * 8));
            GB(h2d(A->todo, todo.data(), todo.size() * 4));
        }
        return true;
    }
    // Two things show only when the chunks have been inflated:
    //  * An entry is a position where a valid dynamic header parses and 512 symbols decode -- a position INSIDE a
    //    block passes that about once in a million candidates (every bit string decodes under a complete code).  The
    //    chunk in front of it ends a block BEHIND it and goes on to the entry after it (inflate_kernel); the wrong
    //    entry's chunk is dropped.  (No room left in its symbol region, or more than two in a row: -21, the two
    //    chunks are merged here and inflated again.)
    //  * A file of several members (lanes joined with `cat a.gz b.gz`): the chunk that meets a final block before its
    //    stop (-20) ends a member if a trailer and a gzip header follow; the next member's first block becomes a chunk
    //    and the segment is inflated again.
    // -> s.ch: the new list of records, with what the unchanged chunks produced; `again`: positions in it that must be inflated
    // (again; none, and nothing else new: *settled); `relayout`: new chunks need room of their own, lay everything out anew
    bool repair(Segment &s, std::vector<uint32_t> &again, bool &relayout, bool *settled)
    {
        std::vector<Rec> &ch = s.ch;
        const uint32_t nc = (uint32_t)ch.size(), n_all = nc + (uint32_t)s.ph.size();
        std::vector<Rec> nxt;
        std::vector<char> drop(nc, 0);
        uint32_t n_drop = 0, n_members = 0, n_over = 0, over_ph = 0;
        auto keep = [&](const Rec &r, bool last, uint64_t trailer) { nxt.push_back(r); nxt.back().last = last; nxt.back().trailer = trailer; };
        // an entry inside a block whose chunk means nothing is no entry: the chunk in front (the last of nxt) takes its bytes
        // and is inflated again
        auto give_to_the_one_in_front = [&](const Rec &r) {
            Rec &pv = nxt.back();
            pv.last = r.last;
            pv.trailer = r.trailer;
            if (r.off == pv.off + pv.cap) pv.cap += r.cap;      // their symbol regions are neighbours
            else relayout = true;
            if (again.empty() || again.back() != (uint32_t)nxt.size() - 1) again.push_back((uint32_t)nxt.size() - 1);
            n_drop++;
        };
        for (uint32_t c = 0; c < nc; c++) {
            if (drop[c]) continue;                                     // its own outcome means nothing
            const uint64_t e = (ch[c].end + 7) / 8;
            if (ch[c].status >= 0) {
                // done; `over` entries behind it were positions inside its blocks: their chunks go, nothing is inflated again
                const uint32_t over = (uint32_t)ch[c].status >> 4;
                const int stc = ch[c].status & 15;
                if (c + over < n_all) {
                    const Chunk &eff = c + over < nc ? ch[c + over] : s.ph[c + over - nc];
                    if (stc == (eff.last ? 1 : 0) && (!eff.last || e == eff.trailer)) {
                        keep(ch[c], eff.last, eff.trailer);
                        nxt.back().status = stc;
                        for (uint32_t k = 1; k <= over; k++) {
                            if (c + k < nc) drop[c + k] = 1;
                            else over_ph = std::max(over_ph, c + k - nc + 1);
                        }
                        n_over += over;
                        continue;
                    }
                }
                ch[c].status = stc == 1 ? 1 : -21;                     // (falls through: a member's end, or not explainable)
            }
            if (ch[c].status == -21 && c + 1 < nc) {                   // ran past the next entry: the two chunks become one
                // (... and with them the entries inside blocks that follow: found with the tables of a block they are not in --
                //  a chunk of the search that held two block starts --, what they decoded means nothing)
                uint32_t k = c + 1;
                while (k + 1 < nc && ch[k + 1].hdr != ~0ull) k++;
                keep(ch[c], ch[k].last, ch[k].trailer);
                for (uint32_t d = c + 1; d <= k; d++) {
                    drop[d] = 1;
                    n_drop++;
                    if (ch[d].off == ch[c].off + nxt.back().cap) nxt.back().cap += ch[d].cap;      // their symbol regions are neighbours
                    else relayout = true;
                }
                again.push_back((uint32_t)nxt.size() - 1);
                continue;
            }
            if (ch[c].status == -20 || ch[c].status == 1) {      // a final block before the next entry / before the file's end (its own, or run over to it)
                const uint64_t hdr = e + 8 + 18 <= in_n ? gzip_header_len(in + e + 8, in_n - (e + 8)) : 0;
                if (!hdr && ch[c].hdr != ~0ull && !nxt.empty()) { give_to_the_one_in_front(ch[c]); continue; }      // (an entry inside a block that decoded garbage)
                if (!hdr) return no("chunk status", ch[c].status * 1000000ll + c);
                keep(ch[c], true, e);
                const uint64_t d = (e + 8 + hdr) * 8;                  // the next member's first block
                bool was_last = ch[c].last;                            // (the new chunk ends the file if what it replaces did)
                uint64_t was_trailer = ch[c].trailer;
                // "entries" within the block, trailer and header -- and entries that claim to lie inside a block of the member that ends here
                for (uint32_t k = c + 1; k < nc && (ch[k].start < d || (ch[k].hdr != ~0ull && ch[k].hdr < d)); k++) {
                    drop[k] = 1;
                    n_drop++;
                    if (ch[k].last) { was_last = true; was_trailer = ch[k].trailer; }
                }
                if (c + 1 >= nc || drop[nc - 1])                       // (the look-ahead entries too)
                    for (size_t k = 0; k < s.ph.size() && s.ph[k].start < d; k++) over_ph = std::max<uint32_t>(over_ph, (uint32_t)k + 1);
                nxt.push_back(Rec{Chunk{d, true, was_last, was_trailer}});
                n_members++;
                relayout = true;
                continue;
            }
            // (the chunk in front did not arrive at this entry: what it decoded means nothing)
            if (ch[c].hdr != ~0ull && !nxt.empty()) { give_to_the_one_in_front(ch[c]); continue; }
            return no("chunk status", ch[c].status * 1000000ll + c);
        }
        if (over_ph) {                                             // look-ahead entries that were run over are no chunks any more
            over_ph = (uint32_t)std::min<size_t>(over_ph, s.ph.size());
            s.consumed_ph += over_ph;
            s.ph.erase(s.ph.begin(), s.ph.begin() + over_ph);
        }
        if (trace && n_over) fprintf(stderr, "[ginflate] %u entries were inside a block: run over\n", n_over);
        ch.swap(nxt);                                              // (nothing dropped or run over: the same list)
        *settled = !n_drop && !n_members;
        if (trace && !*settled)
            fprintf(stderr, "[ginflate] %u entries were inside a block, %u further members found: %s inflated again\n", n_drop, n_members,
                    relayout ? "the segment" : "their chunks");
        return true;
    }
    // the chunks G[s.gi, s.gj) to symbols, s.gj chosen here
    bool inflate_segment(Segment &s, size_t seg_i)
    {
        s.gj = rr ? segs[seg_i].gj : segment_end(s.gi);
        const size_t ph_end = rr ? s.gj + segs[seg_i].n_ph : std::min(G.size(), s.gj + 2);
        for (size_t i = s.gi; i < s.gj; i++) s.ch.push_back(Rec{G[i]});
        s.ph.assign(G.begin() + (long)s.gj, G.begin() + (long)ph_end);
        if (!lay_out(s)) return no("segment", (long long)s.gi);
        const uint32_t max_over = !tn.run_over ? 0u : n_sub ? 4u : 2u;
        std::vector<uint32_t> todo;                                // empty = all chunks
        for (int attempt = 0;; attempt++) {
            const uint32_t nc = (uint32_t)s.ch.size(), n_all = nc + (uint32_t)s.ph.size();
            Staging h;
            if (!chunks_to_device(s, todo, h)) return false;
            const uint32_t n_run = todo.empty() ? nc : (uint32_t)todo.size();
            hipLaunchKernelGGL(inflate_kernel, dim3(n_run), dim3(64), 0, st, d_in, in_n - 8, d_start, d_stop, d_hdr, n_all, A->sym, d_off, d_cap, d_len, d_end, A->status,
                               todo.empty() ? (const uint32_t *)nullptr : A->todo, max_over);
            GB(d2h(h.status.data(), A->status, (uint64_t)nc * 4));
            GB(d2h(h.len.data(), d_len, (uint64_t)nc * 8));
            GB(d2h(h.end.data(), d_end, (uint64_t)nc * 8));
            for (uint32_t c = 0; c < nc; c++) { s.ch[c].status = h.status[c]; s.ch[c].len = h.len[c]; s.ch[c].end = h.end[c]; }
            std::vector<uint32_t> again;
            bool relayout = false, settled = false;
            if (!repair(s, again, relayout, &settled)) return false;
            if (settled) return true;
            if (attempt >= 6 || s.ch.size() + s.ph.size() > cap_chunks - 4) return no("chunk list", (long long)s.ch.size());
            if (relayout) {
                if (!lay_out(s)) return no("symbol budget");
                todo.clear();
            } else {
                todo.swap(again);                                  // (the symbol regions stay where they are)
            }
        }
    }

    // ---- symbols to text -------------------------------------------------------------------------------------------------------------
    bool segment_text(Segment &s)
    {
        const uint32_t nc = (uint32_t)s.ch.size();
        s.m_first = members.empty() ? 0 : members.size() - ((rr && !s.ch[0].fresh) ? 1 : 0);
        s.text_off.assign(nc, 0);
        std::vector<uint64_t> off(nc), len(nc);
        for (uint32_t c = 0; c < nc; c++) {
            const Rec &r = s.ch[c];
            if (r.fresh) members.push_back(Member{total, 0, 0, 0, true, (uint32_t)crc32(0L, Z_NULL, 0), 0});
            if (members.empty() || !members.back().open) return no("member start");
            s.text_off[c] = total;
            off[c] = r.off;
            len[c] = r.len;
            total += r.len;
            members.back().len += r.len;
            if (r.last) {
                const uint8_t *t8 = in + r.trailer;
                Member &m = members.back();
                m.crc = (uint32_t)t8[0] | (uint32_t)t8[1] << 8 | (uint32_t)t8[2] << 16 | (uint32_t)t8[3] << 24;
                m.isize = (uint32_t)t8[4] | (uint32_t)t8[5] << 8 | (uint32_t)t8[6] << 16 | (uint32_t)t8[7] << 24;
                m.open = false;
                if ((uint32_t)(m.len + m.len0) != m.isize) return no("isize", (long long)members.size());      // (range mode: + its part in the slices before)
                ended = r.trailer == in_n - 8;
            }
        }
        last_end_bit = s.ch[nc - 1].end;
        if (total + 64 > text_cap) {                                   // (several members: the last ISIZE said little)
            const uint64_t ncap = std::max(total + 64, text_cap + text_cap / 2);
            uint8_t *nt = nullptr;
            GI(hipMalloc((void **)&nt, ncap));
            const bool ok = hipMemcpyAsync(nt, d_text, s.text_off[0], hipMemcpyDeviceToDevice, st) == hipSuccess && hipStreamSynchronize(st) == hipSuccess;
            hipFree(d_text);
            d_text = nt;
            text_cap = ncap;
            A->text = nt;
            A->text_cap = ncap;
            if (!ok) return no("text copy");
        }
        GB(h2d(d_off, off.data(), (uint64_t)nc * 8));
        GB(h2d(d_len, len.data(), (uint64_t)nc * 8));
        GB(h2d(d_toff, s.text_off.data(), (uint64_t)nc * 8));
        uint32_t group = 1;
        while ((uint64_t)group * group < nc) group++;               // ~sqrt: as many groups as chunks in a group
        group = std::max<uint32_t>(group, 8);
        const uint32_t n_groups = (nc + group - 1) / group;
        hipLaunchKernelGGL(tails_kernel, dim3(16, nc), dim3(256), 0, st, A->sym, d_off, d_len, nc, A->map[0]);
        hipLaunchKernelGGL(group_maps_kernel, dim3(n_groups), dim3(1024), 0, st, A->map[0], nc, group, A->map[1]);
        hipLaunchKernelGGL(group_windows_kernel, dim3(1), dim3(1024), 0, st, A->map[1], nc, group, n_groups,
                           have_prev ? (const uint8_t *)A->prev : (const uint8_t *)nullptr, A->gwin);
        hipLaunchKernelGGL(windows_kernel, dim3(16, nc), dim3(256), 0, st, A->map[1], nc, group, (const uint8_t *)A->gwin, A->win);
        hipLaunchKernelGGL(bytes_kernel, dim3(64, nc), dim3(256), 0, st, A->sym, d_off, d_len, d_toff, A->win, d_text);
        hipLaunchKernelGGL(lastwin_kernel, dim3(WSIZE / 256), dim3(256), 0, st, d_text, total, A->prev);
        GI(hipGetLastError());
        GI(hipStreamSynchronize(st));                          // (the host arrays of this segment go out of scope)
        have_prev = true;
        n_segments++;
        return true;
    }

    // ---- verification: CRC-32 of the text ranges (at, len), by segments of 4 KB from every range's first byte, combined on the host
    // with ONE precomputed operator.  (All members of a file at its end; range mode: every member's part in one slice -- a
    // bgzip slice holds thousands.)
    bool text_crcs(const std::vector<std::pair<uint64_t, uint64_t>> &items, std::vector<uint32_t> &out)
    {
        constexpr int SEG_LOG2 = 12;
        const uint64_t seg = 1ull << SEG_LOG2;
        std::vector<CrcMember> cm;
        uint64_t nseg = 0;
        for (const auto &it : items) {
            if (!it.second) continue;                              // (an empty range has no segment: its CRC is that of nothing)
            cm.push_back(CrcMember{it.first, it.second, nseg});
            nseg += (it.second + seg - 1) >> SEG_LOG2;
        }
        if (d_tab) { hipFreeAsync(d_tab, st); d_tab = nullptr; }      // (range mode: the slice before's)
        if (d_crc) { hipFreeAsync(d_crc, st); d_crc = nullptr; }
        GI(hipMallocAsync((void **)&d_tab, std::max<size_t>(16, cm.size() * sizeof(CrcMember)), st));      // (the member table)
        GI(hipMallocAsync((void **)&d_crc, std::max<uint64_t>(1, nseg) * 4, st));
        std::vector<uint32_t> crcs(std::max<uint64_t>(1, nseg));
        if (nseg) {
            GB(h2d(d_tab, cm.data(), cm.size() * sizeof(CrcMember)));
            hipLaunchKernelGGL(crc_members_kernel, dim3((unsigned)((nseg + 63) / 64)), dim3(64), 0, st, d_text, (const CrcMember *)d_tab, (uint32_t)cm.size(), nseg, SEG_LOG2,
                               d_crc);
            GB(d2h(crcs.data(), d_crc, nseg * 4));
        }
        uint32_t op[32];
        crc_zero_operator(op, SEG_LOG2);
        // the operator as four byte-indexed tables: one application = four lookups (there are 250 segments per MB)
        std::vector<uint32_t> opt(4 * 256);
        for (int byte = 0; byte < 4; byte++)
            for (uint32_t v = 0; v < 256; v++) opt[(size_t)byte * 256 + v] = gf2_times(op, v << (8 * byte));
        out.clear();
        uint64_t si = 0;
        for (const auto &it : items) {
            uint32_t crc = (uint32_t)crc32(0L, Z_NULL, 0);
            for (uint64_t a0 = 0; a0 < it.second; a0 += seg, si++) {
                const uint64_t l = std::min<uint64_t>(seg, it.second - a0);
                if (l == seg) crc = opt[crc & 0xFF] ^ opt[256 + ((crc >> 8) & 0xFF)] ^ opt[512 + ((crc >> 16) & 0xFF)] ^ opt[768 + (crc >> 24)] ^ crcs[si];
                else crc = (uint32_t)crc32_combine(crc, crcs[si], (z_off_t)l);
            }
            out.push_back(crc);
        }
        return true;
    }
    // the whole-file path: every member against its trailer
    bool verify_members()
    {
        std::vector<std::pair<uint64_t, uint64_t>> items;
        for (const Member &m : members) items.emplace_back(m.at, m.len);
        std::vector<uint32_t> crc;
        if (!text_crcs(items, crc)) return false;
        bool crc_ok = true;
        for (size_t mi = 0; mi < members.size(); mi++) crc_ok = crc_ok && crc[mi] == members[mi].crc;
        lap("crc");
        return crc_ok ? true : no("crc");
    }

    // ---- range mode: what lies in front of this slice comes down the chain now (the symbols are ready: the ranks did that
    //      part at the same time); the slice must begin exactly where the one before ended
    bool slice_receive(const Segment &s, const Seg &sg, ChainIn &before)
    {
        if (s.consumed_ph || s.ch.empty()) return no("range: entries dropped at the slice edge", sg.slice);
        if (sg.slice > 0) {
            if (!rr->recv_for(sg.slice)) return no("chain receive", sg.slice);
            if (rr->msg.status < 0) return no("chain: a rank before this one declined", sg.slice);
            if (rr->msg.end_bit != (!bgzf.empty() ? sg.hdr_bit : s.ch[0].start) || rr->msg.carry_len > CARRY_MAX)
                return no("range: the slice before ends elsewhere", sg.slice);
            GB(h2d(A->prev, rr->msg.window, WSIZE));
            have_prev = true;
            before.nl = rr->msg.nl; before.len = rr->msg.len; before.crc = rr->msg.crc;
            before.carry.assign(rr->msg.carry, rr->msg.carry + rr->msg.carry_len);
        } else {
            have_prev = false;
        }
        // the member that is open at the cut goes on in this slice (several members -- lanes joined with cat -- are followed
        // as in the whole-file path: a member that ends inside the slice is checked against its trailer here, the next one
        // starts with nothing in front of it; CRC-32 and length of the open member travel down the chain)
        if (!s.ch[0].fresh) members.push_back(Member{total, 0, 0, 0, true, before.crc, before.len});
        return true;
    }
    // ---- this slice's piece: CRC, newlines, the bytes behind its last complete record; then the chain goes on
    bool slice_piece(const Segment &s, const Seg &sg, const ChainIn &before)
    {
        const uint32_t my_slice = sg.slice;
        const uint64_t p_at = s.text_off[0], p_len = total - s.text_off[0];
        if (p_len < WSIZE && my_slice + 1 < rr->n_slices) return no("range: a slice with less text than a window", my_slice);      // (the window it hands on would reach into another piece)
        // CRC-32 of every member's part in this slice: a member that ended here against its trailer, the open one goes on
        uint32_t crc_now = (uint32_t)crc32(0L, Z_NULL, 0);
        uint64_t len_now = 0;
        std::vector<std::pair<uint64_t, uint64_t>> m_items;
        for (size_t mi = s.m_first; mi < members.size(); mi++) m_items.emplace_back(members[mi].at, members[mi].len);
        std::vector<uint32_t> m_crc;
        if (!text_crcs(m_items, m_crc)) return false;
        for (size_t mi = s.m_first; mi < members.size(); mi++) {
            const Member &m = members[mi];
            const uint32_t c = m.len ? (uint32_t)crc32_combine(m.crc0, m_crc[mi - s.m_first], (z_off_t)m.len) : m.crc0;
            if (!m.open) { if (c != m.crc) return no("crc (range mode)", (long long)mi); }
            else if (mi + 1 == members.size()) { crc_now = c; len_now = m.len0 + m.len; }
            else return no("member left open", (long long)mi);
        }
        unsigned long long p_nl = 0;
        GI(hipMemsetAsync(d_entry, 0, 8, st));                   // (the entries are on the host by now: a free device word)
        hipLaunchKernelGGL(count_nl_kernel, dim3(1024), dim3(256), 0, st, d_text + p_at, p_len, reinterpret_cast<unsigned long long *>(d_entry));
        GB(d2h(&p_nl, d_entry, 8));
        uint64_t keep = p_len;                                   // bytes of the piece up to the end of its last complete record
        if (my_slice + 1 < rr->n_slices) {
            // records end at newlines whose number in the file is a multiple of four: the last such newline of this piece is
            // among its last four; the tail of the piece is looked at on the host
            const uint64_t drop = (before.nl + p_nl) % 4;        // newlines behind the last complete record
            if (p_nl < drop + 1) return no("range: a slice without a complete record", my_slice);
            const uint64_t tail = std::min<uint64_t>(p_len, (uint64_t)CARRY_MAX + 1);
            std::vector<uint8_t> tb(tail);
            GB(d2h(tb.data(), d_text + p_at + (p_len - tail), tail));
            uint64_t seen = 0, q = tail;
            while (q > 0) {                                      // q - 1: the newline that ends the last complete record
                if (tb[q - 1] == '\n') { if (seen == drop) break; seen++; }
                q--;
            }
            if (q == 0) return no("range: a record longer than the chain carries", my_slice);
            keep = p_len - tail + q;
            rr->msg.status = 0;
            rr->msg.crc = crc_now;
            rr->msg.len = len_now;
            rr->msg.nl = before.nl + p_nl;
            rr->msg.end_bit = !bgzf.empty() ? (s.ch.back().trailer + 8) * 8 : s.ch.back().end;      // (bgzip: the next member's header)
            rr->msg.carry_len = (uint32_t)(p_len - keep);
            memcpy(rr->msg.carry, tb.data() + q, p_len - keep);
            GB(d2h(rr->msg.window, A->prev, WSIZE));
            if (!rr->send_from(my_slice)) return no("chain send", my_slice);
        } else if (members.empty() || members.back().open) {
            return no("the last member is not closed (range mode)");     // (every closed member was checked against its trailer above)
        }
        rr->pieces->push_back(GzPiece{p_at, p_len, keep, before.carry});
        rr->duty++;
        rr->received = false;
        return true;
    }

    // ---- the call, step by step.  false: `why` is set, and the caller leaves through declined()
    bool inflate_file()
    {
        if (!plan()) return false;
        scratch_ahead();
        bgzf = bgzf_members(in, in_n);
        {
            std::vector<uint64_t> entry;
            if (!stage_image() || !search(entry) || !chunk_list(entry)) return false;
        }
        if (!enter_blocks() || !no_lonely_stretch() || !take_scratch()) return false;
        size_t seg_i = 0;
        for (size_t gi = 0; gi < G.size(); seg_i++) {
            Segment s;
            s.gi = gi;
            if (!inflate_segment(s, seg_i)) return false;
            if (rr) {
                ChainIn before;
                if (!slice_receive(s, segs[seg_i], before) || !segment_text(s) || !slice_piece(s, segs[seg_i], before)) return false;
                gi = seg_i + 1 < segs.size() ? segs[seg_i + 1].gi : G.size();
            } else {
                if (!segment_text(s)) return false;
                gi = s.gj + s.consumed_ph;
            }
        }
        lap("inflate + windows + bytes");
        if (trace) fprintf(stderr, "[ginflate] %u segments, %zu members\n", n_segments, members.size());
        if (rr) {
            // (every piece was checked as it was made; the owner of the last slice has compared CRC-32 and length with the trailer
            //  and seen the stream end where the trailer begins)
            if (!rr->mine.empty() && rr->mine.back() + 1 == rr->n_slices && (!ended || (last_end_bit + 7) / 8 != in_n - 8))
                return no("stream end (range mode)", (long long)((last_end_bit + 7) / 8));
            return true;
        }
        // the stream must end where the last trailer begins (after padding to a byte)
        if (!ended || members.empty() || members.back().open || (last_end_bit + 7) / 8 != in_n - 8) return no("stream end", (long long)((last_end_bit + 7) / 8));
        return verify_members();
    }
};
#undef GI
#undef GB

}  // namespace

bool gpu_gunzip_impl(const uint8_t *in, uint64_t in_n, char **text_dev, uint64_t *len, void **lease, int fd, RangeRun *rr)
{
    Gunzip g(in, in_n, fd, rr);
    if (!g.inflate_file()) return g.declined();
    g.hand_out(text_dev, len, lease);
    return true;
}

}  // namespace ss

// members the device inflater has produced / has left to the host inflaters, in this process
extern "C" int ss_gz_gpu_counters(uint64_t *handled, uint64_t *declined)
{
    if (!handled || !declined) return SS_EINVAL;
    *handled = ss::g_handled.load();
    *declined = ss::g_declined.load();
    return SS_OK;
}

extern "C" int ss_gz_inflate_gpu(const char *path, char **text, uint64_t *len)
{
    if (!path || !text || !len) return SS_EINVAL;
    const int fd = open(path, O_RDONLY);
    if (fd < 0) return SS_EIO;
    struct stat st;
    if (fstat(fd, &st) != 0 || st.st_size < 20) { close(fd); return SS_EIO; }
    std::vector<uint8_t> buf((size_t)st.st_size);
    uint64_t got = 0;
    while (got < buf.size()) {
        const ssize_t r = pread(fd, buf.data() + got, buf.size() - got, (off_t)got);
        if (r <= 0) break;
        got += (uint64_t)r;
    }
    close(fd);
    if (got != buf.size()) return SS_EIO;
    char *d = nullptr;
    uint64_t n = 0;
    void *lease = nullptr;
    if (!ss::gpu_gunzip(buf.data(), buf.size(), &d, &n, &lease, -1)) return SS_ERANGE;
    char *h = (char *)malloc(std::max<uint64_t>(n, 1));
    if (!h) { ss::gpu_gunzip_done(lease); return SS_ENOMEM; }
    const hipError_t e = n ? hipMemcpy(h, d, n, hipMemcpyDeviceToHost) : hipSuccess;
    ss::gpu_gunzip_done(lease);
    if (e != hipSuccess) { free(h); return SS_EHIP; }
    *text = h;
    *len = n;
    return SS_OK;
}

extern "C" int ss_gz_range_counters(uint64_t *files, uint64_t *pieces)
{
    if (files) *files = ss::g_range_files.load();
    if (pieces) *pieces = ss::g_range_pieces.load();
    return SS_OK;
}
