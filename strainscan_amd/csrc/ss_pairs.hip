// ss_reads_join_pairs_dev / ss_reads_load_pairs: a resident set whose records are the read PAIRS of a sample (`--pairs`).
//
// A resident set keeps no pair map: ss_reads_load's parse threads place their blocks in the order they finish.  Every per-read
// kernel (ss_reads_support, ss_reads_select, ss_reads_resample, ss_reads_classify, ...) decides per record, from the record's
// bytes alone -- so a set whose records ARE the pairs makes all of them work on fragments, unchanged.  The joined record of line i
// of two flat blocks is
//       line1[i] + 'N' + line2[i] + '\n'
// 'N' ends a k-mer window: no k-mer spans the joint, every hit of either mate is a hit of the fragment and there is no other.
//
// A LINE is the bytes between two consecutive '\n' of a block (from the block's start for the first), empty lines included: an
// empty record in one file must not shift the pairing, so this is not the record numbering of record_spans_kernel
// (ss_select.hip), which skips them.  Three steps, on the calling thread's stream:
//   1. line_count_kernel: one wave per 1024-byte tile, 16 bytes per lane, the tile's '\n' counted; hipcub's exclusive sum over the
//      tiles (64-bit) gives every tile's first line and, behind the last tile, the block's lines.
//   2. line_ends_kernel: the same walk writes line_end[i] = the position of the i-th '\n'.  Line i begins at line_end[i - 1] + 1.
//   3. join_kernel.  No scan is needed for the output offsets: with start1[i] bytes of block 1 and start2[i] bytes of block 2 in
//      front of pair i, and the 'N' taking the place of mate 1's '\n', the joined record i begins at start1[i] + start2[i] and
//      the output holds exactly n1 + n2 bytes.  Sixteen lanes per fragment write it in 16-byte aligned pieces of the destination
//      (the piece copy, ss_piece_copy.h): per piece a masked fetch from either block; mate 1 brings its '\n' along, which the 'N'
//      then replaces, mate 2 brings the closing '\n'.  A block below 16 bytes is joined from a private copy padded to 16.
// All byte offsets are 64-bit.
//
// ss_reads_load_pairs brings each file to the device as ONE flat block in file order -- the text in memory (ss_input_text.h:
// mapped, or inflated whole), cut at record boundaries by the chunk rule of the parallel parse where that applies, the chunks
// turned into flat blocks by ss_fastx_to_flat on worker threads and put behind each other BY CHUNK INDEX -- and joins the two.
// ss_reads_load and ingest_inputs are not involved.  ss_reads_load_ordered (`--read_calls`) takes the first half alone: one file as
// one flat block in file order, kept as it is -- so file_to_flat_dev stays here, where both callers reach it.
#include "ss_piece_copy.h"
#include "ss_support.h"
#include "ss_input_text.h"

#include <thread>

#include <hipcub/hipcub.hpp>

using namespace ss::dev;
using ss::SUP_TILE;

namespace ss {
bool text_chunk_starts(const char *t, uint64_t n, std::vector<uint64_t> *starts);      // (ss_ingest.hip)
std::atomic<uint64_t> g_join_pairs_calls{0};      // ss_reads_join_pairs_calls: the joins of this file and of ss_bam_pairs.hip
}

namespace {

// the '\n' among the 16 bytes at off (positions below n only) of one lane
template <bool ALIGNED>
__device__ __forceinline__ uint32_t lane_newlines(const uint8_t *__restrict__ b, uint64_t off, uint64_t n)
{
    if (off >= n) return 0;
    uint32_t w[4];
    load16<ALIGNED>(b, off, n, w);
    uint32_t nl = newline_mask16(w) & 0xFFFFu;
    if (n - off < 16u) nl &= (1u << (uint32_t)(n - off)) - 1u;
    return nl;
}

// one wave per tile: cnt[tile] = its '\n'
template <bool ALIGNED>
__global__ __launch_bounds__(256) void line_count_kernel(const uint8_t *__restrict__ b, uint64_t n, uint64_t n_tiles,
                                                         unsigned long long *__restrict__ cnt)
{
    const uint64_t tile = (uint64_t)blockIdx.x * 4u + (threadIdx.x >> 6);
    if (tile >= n_tiles) return;                                        // (the same for the whole wave)
    const uint64_t off = tile * (uint64_t)SUP_TILE + (uint64_t)(threadIdx.x & 63u) * 16u;
    const uint32_t sum = wave_inclusive_sum((uint32_t)__popc(lane_newlines<ALIGNED>(b, off, n)));
    if ((threadIdx.x & 63u) == 63u) cnt[tile] = sum;
}

// ... and line_end[i] = the position of the i-th '\n' (lines at or beyond n_lines are never written)
template <bool ALIGNED>
__global__ __launch_bounds__(256) void line_ends_kernel(const uint8_t *__restrict__ b, uint64_t n, uint64_t n_tiles,
                                                        const unsigned long long *__restrict__ tile_base, uint64_t n_lines,
                                                        unsigned long long *__restrict__ line_end)
{
    const uint64_t tile = (uint64_t)blockIdx.x * 4u + (threadIdx.x >> 6);
    if (tile >= n_tiles) return;
    const uint64_t off = tile * (uint64_t)SUP_TILE + (uint64_t)(threadIdx.x & 63u) * 16u;
    uint32_t nl = lane_newlines<ALIGNED>(b, off, n);
    const uint32_t mine = (uint32_t)__popc(nl);
    uint64_t r = tile_base[tile] + wave_inclusive_sum(mine) - mine;
    for (; nl; nl &= nl - 1u, r++)
        if (r < n_lines) line_end[r] = off + ((uint32_t)__ffs(nl) - 1u);
}

// Sixteen lanes per fragment; n1, n2 >= 16, dst 16-byte aligned with room for n1 + n2 bytes.
__global__ __launch_bounds__(256) void join_kernel(const uint8_t *__restrict__ src1, uint64_t n1, const unsigned long long *__restrict__ le1,
                                                   const uint8_t *__restrict__ src2, uint64_t n2, const unsigned long long *__restrict__ le2,
                                                   uint64_t n_lines, uint8_t *__restrict__ dst)
{
    const uint64_t g = ((uint64_t)blockIdx.x * 256u + threadIdx.x) >> 4;
    if (g >= n_lines) return;
    const uint64_t s1 = g ? le1[g - 1] + 1u : 0u, s2 = g ? le2[g - 1] + 1u : 0u;
    const uint64_t len1 = le1[g] - s1, len2 = le2[g] - s2;
    if (le1[g] >= n1 || le2[g] >= n2 || s1 > le1[g] || s2 > le2[g]) return;      // (never: the line index lies in its block)
    const uint64_t D = s1 + s2, J = D + len1, M2 = J + 1u, E = M2 + len2 + 1u;    // the fragment: [D, E); 'N' at J; mate 2 (+ '\n') from M2
    write_span(dst, D, E, threadIdx.x & 15u, [&](uint64_t a, uint64_t lo, uint64_t hi) {
        const piece_t x = masked_fetch16(src1, n1, s1, D, M2, a, lo, hi) | masked_fetch16(src2, n2, s2, M2, E, a, lo, hi);
        return J >= a && J < a + 16u ? with_byte(x, (uint32_t)(J - a), 'N') : x;
    });
}

// steps 1 and 2 for one block of n > 0 bytes: *d_le [*n_lines] in `scratch`
int line_index(const uint8_t *b, uint64_t n, ss::PoolScratch &scratch, unsigned long long **d_le, uint64_t *n_lines)
{
    const hipStream_t st = ss::l2s::stream();
    const uint64_t n_tiles = (n + SUP_TILE - 1) / SUP_TILE;
    if (n_tiles >= 0x7FFFFFFFull) return SS_ERANGE;                     // hipcub counts its items in an int
    unsigned long long *d_cnt = nullptr, *d_base = nullptr;
    void *d_tmp = nullptr;
    size_t tmp_bytes = 0;
    SS_HIP(scratch.get((void **)&d_cnt, (n_tiles + 1) * 8));
    SS_HIP(scratch.get((void **)&d_base, (n_tiles + 1) * 8));
    SS_HIP(ss::l2s::set(d_cnt + n_tiles, 0, 8));
    const dim3 grid((unsigned)((n_tiles + 3) / 4));
    const bool al = (((uintptr_t)b) & 15) == 0;
    with_bool(al, [&](auto aligned) {
        hipLaunchKernelGGL(line_count_kernel<decltype(aligned)::value>, grid, dim3(256), 0, st, b, n, n_tiles, d_cnt);
    });
    SS_HIP(hipGetLastError());
    SS_HIP(hipcub::DeviceScan::ExclusiveSum(nullptr, tmp_bytes, d_cnt, d_base, (int)(n_tiles + 1), st));
    SS_HIP(scratch.get(&d_tmp, tmp_bytes));
    SS_HIP(hipcub::DeviceScan::ExclusiveSum(d_tmp, tmp_bytes, d_cnt, d_base, (int)(n_tiles + 1), st));
    unsigned long long total = 0;
    SS_HIP(ss::l2s::copy(&total, d_base + n_tiles, 8, hipMemcpyDeviceToHost));
    *n_lines = total;
    SS_HIP(scratch.get((void **)d_le, total * 8));
    with_bool(al, [&](auto aligned) {
        hipLaunchKernelGGL(line_ends_kernel<decltype(aligned)::value>, grid, dim3(256), 0, st, b, n, n_tiles, d_base, (uint64_t)total, *d_le);
    });
    SS_HIP(hipGetLastError());
    return SS_OK;
}

// ---------------------------------------------------------------------------------------------------------------------------
// one input file -> one flat block on the device, in file order
struct FlatDev { char *d = nullptr; uint64_t len = 0, cap = 0; };

int file_to_flat_dev(const char *path, int device, unsigned threads, FlatDev *out)
{
    if (hipSetDevice(device) != hipSuccess) return SS_EHIP;
    ss::InputText text;
    int rc = text.open_path(path);
    if (rc != SS_OK) return rc;
    std::vector<uint64_t> starts;
    if (!ss::text_chunk_starts(text.p, text.n, &starts)) { starts.assign(1, 0); starts.push_back(text.n); }
    const size_t n_chunks = starts.size() - 1;
    std::vector<char *> flat(n_chunks, nullptr);
    std::vector<uint64_t> flat_len(n_chunks, 0);
    std::atomic<size_t> next(0);
    std::atomic<int> err(SS_OK);
    auto worker = [&] {
        for (size_t c; err == SS_OK && (c = next.fetch_add(1)) < n_chunks;) {
            const uint64_t clen = starts[c + 1] - starts[c];
            char *buf = (char *)malloc(clen + 2);
            if (!buf) { err = SS_ENOMEM; break; }
            uint64_t nr = 0;
            const int r = ss_fastx_to_flat(text.p + starts[c], clen, buf, &flat_len[c], &nr);
            if (r != SS_OK) { free(buf); err = r; break; }
            char *fit = (char *)realloc(buf, std::max<uint64_t>(flat_len[c], 1));     // (the text is twice the bases and more)
            flat[c] = fit ? fit : buf;
        }
    };
    threads = (unsigned)std::min<size_t>(std::max(1u, threads), n_chunks);
    if (threads <= 1) worker();
    else {
        std::vector<std::thread> pool;
        for (unsigned w = 0; w < threads; w++) pool.emplace_back(worker);
        for (auto &th : pool) th.join();
    }
    rc = err;
    uint64_t total = 0;
    for (size_t c = 0; c < n_chunks; c++) total += flat_len[c];
    if (rc == SS_OK && total) {
        if (ss::big_malloc((void **)&out->d, total, &out->cap) != hipSuccess) rc = SS_ENOMEM;
        uint64_t o = 0;
        for (size_t c = 0; rc == SS_OK && c < n_chunks; c++) {          // by chunk index: file order
            if (flat_len[c] && hipMemcpy(out->d + o, flat[c], flat_len[c], hipMemcpyHostToDevice) != hipSuccess) rc = SS_EHIP;
            o += flat_len[c];
        }
        out->len = total;
    }
    for (char *q : flat) free(q);
    if (rc != SS_OK && out->d) { ss::big_put(out->d, out->cap); *out = FlatDev(); }
    return rc;
}

}  // namespace

extern "C" {

int ss_reads_join_pairs_calls(uint64_t *n)
{
    if (!n) return SS_EINVAL;
    *n = ss::g_join_pairs_calls.load();
    return SS_OK;
}

int ss_reads_join_pairs_dev(const void *flat1_dev, uint64_t n1, const void *flat2_dev, uint64_t n2, int order, ss_reads **out)
{
    if (!out) return SS_EINVAL;
    *out = nullptr;
    if ((n1 && !flat1_dev) || (n2 && !flat2_dev)) return SS_EINVAL;
    SS_HIP(hipDeviceSynchronize());                                     // (the blocks may have been written on any stream)
    const uint8_t *b1 = (const uint8_t *)flat1_dev, *b2 = (const uint8_t *)flat2_dev;
    char last[2] = {'\n', '\n'};
    if (n1) SS_HIP(ss::l2s::copy(&last[0], b1 + n1 - 1, 1, hipMemcpyDeviceToHost));
    if (n2) SS_HIP(ss::l2s::copy(&last[1], b2 + n2 - 1, 1, hipMemcpyDeviceToHost));
    if (last[0] != '\n' || last[1] != '\n') return SS_EINVAL;
    ss::PoolScratch scratch;
    unsigned long long *d_le1 = nullptr, *d_le2 = nullptr;
    uint64_t m1 = 0, m2 = 0;
    int rc = n1 ? line_index(b1, n1, scratch, &d_le1, &m1) : SS_OK;
    if (rc == SS_OK && n2) rc = line_index(b2, n2, scratch, &d_le2, &m2);
    if (rc != SS_OK) return rc;
    if (m1 != m2) return SS_EIO;
    if (m1 > 0xFFFFFFFFull) return SS_ERANGE;
    ss::g_join_pairs_calls++;                                           // (a join: the blocks pair up)
    const ss::HipFail fail{"ss_reads_join_pairs_dev"};
    ss_reads *S = nullptr;
    uint8_t *slab = nullptr;
    rc = ss::one_slab_set(m1, n1 + n2, fail.who, &S, &slab);
    if (rc != SS_OK) return rc;
    if (slab) {
        bool bad = false;
        // join_kernel's clamped loads need 16 bytes of source: a block below that is joined from a private copy padded to 16
        const uint8_t *src[2] = {b1, b2};
        uint64_t src_n[2] = {n1, n2};
        for (int f = 0; f < 2 && !bad; f++) {
            if (src_n[f] >= 16) continue;
            uint8_t *pad = nullptr;
            bad = fail(scratch.get((void **)&pad, 16)) || fail(ss::l2s::set(pad, '\n', 16)) ||
                  fail(hipMemcpyAsync(pad, src[f], src_n[f], hipMemcpyDeviceToDevice, ss::l2s::stream()));
            src[f] = pad;
            src_n[f] = 16;
        }
        if (!bad) {
            hipLaunchKernelGGL(join_kernel, dim3((unsigned)((m1 * 16u + 255u) / 256u)), dim3(256), 0, ss::l2s::stream(), src[0], src_n[0], d_le1, src[1],
                               src_n[1], d_le2, m1, slab);
            bad = fail(hipGetLastError());
        }
        bad = fail(ss::l2s::sync()) || bad;
        if (bad) { ss_reads_destroy(S); return SS_EHIP; }
    }
    if (order) {
        rc = ss_reads_order(S);
        if (rc != SS_OK) { ss_reads_destroy(S); return rc; }
    }
    *out = S;
    return SS_OK;
}

int ss_reads_load_pairs(const char *path1, const char *path2, int order, ss_reads **out)
{
    if (!out) return SS_EINVAL;
    *out = nullptr;
    if (!path1 || !path2) return SS_EINVAL;
    int device = 0;
    SS_HIP(hipGetDevice(&device));
    const unsigned threads = std::max(1u, ss::ingest_threads() / 2u);   // the two files share this process's parse threads
    FlatDev flat[2];
    int rcs[2] = {SS_OK, SS_OK};
    std::thread second([&] { rcs[1] = file_to_flat_dev(path2, device, threads, &flat[1]); });
    rcs[0] = file_to_flat_dev(path1, device, threads, &flat[0]);
    second.join();
    int rc = rcs[0] != SS_OK ? rcs[0] : rcs[1];
    if (rc == SS_OK) rc = ss_reads_join_pairs_dev(flat[0].d, flat[0].len, flat[1].d, flat[1].len, order, out);
    for (auto &f : flat)
        if (f.d) ss::big_put(f.d, f.cap);
    return rc;
}

// One file as one ASCII, unbinned slab in FILE ORDER (`--read_calls`): file_to_flat_dev, then what ss_reads_from_flat_dev does
// with order == 0.  Record i of the set is the i-th record of the file that has a sequence.
int ss_reads_load_ordered(const char *path, ss_reads **out)
{
    if (!out) return SS_EINVAL;
    *out = nullptr;
    if (!path || !path[0]) return SS_EINVAL;
    int device = 0;
    SS_HIP(hipGetDevice(&device));
    FlatDev flat;
    int rc = file_to_flat_dev(path, device, std::max(1u, ss::ingest_threads()), &flat);
    if (rc == SS_OK) rc = ss_reads_from_flat_dev(flat.d, flat.len, 0, out);
    if (flat.d) ss::big_put(flat.d, flat.cap);
    if (rc != SS_OK) *out = nullptr;
    return rc;
}

}  // extern "C"
