// ss_reorder.hip -- a resident read set in LOCALITY order.
//
// What bounds the scan of a table of sampled node sets is the number of random 64-byte sectors its page lookups pull
// from memory (ss_mini.hip): ~13 lookups per read, 54 G/s, all the memory system gives.  But a sample
// covers its genomes many times: the reads that start within the same 17 bases of a genome have the same minimizer in
// their first k-mer and share nearly all of their other minimizers too.  In file order such reads are millions of
// records apart -- every lookup misses the 4 MB L2; when they are processed at about the same time, the first read of a
// group pays the sector and the others find it in L2.  Counting does not care about the order of the records (integer
// sums), and the reads are parsed and shipped once per sample but scanned several times (tree scan, one scan per
// identified cluster, two more with -b: identify.py:409, Vote_Strain_L2_Lasso_new_sp.py:354-372,
// identify_low_depth.py:119,124).
//
// "About the same time" is all that is needed: the chip has ~8 K scan waves = ~50 K reads in flight, so a total order
// buys nothing over BINS of a few thousand reads.  Round 2 sorted (hipcub radix sort of 20 M (key, record) pairs, five
// passes over per-record arrays, a gather copy of ragged records at 1.3 TB/s: 9.7 ms per 20 M reads); ragged records are now
// binned in two streaming passes over the slab, with no per-record array at all (records of one length: sorted again, with a
// gather that knows where every record is -- "records of ONE length" below):
//   bin  = top 12 to 22 bits (order_bits) of h = mix30(minimizer of the record's first 31 bases) -- the hash that addresses the
//          index pages (ss_mini.hip), so a bin's FIRST lookups also walk the page table in ascending order;
//          records without a first k-mer (shorter, or a non-ACGT base in it) go to one extra bin at the end
//   pass 1  count_kernel: find the record starts of a 16 KB tile (64 bytes per lane, SWAR newline masks), the end of each
//           record (suffix minimum over the tile + a 512-byte halo), its bin; atomicAdd of the record's slot size to the
//           bin's byte count.  A slot = record + '\n', padded with '\n' to 8 bytes (152 bytes for a 150-base read: nothing
//           added) so that every piece of the copy is an aligned store
//   scan    exclusive prefix over the 4097 bin sizes (one workgroup)
//   pass 2  the same discovery again (cheaper than storing and re-reading 16 bytes per record), a returning atomicAdd
//           on the bin's cursor claims the slot, and the WAVE copies its records together: the records' 16-byte pieces are
//           numbered across the wave (prefix sum of the piece counts), every lane finds the record of its piece by
//           binary search in LDS, loads 16 unaligned bytes, pads behind the record's end with '\n' and stores them
//           aligned -- ~70 pieces for the ~7 records of a wave's 1 KB, two rounds of full-width loads and stores.
// Order inside a bin: the general passes leave it to the atomics (not reproducible run to run; the multiset of records is,
// and so is every count); records of ONE length -- what a sequencer writes, and the usual slab -- are SORTED by their bin
// instead (key pass, stable radix sort, gather: below), so a bin keeps its records in file order and a slab is the same byte
// for byte every time.  ON by default for resident read sets (SS_READS_ORDER=file keeps the file order): it costs ~2-3 ms per
// 20 M reads against ~80 ms of parsing and PCIe for the same reads, and every scan of the set is then 0-35 % faster
// depending on the coverage of the sample (profiles/r03_locality_sweep.json).
//
// THE DRIVER (ss::order_flat_dev) is the sequence of its steps: probe_one_length (the slab's head: is it a candidate for the
// one-length paths, with which L and n_rec) -> Scratch::take (one block, laid out in one place) -> one of three PATHS:
//   bin_sorted    one length, the product: NewSlab::alloc, pack_key_fixed (the one read of the ASCII slab: checks, keys, a packed
//                 file-order intermediate), the sort, gather_packed; gather_fixed (ASCII, from the source, in the same order) when
//                 a byte is outside the alphabet; ss_test_hook 5 = 1: key_fixed, the sort, gather_fixed
//   bin_counted   one length under ss_test_hook 6 = 1: count_fixed, prefix_and_tail, NewSlab::alloc, place_fixed(_packed)
//   bin_general   ragged records: count, prefix_and_tail, NewSlab::alloc, place (+ place_again for tiles beyond the table)
// A one-length path that meets a shorter or longer record says "not of one length" and the general passes run.  Every path
// reports its own three timing figures; the driver stores them, counts the slab and hands the scratch on to the next call.
//
// PACKED slabs.  A slab of one-length records whose every byte is A C G T or N (the pack pass checks the alphabet beside the
// layout) is placed as 2-bit codes + invalid flags, 3 bytes per 8 positions (ss_scan_dev.h IN_PACKED): 57 bytes per 150-base
// read instead of 152.  Positions, slots, bins and tiles are those of the ASCII slab; packed group g is exactly encode16 of its
// bytes [16g, 16g + 16), so every scan kernel sees bit-identical codes and flags, without its encode phase.  The placement is
// meant to gain from the random sectors its scattered writes touch (~3.3 per record ASCII, ~1.9 packed); it gains less: place
// 2.06 -> 1.93 ms per 20 M reads (profiles/r07_packed_ab.md: it also encodes, at 6 waves per SIMD, with byte stores at the edges);
// the sorted path writes the packed slab in order instead (profiles/r08_binning_gather_ab.md), from records it packed in file order
// while it keyed them (profiles/r15_binning_pack_ab.md).  Any other byte (lower case, IUPAC, '\r'): the ASCII gather runs, in the same
// order; ragged records, or ss_test_hook 5 = 1: ASCII.
#include "ss_common.h"

#include <mutex>
#include "ss_scan_dev.h"

#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <chrono>
#include <vector>

namespace {

constexpr int CH = 64;                      // bytes of a slab owned by one lane: that many / 16 loads in flight
constexpr int RB = 256 * CH;                // ... and by one workgroup (16 KB: what bounds these passes is the chain of dependent
                                            // round trips of a workgroup -- load, neighbours, key bytes, atomic -- not its instructions)
constexpr int HALO = 512;                   // bytes behind the tile searched (in parallel) for the end of its last record
constexpr int MAX_ORDER_BITS = 22;          // widest binning key (order_bits): 4 M bins + the one for records without a first k-mer
constexpr uint32_t NO_NL = 0xFFFFFFFFu;     // "no newline" as a tile-relative position
constexpr int TCAP = 2 * CH;                // record starts per tile that the record table holds (reads of ~125 bases and more)

// newline mask of 16 bytes (bit i = byte i is '\n'): exact SWAR zero-byte test on w ^ 0x0A0A0A0A leaves 0x80 in the bytes
// that were '\n'; byte dot products with weights 1, 2, 4, 8 (x 16 for the odd dwords) gather the flags, 128 x the mask
__device__ __forceinline__ uint32_t nl_mask16(const uint4 v)
{
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
    uint32_t z[4];
#pragma unroll
    for (int d = 0; d < 4; d++) {
        const uint32_t x = w[d] ^ 0x0A0A0A0Au;
        z[d] = ~(((x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | x) & 0x80808080u;
    }
    const uint32_t lo = __builtin_amdgcn_udot4(z[1], 0x80402010u, __builtin_amdgcn_udot4(z[0], 0x08040201u, 0u, false), false);
    const uint32_t hi = __builtin_amdgcn_udot4(z[3], 0x80402010u, __builtin_amdgcn_udot4(z[2], 0x08040201u, 0u, false), false);
    return (lo >> 7) | ((hi >> 7) << 8);
}

// 16 bytes at b + i; bytes at or beyond n read as '\n'
__device__ __forceinline__ uint4 load16_nl(const char *__restrict__ b, uint64_t i, uint64_t n)
{
    if (i + 16 <= n) { uint4 v; __builtin_memcpy(&v, b + i, 16); return v; }
    uint32_t w[4] = {0x0A0A0A0Au, 0x0A0A0A0Au, 0x0A0A0A0Au, 0x0A0A0A0Au};
    for (int k = 0; k < 16 && i + k < n; k++) {
        const uint32_t ch = (uint8_t)b[i + k];
        w[k >> 2] = (w[k >> 2] & ~(0xFFu << (8 * (k & 3)))) | (ch << (8 * (k & 3)));
    }
    return make_uint4(w[0], w[1], w[2], w[3]);
}

// 16 bytes at b + i, i < n, 16 <= n; bytes at or beyond n read as 0 (no per-byte path: a funnel shift of the last 16 bytes)
__device__ __forceinline__ uint4 load16_clamped(const char *__restrict__ b, uint64_t i, uint64_t n)
{
    uint4 v;
    if (i + 16 <= n) { __builtin_memcpy(&v, b + i, 16); return v; }
    unsigned __int128 x;
    __builtin_memcpy(&x, b + n - 16, 16);
    x >>= 8u * (uint32_t)(i + 16 - n);
    __builtin_memcpy(&v, &x, 16);
    return v;
}

// bin of a record: top `bits` bits of mix30(minimizer of its first 31 bases) (ordering key of the index, leftmost on
// ties); 1 << bits when the record has no first k-mer.  `b + s .. + 32` is inside the buffer (callers check).
__device__ __forceinline__ uint32_t record_bin(const char *__restrict__ b, uint64_t s, uint64_t len, int bits)
{
    if (len < 31) return 1u << bits;
    uint4 q[2];
    __builtin_memcpy(q, b + s, 32);
    const uint32_t w[8] = {q[0].x, q[0].y, q[0].z, q[0].w, q[1].x, q[1].y, q[1].z, q[1].w};
    uint64_t km = 0;
    uint32_t bad = 0;
#pragma unroll
    for (int d = 0; d < 8; d++) {
        const uint32_t c = (w[d] >> 1) & 0x03030303u;
        const uint32_t letter = __builtin_amdgcn_perm(0u, 0x47544341u, c);          // code -> 'A' 'C' 'T' 'G'
        uint32_t diff = (w[d] & 0xDFDFDFDFu) ^ letter;
        if (d == 7) diff &= 0x00FFFFFFu;                                            // byte 31 is not part of the k-mer
        bad |= diff;
        km |= (uint64_t)__builtin_amdgcn_udot4(c, 0x40100401u, 0u, false) << (8 * d);
    }
    if (bad) return 1u << bits;
    km &= 0x3FFFFFFFFFFFFFFFull;
    uint32_t best = 0xFFFFFFFFu;
#pragma unroll
    for (int i = 0; i < 31 - ss::MINI_M + 1; i++) {
        const uint32_t x = (uint32_t)(km >> (2 * i));
        best = min(best, (ss::mmkey(x) & ss::KEY_MASK) | (uint32_t)i);              // (key, position): leftmost on ties
    }
    const uint32_t x = (uint32_t)(km >> (2 * (best & 31u))) & ss::M30;
    return ss::mix30(x) >> (30 - bits);
}

__device__ __forceinline__ uint32_t wave_incl_sum(uint32_t v, int lane)
{
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const uint32_t o = (uint32_t)__shfl_up((int)v, off, 64);
        if (lane >= off) v += o;
    }
    return v;
}

// ---- what a workgroup knows about its 16 KB tile ------------------------------------------------------------------
// Per-tile record table, written by the first pass and read by the second (so the second neither looks for newlines
// nor keys anything): entry = start in the tile (14 bits) | length (26 bits) | bin (24 bits); a tile with more than
// TCAP record starts (reads shorter than ~125 bases), or a record of 64 MB, says T_OVERFLOW and is discovered again.
constexpr uint32_t T_OVERFLOW = 0xFFFFFFFFu;
constexpr int START_BITS = 14, LEN_BITS = 26, BIN_BITS = 64 - START_BITS - LEN_BITS;
constexpr uint32_t LEN_LIMIT = 1u << LEN_BITS;
static_assert(RB == 1 << START_BITS, "a table entry holds the start within the tile in START_BITS bits");
static_assert((1ull << MAX_ORDER_BITS) < (1ull << BIN_BITS), "a table entry holds every bin, 1 << bits (no first k-mer) included, in BIN_BITS bits");

struct TileLds {
    uint32_t first[5];                      // first newline (tile-relative) of waves 0..3 and of the halo
    uint32_t wcnt[4];                       // records taken by each wave in the current round
    uint32_t more;                          // some lane has another record start left
    uint64_t src[256], dst[256];            // the round's records: where they start, where they go
    uint32_t len[256], bin[256], pend[256]; // length, bin, inclusive count of 16-byte pieces
};

typedef uint64_t mask_t;                    // one bit per byte of the lane's chunk
__device__ __forceinline__ uint32_t mask_ctz(mask_t m) { return (uint32_t)__builtin_ctzll(m); }
struct TileState { mask_t nl, st; uint32_t later; uint64_t tile0, i0; };

// loads the lane's 64 bytes, finds the record starts in them and the first newline behind them (tile + halo)
__device__ __forceinline__ void tile_setup(const char *__restrict__ b, uint64_t n, TileLds &L, TileState &S)
{
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    S.tile0 = (uint64_t)blockIdx.x * RB;
    S.i0 = S.tile0 + (uint64_t)t * CH;
    mask_t nl = ~(mask_t)0;                             // beyond the buffer: newlines
    uint32_t prev = 1u;
    if (S.i0 < n) {
        uint4 v[CH / 16];
#pragma unroll
        for (int k = 0; k < CH / 16; k++) v[k] = load16_nl(b, S.i0 + 16u * k, n);
        prev = S.i0 == 0 ? 1u : (uint32_t)(b[S.i0 - 1] == '\n');
        nl = 0;
#pragma unroll
        for (int k = 0; k < CH / 16; k++) nl |= (mask_t)nl_mask16(v[k]) << (16 * k);
    }
    // first newline at or behind every lane's chunk: suffix minimum over the wave, then over the later waves and the halo
    uint32_t suf = nl ? (uint32_t)t * CH + mask_ctz(nl) : NO_NL;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const uint32_t o = (uint32_t)__shfl_down((int)suf, off, 64);
        if (lane + off < 64) suf = min(suf, o);
    }
    if (lane == 0) L.first[wave] = suf;
    if (wave == 0) {                                    // halo: HALO bytes behind the tile, 32 lanes x 16 bytes
        uint32_t h = NO_NL;
        const uint64_t j0 = S.tile0 + RB + (uint64_t)lane * 16;
        if (lane < HALO / 16) {
            if (j0 < n) {
                const uint32_t m = nl_mask16(load16_nl(b, j0, n));         // (the buffer's end reads as a newline)
                if (m) h = RB + (uint32_t)lane * 16u + (uint32_t)__builtin_ctz(m);
            } else {
                h = RB + (uint32_t)lane * 16u;
            }
        }
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) h = min(h, (uint32_t)__shfl_xor((int)h, off, 64));
        if (lane == 0) L.first[4] = h;
    }
    __syncthreads();
    uint32_t later = (uint32_t)__shfl_down((int)suf, 1, 64);               // first newline behind this lane's chunk
    if (lane == 63) later = NO_NL;
    for (int w = wave + 1; w < 5; w++) later = min(later, L.first[w]);
    const mask_t before = (nl << 1) | prev;                                // bit i = byte i - 1 is a newline
    S.nl = nl; S.later = later;
    S.st = ~nl & before;                                                   // record starts in this chunk
}

// One round: every lane hands in its next record start (a 64-byte chunk starts at most one read, so there is usually one
// round); the records are numbered across the workgroup and land in L.src / L.len.  Returns their number; L.more tells
// whether another round is needed.
__device__ __forceinline__ uint32_t tile_round(const char *__restrict__ b, uint64_t n, TileLds &L, TileState &S)
{
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const bool has = S.st != 0;
    uint64_t s = 0, len = 0;
    if (has) {
        const uint32_t bit = mask_ctz(S.st);
        S.st &= S.st - 1;
        s = S.i0 + bit;
        const mask_t up = bit + 1 < (uint32_t)CH ? S.nl & ~((((mask_t)1) << (bit + 1)) - 1) : (mask_t)0;
        uint64_t e;
        if (up) e = S.i0 + mask_ctz(up);
        else if (S.later != NO_NL) e = S.tile0 + S.later;
        else {                                                             // a record longer than the halo: walk on
            e = S.tile0 + RB + HALO;
            while (e < n) {
                const uint32_t m = nl_mask16(load16_nl(b, e, n));
                if (m) { e += (uint32_t)__builtin_ctz(m); break; }
                e += 16;
            }
            e = min(e, n);
        }
        len = e - s;
    }
    const uint64_t mask = __ballot(has);
    const uint32_t rank = (uint32_t)__popcll(mask & ((1ull << lane) - 1ull));
    if (lane == 0) L.wcnt[wave] = (uint32_t)__popcll(mask);
    if (t == 0) L.more = 0;
    __syncthreads();
    uint32_t base = 0, cnt = 0;
    for (int w = 0; w < 4; w++) { const uint32_t c = L.wcnt[w]; if (w < wave) base += c; cnt += c; }
    if (has) { L.src[base + rank] = s; L.len[base + rank] = (uint32_t)min(len, (uint64_t)0xFFFFFFFFu); }
    if (S.st != 0) L.more = 1;
    __syncthreads();
    return cnt;
}

__host__ __device__ __forceinline__ uint32_t slot_of(uint32_t len) { return (len + 1u + 7u) & ~7u; }     // record + '\n', padded to 8 bytes

// ---- pass 1: bytes per bin, and the tile's record table -----------------------------------------------------------------
__global__ __launch_bounds__(256, 8) __attribute__((amdgpu_num_sgpr(80))) void count_kernel(const char *__restrict__ b, uint64_t n, int bits, unsigned long long *__restrict__ hist,
                                                    uint32_t *__restrict__ tab_cnt, unsigned long long *__restrict__ tab,
                                                    unsigned long long *__restrict__ n_overflow)
{
    __shared__ TileLds L;
    TileState S;
    tile_setup(b, n, L, S);
    const int t = threadIdx.x;
    bool first = true;
    while (true) {
        const uint32_t cnt = tile_round(b, n, L, S);
        const bool more = L.more != 0;
        uint32_t bin = 0, len = 0;
        bool big = false;
        if ((uint32_t)t < cnt) {
            const uint64_t s = L.src[t];
            len = L.len[t];
            bin = (s + 32 <= n) ? record_bin(b, s, len, bits) : (1u << bits);
            atomicAdd(&hist[bin], (unsigned long long)slot_of(len));
            big = len >= LEN_LIMIT;
        }
        if (first) {
            const bool fits = !more && cnt <= (uint32_t)TCAP && !__syncthreads_or(big);
            if (fits && (uint32_t)t < cnt)
                tab[(uint64_t)blockIdx.x * TCAP + t] = (unsigned long long)(L.src[t] - S.tile0) | ((unsigned long long)len << START_BITS) |
                                                        ((unsigned long long)bin << (START_BITS + LEN_BITS));
            if (t == 0) {
                tab_cnt[blockIdx.x] = fits ? cnt : T_OVERFLOW;
                if (!fits) atomicAdd(n_overflow, 1ull);
            }
        }
        first = false;
        if (!more) break;
        __syncthreads();
    }
}

// ---- pass 2: claim the slots, copy -----------------------------------------------------------------------------------------
// The workgroup copies its records together: their 16-byte pieces are numbered across the workgroup (prefix sum of the
// piece counts), every lane finds the record of its piece by binary search in LDS, loads 16 unaligned bytes, pads behind
// the record's end with '\n' and stores them aligned (slots are multiples of 8 bytes).

// the piece at offset c of a record of rlen bytes: its record bytes stay, '\n' behind them
__device__ __forceinline__ void pad_piece(uint32_t (&w)[4], uint32_t rlen, uint32_t c)
{
    const int keep = (int)min(16u, rlen > c ? rlen - c : 0u);              // record bytes in this piece
    if (keep < 16) {
#pragma unroll
        for (int d = 0; d < 4; d++) {
            const int k = keep - 4 * d;
            if (k <= 0) w[d] = 0x0A0A0A0Au;
            else if (k < 4) { const uint32_t m = (1u << (8 * k)) - 1u; w[d] = (w[d] & m) | (0x0A0A0A0Au & ~m); }
        }
    }
}

// the record of piece p: the first of the round's cnt records whose inclusive piece count (L.pend) exceeds p
__device__ __forceinline__ int piece_record(const TileLds &L, uint32_t cnt, uint32_t p)
{
    int lo = 0, hi = (int)cnt - 1;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (L.pend[mid] <= p) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// one piece: the record's bytes from `v`, '\n' behind its end, stored aligned (slots are multiples of 8 bytes)
__device__ __forceinline__ void store_piece(char *__restrict__ dst, uint64_t out, uint4 v, uint32_t rlen, uint32_t rslot, uint32_t c)
{
    uint32_t w[4] = {v.x, v.y, v.z, v.w};
    pad_piece(w, rlen, c);
    char *o8 = static_cast<char *>(__builtin_assume_aligned(dst + out, 8));
    if (c + 16 <= rslot) __builtin_memcpy(o8, w, 16);
    else __builtin_memcpy(o8, w, 8);
}

__device__ __forceinline__ void copy_round(const char *__restrict__ b, uint64_t n, char *__restrict__ dst, TileLds &L, uint32_t cnt)
{
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const uint32_t pieces = (uint32_t)t < cnt ? (slot_of(L.len[t]) + 15u) >> 4 : 0u;
    uint32_t pend = wave_incl_sum(pieces, lane);
    if (lane == 63) L.wcnt[wave] = pend;
    __syncthreads();
    uint32_t total = 0;
    for (int w = 0; w < 4; w++) { const uint32_t c = L.wcnt[w]; if (w < wave) pend += c; total += c; }
    if ((uint32_t)t < cnt) L.pend[t] = pend;
    __syncthreads();
    for (uint32_t p = (uint32_t)t; p < total; p += 256) {
        const int lo = piece_record(L, cnt, p);
        const uint32_t rlen = L.len[lo], rslot = slot_of(rlen), c = (p - (L.pend[lo] - ((rslot + 15u) >> 4))) * 16u;
        const uint4 x = rlen > c ? load16_nl(b, L.src[lo] + c, n) : make_uint4(0x0A0A0A0Au, 0x0A0A0A0Au, 0x0A0A0A0Au, 0x0A0A0A0Au);
        store_piece(dst, L.dst[lo] + c, x, rlen, rslot, c);
    }
}

// the usual tile: everything is in the table.  The chain of dependent round trips is what bounds this pass, so it is kept
// short: table entries and count together; the returning atomics that claim the slots are ISSUED, and while they are on
// their way every lane finds its pieces (up to PRE of them: ~1100 pieces per tile of 150-base reads over 256 lanes) and
// loads their bytes -- neither needs the destination; only the stores wait for it.
constexpr int PRE = 6;
__global__ __launch_bounds__(256, 8) __attribute__((amdgpu_num_sgpr(80))) void place_kernel(
    const char *__restrict__ b, uint64_t n, unsigned long long *__restrict__ cursor, const uint32_t *__restrict__ tab_cnt,
    const unsigned long long *__restrict__ tab, char *__restrict__ dst)
{
    __shared__ TileLds L;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    static_assert(TCAP <= 256, "one table entry per thread");
    const unsigned long long e = t < TCAP ? tab[(uint64_t)blockIdx.x * TCAP + t] : 0ull;     // (in flight together with the count)
    const uint32_t known = tab_cnt[blockIdx.x];
    if (known == T_OVERFLOW || known == 0) return;
    uint64_t d0 = 0;
    uint32_t pieces = 0;
    if ((uint32_t)t < known) {
        const uint32_t len = (uint32_t)(e >> START_BITS) & (LEN_LIMIT - 1u);
        L.src[t] = (uint64_t)blockIdx.x * RB + (uint32_t)(e & (uint32_t)(RB - 1));
        L.len[t] = len;
        d0 = atomicAdd(&cursor[(uint32_t)(e >> (START_BITS + LEN_BITS))], (unsigned long long)slot_of(len));      // (answer needed at the stores)
        pieces = (slot_of(len) + 15u) >> 4;
    }
    uint32_t pend = wave_incl_sum(pieces, lane);
    if (lane == 63) L.wcnt[wave] = pend;
    __syncthreads();
    uint32_t total = 0;
    for (int w = 0; w < 4; w++) { const uint32_t c = L.wcnt[w]; if (w < wave) pend += c; total += c; }
    if ((uint32_t)t < known) L.pend[t] = pend;
    __syncthreads();
    uint4 v[PRE];
    uint32_t rec[PRE], off[PRE];
#pragma unroll
    for (int r = 0; r < PRE; r++) {
        const uint32_t p = (uint32_t)t + 256u * r;
        rec[r] = 0; off[r] = 0;
        v[r] = make_uint4(0x0A0A0A0Au, 0x0A0A0A0Au, 0x0A0A0A0Au, 0x0A0A0A0Au);
        if (p < total) {
            const int lo = piece_record(L, known, p);
            const uint32_t rlen = L.len[lo], c = (p - (L.pend[lo] - ((slot_of(rlen) + 15u) >> 4))) * 16u;
            rec[r] = (uint32_t)lo; off[r] = c;
            if (rlen > c) v[r] = load16_nl(b, L.src[lo] + c, n);
        }
    }
    if ((uint32_t)t < known) L.dst[t] = d0;
    __syncthreads();
#pragma unroll
    for (int r = 0; r < PRE; r++) {
        const uint32_t p = (uint32_t)t + 256u * r;
        if (p < total) {
            const uint32_t rlen = L.len[rec[r]];
            store_piece(dst, L.dst[rec[r]] + off[r], v[r], rlen, slot_of(rlen), off[r]);
        }
    }
    for (uint32_t p = (uint32_t)t + 256u * PRE; p < total; p += 256) {    // long records: the rest, piece by piece
        const int lo = piece_record(L, known, p);
        const uint32_t rlen = L.len[lo], rslot = slot_of(rlen), c = (p - (L.pend[lo] - ((rslot + 15u) >> 4))) * 16u;
        const uint4 x = rlen > c ? load16_nl(b, L.src[lo] + c, n) : make_uint4(0x0A0A0A0Au, 0x0A0A0A0Au, 0x0A0A0A0Au, 0x0A0A0A0Au);
        store_piece(dst, L.dst[lo] + c, x, rlen, rslot, c);
    }
}

// a tile whose records did not fit the table (short reads, several record starts in one lane's chunk): found and keyed again
__global__ __launch_bounds__(256) void place_again_kernel(const char *__restrict__ b, uint64_t n, int bits, unsigned long long *__restrict__ cursor,
                                                          const uint32_t *__restrict__ tab_cnt, char *__restrict__ dst)
{
    __shared__ TileLds L;
    const int t = threadIdx.x;
    if (tab_cnt[blockIdx.x] != T_OVERFLOW) return;
    TileState S;
    tile_setup(b, n, L, S);
    while (true) {
        const uint32_t cnt = tile_round(b, n, L, S);
        const bool more = L.more != 0;
        if ((uint32_t)t < cnt) {
            const uint64_t s = L.src[t];
            const uint32_t len = L.len[t];
            const uint32_t bin = (s + 32 <= n) ? record_bin(b, s, len, bits) : (1u << bits);
            L.dst[t] = atomicAdd(&cursor[bin], (unsigned long long)slot_of(len));
        }
        __syncthreads();
        copy_round(b, n, dst, L, cnt);
        if (!more) break;
        __syncthreads();
    }
}

// ---- records of ONE length (what a sequencer writes: every read 150 bases) ---------------------------------------------
// The general passes above spend their time finding out where records begin and end -- newline masks, a suffix minimum
// over the tile, a halo, record tables in LDS, a binary search per copied piece: chains of dependent round trips that hold
// them at 2.4-2.5 TB/s (profiles/r05_sampled_kernel_stats.csv: 1.28 + 2.43 ms per 20 M reads).  When every record of the
// slab has the same length L (the slab is n_rec x (L + 1) bytes, the first newline says L) record i starts at i * (L + 1)
// and nothing has to be found: a WAVE owns 64 consecutive records (9.7 KB for L = 150), no LDS, no barrier.
//   count_fixed   streams the wave's span in 16-byte pieces and CHECKS it -- a newline at offset L of every record and
//                 nowhere else; one violation anywhere sets a flag and the caller runs the general passes instead -- and
//                 every lane keys its own record from its first 32 bytes (in cache by then); bin sizes by atomicAdd, the
//                 record's bin kept (4 bytes per record) for the second pass
//   place_fixed   the returning atomicAdd on the bin's cursor is issued first; while it is on its way the lanes load the
//                 span's pieces (numbered across the wave: consecutive lanes, consecutive 16 bytes); the destination of
//                 a piece's record comes from the owning lane by a wave shuffle; aligned stores, padded with '\n'
// These two (and place_fixed_packed) are what ss_test_hook 6 = 1 runs; the product sorts instead (pack_key_fixed, gather_packed below).
constexpr uint32_t FIX_MIN_L = 32, FIX_MAX_L = 1023;

// non-zero unless every byte of w is 'A' 'C' 'G' 'T' 'N' or '\n' -- upper case only: a packed slab reads back as exactly these
__device__ __forceinline__ uint32_t not_packable4(uint32_t w)
{
    auto zb = [](uint32_t x) { return ~(((x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | x) & 0x80808080u; };      // 0x80 where a byte is zero
    const uint32_t letter = __builtin_amdgcn_perm(0u, 0x47544341u, (w >> 1) & 0x03030303u);           // code -> 'A' 'C' 'T' 'G'
    return (zb(w ^ letter) | zb(w ^ 0x4E4E4E4Eu) | zb(w ^ 0x0A0A0A0Au)) ^ 0x80808080u;
}

__global__ __launch_bounds__(256, 8) void count_fixed_kernel(const char *__restrict__ b, uint64_t n, uint64_t n_rec, uint32_t L, uint32_t magic_l1, int bits,
                                                             unsigned long long *__restrict__ hist, uint32_t *__restrict__ bins,
                                                             unsigned long long *__restrict__ not_fixed, unsigned long long *__restrict__ not_packable)
{
    const int lane = threadIdx.x & 63;
    const uint64_t r0 = ((uint64_t)blockIdx.x * 4u + (threadIdx.x >> 6)) * 64u;
    if (r0 >= n_rec) return;
    const uint32_t L1 = L + 1u, nr = (uint32_t)min((uint64_t)64, n_rec - r0), span = nr * L1;
    const uint64_t base = r0 * L1;
    bool bad = false;
    uint32_t alpha = 0;
    for (uint32_t off = (uint32_t)lane * 16u; off < span; off += 1024u) {
        const uint4 v = load16_nl(b, base + off, n);
        const uint32_t m = nl_mask16(v);
        const uint32_t pos = off - __umulhi(off, magic_l1) * L1;           // offset of the piece's first byte within its record
        const uint32_t valid = span - off >= 16u ? 0xFFFFu : (1u << (span - off)) - 1u;
        const uint32_t want = L - pos < 16u ? 1u << (L - pos) : 0u;        // (L >= 32: at most one record end in 16 bytes)
        bad |= ((m ^ want) & valid) != 0u;
        alpha |= not_packable4(v.x) | not_packable4(v.y) | not_packable4(v.z) | not_packable4(v.w);      // (bytes past the span: the
    }                                                                      // next wave's records, or padding that must be '\n')
    if (r0 + nr == n_rec) {                                                // behind the last record: newlines only (padding)
        for (uint64_t i = base + span + (uint32_t)lane; i < n; i += 64) bad |= b[i] != '\n';
    }
    if (__ballot(bad)) { if (lane == 0) atomicOr(not_fixed, 1ull); return; }
    if (__ballot(alpha != 0u) && lane == 0) atomicOr(not_packable, 1ull);
    if ((uint32_t)lane < nr) {
        const uint32_t bin = record_bin(b, base + (uint64_t)lane * L1, L, bits);      // (s + 32 <= s + L + 1 <= n)
        bins[r0 + lane] = bin;
        atomicAdd(&hist[bin], (unsigned long long)slot_of(L));
    }
}

constexpr int FPRE = 5;                     // pieces a lane has in flight: 64 lanes x 5 = the 640 pieces of 64 records of 150 bases
__global__ __launch_bounds__(256, 8) void place_fixed_kernel(const char *__restrict__ b, uint64_t n, uint64_t n_rec, uint32_t L, uint32_t magic_p,
                                                             unsigned long long *__restrict__ cursor, const uint32_t *__restrict__ bins,
                                                             char *__restrict__ dst)
{
    const int lane = threadIdx.x & 63;
    const uint64_t r0 = ((uint64_t)blockIdx.x * 4u + (threadIdx.x >> 6)) * 64u;
    if (r0 >= n_rec) return;
    const uint32_t L1 = L + 1u, nr = (uint32_t)min((uint64_t)64, n_rec - r0), slot = slot_of(L), P = (slot + 15u) >> 4, total = nr * P;
    const uint64_t base = r0 * L1;
    unsigned long long d0 = 0;
    if ((uint32_t)lane < nr) d0 = atomicAdd(&cursor[bins[r0 + lane]], (unsigned long long)slot);      // (answer needed at the stores)
    for (uint32_t p0 = 0; p0 < total; p0 += 64u * FPRE) {
        uint4 v[FPRE];
        uint32_t rec[FPRE], off[FPRE];
#pragma unroll
        for (int r = 0; r < FPRE; r++) {
            const uint32_t p = p0 + (uint32_t)lane + 64u * r;
            rec[r] = min(__umulhi(p, magic_p), nr - 1u);
            off[r] = (p - rec[r] * P) * 16u;
            v[r] = make_uint4(0x0A0A0A0Au, 0x0A0A0A0Au, 0x0A0A0A0Au, 0x0A0A0A0Au);
            if (p < total && L > off[r]) v[r] = load16_nl(b, base + (uint64_t)rec[r] * L1 + off[r], n);
        }
#pragma unroll
        for (int r = 0; r < FPRE; r++) {
            const uint32_t p = p0 + (uint32_t)lane + 64u * r;
            const uint32_t lo = (uint32_t)__shfl((int)(uint32_t)d0, (int)rec[r], 64), hi = (uint32_t)__shfl((int)(uint32_t)(d0 >> 32), (int)rec[r], 64);
            if (p < total) store_piece(dst, (((uint64_t)hi << 32) | lo) + off[r], v[r], L, slot, off[r]);
        }
    }
}

// ---- the same placement into a PACKED slab (ss_scan_dev.h IN_PACKED) ------------------------------------------------------
// Positions as in the ASCII slab (a record at its bin cursor, slot_of(L) positions), but every 8 positions are one 3-byte unit:
// a record is one contiguous span of 3 slot / 8 bytes (57 for 150 bases) at byte 3 (cursor / 8), anywhere modulo 4.  The
// wave's records are encoded first (pieces numbered across the wave as in place_fixed: consecutive lanes, consecutive 16 bytes
// of the source; encode16, the record's '\n' padding included) into LDS, record r at byte r A + 4 of the wave's area, while the
// returning atomics are on their way; then every lane stores one destination dword of a record's span, read back from LDS with
// the span's alignment.  A record's first and last dword may share bytes with its neighbours: those go out as byte stores.
// Long reads take several rounds of G records (the wave's LDS holds 64 records of up to 151 bases at once).
constexpr uint32_t PK_LDS = 4352;           // bytes of LDS per wave: 64 records x 68 bytes (L <= 151)
constexpr int FPK = 4;                      // pieces a lane has in flight (the kernel takes 80 VGPRs: six waves per SIMD, no scratch)

__global__ __launch_bounds__(256, 6) void place_fixed_packed_kernel(const char *__restrict__ b, uint64_t n, uint64_t n_rec, uint32_t L,
                                                                    uint32_t P, uint32_t magic_p, uint32_t A, uint32_t G, uint32_t ND,
                                                                    uint32_t magic_nd, unsigned long long *__restrict__ cursor,
                                                                    const uint32_t *__restrict__ bins, uint8_t *__restrict__ dst)
{
    __shared__ uint32_t lds[4][PK_LDS / 4 + 1];   // (+1: the second dword of the last record's last read)
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint64_t r0 = ((uint64_t)blockIdx.x * 4u + (uint32_t)wave) * 64u;
    if (r0 >= n_rec) return;
    const uint32_t L1 = L + 1u, nr = (uint32_t)min((uint64_t)64, n_rec - r0), slot = slot_of(L), B = slot / 8u * 3u;
    const uint64_t base = r0 * L1;
    uint32_t *W = lds[wave];
    uint8_t *W8 = reinterpret_cast<uint8_t *>(W);
    unsigned long long d0 = 0;
    if ((uint32_t)lane < nr) d0 = atomicAdd(&cursor[bins[r0 + lane]], (unsigned long long)slot);      // (answer needed at the stores)
    for (uint32_t c0 = 0; c0 < nr; c0 += G) {
        const uint32_t nc = min(G, nr - c0), total = nc * P;
        for (uint32_t p0 = 0; p0 < total; p0 += 64u * FPK) {
            uint4 v[FPK];                                                  // (piece, record and offset are worked out twice: registers)
#pragma unroll
            for (int r = 0; r < FPK; r++) {
                const uint32_t p = p0 + (uint32_t)lane + 64u * r, rec = min(__umulhi(p, magic_p), nc - 1u), off = (p - rec * P) * 16u;
                v[r] = make_uint4(0x0A0A0A0Au, 0x0A0A0A0Au, 0x0A0A0A0Au, 0x0A0A0A0Au);
                if (p < total && L > off) v[r] = load16_nl(b, base + (uint64_t)(c0 + rec) * L1 + off, n);
            }
#pragma unroll
            for (int r = 0; r < FPK; r++) {
                const uint32_t p = p0 + (uint32_t)lane + 64u * r, rec = min(__umulhi(p, magic_p), nc - 1u), off = (p - rec * P) * 16u;
                if (p >= total) continue;
                uint32_t w[4] = {v[r].x, v[r].y, v[r].z, v[r].w};
                pad_piece(w, L, off);
                uint32_t code, inv;
                ss::dev::encode16(w, code, inv);
                // the group's 6 bytes: code[0..15] inv[0..7] code[16..31] inv[8..15] (2-byte aligned in LDS)
                uint16_t *q = reinterpret_cast<uint16_t *>(W8 + rec * A + 4u + (off >> 4) * 6u);
                q[0] = (uint16_t)code;
                q[1] = (uint16_t)((inv & 0xFFu) | ((code >> 8) & 0xFF00u));
                q[2] = (uint16_t)((code >> 24) | (inv & 0xFF00u));
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        // the destination dwords of the records' spans: item i = record i / ND, its dword i % ND (counted from the dword of its first byte)
        const uint32_t items = nc * ND;
        for (uint32_t i0 = 0; i0 < items; i0 += 64u) {                      // (uniform trip count: every lane takes part in the shuffles)
            const uint32_t i = i0 + (uint32_t)lane, rec = min(__umulhi(i, magic_nd), nc - 1u), jl = i - rec * ND;
            const uint32_t lo = (uint32_t)__shfl((int)(uint32_t)d0, (int)(c0 + rec), 64), hi = (uint32_t)__shfl((int)(uint32_t)(d0 >> 32), (int)(c0 + rec), 64);
            const uint64_t D = ((((uint64_t)hi << 32) | lo) >> 3) * 3u;    // the record's first byte in the packed slab
            const int o = (int)(4u * jl) - (int)(D & 3u);                   // record byte at the dword's first byte (-3 .. )
            if (i < items && o < (int)B) {
                const uint32_t x = rec * A + 4u + (uint32_t)o;              // (>= rec A + 1)
                const uint32_t val = __builtin_amdgcn_alignbyte(W[(x >> 2) + 1u], W[x >> 2], x & 3u);
                uint8_t *out = dst + (D & ~3ull) + 4u * jl;
                if (o >= 0 && o + 4 <= (int)B) {
                    *reinterpret_cast<uint32_t *>(__builtin_assume_aligned(out, 4)) = val;
                } else {
#pragma unroll
                    for (int k = 0; k < 4; k++)
                        if (o + k >= 0 && o + k < (int)B) out[k] = (uint8_t)(val >> (8 * k));
                }
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");             // (the next round's LDS writes come behind these reads)
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
}

// ---- records of one length, SORTED: keys, a stable radix sort, a gather in output order -----------------------------------------
// The two passes above pay for random-address atomics (one per record on the bin counters, one returning one on the cursors) and
// for scattered partial writes.  With every slot of one size, the output position of a record is its RANK in bin order, times the
// slot: so the records' keys are sorted instead, and the copy reads at random and writes in order.
// The ASCII slab is read ONCE, in order, by the pass that does everything its bytes are needed for; what is moved at random
// afterwards is the packed record, one aligned 64-byte sector per 150-base read instead of ~3.4 sectors of ASCII.
//   pack_key_fixed  a wave owns 64 consecutive SOURCE records, one contiguous span, streamed in 16-byte pieces numbered across the
//                 wave.  Every piece is CHECKED (a newline at offset L of its record and none before it; only newlines behind the
//                 last record; A C G T N only), padded with '\n', encoded (encode16) and put into LDS, record r at r Rt
//                 (R = slot / 8 x 3 bytes packed, 57 for 150 bases; Rt = R rounded up to 16: 64); the wave's nr Rt bytes go out
//                 as whole aligned 16-byte stores to the file-order INTERMEDIATE at r0 Rt (bytes R .. Rt - 1 of a record are
//                 never read).  Then every lane keys its own record from its first 32 ASCII bytes (in cache by then): key[i] =
//                 its bin (record_bin), val[i] = i; no atomics but the flags, set only while still clear (atomics on ONE address
//                 from every wave queue up for ms).  A wave that finds not_packable set stops encoding and only keys -- a
//                 lower-case slab costs what key_fixed costs --; one that finds not_fixed set returns
//   (sort)        hipcub::DeviceRadixSort::SortPairs over the key bits [0, bits + 1): stable, so a bin keeps its records in file
//                 order and a binned slab is the same byte for byte from run to run
//   gather_packed a wave owns 64 consecutive OUTPUT records; output record j is record perm[j] of the intermediate: Rt / 16
//                 aligned 16-byte loads, all of the wave's in flight at once (4 per lane for 150 bases), into LDS at stride Rt;
//                 the round's span of G R bytes is read back at stride R (dword by dword, alignbyte) and goes out as aligned
//                 16-byte stores (rounds of G records, G R a multiple of 16: every round's span starts aligned).  No checks, no
//                 encode; nothing to do once either flag is set
//   key_fixed     (ss_test_hook 5 = 1: an ASCII slab wanted) one lane per record: key and val as above.  A cheap check beside
//                 it: the byte in front of every record start, and the last record's newline and the padding behind it, must be
//                 '\n' (what a shorter, longer or empty record shifts); else not_fixed, and the gather does nothing
//   gather_fixed  the ASCII gather FROM THE SOURCE, for hook 5 and for a slab with a byte outside the alphabet (same perm): the
//                 pieces of the wave's 64 output records are loaded at random, CHECKED (a newline at offset L and none before
//                 it), padded with '\n' and put into LDS in output layout; then the span goes out as aligned 16-byte stores
__global__ __launch_bounds__(256) void key_fixed_kernel(const char *__restrict__ b, uint64_t n, uint64_t n_rec, uint32_t L, int bits,
                                                        uint32_t *__restrict__ key, uint32_t *__restrict__ val,
                                                        unsigned long long *__restrict__ not_fixed)
{
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= n_rec) return;
    const uint64_t s = i * (L + 1u);
    bool bad = i > 0 && b[s - 1] != '\n';
    if (i + 1 == n_rec)
        for (uint64_t k = s + L; k < n; k++) bad |= b[k] != '\n';         // (fewer than 64 + 1 bytes: the host chose L so)
    key[i] = record_bin(b, s, L, bits);                                     // (s + 32 <= s + L + 1 <= n)
    val[i] = (uint32_t)i;
    const uint64_t m = __ballot(bad);                                       // (a flag already set is not set again: atomics on ONE
    if (m && (uint32_t)(threadIdx.x & 63) == (uint32_t)__builtin_ctzll(m) &&       // address from every wave queue up for ms)
        !*(volatile unsigned long long *)not_fixed) atomicOr(not_fixed, 1ull);
}

constexpr uint32_t GX_LDS_PK = 6144, GX_LDS_ASCII = 8192;    // LDS a wave may take: 16 records of the longest slot (1024 positions)
constexpr int GPK = 3;                      // pieces a lane of the ASCII gather has in flight (62 VGPRs, no scratch)
constexpr int PKP = 2;                      // ... of the pack pass (63 VGPRs: eight waves per SIMD, no scratch; 3 pieces: as fast;
                                            // 4 at six waves: 8 spilled, slower)
constexpr int GQ = 4;                       // ... of the packed gather: 64 lanes x 4 = the 256 pieces of 64 packed records of 150 bases

// bytes of a packed record (3 per 8 positions), and its stride in the file-order intermediate: whole 16-byte pieces
__host__ __device__ __forceinline__ uint32_t packed_row(uint32_t slot) { return slot / 8u * 3u; }
__host__ __device__ __forceinline__ uint32_t packed_stride(uint32_t slot) { return (packed_row(slot) + 15u) & ~15u; }

// records per round of a gather: G <= 64, G R a multiple of 16 (every round's span starts aligned) and at most lim bytes.  The
// ASCII gather's LDS is those G R bytes per wave; the packed gather holds the round at stride Rt <= R + 15, G Rt + 16 bytes per
// wave (7.1 KB at most, 28.5 KB per workgroup)
inline uint32_t gather_rows(bool pk, uint32_t L)
{
    const uint32_t slot = slot_of(L), R = pk ? packed_row(slot) : slot, lim = pk ? GX_LDS_PK : GX_LDS_ASCII;
    uint32_t G = 64;
    while (G > 1 && (G * R > lim || (G * R) % 16u)) G--;
    return G;
}
// records per round of the pack pass: G Rt within the wave's LDS (Rt is a multiple of 16 already)
inline uint32_t pack_rows(uint32_t L) { return std::min<uint32_t>(64u, GX_LDS_PK / packed_stride(slot_of(L))); }

// 16 aligned bytes that are touched once -- the intermediate's 1.28 GB per 20 M reads, written, read back at random, and the
// new slab's 1.14 GB: marked non-temporal, they do not push what is still to be read out of the caches (pack + key + sort 1.73 ->
// 1.53 ms, packed gather + tail 0.75 -> 0.70 ms per 20 M reads of 150 bases; the same mark on the pack pass's reads of the source
// costs 0.3 ms: profiles/r15_binning_pack_ab.md)
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ uint4 load16_once(const void *p)
{
    const u32x4 x = __builtin_nontemporal_load(static_cast<const u32x4 *>(__builtin_assume_aligned(p, 16)));
    return make_uint4(x.x, x.y, x.z, x.w);
}
__device__ __forceinline__ void store16_once(void *p, const uint4 v)
{
    const u32x4 x = {v.x, v.y, v.z, v.w};
    __builtin_nontemporal_store(x, static_cast<u32x4 *>(__builtin_assume_aligned(p, 16)));
}

// the pack + key pass: see "records of one length, SORTED" above.  A wave that sees not_packable set only keys (and checks the
// padding behind the last record: the ASCII gather checks every record, not what follows them); one that sees not_fixed returns.
// Bytes R .. Rt - 1 of a record are indeterminate by design: nobody writes them in LDS, they travel to the intermediate and into
// the gather's LDS as they are, and the gather's read at stride R never takes them (its `keep` mask and the record's wrap).
__global__ __launch_bounds__(256, 8) void pack_key_fixed_kernel(const char *__restrict__ b, uint64_t n, uint64_t n_rec, uint32_t L, uint32_t P,
                                                                uint32_t magic_p, uint32_t G, int bits, uint32_t *__restrict__ key,
                                                                uint32_t *__restrict__ val, uint8_t *__restrict__ inter,
                                                                unsigned long long *__restrict__ not_fixed, unsigned long long *__restrict__ not_packable)
{
    extern __shared__ uint4 gx_lds[];       // 4 waves x G Rt bytes
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint64_t r0 = ((uint64_t)blockIdx.x * 4u + (uint32_t)wave) * 64u;
    if (r0 >= n_rec || __ballot(*(volatile unsigned long long *)not_fixed != 0ull)) return;
    const bool pack = __ballot(*(volatile unsigned long long *)not_packable != 0ull) == 0ull;
    const uint32_t L1 = L + 1u, nr = (uint32_t)min((uint64_t)64, n_rec - r0), slot = slot_of(L), Rt = packed_stride(slot);
    const uint64_t base = r0 * L1;
    uint4 *W = gx_lds + (size_t)wave * (G * Rt / 16u);
    uint8_t *W8 = reinterpret_cast<uint8_t *>(W);
    bool bad = false;
    uint32_t alpha = 0;
    for (uint32_t c0 = 0; pack && c0 < nr; c0 += G) {
        const uint32_t nc = min(G, nr - c0), total = nc * P;
        for (uint32_t p0 = 0; p0 < total; p0 += 64u * PKP) {
            uint4 v[PKP];                                                  // (piece, record and offset are worked out twice: registers)
#pragma unroll
            for (int r = 0; r < PKP; r++) {
                const uint32_t p = p0 + (uint32_t)lane + 64u * r, rec = min(__umulhi(p, magic_p), nc - 1u), off = (p - rec * P) * 16u;
                v[r] = make_uint4(0x0A0A0A0Au, 0x0A0A0A0Au, 0x0A0A0A0Au, 0x0A0A0A0Au);
                if (p < total && L >= off) v[r] = load16_clamped(b, base + (uint64_t)(c0 + rec) * L1 + off, n);      // (the piece of byte L is
                                                                    // loaded too; bytes behind byte L < n are neither checked nor kept)
            }
#pragma unroll
            for (int r = 0; r < PKP; r++) {
                const uint32_t p = p0 + (uint32_t)lane + 64u * r, rec = min(__umulhi(p, magic_p), nc - 1u), off = (p - rec * P) * 16u;
                if (p >= total) continue;
                uint32_t w[4] = {v[r].x, v[r].y, v[r].z, v[r].w};
                if (L >= off) {                                             // a newline at byte L, none before it
                    const uint32_t m = nl_mask16(v[r]), e = L - off;
                    const uint32_t want = e < 16u ? 1u << e : 0u, valid = e < 16u ? (2u << e) - 1u : 0xFFFFu;
                    bad |= ((m ^ want) & valid) != 0u;
                }
                pad_piece(w, L, off);
                alpha |= not_packable4(w[0]) | not_packable4(w[1]) | not_packable4(w[2]) | not_packable4(w[3]);
                uint32_t code, inv;
                ss::dev::encode16(w, code, inv);
                // the group's 6 bytes: code[0..15] inv[0..7] code[16..31] inv[8..15] (2-byte aligned in LDS); the last piece of a
                // slot of 8 x odd positions has only its first 3 (the byte behind them is one of R .. Rt - 1: never read)
                uint16_t *q = reinterpret_cast<uint16_t *>(W8 + rec * Rt + (off >> 4) * 6u);
                q[0] = (uint16_t)code;
                q[1] = (uint16_t)((inv & 0xFFu) | ((code >> 8) & 0xFF00u));
                if (off + 16u <= slot) q[2] = (uint16_t)((code >> 24) | (inv & 0xFF00u));
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        // the round's records: nc Rt bytes at (r0 + c0) Rt of the intermediate, whole aligned 16-byte stores
        uint8_t *out = inter + (r0 + c0) * Rt;
        for (uint32_t q = (uint32_t)lane * 16u; q < nc * Rt; q += 1024u) store16_once(out + q, W[q >> 4]);
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");             // (the next round's LDS writes come behind these reads)
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
    if (r0 + nr == n_rec) {                                                // behind the last record: newlines only (padding)
        for (uint64_t i = base + (uint64_t)nr * L1 + (uint32_t)lane; i < n; i += 64) bad |= b[i] != '\n';
    }
    if (__ballot(bad)) { if (lane == 0 && !*(volatile unsigned long long *)not_fixed) atomicOr(not_fixed, 1ull); return; }
    if (__ballot(alpha != 0u) && lane == 0 && !*(volatile unsigned long long *)not_packable) atomicOr(not_packable, 1ull);
    if ((uint32_t)lane < nr) {
        key[r0 + lane] = record_bin(b, base + (uint64_t)lane * L1, L, bits);      // (from the ASCII bytes, in cache by now; s + 32 <= s + L + 1 <= n)
        val[r0 + lane] = (uint32_t)(r0 + lane);
    }
}

// the packed gather: output record j of the wave is record perm[r0 + j] of the intermediate, Rt / 16 aligned pieces; they land in
// LDS at stride Rt (piece p of the round at W[p]) and the round's span is read back at stride R, dword by dword
__global__ __launch_bounds__(256, 8) void gather_packed_kernel(const uint8_t *__restrict__ inter, uint64_t n_rec, uint32_t R, uint32_t magic_r,
                                                               uint32_t Q, uint32_t magic_q, uint32_t G, const uint32_t *__restrict__ perm,
                                                               uint8_t *__restrict__ dst, const unsigned long long *__restrict__ not_fixed,
                                                               const unsigned long long *__restrict__ not_packable)
{
    extern __shared__ uint4 gx_lds[];       // 4 waves x (G Rt + 16) bytes (+16: the second dword of the last record's last read)
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint64_t r0 = ((uint64_t)blockIdx.x * 4u + (uint32_t)wave) * 64u;
    // nothing to do once the slab is known not to be of one length, or not packable: the general passes, or the ASCII gather, come next
    if (r0 >= n_rec || *(volatile const unsigned long long *)not_fixed || *(volatile const unsigned long long *)not_packable) return;
    const uint32_t nr = (uint32_t)min((uint64_t)64, n_rec - r0), Rt = Q * 16u;
    uint4 *W = gx_lds + (size_t)wave * (G * Q + 1u);
    const uint32_t *W32 = reinterpret_cast<const uint32_t *>(W);
    const uint8_t *W8 = reinterpret_cast<const uint8_t *>(W);
    const uint32_t mine = (uint32_t)lane < nr ? min(perm[r0 + lane], (uint32_t)(n_rec - 1u)) : 0u;      // source of the wave's output record `lane`
    for (uint32_t c0 = 0; c0 < nr; c0 += G) {
        const uint32_t nc = min(G, nr - c0), total = nc * Q;
        for (uint32_t p0 = 0; p0 < total; p0 += 64u * GQ) {                 // (uniform trip count: every lane takes part in the shuffles;
            uint4 v[GQ];                                                    // Q = 1 has no 32-bit reciprocal)
#pragma unroll
            for (int r = 0; r < GQ; r++) {
                const uint32_t p = p0 + (uint32_t)lane + 64u * r, rec = min(Q == 1u ? p : __umulhi(p, magic_q), nc - 1u), k = p - rec * Q;
                const uint32_t s = (uint32_t)__shfl((int)mine, (int)(c0 + rec), 64);
                v[r] = make_uint4(0u, 0u, 0u, 0u);
                if (p < total) v[r] = load16_once(inter + (uint64_t)s * Rt + k * 16u);
            }
#pragma unroll
            for (int r = 0; r < GQ; r++) {
                const uint32_t p = p0 + (uint32_t)lane + 64u * r;
                if (p < total) W[p] = v[r];
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        // the round's span: nc R bytes at (r0 + c0) R -- 16-byte aligned, whole 16-byte stores but at the slab's very end
        const uint32_t span = nc * R;
        uint8_t *out = dst + (r0 + c0) * R;
        for (uint32_t q = (uint32_t)lane * 16u; q < span; q += 1024u) {
            uint32_t rec = __umulhi(q, magic_r), o = q - rec * R;           // span byte q = byte o of the round's record rec
            if (q + 16u <= span) {
                uint32_t w[4];
#pragma unroll
                for (int d = 0; d < 4; d++) {
                    const uint32_t x = rec * Rt + o;
                    w[d] = __builtin_amdgcn_alignbyte(W32[(x >> 2) + 1u], W32[x >> 2], x & 3u);
                    if (o + 4u > R) {                                       // the record's last 1 to 3 bytes, then the next record's first
                        const uint32_t keep = 8u * (R - o);                 // (R >= 15: a dword touches two records at most)
                        w[d] = (w[d] & ((1u << keep) - 1u)) | (W32[((rec + 1u) * Rt) >> 2] << keep);
                    }
                    o += 4u;
                    if (o >= R) { o -= R; rec++; }
                }
                store16_once(out + q, make_uint4(w[0], w[1], w[2], w[3]));
            } else {
                for (uint32_t k = q; k < span; k++) {
                    out[k] = W8[rec * Rt + o];
                    if (++o == R) { o = 0; rec++; }
                }
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");             // (the next round's LDS writes come behind these reads)
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
}

// the ASCII gather, from the source: hook 5, or a slab with a byte outside the alphabet
__global__ __launch_bounds__(256, 8) void gather_fixed_kernel(const char *__restrict__ b, uint64_t n, uint64_t n_rec, uint32_t L,
                                                              uint32_t P, uint32_t magic_p, uint32_t G, const uint32_t *__restrict__ perm,
                                                              uint8_t *__restrict__ dst, unsigned long long *__restrict__ not_fixed)
{
    extern __shared__ uint4 gx_lds[];       // 4 waves x G R bytes
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint64_t r0 = ((uint64_t)blockIdx.x * 4u + (uint32_t)wave) * 64u;
    // nothing to do once the slab is known not to be of one length: the general passes come next
    if (r0 >= n_rec || *(volatile unsigned long long *)not_fixed) return;
    const uint32_t L1 = L + 1u, nr = (uint32_t)min((uint64_t)64, n_rec - r0), slot = slot_of(L), R = slot;
    uint4 *W = gx_lds + (size_t)wave * (G * R / 16u);
    uint8_t *W8 = reinterpret_cast<uint8_t *>(W);
    const uint32_t mine = (uint32_t)lane < nr ? perm[r0 + lane] : 0u;      // source of the wave's output record `lane`
    bool bad = false;
    for (uint32_t c0 = 0; c0 < nr; c0 += G) {
        const uint32_t nc = min(G, nr - c0), total = nc * P;
        for (uint32_t p0 = 0; p0 < total; p0 += 64u * GPK) {                // (uniform trip count: every lane takes part in the shuffles)
            uint4 v[GPK];
#pragma unroll
            for (int r = 0; r < GPK; r++) {
                const uint32_t p = p0 + (uint32_t)lane + 64u * r, rec = min(__umulhi(p, magic_p), nc - 1u), off = (p - rec * P) * 16u;
                const uint32_t s = (uint32_t)__shfl((int)mine, (int)(c0 + rec), 64);
                v[r] = make_uint4(0x0A0A0A0Au, 0x0A0A0A0Au, 0x0A0A0A0Au, 0x0A0A0A0Au);
                if (p < total && L >= off) v[r] = load16_clamped(b, (uint64_t)s * L1 + off, n);  // (the piece of byte L is loaded too;
                                                                    // bytes behind byte L < n are neither checked nor kept)
            }
#pragma unroll
            for (int r = 0; r < GPK; r++) {
                const uint32_t p = p0 + (uint32_t)lane + 64u * r, rec = min(__umulhi(p, magic_p), nc - 1u), off = (p - rec * P) * 16u;
                if (p >= total) continue;
                uint32_t w[4] = {v[r].x, v[r].y, v[r].z, v[r].w};
                if (L >= off) {                                             // a newline at byte L, none before it
                    const uint32_t m = nl_mask16(v[r]), e = L - off;
                    const uint32_t want = e < 16u ? 1u << e : 0u, valid = e < 16u ? (2u << e) - 1u : 0xFFFFu;
                    bad |= ((m ^ want) & valid) != 0u;
                }
                pad_piece(w, L, off);
                uint64_t *q = reinterpret_cast<uint64_t *>(W8 + rec * R + off);      // (8-byte aligned: slots are multiples of 8)
                q[0] = (uint64_t)w[0] | ((uint64_t)w[1] << 32);
                if (off + 16u <= slot) q[1] = (uint64_t)w[2] | ((uint64_t)w[3] << 32);
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        // the round's span: nc R bytes at (r0 + c0) R -- 16-byte aligned, whole 16-byte stores but at the slab's very end
        const uint32_t span = nc * R;
        uint8_t *out = dst + (r0 + c0) * R;
        for (uint32_t q = (uint32_t)lane * 16u; q < span; q += 1024u) {
            if (q + 16u <= span) *reinterpret_cast<uint4 *>(__builtin_assume_aligned(out + q, 16)) = W[q >> 4];
            else for (uint32_t k = q; k < span; k++) out[k] = W8[k];
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");             // (the next round's LDS writes come behind these reads)
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
    if (__ballot(bad) && lane == 0 && !*(volatile unsigned long long *)not_fixed) atomicOr(not_fixed, 1ull);
}

// ---- exclusive prefix over the bin sizes (up to 4 M of them): block sums, their prefix, local prefixes ----------------------
constexpr int SCAN_PER = 4096;              // entries per workgroup of 1024 threads

__global__ __launch_bounds__(1024) void scan_sums_kernel(const unsigned long long *__restrict__ v, uint32_t n, unsigned long long *__restrict__ sums)
{
    __shared__ unsigned long long s_w[16];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const uint32_t i0 = blockIdx.x * SCAN_PER + (uint32_t)t * 4u;
    unsigned long long x = 0;
    for (uint32_t i = i0; i < min(n, i0 + 4u); i++) x += v[i];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) x += (unsigned long long)__shfl_xor((long long)x, off, 64);
    if (lane == 0) s_w[wave] = x;
    __syncthreads();
    if (t == 0) { unsigned long long r = 0; for (int w = 0; w < 16; w++) r += s_w[w]; sums[blockIdx.x] = r; }
}

__global__ __launch_bounds__(1024) void scan_top_kernel(unsigned long long *__restrict__ sums, uint32_t nb, unsigned long long *__restrict__ total)
{
    __shared__ unsigned long long s_part[1024];
    const int t = threadIdx.x;
    const uint32_t per = (nb + 1023u) / 1024u, a = min(nb, (uint32_t)t * per), e = min(nb, a + per);
    unsigned long long sum = 0;
    for (uint32_t i = a; i < e; i++) sum += sums[i];
    s_part[t] = sum;
    __syncthreads();
    if (t == 0) {
        unsigned long long run = 0;
        for (int i = 0; i < 1024; i++) { const unsigned long long v = s_part[i]; s_part[i] = run; run += v; }
        *total = run;
    }
    __syncthreads();
    unsigned long long run = s_part[t];
    for (uint32_t i = a; i < e; i++) { const unsigned long long v = sums[i]; sums[i] = run; run += v; }
}

__global__ __launch_bounds__(1024) void scan_apply_kernel(unsigned long long *__restrict__ v, uint32_t n, const unsigned long long *__restrict__ sums)
{
    __shared__ unsigned long long s_w[16];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const uint32_t i0 = blockIdx.x * SCAN_PER + (uint32_t)t * 4u;
    unsigned long long x[4], mine = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) { x[k] = i0 + k < n ? v[i0 + k] : 0ull; mine += x[k]; }
    unsigned long long incl = mine;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const unsigned long long o = (unsigned long long)__shfl_up((long long)incl, off, 64);
        if (lane >= off) incl += o;
    }
    if (lane == 63) s_w[wave] = incl;
    __syncthreads();
    unsigned long long run = sums[blockIdx.x] + incl - mine;
    for (int w = 0; w < wave; w++) run += s_w[w];
#pragma unroll
    for (int k = 0; k < 4; k++) { if (i0 + k < n) v[i0 + k] = run; run += x[k]; }
}

// bin width: about four records per bin for the block at hand (reads that share their first minimizer then sit in the
// same scan tile or the next), 12 bits at least, MAX_ORDER_BITS at most (4 M counters = 32 MB)
int order_bits(uint64_t n_bytes)
{
    int bits = 12;
    while (bits < MAX_ORDER_BITS && (n_bytes / 152) >> (bits + 2)) bits++;
    return bits;
}

}  // namespace

namespace ss {

static std::mutex g_scr_mu;
static uint64_t g_order_n[2] = {0, 0};        // slabs binned by the one-length passes / by the general ones (ss_reads_order_counters)
static double g_order_ms[3] = {0, 0, 0};      // the last order_flat_dev, as its path reported them (reorder_timing in ss_common.h)
static char *g_scr = nullptr;            // the scratch of the last call (bin cursors, per-tile record tables), kept for the next
static uint64_t g_scr_cap = 0;

std::atomic<long long> g_hook_ascii_slabs{0};      // ss_test_hook(5, ...): 1 = binned slabs of one length stay ASCII
std::atomic<long long> g_hook_atomic_binning{0};   // ss_test_hook(6, ...): 1 = slabs of one length go through the count + atomic placement

namespace {

// ---- order_flat_dev, step by step ------------------------------------------------------------------------------------------
// probe_one_length -> Scratch::take -> one of bin_sorted / bin_counted (slabs of one length; either may answer "not of one
// length after all") -> bin_general -> timing, counters, *out.  Every path takes its new slab through NewSlab::alloc and, but
// for the sorted one, its cursors through prefix_and_tail; nothing else is shared between them.
typedef std::chrono::steady_clock Clock;
inline double ms_between(Clock::time_point a, Clock::time_point b) { return std::chrono::duration<double, std::milli>(b - a).count(); }

enum class Binned { done, not_one_length, failed };
enum { T_TOTAL = 0, T_FLAG = 1, T_ALPHA = 2 };      // the tail words behind the bin sizes: positions of the new slab; tiles that did not
                                                    // fit the table (general) / "not of one length"; a byte other than A C G T N

inline bool hip_ok(hipError_t e, const char *what, int line)
{
    if (e != hipSuccess) ss::set_last_error(what, __FILE__, line, hipGetLastError());
    return e == hipSuccess;
}
#define SS_R(call) do { if (!hip_ok((call), #call, __LINE__)) return Binned::failed; } while (0)
struct Owner { Owner() = default; Owner(const Owner &) = delete; Owner &operator=(const Owner &) = delete; };      // of device memory, of events

// what a call knows before anything runs
struct Call {
    const char *src;
    uint64_t n;
    int bits;
    uint32_t n_bins;
    unsigned nb, nsb;                          // tiles of the general passes; workgroups of the prefix
    Clock::time_point t_begin = Clock::now();
    Call(const char *src_, uint64_t n_) : src(src_), n(n_), bits(order_bits(n_)), n_bins((1u << bits) + 1u), nb((unsigned)((n_ + RB - 1) / RB)),
                                          nsb((n_bins + SCAN_PER - 1) / SCAN_PER) {}
    void lap(const char *what) const
    {
        static const bool trace = getenv("SS_INGEST_TRACE") != nullptr;
        if (!trace) return;
        hipDeviceSynchronize();
        fprintf(stderr, "[reorder] %-22s at %.4f s\n", what, std::chrono::duration<double>(Clock::now() - t_begin).count());
    }
    // the end of a path that placed its records: everything has run
    hipError_t finish(Clock::time_point *t_end) const
    {
        hipError_t e = hipGetLastError();
        if (e == hipSuccess) e = hipDeviceSynchronize();
        lap("place");
        *t_end = Clock::now();
        return e;
    }
};

// records of one length: the first newline says which (L = 0: not a candidate); the passes check every record against it
struct OneLength { uint32_t L = 0; uint64_t n_rec = 0; };

hipError_t probe_one_length(const char *src, uint64_t n, OneLength *one)
{
    *one = OneLength();
    static const bool fixed_allowed = [] { const char *e = getenv("SS_ORDER_FIXED"); return !(e && !strcmp(e, "0")); }();
    if (!fixed_allowed || n < 64) return hipSuccess;
    char head[FIX_MAX_L + 2];
    const size_t hn = (size_t)std::min<uint64_t>(n, sizeof(head));
    const hipError_t e = hipMemcpy(head, src, hn, hipMemcpyDeviceToHost);
    if (e != hipSuccess) return e;
    const void *nl = memchr(head, '\n', hn);
    if (!nl) return hipSuccess;
    const uint32_t L = (uint32_t)((const char *)nl - head);
    // (fewer than 64 bytes behind the last record: what key_fixed_kernel's one lane checks for '\n')
    if (L >= FIX_MIN_L && L <= FIX_MAX_L && n / (L + 1) >= 1 && n - (n / (L + 1)) * (L + 1) < 64) { one->L = L; one->n_rec = n / (L + 1); }
    return hipSuccess;
}

// The file-order intermediate of the sorted path (pack_key_fixed_kernel writes it, gather_packed_kernel reads it): n_rec records
// at stride Rt.  A large packed slab takes a block of its ASCII size (NewSlab::get_block) and uses 3/8 of it: the intermediate
// lives in the unused tail of that block when it fits (150 bases: 1.14 + 1.28 GB in 3.04 GB), else -- every slab below
// BIG_KEEP_MIN, and the few lengths whose Rt is more than 5/8 of the slot (slot 48: R = 18, Rt = 32) -- in the call's scratch
// (which, grown for a large slab, is not kept for the next call); no intermediate under ss_test_hook 5 = 1.
// A function of n_rec and L alone, worked out here and nowhere else, before anything is allocated.
inline uint64_t slab_positions(uint64_t total) { return std::max<uint64_t>((total + 15) & ~15ull, 16); }
inline uint64_t packed_block_bytes(uint64_t cap) { return std::max<uint64_t>(ss::dev::in_bytes(true, cap) + 8, cap >= ss::BIG_KEEP_MIN ? cap : 0); }
struct PackPlan {
    uint64_t bytes = 0, slab_off = 0;          // of the intermediate; where it begins in the new slab's block (in_slab)
    bool in_slab = false, large = false;       // large: the slab takes a kept block (BIG_KEEP_MIN and more)
    uint64_t scratch_bytes() const { return in_slab ? 0 : bytes; }
    explicit PackPlan(const OneLength &one)
    {
        if (!one.L) return;
        const uint64_t cap = slab_positions(one.n_rec * ::slot_of(one.L));
        bytes = one.n_rec * packed_stride(::slot_of(one.L));
        slab_off = (ss::dev::in_bytes(true, cap) + 8 + 255) & ~255ull;
        in_slab = slab_off + bytes <= packed_block_bytes(cap);
        large = cap >= ss::BIG_KEEP_MIN;
    }
};

// The scratch of a call, one allocation: bin sizes / cursors + the three tail words, block sums of the prefix, per-tile record
// counts, and a region that is the record table of the general passes, or the 4-byte bins of the count + atomic placement, or
// the sort's keys, values (twice each) and temporary storage, and behind them the file-order intermediate where the new slab's
// block does not hold it (PackPlan) -- sized for whichever of those the call may come to use.
// The scratch of the call before is kept (0.35 GB for 20 M reads: two driver calls fewer per sample); keep() hands the larger
// of the two blocks on to the next call.  A call that fails frees its block.
class Scratch : Owner {
public:
    struct Sort { uint32_t *k0, *k1, *v0, *v1; void *temp; size_t temp_bytes; };
    ~Scratch() { if (d_) hipFree(d_); }

    hipError_t take(const Call &c, const OneLength &one, bool for_sort, uint64_t inter_bytes, bool inter_of_large_slab)
    {
        n_bins_ = c.n_bins;
        if (for_sort) {
            hipcub::DoubleBuffer<uint32_t> k(nullptr, nullptr), v(nullptr, nullptr);
            const hipError_t e = hipcub::DeviceRadixSort::SortPairs(nullptr, sort_tb_, k, v, (int)one.n_rec, 0, c.bits + 1);
            if (e != hipSuccess) return e;
        }
        a4_ = (one.n_rec * 4 + 255) & ~255ull;
        o_sums_ = ((uint64_t)c.n_bins + 3) * 8;
        o_cnt_ = o_sums_ + ((uint64_t)c.nsb + 1) * 8;
        o_region_ = (o_cnt_ + (uint64_t)c.nb * 4 + 255) & ~255ull;
        o_inter_ = o_region_ + 4 * a4_ + ((sort_tb_ + 255) & ~255ull);
        const uint64_t bytes = std::max<uint64_t>(o_region_ + std::max<uint64_t>((uint64_t)c.nb * TCAP * 8, a4_), for_sort ? o_inter_ + inter_bytes : 0);
        // a LARGE slab's intermediate that does not fit its block (PackPlan) makes this block 0.64 GB per 20 M reads, for one call:
        // it is not handed on (a slab below BIG_KEEP_MIN adds 171 MB at most, to a block that is kept as before)
        transient_ = for_sort && inter_bytes && inter_of_large_slab;
        {
            std::lock_guard<std::mutex> g(g_scr_mu);
            if (g_scr && g_scr_cap >= bytes) { d_ = g_scr; cap_ = g_scr_cap; g_scr = nullptr; g_scr_cap = 0; }
        }
        if (d_) return hipSuccess;
        cap_ = bytes;
        return hipMalloc((void **)&d_, bytes);
    }
    void keep()
    {
        if (!transient_) {
            std::lock_guard<std::mutex> g(g_scr_mu);
            if (!g_scr || g_scr_cap < cap_) { std::swap(g_scr, d_); std::swap(g_scr_cap, cap_); }
        }
        if (d_) hipFree(d_);
        d_ = nullptr;
    }

    unsigned long long *hist() const { return (unsigned long long *)d_; }             // n_bins bin sizes, then cursors
    unsigned long long *tail() const { return hist() + n_bins_; }                      // T_TOTAL, T_FLAG, T_ALPHA
    uint64_t hist_bytes() const { return o_sums_; }                                    // ... what a count pass zeroes: both
    unsigned long long *sums() const { return (unsigned long long *)(d_ + o_sums_); }
    uint32_t *tile_counts() const { return (uint32_t *)(d_ + o_cnt_); }
    unsigned long long *table() const { return (unsigned long long *)(d_ + o_region_); }
    uint32_t *bins() const { return (uint32_t *)(d_ + o_region_); }
    Sort sort() const
    {
        uint32_t *a = (uint32_t *)(d_ + o_region_);
        return Sort{a, a + a4_ / 4, a + 2 * (a4_ / 4), a + 3 * (a4_ / 4), d_ + o_region_ + 4 * a4_, sort_tb_};
    }
    uint8_t *intermediate() const { return (uint8_t *)(d_ + o_inter_); }               // (a sorting call whose plan is not in_slab)

private:
    char *d_ = nullptr;
    uint64_t cap_ = 0, o_sums_ = 0, o_cnt_ = 0, o_region_ = 0, o_inter_ = 0, a4_ = 0;       // a4_: one per-record array of 4-byte entries
    uint32_t n_bins_ = 0;
    size_t sort_tb_ = 0;
    bool transient_ = false;
};

// The new slab: `total` positions of records, `cap` positions in all (a multiple of 16), in a block of real_cap bytes (a kept
// block may be larger).  Freed unless a path hands it out (release) or back (put_back).
struct NewSlab : Owner {
    char *d = nullptr;
    uint64_t total = 0, cap = 0, real_cap = 0;
    bool packed = false;
    Clock::time_point t_alloc;
    ~NewSlab() { if (d) hipFree(d); }

    hipError_t alloc(const Call &c, bool pk, uint64_t total_)
    {
        total = total_; packed = pk;
        cap = slab_positions(total);
        const hipError_t e = get_block();
        t_alloc = Clock::now();
        c.lap("new slab");
        return e;
    }
    // the packed gather met a byte other than A C G T N: an ASCII slab instead, in this block if it holds one
    hipError_t make_ascii()
    {
        packed = false;
        if (real_cap >= cap) return hipSuccess;
        put_back();
        return get_block();
    }
    // behind the records: packed, '\n' (code 1, invalid) up to the 16-position boundary -- at most one 3-byte unit (slots are
    // multiples of 8) --, then the slack behind the last group (not the rest of a larger block); ASCII, '\n' up to the boundary
    hipError_t fill_tail() const
    {
        hipError_t e = hipSuccess;
        if (packed) {
            const uint64_t t0 = total / 8u * 3u, t1 = ss::dev::in_bytes(true, cap) + 8;
            e = hipMemsetAsync(d + t0, 0xFF, t1 - t0, 0);
            if (e == hipSuccess && cap > total) e = hipMemsetAsync(d + t0, 0x55, 2, 0);
        } else if (cap > total) {
            e = hipMemsetAsync(d + total, '\n', cap - total, 0);
        }
        return e;
    }
    void put_back() { ss::big_put(d, real_cap); d = nullptr; }
    char *release() { char *p = d; d = nullptr; return p; }

private:
    // packed: 6 bytes per 16 positions, and 8 bytes behind them that the scans' 8-byte loads may touch (IN_PACKED).  A slab whose
    // ASCII form would be a block the process keeps (ss::big_put) still takes a block of that size: destroyed, it goes back to
    // the kept blocks and must serve what comes next -- the next sample's file-order slab, or its binning -- which a block of the
    // packed size cannot (a fresh 3 GB from the driver: ~60 ms against 0.02).  The bytes written and scanned are the packed ones;
    // the sorted path keeps its file-order intermediate in the rest while it runs (PackPlan).
    hipError_t get_block()
    {
        const uint64_t bytes = packed ? packed_block_bytes(cap) : cap;
        return ss::big_malloc((void **)&d, bytes, &real_cap);
    }
};

struct EventPair : Owner {
    hipEvent_t ev[2] = {nullptr, nullptr};
    ~EventPair() { for (hipEvent_t e : ev) if (e) hipEventDestroy(e); }
    hipError_t create() { const hipError_t e = hipEventCreate(&ev[0]); return e == hipSuccess ? hipEventCreate(&ev[1]) : e; }
};

// bin sizes -> exclusive prefix (the bins' cursors) -> the first n_tail tail words on the host
hipError_t prefix_and_tail(const Call &c, const Scratch &scr, unsigned long long *tail, int n_tail)
{
    hipLaunchKernelGGL(scan_sums_kernel, dim3(c.nsb), dim3(1024), 0, 0, scr.hist(), c.n_bins, scr.sums());
    hipLaunchKernelGGL(scan_top_kernel, dim3(1), dim3(1024), 0, 0, scr.sums(), c.nsb, scr.tail());
    hipLaunchKernelGGL(scan_apply_kernel, dim3(c.nsb), dim3(1024), 0, 0, scr.hist(), c.n_bins, scr.sums());
    return hipMemcpy(tail, scr.tail(), 8 * (size_t)n_tail, hipMemcpyDeviceToHost);
}

// the figures of a path that counts, allocates and places (ss_reads_order_timing): from the call's start, so a one-length
// attempt that failed before is in the first
hipError_t finish_counted(const Call &c, Clock::time_point t_counted, const NewSlab &slab, double ms[3])
{
    Clock::time_point t_end;
    const hipError_t e = c.finish(&t_end);
    ms[0] = ms_between(c.t_begin, t_counted); ms[1] = ms_between(t_counted, slab.t_alloc); ms[2] = ms_between(slab.t_alloc, t_end);
    return e;
}

// One length, sorted: the new slab's size is known before anything runs (n_rec slots), so its block is taken first, and the
// flags are read once, after the gather.  Packed slab wanted: pack + key, sort, packed gather; a byte outside the alphabet (seen
// by the pack pass): the ASCII gather from the source, in the same order, and a second look at the layout flag.  ss_test_hook
// 5 = 1: key, sort, ASCII gather.  Figures: pack / key + sort (on the device), allocation (from the call's start), gather +
// tail -- the first and the last add up to the kernels' wall time.
Binned bin_sorted(const Call &c, const OneLength &one, bool want_packed, const PackPlan &plan, const Scratch &scr, NewSlab &slab, double ms[3])
{
    const uint32_t slot = ::slot_of(one.L), P = (slot + 15u) >> 4, magic_p = (uint32_t)(((1ull << 32) + P - 1) / P);
    const unsigned nbf = (unsigned)((one.n_rec + 255) / 256);
    SS_R(slab.alloc(c, want_packed, one.n_rec * slot));
    const Scratch::Sort s = scr.sort();
    unsigned long long *flags = scr.tail();
    EventPair t;
    SS_R(t.create());
    auto gather_ascii = [&](const uint32_t *perm) {
        const uint32_t G = gather_rows(false, one.L);
        hipLaunchKernelGGL(gather_fixed_kernel, dim3(nbf), dim3(256), 4u * G * slot, 0, c.src, c.n, one.n_rec, one.L, P, magic_p, G, perm,
                           (uint8_t *)slab.d, flags + T_FLAG);
    };
    const bool packing = slab.packed;
    uint8_t *inter = !packing ? nullptr : plan.in_slab ? (uint8_t *)slab.d + plan.slab_off : scr.intermediate();
    unsigned long long tail[3] = {0, 0, 0};
    SS_R(hipMemsetAsync(flags, 0, 24, 0));
    SS_R(hipEventRecord(t.ev[0], 0));
    if (packing) {
        const uint32_t G = pack_rows(one.L);
        hipLaunchKernelGGL(pack_key_fixed_kernel, dim3(nbf), dim3(256), 4u * G * packed_stride(slot), 0, c.src, c.n, one.n_rec, one.L, P, magic_p, G,
                           c.bits, s.k0, s.v0, inter, flags + T_FLAG, flags + T_ALPHA);
    } else {
        hipLaunchKernelGGL(key_fixed_kernel, dim3(nbf), dim3(256), 0, 0, c.src, c.n, one.n_rec, one.L, c.bits, s.k0, s.v0, flags + T_FLAG);
    }
    hipcub::DoubleBuffer<uint32_t> dk(s.k0, s.k1), dv(s.v0, s.v1);
    size_t temp_bytes = s.temp_bytes;
    SS_R(hipcub::DeviceRadixSort::SortPairs(s.temp, temp_bytes, dk, dv, (int)one.n_rec, 0, c.bits + 1, 0));
    SS_R(hipEventRecord(t.ev[1], 0));
    const uint32_t *perm = dv.Current();
    if (packing) {
        const uint32_t G = gather_rows(true, one.L), R = packed_row(slot), Q = packed_stride(slot) / 16u;
        hipLaunchKernelGGL(gather_packed_kernel, dim3(nbf), dim3(256), 4u * (G * Q + 1u) * 16u, 0, inter, one.n_rec, R, (uint32_t)(((1ull << 32) + R - 1) / R),
                           Q, (uint32_t)(((1ull << 32) + Q - 1) / Q), G, perm, (uint8_t *)slab.d, flags + T_FLAG, flags + T_ALPHA);
    } else {
        gather_ascii(perm);
    }
    SS_R(slab.fill_tail());
    SS_R(hipMemcpy(tail + T_FLAG, flags + T_FLAG, 16, hipMemcpyDeviceToHost));
    if (tail[T_FLAG] == 0 && packing && tail[T_ALPHA]) {            // a byte other than A C G T N: the same order, ASCII
        SS_R(slab.make_ascii());
        gather_ascii(perm);
        SS_R(slab.fill_tail());
        // (the pack pass's waves stop checking once the slab is known not packable: the layout is checked by the ASCII gather)
        SS_R(hipMemcpy(tail + T_FLAG, flags + T_FLAG, 8, hipMemcpyDeviceToHost));
    }
    SS_R(hipGetLastError());
    if (tail[T_FLAG]) { slab.put_back(); return Binned::not_one_length; }       // some record is shorter or longer after all
    float ms_key_sort = -1.f;
    SS_R(hipEventElapsedTime(&ms_key_sort, t.ev[0], t.ev[1]));
    Clock::time_point t_end;
    SS_R(c.finish(&t_end));
    ms[0] = ms_key_sort; ms[1] = ms_between(c.t_begin, slab.t_alloc); ms[2] = ms_between(slab.t_alloc, t_end) - ms_key_sort;
    return Binned::done;
}

// One length, ss_test_hook 6: the count + atomic placement (count_fixed checks the layout and the alphabet)
Binned bin_counted(const Call &c, const OneLength &one, const Scratch &scr, NewSlab &slab, double ms[3])
{
    const uint32_t L1 = one.L + 1u, slot = ::slot_of(one.L), P = (slot + 15u) >> 4;
    const unsigned nbf = (unsigned)((one.n_rec + 255) / 256);
    unsigned long long tail[3] = {0, 0, 0};
    SS_R(hipMemsetAsync(scr.hist(), 0, scr.hist_bytes(), 0));
    hipLaunchKernelGGL(count_fixed_kernel, dim3(nbf), dim3(256), 0, 0, c.src, c.n, one.n_rec, one.L, (uint32_t)(((1ull << 32) + L1 - 1) / L1), c.bits,
                       scr.hist(), scr.bins(), scr.tail() + T_FLAG, scr.tail() + T_ALPHA);
    SS_R(prefix_and_tail(c, scr, tail, 3));
    if (tail[T_FLAG]) return Binned::not_one_length;                 // some record is shorter or longer after all
    c.lap("count + prefix");
    const Clock::time_point t_counted = Clock::now();
    SS_R(slab.alloc(c, tail[T_ALPHA] == 0 && g_hook_ascii_slabs.load() == 0, tail[T_TOTAL]));
    if (slab.packed) {
        // a record's LDS area: 4 bytes in front (a span's first dword may begin before it), its groups, 4 behind
        const uint32_t B = slot / 8u * 3u, A = (6u * P + 8u + 3u) & ~3u;
        const uint32_t G = std::min<uint32_t>(64u, PK_LDS / A), ND = ((B + 2u) >> 2) + 1u;      // records per round; dwords a span touches
        hipLaunchKernelGGL(place_fixed_packed_kernel, dim3(nbf), dim3(256), 0, 0, c.src, c.n, one.n_rec, one.L, P, (uint32_t)(((1ull << 32) + P - 1) / P),
                           A, G, ND, (uint32_t)(((1ull << 32) + ND - 1) / ND), scr.hist(), (const uint32_t *)scr.bins(), (uint8_t *)slab.d);
    } else {
        hipLaunchKernelGGL(place_fixed_kernel, dim3(nbf), dim3(256), 0, 0, c.src, c.n, one.n_rec, one.L, (uint32_t)(((1ull << 32) + P - 1) / P),
                           scr.hist(), (const uint32_t *)scr.bins(), slab.d);
    }
    SS_R(slab.fill_tail());
    SS_R(finish_counted(c, t_counted, slab, ms));
    return Binned::done;
}

// The general passes: ragged records, or a slab that was not of one length after all
Binned bin_general(const Call &c, const Scratch &scr, NewSlab &slab, double ms[3])
{
    unsigned long long tail[2] = {0, 0};
    SS_R(hipMemsetAsync(scr.hist(), 0, scr.hist_bytes(), 0));
    hipLaunchKernelGGL(count_kernel, dim3(c.nb), dim3(256), 0, 0, c.src, c.n, c.bits, scr.hist(), scr.tile_counts(), scr.table(), scr.tail() + T_FLAG);
    SS_R(prefix_and_tail(c, scr, tail, 2));
    c.lap("count + prefix");
    const Clock::time_point t_counted = Clock::now();
    SS_R(slab.alloc(c, false, tail[T_TOTAL]));
    hipLaunchKernelGGL(place_kernel, dim3(c.nb), dim3(256), 0, 0, c.src, c.n, scr.hist(), scr.tile_counts(), scr.table(), slab.d);
    if (tail[T_FLAG]) hipLaunchKernelGGL(place_again_kernel, dim3(c.nb), dim3(256), 0, 0, c.src, c.n, c.bits, scr.hist(), scr.tile_counts(), slab.d);
    SS_R(slab.fill_tail());
    SS_R(finish_counted(c, t_counted, slab, ms));
    return Binned::done;
}
#undef SS_R

}  // namespace

// src[0, n) (a flat base block on the device) -> a new slab with the records binned: out->d (hipMalloc'ed or a kept block),
// out->cap; an ASCII slab of out->used bytes (a multiple of 16, '\n' padded), or -- records of one length, every byte of them
// A C G T N -- a packed one of out->n_pos positions (the same multiple of 16) in out->used bytes.
int order_flat_dev(const char *src, uint64_t n, ss_reads::Slab *out)
{
    *out = ss_reads::Slab();
    const Call c(src, n);
    OneLength one;
    if (!hip_ok(probe_one_length(src, n, &one), "hipMemcpy", __LINE__)) return SS_EHIP;
    // the sorted one-length path (ss_test_hook 6 = 1: the count + atomic placement instead); hipcub counts its items in an int
    const bool sorted = one.L && g_hook_atomic_binning.load() == 0 && one.n_rec < (1ull << 31);
    const bool want_packed = g_hook_ascii_slabs.load() == 0;       // (ss_test_hook 5 = 1: no pack pass, no intermediate)
    const PackPlan plan(one);
    Scratch scr;
    if (!hip_ok(scr.take(c, one, sorted, sorted && want_packed ? plan.scratch_bytes() : 0, plan.large), "Scratch::take", __LINE__)) return SS_EHIP;
    NewSlab slab;
    double ms[3] = {0, 0, 0};
    Binned r = Binned::not_one_length;
    if (one.L) r = sorted ? bin_sorted(c, one, want_packed, plan, scr, slab, ms) : bin_counted(c, one, scr, slab, ms);
    const bool fixed = r == Binned::done;
    if (r == Binned::not_one_length) r = bin_general(c, scr, slab, ms);
    if (r != Binned::done) return SS_EHIP;
    {
        // where the call's time went (ss_reads_order_timing): the driver's allocation of the new slab is not the kernels' time,
        // and on some boxes a fresh 3 GB allocation takes 60-90 ms
        std::lock_guard<std::mutex> g(g_scr_mu);
        for (int i = 0; i < 3; i++) g_order_ms[i] = ms[i];
        g_order_n[fixed ? 0 : 1]++;
    }
    scr.keep();
    out->cap = slab.real_cap; out->binned = true;
    out->used = slab.packed ? ss::dev::in_bytes(true, slab.cap) : slab.cap;
    if (slab.packed) { out->packed = true; out->n_pos = slab.cap; out->L = one.L; out->slot = ::slot_of(one.L); }
    out->d = slab.release();
    return SS_OK;
}

void reorder_timing(double out[3])
{
    std::lock_guard<std::mutex> g(g_scr_mu);
    for (int i = 0; i < 3; i++) out[i] = g_order_ms[i];
}

void reorder_counters(uint64_t out[2])
{
    std::lock_guard<std::mutex> g(g_scr_mu);
    out[0] = g_order_n[0]; out[1] = g_order_n[1];
}

void reorder_release()
{
    char *d = nullptr;
    {
        std::lock_guard<std::mutex> g(g_scr_mu);
        std::swap(d, g_scr);
        g_scr_cap = 0;
    }
    if (d) hipFree(d);
}

// Policy: ALWAYS, unless SS_READS_ORDER=file.  Binning 20 M one-length reads costs ~2.2 ms of kernel time once per sample
// (sorted path: pack + key 1.0, sort 0.5, packed gather 0.7; ragged reads ~3.6); a tree scan of
// the binned set is 1.8 ms faster than in file order on sampled node sets (5.6 -> 3.8 ms), 0.7 ms on contiguous ones, a
// cluster scan 6 ms (16.8 -> 10.6: the hits of a locus' reads are added up in LDS).  So it pays from the SECOND scan of a sample
// on -- the tree scan + one cluster's scan, or the two scans of -b -- and a sample that is scanned exactly once (every
// identified cluster single-strain) loses ~0.4 ms per 20 M one-length reads, beside ~80 ms of text ingest for the same reads.  The
// loader cannot know which it will be: the clusters are identified by the first scan.
bool reads_order_wanted()
{
    const char *e = getenv("SS_READS_ORDER");
    return !(e && (!strcmp(e, "file") || !strcmp(e, "0") || !strcmp(e, "off")));
}

int reads_order_for_locality(ss_reads *R, bool force)
{
    if (!R) return SS_EINVAL;
    if (!force && !reads_order_wanted()) return SS_OK;
    uint64_t bytes = 0;
    // (asked ONCE: the driver takes ~1 ms to answer, as long as the binning of a 1 M-read file; every slab replaces one of about its size)
    size_t mem_free = 0, mem_total = 0;
    const bool known = hipMemGetInfo(&mem_free, &mem_total) == hipSuccess;
    for (auto &sl : R->slabs) {
        // (the binned copy lives beside the slab until it replaces it: a slab that leaves no room for that stays in file order)
        const bool room = known && mem_free > sl.used + sl.used / 8 + (1ull << 30);
        if (sl.used >= 64 && (room || force)) {
            ss_reads::Slab nsl;
            const int rc = order_flat_dev(sl.d, sl.used, &nsl);
            if (rc) return rc;
            ss::big_put(sl.d, sl.cap);                    // (kept for the next slab's binned copy)
            sl = nsl;
        }
        bytes += sl.cap;
    }
    R->device_bytes = bytes;
    return SS_OK;
}

}  // namespace ss
