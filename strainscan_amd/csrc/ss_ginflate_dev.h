// The device code of the gunzip (ss_ginflate.hip, which alone includes this and launches the kernels): bit reader, Huffman
// tables, block_begin / block_body and the kernels sync, subsync, inflate, tails, group_maps, group_windows, windows, bytes,
// lastwin, crc_members, count_nl.  Everything is in the anonymous namespace of that one translation unit.
#pragma once
#include "ss_ginflate.h"
#include "ss_scan_dev.h"

namespace {

using ss::WSIZE;
using ss::dev::wave_inclusive_sum;
constexpr uint16_t UNRES = 0x8000;          // symbol = UNRES | index into the 32 KB in front of the chunk
constexpr int RING = 2048;                  // most recent symbols of a wave, in LDS
constexpr int LITBITS = 9;                  // bits of the literal/length code's direct table
constexpr int STAGE = 1024;                 // compressed bytes staged in LDS at a time (two halves); LDS decides the waves per SIMD
constexpr uint32_t STAGE_DW = STAGE / 4, HALF_DW = STAGE_DW / 2, STAGE_MASK = STAGE_DW - 1;
static_assert(STAGE == 1024 || STAGE == 2048, "a half is filled by one 8- or 16-byte load per lane");

// length code li = symbol - 257 and distance code ds -> base value and extra bits (RFC 1951 3.2.5), computed: a table
// lookup with a data-dependent index is a memory (or LDS) round trip in the middle of a dependent chain
__device__ __forceinline__ void len_code(int li, uint32_t &base, int &extra)
{
    extra = li < 8 || li == 28 ? 0 : (li >> 2) - 1;
    base = li < 8 ? 3u + (uint32_t)li : li == 28 ? 258u : 3u + ((4u + ((uint32_t)li & 3u)) << extra);
}
__device__ __forceinline__ void dist_code(int ds, uint32_t &base, int &extra)
{
    extra = ds < 4 ? 0 : (ds >> 1) - 1;
    base = ds < 4 ? 1u + (uint32_t)ds : 1u + ((2u + ((uint32_t)ds & 1u)) << extra);
}
__constant__ uint8_t c_cl_order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};

// ---- the per-lane header check ------------------------------------------------------------------------------------
// Could a NON-FINAL DYNAMIC block header start at bit `p`?  One unaligned 16-byte load per lane (the header bits and the
// code-length code's lengths: 17 + at most 57 bits), a 64-byte table in LDS: block type, HLIT / HDIST in range, and the
// code-length code complete (zlib insists on that).  About one position in 2000 passes; those are then parsed and
// decoded by the whole wave (read_dynamic + inflate_block), which is the real test.
__device__ __forceinline__ uint4 header_bytes(const uint8_t *in, uint64_t p)
{
    uint4 v;
    __builtin_memcpy(&v, in + (p >> 3), 16);
    return v;
}
// The Kraft sum is taken two fields at a time from a 64-entry table in LDS (kraft2[a | b << 3] = the weights of the lengths a and
// b, 128 >> l for l > 0): ten look-ups instead of a loop of up to 19 steps that a wave runs as long as its longest lane (nearly
// always 19; round 5: sync_kernel 7.3 -> 6.4 ms per 410 MB file, the same candidates).  The fields beyond HCLEN are masked off first.
__device__ __forceinline__ bool header_prefilter_lut(const uint4 v, uint64_t p, const uint8_t *kraft2)
{
    uint64_t lo = (uint64_t)v.x | (uint64_t)v.y << 32, hi = (uint64_t)v.z | (uint64_t)v.w << 32;
    const int sh = (int)(p & 7);
    if (sh) { lo = (lo >> sh) | (hi << (64 - sh)); hi >>= sh; }
    if ((lo & 7u) != 4u) return false;
    const uint32_t hlit = (uint32_t)(lo >> 3) & 31u, hdist = (uint32_t)(lo >> 8) & 31u, hclen = ((uint32_t)(lo >> 13) & 15u) + 4u;
    if (hlit > 29u || hdist > 29u) return false;
    uint64_t w = (lo >> 17) | (hi << 47);                        // the 3-bit lengths, 57 bits at most
    w &= (1ull << (3u * hclen)) - 1ull;                          // (3 * 19 = 57 < 64)
    uint32_t kraft = 0;
#pragma unroll
    for (int i = 0; i < 10; i++) kraft += kraft2[(uint32_t)(w >> (6 * i)) & 63u];
    return kraft == 128u;
}

// ---- per-wave decoder state: tables, ring and staging in LDS -------------------------------------------------------------
template <int PB, int MAXSYM>
struct LHuff {
    uint16_t tent[1 << PB];          // symbol | code length << 9 for every PB-bit pattern; 0 = code longer than PB bits
    // canonical code, for the codes longer than PB bits: ub[l] = the end of the length-l codes among the 15-bit left-justified
    // code values (they are sorted by length: a code's length is the number of ub[] it has reached), delta[l] = where the
    // length-l symbols start in sorted[] minus the first length-l code
    uint16_t ub[16];
    int16_t delta[16];
    uint16_t sorted[MAXSYM];
    int maxlen;
};
struct WaveState {
    union {                              // the code-length code is dead when the literal/length code is built from what it decoded
        LHuff<LITBITS, 288> lit;
        LHuff<7, 19> clc;
    };
    LHuff<8, 32> dist;
    alignas(16) uint8_t lens[320];       // (code lengths while a header is read; 64 words of scratch while a block's items are decoded)
    alignas(16) uint16_t ring[RING];
    alignas(16) uint32_t stage[STAGE / 4];
};

// Bit positions over the LDS stage (STAGE_DW dwords = two halves; the wave refills a half with one load per lane when the
// position has left it).  `bp` is the absolute bit position of the next unread bit; the block loop below lets the 64
// lanes decode at bp + lane, the headers are read through a small scalar cache (buf / cnt) of the bits at bp.
// Everything here is called wave-uniformly; LDS operations of one wave execute in order, so no barrier is needed
// between the lanes' stores and the loads that follow.
// Positions are RELATIVE to `base` (a bit position of the file, a multiple of a stage's bits, at or below everything the
// wave will look at) and 32 bits wide (round 4): the window loop compares the position with four limits per window, and
// 64-bit scalars can only be compared on the VALU (no s_cmp_lt_u64) and cost two SGPRs each -- the loop restored ~30 of them
// from spill lanes per window.  A wave stays within ~512 MB of its base (SB_CAP); beyond, the position is "past the end".
constexpr uint32_t SB_CAP = 0xFFF00000u, SB_NEVER = 0xFFFFFFFFu;
struct SBits {
    const uint32_t *in;      // global, dword aligned, padded with zeros behind the data: the dword of relative position 0
    uint64_t base;           // the file's bit position of relative position 0
    uint32_t nbits;          // bits of data from `base` on (capped)
    uint32_t bp;             // next bit
    uint32_t staged_to;      // dword index up to which the stage holds data: it covers [staged_to - STAGE_DW, staged_to)
    uint64_t buf;            // scalar cache: cnt bits from bp on
    int cnt;
};
__device__ __forceinline__ void sb_fill_half(WaveState &S, const SBits &b, uint32_t w0)
{
    // dwords [w0, w0 + HALF_DW) -> stage; w0 is a multiple of HALF_DW
    const int lane = threadIdx.x & 63;
    if constexpr (HALF_DW == 256) {
        const uint4 v = *reinterpret_cast<const uint4 *>(b.in + w0 + (uint64_t)lane * 4);
        *reinterpret_cast<uint4 *>(&S.stage[(w0 & STAGE_MASK) + lane * 4]) = v;
    } else {
        const uint2 v = *reinterpret_cast<const uint2 *>(b.in + w0 + (uint64_t)lane * 2);
        *reinterpret_cast<uint2 *>(&S.stage[(w0 & STAGE_MASK) + lane * 2]) = v;
    }
    __builtin_amdgcn_wave_barrier();
}
// the dwords [bp >> 5, (bp >> 5) + HALF_DW) are in the stage afterwards (a start, a jump or a step back reloads both halves;
// the sync search tries positions a few bits apart and finds its data still there)
__device__ __forceinline__ void sb_stage(WaveState &S, SBits &b)
{
    const uint32_t w = b.bp >> 5;
    if (w >= b.staged_to || w + STAGE_DW < b.staged_to) {
        const uint32_t h0 = w & ~(uint32_t)(HALF_DW - 1);
        __builtin_amdgcn_wave_barrier();
        sb_fill_half(S, b, h0);
        sb_fill_half(S, b, h0 + HALF_DW);
        b.staged_to = h0 + STAGE_DW;
    } else {
        while (w + HALF_DW >= b.staged_to) {     // the half behind the position is refilled with the data behind the other one
            sb_fill_half(S, b, b.staged_to);
            b.staged_to += HALF_DW;
        }
    }
}
// `bitpos`: where the wave starts; `lowest`: the lowest position it will ever seek to (a chunk that begins inside a block
// goes back to that block's header first)
__device__ __forceinline__ void sb_init(SBits &b, const uint8_t *p, uint64_t n, uint64_t bitpos, uint64_t lowest = ~0ull)
{
    const uint64_t base_dw = (min(bitpos, lowest) >> 5) & ~(uint64_t)(STAGE_DW - 1);
    b.in = reinterpret_cast<const uint32_t *>(p) + base_dw;
    b.base = base_dw << 5;
    const uint64_t total = n * 8;
    b.nbits = total <= b.base ? 0u : (uint32_t)min(total - b.base, (uint64_t)SB_CAP);
    b.bp = (uint32_t)min(bitpos - b.base, (uint64_t)SB_NEVER - 1);
    b.staged_to = 0; b.buf = 0; b.cnt = 0;
}
__device__ __forceinline__ void sb_seek(SBits &b, uint32_t rel) { b.bp = rel; b.cnt = 0; }                      // relative
// a position of the file -> relative (SB_NEVER: none, or out of this wave's reach)
__device__ __forceinline__ uint32_t sb_rel(const SBits &b, uint64_t bitpos)
{
    return (bitpos == ~0ull || bitpos - b.base >= (uint64_t)SB_CAP) ? SB_NEVER : (uint32_t)(bitpos - b.base);
}
__device__ __forceinline__ void sb_seek_abs(SBits &b, uint64_t bitpos) { sb_seek(b, sb_rel(b, bitpos)); }
// scalar cache: at least 33 bits from bp on.  Every lane reads the same words: telling the compiler so (readfirstlane)
// keeps the header logic on the scalar unit
__device__ __forceinline__ void sb_load(WaveState &S, SBits &b)
{
    sb_stage(S, b);
    const uint32_t w = b.bp >> 5;
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)S.stage[w & STAGE_MASK]);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)S.stage[(w + 1) & STAGE_MASK]);
    const int sh = (int)(b.bp & 31);
    b.buf = (((uint64_t)hi << 32) | lo) >> sh;
    b.cnt = 64 - sh;
}
__device__ __forceinline__ void sb_need(WaveState &S, SBits &b, int k) { if (b.cnt < k) sb_load(S, b); }      // k <= 33
__device__ __forceinline__ uint32_t sb_peek(SBits &b, int k) { return (uint32_t)(b.buf & ((1ull << k) - 1)); }
__device__ __forceinline__ void sb_drop(SBits &b, int k) { b.buf >>= k; b.cnt -= k; b.bp += (uint32_t)k; }
__device__ __forceinline__ uint32_t sb_get(WaveState &S, SBits &b, int k)      // k <= 32
{
    sb_need(S, b, k);
    const uint32_t v = sb_peek(b, k);
    sb_drop(b, k);
    return v;
}
__device__ __forceinline__ uint64_t sb_bitpos(const SBits &b) { return b.base + b.bp; }                         // of the file
__device__ __forceinline__ bool sb_past_end(const SBits &b) { return b.bp > b.nbits; }

// canonical code from the lengths lens[0 .. n) (LDS): 0 complete, 1 incomplete, -1 over-subscribed (nothing built).
// The 64 lanes hold the lengths of symbols lane, lane + 64, ...; a ballot per code length counts the codes and ranks a
// lane's symbol among those of its length, so the Kraft sum rejects a wrong header (the sync search sees ~80 per chunk)
// before any table is written.
template <int PB, int MAXSYM, int MAXLEN = 15>
__device__ int huff_build(LHuff<PB, MAXSYM> &h, const uint8_t *lens, int n)
{
    constexpr int NS = (MAXSYM + 63) / 64;
    const int lane = threadIdx.x & 63;
    __syncthreads();
    int ls[NS];
#pragma unroll
    for (int s = 0; s < NS; s++) ls[s] = lane + 64 * s < n ? (int)lens[lane + 64 * s] : 0;
    uint32_t cnt[16];
    cnt[0] = 0;
#pragma unroll
    for (int l = 1; l <= MAXLEN; l++) {
        uint32_t c = 0;
#pragma unroll
        for (int s = 0; s < NS; s++) c += (uint32_t)__popcll(__ballot(ls[s] == l));
        cnt[l] = c;
    }
    int left = 1, maxlen = 0;
    bool over = false;
#pragma unroll
    for (int l = 1; l <= MAXLEN; l++) {
        left = 2 * left - (int)cnt[l];
        over = over || left < 0;
        if (cnt[l]) maxlen = l;
    }
    if (over) return -1;
    for (int e = lane; e < (1 << PB); e += 64) h.tent[e] = 0;
    __syncthreads();
    uint32_t code = 0, off = 0;
#pragma unroll
    for (int l = 1; l <= MAXLEN; l++) {
        const uint32_t c = cnt[l];
        if (lane == 0) { h.ub[l] = (uint16_t)((code + c) << (15 - l)); h.delta[l] = (int16_t)((int)off - (int)code); }
        if (c) {
            uint32_t running = 0;
#pragma unroll
            for (int s = 0; s < NS; s++) {
                const uint64_t bl = __ballot(ls[s] == l);
                if (ls[s] == l) {
                    const uint32_t k = running + (uint32_t)__popcll(bl & (lane ? (~0ull >> (64 - lane)) : 0ull));
                    const uint16_t sym = (uint16_t)(lane + 64 * s);
                    h.sorted[off + k] = sym;
                    if (l <= PB) {
                        const uint32_t r = __brev(code + k) >> (32 - l);
                        for (uint32_t e = r; e < (1u << PB); e += 1u << l) h.tent[e] = (uint16_t)(sym | (l << 9));
                    }
                }
                running += (uint32_t)__popcll(bl);
            }
        }
        code = (code + c) << 1;
        off += c;
    }
    if (lane == 0) h.maxlen = maxlen;
    __syncthreads();
    return left > 0 ? 1 : 0;
}
// inclusive prefix MAXIMUM over the 64 lanes (unsigned, 0 = nothing yet), the six DPP steps of wave_inclusive_sum
__device__ __forceinline__ uint32_t wave_inclusive_max(uint32_t v)
{
    int x = (int)v;
#define SS_MAXU(a, b) (int)max((uint32_t)(a), (uint32_t)(b))
    x = SS_MAXU(x, __builtin_amdgcn_update_dpp(0, x, 0x111, 0xf, 0xf, false));      // row_shr:1
    x = SS_MAXU(x, __builtin_amdgcn_update_dpp(0, x, 0x112, 0xf, 0xf, false));      // row_shr:2
    x = SS_MAXU(x, __builtin_amdgcn_update_dpp(0, x, 0x114, 0xf, 0xf, false));      // row_shr:4
    x = SS_MAXU(x, __builtin_amdgcn_update_dpp(0, x, 0x118, 0xf, 0xf, false));      // row_shr:8
    x = SS_MAXU(x, __builtin_amdgcn_update_dpp(0, x, 0x142, 0xa, 0xf, false));      // row_bcast:15 into rows 1 and 3
    x = SS_MAXU(x, __builtin_amdgcn_update_dpp(0, x, 0x143, 0xc, 0xf, false));      // row_bcast:31 into rows 2 and 3
#undef SS_MAXU
    return (uint32_t)x;
}

__device__ bool read_dynamic(WaveState &S, SBits &b, bool &dist_usable)
{
    const int hlit = (int)sb_get(S, b, 5) + 257, hdist = (int)sb_get(S, b, 5) + 1, hclen = (int)sb_get(S, b, 4) + 4;
    if (hlit > 286 || hdist > 30) return false;
    __syncthreads();
    if ((threadIdx.x & 63) < 19) S.lens[threadIdx.x & 63] = 0;
    __syncthreads();
    {
        // the HCLEN 3-bit lengths (at most 57 bits) in one go: lane i takes the i-th
        sb_stage(S, b);
        const int li = threadIdx.x & 63;
        const uint32_t p = b.bp + 3u * (uint32_t)li;
        const uint32_t w = p >> 5, sh = p & 31u;
        const uint32_t d0 = S.stage[w & STAGE_MASK], d1 = S.stage[(w + 1) & STAGE_MASK];
        const uint32_t v = (uint32_t)((((uint64_t)d1 << 32) | d0) >> sh) & 7u;
        if (li < hclen) S.lens[c_cl_order[li]] = (uint8_t)v;
        sb_seek(b, b.bp + 3u * (uint32_t)hclen);
    }
    if (__builtin_amdgcn_readfirstlane(huff_build<7, 19, 7>(S.clc, S.lens, 19)) != 0) return false;   // (a call's result arrives in a VGPR)
    // the code lengths themselves, as the block loop decodes its symbols: the 64 lanes decode a code-length symbol (with its
    // extra bits: at most 14 bits) at 64 bit positions, the wave follows the chain from bp and hands every item on it
    // its value ("repeat the previous length" resolved on the way) and its place; the lanes then store their runs.
    // [One symbol at a time was ~300 cycles x 300 symbols for each of the ~80 candidates a chunk's sync search tries.]
    __shared__ uint8_t s_all[320];
    const int total = hlit + hdist, lane = threadIdx.x & 63;
    int i = 0, prev = -1;
    uint32_t kraft_lit = 0;
    while (i < total) {
        sb_stage(S, b);
        const uint32_t p = b.bp + (uint32_t)lane;
        const uint32_t w = p >> 5, sh = p & 31u;
        const uint32_t d0 = S.stage[w & STAGE_MASK], d1 = S.stage[(w + 1) & STAGE_MASK];
        const uint32_t bits = (uint32_t)((((uint64_t)d1 << 32) | d0) >> sh);
        const uint32_t e = S.clc.tent[bits & 127u];
        const uint32_t l = e >> 9, sy = e & 511u;
        const uint32_t xb = sy == 16 ? 2u : sy == 17 ? 3u : sy == 18 ? 7u : 0u;
        const uint32_t x = (bits >> l) & ((1u << xb) - 1u);
        const uint32_t rep = sy < 16 ? 1u : sy == 18 ? 11u + x : 3u + x;
        const uint32_t pk = e ? ((l + xb) | (rep << 4) | ((sy < 16 ? sy : sy == 16 ? 16u : 0u) << 12)) : 0u;      // bits | run | value (16 = copy)
        // the chain from bp (an undecodable position steps out of the window), then by prefix sum and ballots: which of
        // its items still belong to the lengths, where their runs go, and what "copy" copies
        const uint32_t step = (pk & 15u) ? (pk & 15u) : 64u;
        uint64_t chain = 0;
        uint32_t pos = 0;
        do {
            chain |= 1ull << pos;
            pos += (uint32_t)__builtin_amdgcn_readlane((int)step, (int)pos);
        } while (pos < 64);
        const bool on = (chain >> lane) & 1ull;
        const uint32_t incl = wave_inclusive_sum(on ? rep : 0u), before = incl - (on ? rep : 0u);
        const uint32_t left = (uint32_t)(total - i);
        const bool used = on && before < left;
        const uint64_t usedm = __ballot(used);                                   // lane 0 is in it
        const int lu = 63 - __clzll((long long)usedm);
        const uint32_t end = (uint32_t)__builtin_amdgcn_readlane((int)incl, lu);
        if (__ballot(used && (pk & 15u) == 0) || end > left) return false;      // undecodable, or a run beyond the last length
        const uint32_t vc = pk >> 12;
        const uint64_t sources = __ballot(used && vc != 16u) & ((lane == 63 ? 0ull : (~0ull << (lane + 1))) ^ ~0ull);   // at or below this lane
        const int src = sources ? 63 - __clzll((long long)sources) : -1;
        const int got = __shfl((int)vc, src < 0 ? 0 : src, 64);
        const int val = src < 0 ? prev : got;
        if (__ballot(used && val < 0)) return false;                             // "repeat the previous length" with none before
        // Kraft sums as the lengths arrive: a position that is no header -- the sync search tries ~40 per chunk -- decodes to
        // random lengths, and those over-subscribe a code within the first window or two (a symbol adds 1 700 / 32 768 on average):
        // out here, not after all ~300 lengths and the counting of huff_build
        {
            const uint32_t idx0 = (uint32_t)i + before;                          // (the literal/length code's lengths come first)
            const uint32_t n_lit = !used || idx0 >= (uint32_t)hlit ? 0u : min(rep, (uint32_t)hlit - idx0);
            const uint32_t unit = val > 0 ? (1u << (15 - val)) : 0u;
            kraft_lit += (uint32_t)__builtin_amdgcn_readlane((int)wave_inclusive_sum(n_lit * unit), 63);
            if (kraft_lit > 32768u) return false;
        }
        if (used)
            for (uint32_t r = 0; r < rep; r++) s_all[i + (int)before + (int)r] = (uint8_t)val;
        prev = __builtin_amdgcn_readlane(val, lu);
        i += (int)end;
        sb_seek(b, b.bp + (uint32_t)lu + (uint32_t)__builtin_amdgcn_readlane((int)step, lu));
        if (sb_past_end(b)) return false;
    }
    __syncthreads();
    if (__builtin_amdgcn_readfirstlane((int)s_all[256]) == 0) return false;
    for (int k = threadIdx.x & 63; k < hlit + hdist; k += 64) S.lens[k] = s_all[k];
    __syncthreads();
    const int rl = __builtin_amdgcn_readfirstlane(huff_build(S.lit, S.lens, hlit));
    if (rl < 0 || (rl > 0 && __builtin_amdgcn_readfirstlane(S.lit.maxlen) != 1)) return false;
    const int rd = __builtin_amdgcn_readfirstlane(huff_build(S.dist, S.lens + hlit, hdist));
    const int dmax = __builtin_amdgcn_readfirstlane(S.dist.maxlen);
    if (rd < 0 || (rd > 0 && dmax > 1)) return false;
    dist_usable = dmax > 0;
    return !sb_past_end(b);
}

__device__ void fixed_codes(WaveState &S)
{
    __syncthreads();
    for (int i = threadIdx.x & 63; i < 288; i += 64) S.lens[i] = i < 144 ? 8 : i < 256 ? 9 : i < 280 ? 7 : 8;
    __syncthreads();
    huff_build(S.lit, S.lens, 288);
    __syncthreads();
    for (int i = threadIdx.x & 63; i < 30; i += 64) S.lens[i] = 5;
    __syncthreads();
    huff_build(S.dist, S.lens, 30);
}

// Output of a wave: symbols go to the LDS ring first; whenever 1024 new ones have gathered, the 64 lanes write them to
// global memory together (128 contiguous bytes per store instruction).  A match reads its source from the ring when it
// is at most RING_REACH symbols back (always true for what is not flushed yet) and from global memory otherwise --
// data flushed at least two flushes ago; every flush first waits for the stores of the one before.
constexpr uint32_t RING_REACH = RING - 264;
struct OutState {
    uint16_t *out;           // null: count only
    uint32_t cap, n, flushed;        // symbols: a chunk's output is far below 2^31 (its region is capped when the state is made)
};
__device__ __forceinline__ void out_flush(WaveState &S, OutState &o, uint32_t upto)
{
    const int lane = threadIdx.x & 63;
    __threadfence_block();
    for (uint32_t i = o.flushed + (uint32_t)lane; i < upto; i += 64) o.out[i] = S.ring[i & (RING - 1)];
    o.flushed = upto;
}

// a code longer than the table's PB bits (or none at all), per lane, without a loop: the 15 bits as a left-justified code
// value; canonical codes are sorted by length, so the length is PB + 1 + the number of ends ub[PB + 1 .. 14] the value has reached
template <int PB, int MAXSYM>
__device__ __forceinline__ int lane_long(const LHuff<PB, MAXSYM> &h, uint32_t v, int maxlen, int &len)
{
    (void)maxlen;
    const uint32_t c15 = __brev(v & 0x7FFFu) >> 17;                  // the first bit of the stream is the code's most significant
    uint32_t l = PB + 1;
#pragma unroll
    for (int k = PB + 1; k <= 14; k++) l += c15 >= (uint32_t)h.ub[k] ? 1u : 0u;
    const bool ok = c15 < (uint32_t)h.ub[l];                           // (beyond the last code: an incomplete code's unused values)
    len = ok ? (int)l : 0;
    const int at = (int)h.delta[l] + (int)(c15 >> (15u - l));
    return ok ? (int)h.sorted[ok ? at : 0] : -1;
}

// `len` symbols from `dist` back to position n of the wave's output (the 64 lanes together)
__device__ __forceinline__ void copy_match(WaveState &S, const OutState &o, uint32_t n, uint32_t len, uint32_t dist)
{
    const int lane = threadIdx.x & 63;
    const uint32_t n32 = n;
    const bool overlaps = dist < len;                  // (uniform: the division below is rarely reached)
    for (uint32_t base = 0; base < len; base += 64) {
        const uint32_t i = base + (uint32_t)lane;
        if (i < len) {
            const uint32_t k = overlaps ? i % dist : i;             // a match that overlaps itself repeats with period dist
            const int32_t sp = (int32_t)(n32 - dist + k);
            uint16_t v;
            if (sp < 0) v = (uint16_t)(UNRES | (uint32_t)((int32_t)WSIZE + sp));
            else if (n32 - (uint32_t)sp <= RING_REACH) v = S.ring[sp & (RING - 1)];
            else v = o.out[sp];
            // sources lie in front of n, destinations behind it, and a ring slot is never both within one
            // match (a source that far back is read from global memory): no hazard between the pieces
            S.ring[(n32 + i) & (RING - 1)] = v;
        }
    }
}

// The symbols of a compressed block (block_body below): the 64 lanes decode SPECULATIVELY at the 64 bit positions bp .. bp + 63 -- each a
// whole item (literal, end of block, or length + extra + distance + extra: at most 48 bits, every lane has 64) --, then
// the wave follows the chain of item lengths from bp (one readlane per item on the scalar unit) and the lanes ON the
// chain deliver at the offsets a prefix sum over their output lengths gives them: the literals in one store; the
// matches whose source was flushed to global memory long ago (85 % of them in FASTQ: k-mers seen 10 KB earlier) load
// their few symbols TOGETHER -- one memory round trip per window of ~18 items instead of one per match --; matches
// that read the ring (their source may be this window's own output) follow one by one.  [A wave-uniform decoder -- one
// table lookup and ~40 instructions per symbol, 63 lanes idle, every far match a round trip -- took 47 ms per 1 M reads.]
constexpr uint32_t F_MATCH = 64u, F_EOB = 128u, F_BAD = 256u;
constexpr uint32_t FAR_MAX = 12;            // longest match of the batched kind (one 2-byte load per symbol and lane)
constexpr uint32_t WIN_MAX = RING - RING_REACH;      // 264: a window that delivers more goes item by item (ring aliasing)
// the block's first bits: BFINAL, BTYPE and the code tables (a stored block is copied here and now).
// 0 = tables in LDS, block_body follows; 10 + BFINAL = a stored block, done; < 0 = error
struct BlockCtx { uint32_t bfinal; bool dist_usable; };
__device__ int block_begin(WaveState &S, SBits &b, OutState &o, BlockCtx &cx)
{
    const int lane = threadIdx.x & 63;
    const bool store = o.out != nullptr;
    const uint32_t bfinal = sb_get(S, b, 1), btype = sb_get(S, b, 2);
    cx.bfinal = bfinal;
    cx.dist_usable = true;
    if (btype == 3) return -1;
    uint32_t n = o.n;
#define GI_RET(v) do { o.n = n; return (v); } while (0)
    if (btype == 0) {
        sb_seek(b, (b.bp + 7u) & ~7u);
        const uint32_t len = sb_get(S, b, 16), nlen = sb_get(S, b, 16);
        if (sb_past_end(b) || (len ^ 0xFFFFu) != nlen) GI_RET(-2);
        if (b.bp + 8u * len > b.nbits) GI_RET(-3);
        if (store) {
            if (n + len > o.cap) GI_RET(-9);
            const uint8_t *src = reinterpret_cast<const uint8_t *>(b.in) + (b.bp >> 3);
            uint32_t done = 0;
            while (done < len) {
                if (n - o.flushed >= 1024) out_flush(S, o, n);
                const uint32_t take = min(len - done, 1024u - (n - o.flushed));
                for (uint32_t i = (uint32_t)lane; i < take; i += 64) S.ring[(n + i) & (RING - 1)] = src[done + i];
                n += take;
                done += take;
            }
        } else {
            n += len;
        }
        sb_seek(b, b.bp + 8u * len);
        GI_RET(10 + (int)bfinal);
    }
    if (btype == 1) fixed_codes(S);
    else if (!read_dynamic(S, b, cx.dist_usable)) GI_RET(-4);
    return 0;
#undef GI_RET
}

// The items of a compressed block from the current position (the block's first item, or -- a chunk that was entered inside a
// block, or one that goes on behind an entry it ran over -- any item's first bit) to its end-of-block code.
// 0 = block done, 1 = final block done, 2 = probe satisfied, 3 = stopped exactly AT mid_target (an item's first bit inside
// this block: the next chunk's entry), 4 = mid_target lies behind the position and was not an item's first bit, < 0 = error.
__device__ int block_body(WaveState &S, SBits &b, OutState &o, bool known_window, const BlockCtx cx, uint64_t probe_symbols, uint32_t stop_bits,
                          uint32_t mid_target)      // (stop_bits, mid_target: relative positions, sb_rel; SB_NEVER = none)
{
    const int lane = threadIdx.x & 63;
    const bool store = o.out != nullptr;
    const uint32_t bfinal = cx.bfinal;
    const bool dist_usable = cx.dist_usable;
    uint32_t n = o.n;
    const int lit_maxlen = __builtin_amdgcn_readfirstlane(S.lit.maxlen), dist_maxlen = __builtin_amdgcn_readfirstlane(S.dist.maxlen);
    const uint32_t probe_end = probe_symbols >= 0x7FFFFFFFull ? SB_NEVER : n + (uint32_t)probe_symbols;
    const uint32_t end_bits = b.nbits;
    const uint64_t mine_below = lane ? (~0ull >> (64 - lane)) : 0ull;
    // the window whose far matches are still loading while the next one is decoded (software pipeline: a far match reads
    // what this wave wrote tens of KB ago -- with thousands of waves at work that is HBM or the Infinity Cache, ~2 us)
    bool p_active = false, p_fv = false;
    uint64_t p_farmask = 0, p_near = 0;
    uint32_t p_at = 0, p_mlen = 0, p_val = 0, p_fdst = 0;
    uint16_t p_fg = 0;
    int ret = 0;
#define GI_FINISH()                                                                                                          \
    do {                                                                                                                     \
        if (p_active) {                                                                                                      \
            if (p_farmask && p_fv) S.ring[p_fdst & (RING - 1)] = p_fg;                                                       \
            uint64_t mt_ = p_near;                                                                                           \
            while (mt_) {                                                                                                    \
                const int fm_ = __ffsll((long long)mt_) - 1;                                                                 \
                mt_ &= mt_ - 1;                                                                                              \
                copy_match(S, o, (uint32_t)__builtin_amdgcn_readlane((int)p_at, fm_), (uint32_t)__builtin_amdgcn_readlane((int)p_mlen, fm_), \
                           (uint32_t)__builtin_amdgcn_readlane((int)p_val, fm_));                                            \
            }                                                                                                                \
            p_active = false;                                                                                                \
        }                                                                                                                    \
    } while (0)
#define GI_OUT(v) do { ret = (v); goto out; } while (0)
    for (;;) {
        if (store && n - o.flushed >= 1024) { GI_FINISH(); out_flush(S, o, n); }
        if (n >= probe_end) GI_OUT(2);                     // sync search: the header was valid and this many symbols decoded
        if (b.bp > end_bits) GI_OUT(-5);
        if (b.bp > stop_bits) GI_OUT(-21);                 // ran past the next chunk's entry: that entry was not a block's start
        if (b.bp >= mid_target) GI_OUT(b.bp == mid_target ? 3 : 4);
        sb_stage(S, b);
        // ---- every lane: the item at bp + lane
        uint32_t info, val = 0, mlen = 0;                  // info = bits of the item | F_*; val = literal byte or match distance
        {
            const uint32_t p = b.bp + (uint32_t)lane;
            const uint32_t w = p >> 5, sh = p & 31u;
            const uint32_t d0 = S.stage[w & STAGE_MASK], d1 = S.stage[(w + 1) & STAGE_MASK], d2 = S.stage[(w + 2) & STAGE_MASK];
            uint64_t bits = (((uint64_t)d1 << 32) | d0) >> sh;
            if (sh) bits |= (uint64_t)d2 << (64 - sh);
            const uint32_t e = S.lit.tent[(uint32_t)bits & ((1u << LITBITS) - 1)];
            int l = (int)(e >> 9), sym = (int)(e & 511u);
            if (e == 0) sym = lane_long(S.lit, (uint32_t)bits & 0x7FFFu, lit_maxlen, l);
            if (sym < 0 || sym > 285) info = F_BAD;
            else if (sym < 256) { info = (uint32_t)l; val = (uint32_t)sym; }
            else if (sym == 256) info = (uint32_t)l | F_EOB;
            else {
                int xb, xd;
                uint32_t base;
                len_code(sym - 257, base, xb);
                mlen = base + ((uint32_t)(bits >> l) & ((1u << xb) - 1u));
                l += xb;
                const uint32_t v = (uint32_t)(bits >> l) & 0x7FFFu;
                const uint32_t de = S.dist.tent[v & 255u];
                int dl = (int)(de >> 9), ds = (int)(de & 511u);
                if (de == 0) ds = lane_long(S.dist, v, dist_maxlen, dl);
                if (!dist_usable || ds < 0 || ds > 29) info = F_BAD;
                else {
                    dist_code(ds, base, xd);
                    val = base + ((uint32_t)(bits >> (l + dl)) & ((1u << xd) - 1u));
                    info = (uint32_t)(l + dl + xd) | F_MATCH;
                }
            }
        }
        // ---- the chain of items from bp: a stopping item (end of block, undecodable) steps out of the window
        const uint32_t step = (info & (F_EOB | F_BAD)) ? 64u : (info & 63u);
        // (three scalar instructions, a readlane and the branch per item: the bit is set in place, the last item is looked up
        //  afterwards -- the scalar unit is shared by the CU's four SIMDs and this kernel keeps it as busy as the vector units)
        uint64_t chain = 0;
        uint32_t pos = 0;
        do {
            asm volatile("s_bitset1_b64 %0, %1" : "+s"(chain) : "s"(pos));
            pos += (uint32_t)__builtin_amdgcn_readlane((int)step, (int)pos);
        } while (pos < 64);
        const uint32_t last = 63u - (uint32_t)__clzll((long long)chain);
        uint32_t stop = (uint32_t)__builtin_amdgcn_readlane((int)info, (int)last);
        stop = (stop & (F_EOB | F_BAD)) ? stop : 0u;
        if (stop) { chain &= ~(1ull << last); pos = last; }
        if (mid_target - b.bp < 64u && ((chain >> (mid_target - b.bp)) & 1ull)) {      // the next chunk begins at an item of this window
            pos = mid_target - b.bp;
            chain &= (1ull << pos) - 1ull;
            stop = 0;
        }
        if (stop & F_BAD) GI_OUT(-5);
        // ---- deliver
        const bool on = (chain >> lane) & 1ull, is_match = on && (info & F_MATCH);
        const uint64_t matches = __ballot(is_match);
        const uint32_t olen = on ? (is_match ? mlen : 1u) : 0u;
        const uint32_t incl = wave_inclusive_sum(olen);
        const uint32_t total = (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
        const uint32_t at = n + (incl - olen);             // where this lane's item goes
        if (known_window && __ballot(is_match && val > at)) GI_OUT(-8);
        if (store) {
            if (n + total > o.cap) GI_OUT(-9);
            GI_FINISH();                                   // the window before this one: its far symbols have arrived by now
            if (total <= WIN_MAX) {
                if (on && !is_match) S.ring[at & (RING - 1)] = (uint16_t)val;
                // matches from far back, few symbols: all their loads in flight together, and left in flight
                const bool far = is_match && mlen <= FAR_MAX && val > RING_REACH + mlen - 1;      // every symbol beyond the ring's reach
                // ONE LANE PER SYMBOL of those matches (a window has ~4 of them, ~30 symbols): a prefix sum over their lengths
                // gives every match its run of slots, the match's lane number is dropped at the run's first slot (LDS) and
                // spread over the run by a prefix maximum; slot t then fetches its match's position and distance (two
                // bpermutes) and loads ITS symbol -- one load instruction per window instead of twelve
                const uint32_t fl = far ? mlen : 0u;
                const uint32_t fincl = wave_inclusive_sum(fl);
                const bool far2 = far && fincl <= 64u;     // (what does not fit the 64 slots goes the near way)
                p_farmask = __ballot(far2);
                if (p_farmask) {
                    uint32_t *own = reinterpret_cast<uint32_t *>(S.lens);
                    __builtin_amdgcn_wave_barrier();
                    own[lane] = 0u;
                    __builtin_amdgcn_wave_barrier();
                    if (far2) own[fincl - fl] = (uint32_t)lane + 1u;
                    __builtin_amdgcn_wave_barrier();
                    const uint32_t ow = wave_inclusive_max(own[lane]);
                    const uint32_t slots = (uint32_t)__builtin_amdgcn_readlane((int)fincl, 63 - __clzll((long long)p_farmask));
                    const int from = (int)((ow ? ow - 1u : 0u) << 2);
                    const uint32_t o_at = (uint32_t)__builtin_amdgcn_ds_bpermute(from, (int)at);
                    const uint32_t o_vf = (uint32_t)__builtin_amdgcn_ds_bpermute(from, (int)(val | ((fincl - fl) << 16)));      // distance <= 32768 | first slot
                    const uint32_t k = (uint32_t)lane - (o_vf >> 16);
                    const int32_t sp = (int32_t)o_at - (int32_t)(o_vf & 0xFFFFu) + (int32_t)k;
                    p_fv = (uint32_t)lane < slots;
                    uint16_t g = (uint16_t)(UNRES | (uint32_t)((int32_t)WSIZE + sp));
                    if (p_fv && sp >= 0) g = o.out[sp];
                    p_fg = g;
                    p_fdst = o_at + k;
                }
                p_at = at; p_mlen = mlen; p_val = val;
                p_near = matches & ~p_farmask;
                p_active = true;
                n += total;
            } else {
                // a window that delivers a lot (long matches): item by item, flushing on the way
                uint64_t rem = chain, mt = matches;
                for (;;) {
                    const int fm = mt ? __ffsll((long long)mt) - 1 : 64;
                    const uint64_t lits = (fm == 64 ? rem : rem & ((1ull << fm) - 1));
                    if ((lits >> lane) & 1ull) S.ring[(n + (uint32_t)__popcll(lits & mine_below)) & (RING - 1)] = (uint16_t)val;
                    n += (uint32_t)__popcll(lits);
                    if (fm == 64) break;
                    const uint32_t len = (uint32_t)__builtin_amdgcn_readlane((int)mlen, fm), dist = (uint32_t)__builtin_amdgcn_readlane((int)val, fm);
                    if (n - o.flushed >= 1024) out_flush(S, o, n);
                    copy_match(S, o, n, len, dist);
                    n += len;
                    mt &= mt - 1;
                    rem = fm == 63 ? 0ull : rem & ~((2ull << fm) - 1ull);
                }
            }
        } else {
            n += total;
        }
        if (stop & F_EOB) {
            sb_seek(b, b.bp + pos + (stop & 63u));
            GI_OUT(sb_past_end(b) ? -5 : (int)bfinal);
        }
        sb_seek(b, b.bp + pos);
    }
out:
    if (store) GI_FINISH();
    o.n = n;
    return ret;
#undef GI_FINISH
#undef GI_OUT
}

// One block from the current position.  0 = block done, 1 = final block done, 2 = probe satisfied, < 0 = error.
__device__ int inflate_block(WaveState &S, SBits &b, OutState &o, bool known_window, uint64_t probe_symbols = ~0ull, uint32_t stop_bits = SB_NEVER)
{
    BlockCtx cx;
    const int r = block_begin(S, b, o, cx);
    if (r != 0) return r >= 10 ? r - 10 : r;
    return block_body(S, b, o, known_window, cx, probe_symbols, stop_bits, SB_NEVER);
}

__device__ unsigned g_sync_tries;      // candidates that passed the header check and were decoded (trace)

// ---- kernels ------------------------------------------------------------------------------------------------------
// A: entry point of every chunk (chunk 0: the start of the deflate data)
// slice_chunks != 0 (several ranks share a file, gpu_gunzip's range mode): a rank looks for entries only in the slices it
// owns (slice s belongs to rank s mod world) and in the first `look` chunks behind each of them (where its last chunk stops)
__global__ __launch_bounds__(64) void sync_kernel(const uint8_t *in, uint64_t in_n, uint64_t data_off, uint64_t chunk_bytes,
                                                  uint32_t n_chunks, uint64_t *entry /* bit position or ~0 */, uint64_t probe, int count_tries,
                                                  uint32_t slice_chunks, uint32_t rank, uint32_t world, uint32_t look, uint32_t c0)
{
    __shared__ WaveState S;
    const uint32_t c = blockIdx.x + c0;                       // (c0: the search runs piece by piece while the image arrives)
    const int lane = threadIdx.x & 63;
    if (slice_chunks) {
        const uint32_t sl = c / slice_chunks, within = c % slice_chunks;
        const bool mine = sl % world == rank || (sl > 0 && (sl - 1) % world == rank && within < look);
        if (!mine) { if (lane == 0) entry[c] = ~0ull; return; }
    }
    if (c == 0) { if (lane == 0) entry[0] = data_off * 8; return; }
    const uint64_t lo = (data_off + (uint64_t)c * chunk_bytes) * 8, hi = min(in_n * 8, lo + chunk_bytes * 8);
    uint64_t found = ~0ull;
    SBits b;
    sb_init(b, in, in_n, lo);
    // Two sieves.  The first 13 bits (type, HLIT, HDIST) are tested for every position -- a lane takes the eight positions of one
    // byte from a single 4-byte load --; the one in nine that passes is QUEUED, and the second sieve -- the code-length code's
    // Kraft sum, a loop of up to 19 steps that a wave runs as long as its slowest lane -- only sees full waves of queued
    // positions (a ninth of the loop's executions).  The queue is in position order, so the first confirmed entry is still
    // the first in the chunk.  (lo and hi are whole bytes.)
    uint32_t *queue = reinterpret_cast<uint32_t *>(S.ring);      // (1024 words, a ring; the LDS ring holds output, and the search produces none)
    constexpr uint32_t QMASK = RING * 2 / 4 - 1;
    static_assert(RING * 2 / 4 >= 1024, "the queue takes up to 63 + 512 positions");
    __shared__ uint8_t kraft2[64];                          // (8080 + 64 bytes: still 20 workgroups of one wave per CU)
    {
        const uint32_t la = (uint32_t)lane & 7u, lb = (uint32_t)lane >> 3;
        kraft2[lane] = (uint8_t)((la ? 128u >> la : 0u) + (lb ? 128u >> lb : 0u));
    }
    __builtin_amdgcn_wave_barrier();
    uint32_t qh = 0, qn = 0;
    auto word_at = [&](uint64_t p) { uint32_t w; __builtin_memcpy(&w, in + (p >> 3) + (uint64_t)lane, 4); return w; };
    uint32_t ahead = word_at(lo);                           // the next 512 positions' bytes are loaded while these are tested
    for (uint64_t p0 = lo; p0 < hi && found == ~0ull; p0 += 512) {
        const uint32_t w = ahead;
        ahead = word_at(p0 + 512);                          // (the input is padded by 8 KB)
        const uint64_t pl = p0 + 8ull * (uint64_t)lane;
        // all eight positions of the byte at once, bit j of every term = the test at position j: BFINAL = 0 and BTYPE = 2 are
        // "bits j, j + 1 clear, bit j + 2 set"; a five-bit field (LSB first) is 30 or 31 iff its upper four bits are all set:
        // HLIT at j + 3 .. j + 7, HDIST at j + 8 .. j + 12 (bit 19 of the word at most)
        const uint32_t nw = ~w;
        const uint32_t type_ok = nw & (nw >> 1) & (w >> 2);
        const uint32_t hlit_big = (w >> 4) & (w >> 5) & (w >> 6) & (w >> 7);
        const uint32_t hdist_big = (w >> 9) & (w >> 10) & (w >> 11) & (w >> 12);
        uint32_t m8 = type_ok & ~hlit_big & ~hdist_big & 0xFFu;
        if (pl >= hi) m8 = 0;
        const uint32_t cnt = (uint32_t)__popc(m8);
        const uint32_t incl = wave_inclusive_sum(cnt);
        uint32_t at = qh + qn + incl - cnt;
        while (__ballot(m8 != 0u)) {
            if (m8) {
                const int j = __ffs((int)m8) - 1;
                m8 &= m8 - 1u;
                queue[at & QMASK] = (uint32_t)(pl - lo) + (uint32_t)j;
                at++;
            }
        }
        qn += (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
        const bool last = p0 + 512 >= hi;
        while ((qn >= 64u || (last && qn > 0u)) && found == ~0ull) {
            const uint32_t take = min(qn, 64u);
            __builtin_amdgcn_wave_barrier();
            const uint32_t q = (uint32_t)lane < take ? queue[(qh + (uint32_t)lane) & QMASK] : 0u;
            const uint64_t pos = lo + (uint64_t)q;
            const bool ok = (uint32_t)lane < take && header_prefilter_lut(header_bytes(in, pos), pos, kraft2);
            uint64_t m = __ballot(ok);
            while (m && found == ~0ull) {
                const int l = __ffsll((long long)m) - 1;
                m &= m - 1;
                const uint64_t cand = lo + (uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)q, l);
                // confirm with the whole wave: a complete, valid header (zlib's rules) and 512 symbols that decode: a
                // position inside a block passes this with negligible probability, and if one ever does, the chunk in front
                // runs over it (inflate_kernel)
                sb_seek_abs(b, cand);
                OutState o{nullptr, 0, 0, 0};
                const int r = inflate_block(S, b, o, false, probe);
                if (count_tries && lane == 0) atomicAdd(&g_sync_tries, 1u);
                if (r == 2 || (r == 0 && o.n > 0)) found = cand;
            }
            __builtin_amdgcn_wave_barrier();
            qh = (qh + take) & QMASK;
            qn -= take;
        }
    }
    if (lane == 0) entry[c] = found;
}

// A2: entries INSIDE blocks.  A block is the unit the search can find (a sync point exists only at a block's start), and a
// wave that decodes 30-60 KB of deflate data alone is what the inflate kernel waits for.  But Huffman-coded data
// synchronises itself: decode from ANY bit with the block's tables and after a few dozen items the decoder is on the true
// item boundaries.  One wave per wanted position `from` inside the block whose header is at `hdr`: parse the header, then
// window by window (64 bits) every lane decodes the item at its bit as the inflate kernel does; all 64 offsets are
// hypotheses at first, a window maps the live ones to the offsets at which their chains enter the next window (chains
// followed by pointer doubling: six bpermutes), dead ends (undecodable, end of block) drop out.  When ONE offset is left it is the
// true chain -- the true one never dies before the block ends -- and becomes the entry: a chunk that begins there with
// `hdr`'s tables.  Verified when the chunks are inflated: the chunk in front must arrive exactly there, inside that block.
constexpr int SUB_WINDOWS = 48;
__device__ __forceinline__ uint32_t lane_item_bits(const WaveState &S, uint64_t bits, int lit_maxlen, int dist_maxlen, bool dist_usable)
{
    const uint32_t e = S.lit.tent[(uint32_t)bits & ((1u << LITBITS) - 1)];
    int l = (int)(e >> 9), sym = (int)(e & 511u);
    if (e == 0) sym = lane_long(S.lit, (uint32_t)bits & 0x7FFFu, lit_maxlen, l);
    if (sym < 0 || sym > 285 || sym == 256) return 0;           // undecodable, or the end of the block: the hypothesis ends
    if (sym < 256) return (uint32_t)l;
    int xb, xd;
    uint32_t base;
    len_code(sym - 257, base, xb);
    l += xb;
    const uint32_t v = (uint32_t)(bits >> l) & 0x7FFFu;
    const uint32_t de = S.dist.tent[v & 255u];
    int dl = (int)(de >> 9), ds = (int)(de & 511u);
    if (de == 0) ds = lane_long(S.dist, v, dist_maxlen, dl);
    if (!dist_usable || ds < 0 || ds > 29) return 0;
    dist_code(ds, base, xd);
    return (uint32_t)(l + dl + xd);
}
__global__ __launch_bounds__(64) void subsync_kernel(const uint8_t *in, uint64_t in_n, const uint64_t *hdr, const uint32_t *first /* [n_blocks + 1] */,
                                                     const uint64_t *from, const uint64_t *limit, uint32_t n_blocks, uint64_t *entry)
{
    __shared__ WaveState S;
    __shared__ uint32_t flag[64];
    const uint32_t blk = blockIdx.x;                          // one wave per block: its header is parsed once for all its positions
    if (blk >= n_blocks) return;
    const int lane = threadIdx.x & 63;
    SBits b;
    sb_init(b, in, in_n, hdr[blk]);
    OutState o{nullptr, 0, 0, 0};
    BlockCtx cx;
    const bool usable = block_begin(S, b, o, cx) == 0;
    const uint64_t body = sb_bitpos(b);
    const int lit_maxlen = __builtin_amdgcn_readfirstlane(S.lit.maxlen), dist_maxlen = __builtin_amdgcn_readfirstlane(S.dist.maxlen);
    for (uint32_t i = first[blk]; i < first[blk + 1]; i++) {
        uint64_t found = ~0ull;
        const uint64_t p0 = from[i], lim = limit[i];
        if (usable && p0 >= body) {
            uint64_t live = ~0ull;
            for (int w = 0; w < SUB_WINDOWS; w++) {
                const uint64_t base = p0 + 64ull * (uint64_t)w;
                if (base + 192 > lim) break;
                sb_seek_abs(b, base);
                if (b.bp == SB_NEVER) break;                  // (out of this wave's reach: no entry here)
                sb_stage(S, b);
                const uint32_t p = b.bp + (uint32_t)lane;     // the stage is addressed by relative positions
                const uint32_t wd = p >> 5, sh = p & 31u;
                const uint32_t d0 = S.stage[wd & STAGE_MASK], d1 = S.stage[(wd + 1) & STAGE_MASK], d2 = S.stage[(wd + 2) & STAGE_MASK];
                uint64_t bits = (((uint64_t)d1 << 32) | d0) >> sh;
                if (sh) bits |= (uint64_t)d2 << (64 - sh);
                const uint32_t step = lane_item_bits(S, bits, lit_maxlen, dist_maxlen, cx.dist_usable);
                uint32_t e = step ? (uint32_t)lane + step : 255u;              // < 64: the chain goes on at that lane; 255: dead
#pragma unroll
                for (int r = 0; r < 6; r++) {
                    const uint32_t t = (uint32_t)__builtin_amdgcn_ds_bpermute((int)((e & 63u) << 2), (int)e);
                    if (e < 64u) e = t;
                }
                __builtin_amdgcn_wave_barrier();
                flag[lane] = 0u;
                __builtin_amdgcn_wave_barrier();
                if (((live >> lane) & 1ull) && e != 255u) flag[e - 64u] = 1u; // (an item has at most 48 bits: e - 64 < 48)
                __builtin_amdgcn_wave_barrier();
                live = __ballot(flag[lane] != 0u);
                if (!live) break;
                if (__popcll(live) == 1) { found = base + 64ull + (uint64_t)(__ffsll((long long)live) - 1); break; }
            }
        }
        if (lane == 0) entry[i] = found;
    }
}

// B: every listed chunk from its entry to the next entry (or the end of the stream).  An entry is a block's start
// (hdr[c] = ~0) or an item's first bit inside the block whose header is at hdr[c] (subsync_kernel).
__global__ __launch_bounds__(64) void inflate_kernel(const uint8_t *in, uint64_t in_n, const uint64_t *start, const uint64_t *stop, const uint64_t *hdr,
                                                     uint32_t n_chunks, uint16_t *sym, const uint64_t *sym_off, const uint64_t *sym_cap,
                                                     uint64_t *out_len, uint64_t *end_bit, int *status, const uint32_t *only, uint32_t max_over)
{
    __shared__ WaveState S;
    const uint32_t c = only ? only[blockIdx.x] : blockIdx.x;      // (a second pass inflates the changed chunks only)
    if (c >= n_chunks) return;
    const int lane = threadIdx.x & 63;
    SBits b;
    const uint64_t s0 = start[c];
    const bool fresh = (s0 >> 63) != 0;                     // the first chunk of a member: nothing lies in front of it
    const uint64_t first_bit = s0 & ~(1ull << 63);
    sb_init(b, in, in_n, first_bit, hdr[c]);                 // (hdr[c]: ~0, or the header of the block the chunk begins in -- in front of it)
    OutState o{sym ? sym + sym_off[c] : nullptr, (uint32_t)min(sym_cap[c], (uint64_t)0x7FFF0000u), 0, 0};
    // A block that ends BEHIND the next chunk's entry: that entry was no block's start (a position inside a block passes the
    // sync search about once in a million candidates).  The chunk simply goes on to the entry after it -- its symbol
    // region (12x its input) has room for two or three chunks of FASTQ -- and says how many entries it ran over; within
    // a block it gives up beyond the second entry ahead (what itself started at a wrong entry decodes garbage).
    // An entry INSIDE a block (hdr != ~0) is met when this chunk, in the block with that header, arrives at an item's first
    // bit exactly there; if it passes it, or is in another block, the entry was wrong and is run over like the others.
    const uint64_t stop0 = stop[c];
    uint64_t stop_at = stop0;
    const uint64_t hard = stop[min(c + max_over, n_chunks - 1)];
    uint32_t skipped = 0;
    int st = 0;
    uint64_t block_at = hdr[c];                             // the header of the block the position is in
    bool resume = block_at != ~0ull;
    for (;;) {
        BlockCtx cx;
        int r;
        if (resume) {                                        // a chunk that begins inside a block: its tables first
            sb_seek_abs(b, block_at);
            OutState none{nullptr, 0, 0, 0};
            r = block_begin(S, b, none, cx);
            if (r != 0 || first_bit < sb_bitpos(b)) { st = -22; break; }
            sb_seek_abs(b, first_bit);
            resume = false;
        } else {
            block_at = sb_bitpos(b);
            r = block_begin(S, b, o, cx);
        }
        if (r == 0) {
            for (;;) {
                const uint32_t k = c + 1 + skipped;
                const uint64_t mid = (k < n_chunks && skipped <= max_over && hdr[k] == block_at) ? (start[k] & ~(1ull << 63)) : ~0ull;
                r = block_body(S, b, o, fresh, cx, ~0ull, sb_rel(b, hard), sb_rel(b, mid));
                if (r == 4 && skipped < max_over) { stop_at = stop[c + ++skipped]; continue; }      // not an item's first bit: a wrong entry, run over
                break;
            }
            if (r == 4) { st = -21; break; }
            if (r == 3) { st = 0; stop_at = sb_bitpos(b); break; }              // exactly at the next (not skipped) entry
        } else if (r >= 10) {
            r -= 10;
        }
        if (r < 0) { st = (r == -9 && sb_bitpos(b) > stop0) ? -21 : r; break; }      // (no room for more than its own: the host merges the two)
        const uint64_t pos = sb_bitpos(b);
        // (an entry inside a block cannot lie at a block's end -- it claims a header in front of it --: wrong, run over as well)
        while (skipped < max_over && c + skipped + 1 < n_chunks && (pos > stop_at || (pos == stop_at && hdr[c + 1 + skipped] != ~0ull)))
            stop_at = stop[c + ++skipped];
        if (r == 1) { st = (stop_at == ~0ull) ? 1 : -20; break; }      // the final block ends the LAST chunk of a member only
        if (pos == stop_at) {
            const uint32_t k = c + 1 + skipped;
            st = (k < n_chunks && hdr[k] != ~0ull) ? -21 : 0;
            break;
        }
        if (pos > stop_at) { st = -21; break; }
    }
    if (st >= 0 && o.out) out_flush(S, o, o.n);
    const uint64_t n = o.n;
    if (lane == 0) { out_len[c] = n; end_bit[c] = sb_bitpos(b); status[c] = st >= 0 ? st + 16 * (int)skipped : st; }
}

// C: windows.  The 32 KB in front of chunk c + 1 are the last 32 KB of chunk c's output, in which a symbol may still
//    point into chunk c's own window, and so on down the chain.  The tails are treated as maps "window of c -> window of
//    c + 1" (an entry is a byte or an index into the previous window) and composed (below).
__global__ __launch_bounds__(256) void tails_kernel(const uint16_t *sym, const uint64_t *sym_off, const uint64_t *out_len,
                                                    uint32_t n_chunks, uint16_t *map)
{
    const uint32_t c = blockIdx.y;                            // map[c] : window of chunk c -> window of chunk c + 1
    const uint64_t L = out_len[c];
    const uint16_t *sy = sym + sym_off[c];
    const uint32_t i0 = (blockIdx.x * 256 + threadIdx.x) * 8;      // eight entries (16 bytes) per lane
    uint16_t e[8];
    if (L >= WSIZE - i0) {
        __builtin_memcpy(e, sy + (L - (WSIZE - i0)), 16);          // 2-byte aligned: an unaligned 16-byte load
    } else {
#pragma unroll
        for (uint32_t k = 0; k < 8; k++) {
            const uint32_t i = i0 + k;
            e[k] = L >= WSIZE - i ? sy[L - (WSIZE - i)] : (uint16_t)(UNRES | (i + (uint32_t)L));      // the chunk was shorter than
        }                                                                                           // the window: its own window shifts in
    }
    __builtin_memcpy(map + (uint64_t)c * WSIZE + i0, e, 16);
}
// Two levels instead of log2(n_chunks) doubling rounds over all maps (every chunk of a FASTQ file hands lines like
// "+\n" down from the chunk before, so the chains are as long as the file and no round finishes early: twelve passes
// over 260 MB for a 130 MB file).  Chunks are grouped, GROUP consecutive ones:
//   1  one workgroup per group composes its maps IN ORDER, the running map (window at the group's start -> window behind
//      chunk c) in LDS: a 32 K-entry gather per chunk, the next chunk's tail prefetched meanwhile;
//   2  one workgroup walks the groups: the window at the start of group g + 1 = the last map of group g applied to the
//      window at the start of g (32 KB of bytes in LDS);
//   3  every chunk's window = its composed map applied to its group's start window, all in parallel.
__global__ __launch_bounds__(1024) void group_maps_kernel(const uint16_t *tails, uint32_t n_chunks, uint32_t group, uint16_t *maps)
{
    __shared__ uint16_t cur[WSIZE];                        // 64 KB
    const uint32_t c0 = blockIdx.x * group, c1 = min(c0 + group, n_chunks);
    const uint32_t tid = threadIdx.x;
    uint4 nx[4], v[4];
#pragma unroll
    for (int k = 0; k < 4; k++) nx[k] = *reinterpret_cast<const uint4 *>(tails + (uint64_t)c0 * WSIZE + ((uint32_t)k * 1024 + tid) * 8);
    for (uint32_t c = c0; c < c1; c++) {
#pragma unroll
        for (int k = 0; k < 4; k++) v[k] = nx[k];
        if (c + 1 < c1) {
#pragma unroll
            for (int k = 0; k < 4; k++) nx[k] = *reinterpret_cast<const uint4 *>(tails + (uint64_t)(c + 1) * WSIZE + ((uint32_t)k * 1024 + tid) * 8);
        }
        if (c > c0) {
#pragma unroll
            for (int k = 0; k < 4; k++) {
                if ((v[k].x | v[k].y | v[k].z | v[k].w) & 0x80008000u) {
                    uint16_t e[8];
                    __builtin_memcpy(e, &v[k], 16);
#pragma unroll
                    for (int j = 0; j < 8; j++)
                        if (e[j] & UNRES) e[j] = cur[e[j] & (WSIZE - 1)];
                    __builtin_memcpy(&v[k], e, 16);
                }
            }
        }
        __syncthreads();                                   // all gathers from the running map are done
#pragma unroll
        for (int k = 0; k < 4; k++) {
            *reinterpret_cast<uint4 *>(&cur[((uint32_t)k * 1024 + tid) * 8]) = v[k];
            *reinterpret_cast<uint4 *>(maps + (uint64_t)c * WSIZE + ((uint32_t)k * 1024 + tid) * 8) = v[k];
        }
        __syncthreads();
    }
}
// gwin[g] = the window in front of the first chunk of group g (bytes)
__global__ __launch_bounds__(1024) void group_windows_kernel(const uint16_t *maps, uint32_t n_chunks, uint32_t group, uint32_t n_groups,
                                                             const uint8_t *w0, uint8_t *gwin)
{
    __shared__ uint8_t w[WSIZE];
    const uint32_t tid = threadIdx.x;
    for (uint32_t i = tid; i < WSIZE; i += 1024) w[i] = w0 ? w0[i] : (uint8_t)0;     // the 32 KB in front of the first chunk: the end of
                                                                                  // the text so far (a file's first chunk: nothing, never read)
    __syncthreads();
    for (uint32_t g = 0; g < n_groups; g++) {
        for (uint32_t i = tid; i < WSIZE; i += 1024) gwin[(uint64_t)g * WSIZE + i] = w[i];
        if (g + 1 == n_groups) break;
        const uint16_t *m = maps + (uint64_t)(min((g + 1) * group, n_chunks) - 1) * WSIZE;      // the group's last composed map
        uint8_t nw[32];
#pragma unroll
        for (int k = 0; k < 32; k++) {
            const uint16_t e = m[(uint32_t)k * 1024 + tid];
            nw[k] = (e & UNRES) ? w[e & (WSIZE - 1)] : (uint8_t)e;
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < 32; k++) w[(uint32_t)k * 1024 + tid] = nw[k];
        __syncthreads();
    }
}
// win[c + 1] = bytes of the composed map of chunk c over its group's start window; win[0] = the window in front of the segment
__global__ __launch_bounds__(256) void windows_kernel(const uint16_t *maps, uint32_t n_chunks, uint32_t group, const uint8_t *gwin, uint8_t *win)
{
    const uint32_t c = blockIdx.y;
    const uint32_t i0 = (blockIdx.x * 256 + threadIdx.x) * 8;
    uint2 o = *reinterpret_cast<const uint2 *>(gwin + i0);      // the first chunk: what lies in front of the segment (group 0's start)
    if (c) {
        const uint4 v = *reinterpret_cast<const uint4 *>(maps + (uint64_t)(c - 1) * WSIZE + i0);
        if ((v.x | v.y | v.z | v.w) & 0x80008000u) {
            const uint8_t *gw = gwin + (uint64_t)((c - 1) / group) * WSIZE;
            uint16_t e[8];
            uint8_t by[8];
            __builtin_memcpy(e, &v, 16);
#pragma unroll
            for (int j = 0; j < 8; j++) by[j] = (e[j] & UNRES) ? gw[e[j] & (WSIZE - 1)] : (uint8_t)e[j];
            __builtin_memcpy(&o, by, 8);
        } else {
            o.x = (v.x & 0xFFu) | ((v.x >> 8) & 0xFF00u) | ((v.y & 0xFFu) << 16) | ((v.y << 8) & 0xFF000000u);
            o.y = (v.z & 0xFFu) | ((v.z >> 8) & 0xFF00u) | ((v.w & 0xFFu) << 16) | ((v.w << 8) & 0xFF000000u);
        }
    }
    *reinterpret_cast<uint2 *>(win + (uint64_t)c * WSIZE + i0) = o;
}

// D: symbols -> bytes
__global__ __launch_bounds__(256) void bytes_kernel(const uint16_t *sym, const uint64_t *sym_off, const uint64_t *out_len,
                                                    const uint64_t *text_off, const uint8_t *win, uint8_t *text)
{
    const uint32_t c = blockIdx.y;
    const uint64_t L = out_len[c];
    const uint16_t *sy = sym + sym_off[c];
    const uint8_t *w = win + (uint64_t)c * WSIZE;
    uint8_t *dst = text + text_off[c];
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < L; i += (uint64_t)gridDim.x * 256) {
        const uint16_t s = sy[i];
        dst[i] = (s & UNRES) ? w[s & (WSIZE - 1)] : (uint8_t)s;
    }
}

// the last 32 KB of the text so far = the window in front of the next segment's first chunk
__global__ __launch_bounds__(256) void lastwin_kernel(const uint8_t *text, uint64_t total, uint8_t *prev)
{
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i < WSIZE) prev[i] = total >= WSIZE - i ? text[total - (WSIZE - i)] : (uint8_t)0;
}

// CRC-32 (zlib's polynomial) of the members of a file, one lane per segment of 2^lg bytes from every member's first byte (any
// alignment), byte-wise table in LDS: segment s belongs to the member
// m with first[m] <= s < first[m + 1] (binary search: a bgzip file has thousands) and begins (s - first[m]) << lg bytes into it.
// Nothing but the member table travels to the device (a list of the segments would be 12 bytes per 4 KB of text); the byte
// table is made here.
struct CrcMember { uint64_t at, len, first; };
__global__ __launch_bounds__(64) void crc_members_kernel(const uint8_t *text, const CrcMember *mem, uint32_t n_mem, uint64_t n_seg, int lg, uint32_t *crc)
{
    __shared__ uint32_t tab[256];
    for (int i = threadIdx.x; i < 256; i += 64) {
        uint32_t k = (uint32_t)i;
        for (int j = 0; j < 8; j++) k = (k & 1u) ? 0xEDB88320u ^ (k >> 1) : k >> 1;
        tab[i] = k;
    }
    __syncthreads();
    const uint64_t s = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= n_seg) return;
    uint32_t lo = 0, hi = n_mem - 1;                         // the last member whose first segment is <= s
    while (lo < hi) {
        const uint32_t mid = (lo + hi + 1) >> 1;
        if (mem[mid].first <= s) lo = mid; else hi = mid - 1;
    }
    const uint64_t a0 = (s - mem[lo].first) << lg;
    uint64_t i = mem[lo].at + a0;
    const uint64_t e = i + min((uint64_t)1 << lg, mem[lo].len - a0);
    uint32_t k = 0xFFFFFFFFu;
    for (; i < e && (i & 3); i++) k = tab[(k ^ text[i]) & 0xFFu] ^ (k >> 8);
    for (; i + 4 <= e; i += 4) {
        const uint32_t w = *reinterpret_cast<const uint32_t *>(text + i);
        k = tab[(k ^ w) & 0xFFu] ^ (k >> 8);
        k = tab[(k ^ (w >> 8)) & 0xFFu] ^ (k >> 8);
        k = tab[(k ^ (w >> 16)) & 0xFFu] ^ (k >> 8);
        k = tab[(k ^ (w >> 24)) & 0xFFu] ^ (k >> 8);
    }
    for (; i < e; i++) k = tab[(k ^ text[i]) & 0xFFu] ^ (k >> 8);
    crc[s] = k ^ 0xFFFFFFFFu;
}

// GF(2) operator "append seg zero bytes" for CRC-32 (zlib's crc32_combine builds it anew for every call; here all segments
// but the last have the same length, so it is built once)
uint32_t gf2_times(const uint32_t *mat, uint32_t vec)
{
    uint32_t sum = 0;
    for (int i = 0; vec; vec >>= 1, i++) if (vec & 1u) sum ^= mat[i];
    return sum;
}
// newlines of text[0, n): 16 bytes per lane and step (SWAR zero-byte test on w ^ 0x0A0A0A0A), the ragged ends byte by byte
__global__ __launch_bounds__(256) void count_nl_kernel(const uint8_t *text, uint64_t n, unsigned long long *out)
{
    unsigned long long c = 0;
    const uint64_t head = std::min<uint64_t>(n, (16 - ((uintptr_t)text & 15)) & 15), body = (n - head) / 16;
    const uint4 *t4 = reinterpret_cast<const uint4 *>(text + head);
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < body; i += (uint64_t)gridDim.x * 256) {
        const uint4 v = t4[i];
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int d = 0; d < 4; d++) {
            const uint32_t x = w[d] ^ 0x0A0A0A0Au;
            c += (unsigned)__popc(~(((x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | x) & 0x80808080u);
        }
    }
    if (blockIdx.x == 0) {
        for (uint64_t i = threadIdx.x; i < head; i += 256) c += text[i] == '\n' ? 1u : 0u;
        for (uint64_t i = head + body * 16 + threadIdx.x; i < n; i += 256) c += text[i] == '\n' ? 1u : 0u;
    }
    for (int off = 32; off > 0; off >>= 1) c += __shfl_down(c, off, 64);
    if ((threadIdx.x & 63) == 0 && c) atomicAdd(out, c);
}

}  // namespace
