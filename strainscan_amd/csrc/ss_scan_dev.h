// Device helpers shared by the scan kernels (flat table: ss_scan.hip; page index: ss_mini.hip, ss_minik.hip) and the index builds.
#pragma once
#include "ss_common.h"
#include <stdlib.h>
#include <type_traits>

namespace ss {

// ---- minimizers of the k = 31 index (ss_mini.hip) and of the locality order of resident reads (ss_reorder.hip) ----
constexpr int MINI_M = 15;                       // minimizer length (30 bits)
constexpr uint32_t M30 = 0x3FFFFFFFu;

// Ordering key of a 30-bit m-mer: the m-mer with the smallest key, leftmost on ties, is the
// minimizer of a k-mer.  key = lo24(x) * C1 + C0 with C1 = an odd 19-bit constant << 5 and C0 a
// multiple of 32: ONE v_mad_u32_u24 per m-mer on the device (full rate; the 24-bit multiplier
// ignores the operand's upper bits, so the device never masks the window).  The key orders the
// m-mers by their first 12 bases (a bijection of those 24 bits onto the 27 key bits); m-mers that
// agree there tie and resolve leftmost like any other tie.  The low five bits are zero by
// construction: the kernel adds the m-mer's index there (for free, inside C0), so ONE v_min_u32
// per step compares (key, position).  The constant keeps poly-A from being everybody's minimizer.
// It need not be injective: a bucket is named by the m-mer itself and holds full k-mers.
constexpr uint32_t MMK_C1 = 0x4F1BBu << 5, MMK_C0 = 0x7F4A7C00u;
__host__ __device__ __forceinline__ uint32_t mmkey(uint32_t x)
{
    return (x & 0xFFFFFFu) * MMK_C1 + MMK_C0;
}
constexpr uint32_t KEY_MASK = ~31u;

// Once per RUN: h = mix30(minimizer), a bijection of the 30 bits (odd multipliers modulo 2^30, xor-shifts).
// Page = high half of (h << 2) x n_pages (any table size, no power-of-two rounding); tags = low bits of h.
__host__ __device__ __forceinline__ uint32_t mulhi32(uint32_t a, uint32_t b)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __umulhi(a, b);
#else
    return (uint32_t)(((uint64_t)a * b) >> 32);
#endif
}
__host__ __device__ __forceinline__ uint32_t mix30(uint32_t x)
{
    uint32_t h = (x * 0x9E3779B1u) & M30;
    h ^= h >> 15;
    h = (h * 0x2C1B3C6Du) & M30;
    h ^= h >> 14;
    return h;
}

// ---- the page index of ss_mini.hip (built by ss_mini_build.hip on the host, by ss_build_dev.hip on the device) ----
constexpr uint32_t HDR_MULTI = 1u << 17;
__host__ __device__ __forceinline__ uint32_t page_of(uint32_t h, uint32_t n_pages) { return mulhi32(h << 2, n_pages); }
constexpr uint32_t PG_SLOTS = 8;                          // slots per 64-byte page
constexpr uint32_t PG_MIN_PAGES = 4096;                   // >= 2^11: (page, low 20 bits of h) determines h
// A page, structure of arrays, so that ONE 16-byte load decides almost every lookup:
//   bytes  0.. 7  tag8[8]   h & 0xFF of the slot's minimizer                         (0xFF when empty)
//   bytes  8..15  hi8[8]    inline k-mer: e = 16 - offset (5 bits); bucket reference: 0x80 | mask bit 16 << 6 | h[13:8]
//                           (0x7F when empty: an inline slot with the impossible e = 31)
//   bytes 16..47  lo32[8]   inline: flank32; reference: multi << 31 | bucket start
//   bytes 48..63  mid16[8]  inline: h[19:8] << 4; reference: mask bits 0..15
// Only slots whose tag8 (and e range / reference filter bits) match have their lo32 / mid16 read, from the sector the
// first load has just brought into the L1.
constexpr uint8_t PG_EMPTY_TAG = 0xFF, PG_EMPTY_HI = 0x7F;
constexpr uint32_t START_MASK = 0x3FFFFFFFu;
// bit 30 of a bucket reference's lo32 (round 4): the bucket is SOLID -- one database k-mer per offset, the offsets a contiguous
// range, and the k-mer of offset o + 1 is the k-mer of offset o moved one base to the left: its k-mers are one stretch of
// cnt + 30 bases (a super-k-mer), and a run of a read is verified against that stretch by ONE lane (ss_mini.hip phase 3a)
constexpr uint32_t PG_SOLID = 1u << 30;
// How many database k-mers of one minimizer are kept INLINE in page slots (more go to a bucket).  Two, where a table's
// minimizers mostly own one or two k-mers (the sampled node sets of a tree: one sector answers a lookup); NONE, where such
// minimizers are the exception (every k-mer of a genome: 3 % of them) -- there an inline k-mer's hit is an atomic of its own,
// one (instruction, line) request per hit, while a bucket's hits share lines and, in a cluster scan, the LDS counters: the
// cluster scan 7.4 -> 6.5 ms without inline k-mers, a contiguous tree table unchanged (round 4).  SS_INLINE_MAX overrides.
inline uint32_t choose_inline_max(uint64_t kmers_of_small_minimizers /* <= 2 k-mers */, uint64_t n_distinct)
{
    if (const char *e = getenv("SS_INLINE_MAX")) { const int v = atoi(e); return (uint32_t)(v < 0 ? 0 : v > 8 ? 8 : v); }
    return kmers_of_small_minimizers * 8 < n_distinct ? 0u : 2u;
}
// the 16 bases of a k-mer that are not its minimizer: rotate the 62-bit key right by 2 * offset (the minimizer
// comes to stand in bits 0..29), the upper 32 bits = bases behind the minimizer, then the bases in front of it
__host__ __device__ __forceinline__ uint32_t flank_of_key(uint64_t key, uint32_t off)
{
    const uint64_t M62 = (1ull << 62) - 1;
    const uint64_t r = off ? (((key >> (2 * off)) | (key << (62 - 2 * off))) & M62) : key;
    return (uint32_t)(r >> 30);
}

// the same for a k-mer of any length MINI_M + 2 <= k <= 31 (round 6: `-k` other than 31 on the page index): the key has 2 k bits,
// the flank k - 15 bases (2 k - 30 bits).  k = 31 gives flank_of_key.
constexpr int MINI_K_MIN = MINI_M + 2;           // 17: at least three m-mers per k-mer (below that the flat table serves)
__host__ __device__ __forceinline__ uint32_t flank_of_key_k(uint64_t key, uint32_t off, int k)
{
    const uint64_t M = (1ull << (2 * k)) - 1;
    const uint64_t r = off ? (((key >> (2 * off)) | (key << (2 * k - 2 * off))) & M) : key;
    return (uint32_t)(r >> 30);
}

// minimizer (the m-mer itself) of a k-mer and its LEFTMOST offset inside the k-mer
__host__ __device__ inline uint32_t mini_of_key(uint64_t key, int k, uint32_t *offset)
{
    const int w = k - MINI_M + 1;
    uint32_t best = 0, bo = 0, bx = 0;
    for (int i = 0; i < w; i++) {
        const uint32_t x = (uint32_t)(key >> (2 * i)) & M30;
        const uint32_t h = mmkey(x) & KEY_MASK;
        if (i == 0 || h < best) { best = h; bo = (uint32_t)i; bx = x; }
    }
    *offset = bo;
    return bx;
}

}  // namespace ss

namespace ss { namespace dev {

constexpr int SCAN_THREADS = 256;
constexpr int PPT = 16;                        // k-mer start positions per thread per tile
constexpr int TILE = SCAN_THREADS * PPT;       // bytes of the base stream per tile

// ---------------------------------------------------------------------------------------------
// 16 ASCII bases (4 dwords) -> 32 bits of 2-bit codes (base i at bits 2i) + 16 invalid flags.
// SWAR + byte permute + byte dot products: no per-byte loop, no LDS lookup table, no multiplies.
// ---------------------------------------------------------------------------------------------
// Per dword: code bytes c = (ascii >> 1) & 3; a byte permute looks up the upper-case letter each
// code stands for ('A','C','T','G'), so one xor with the case-folded input leaves a non-zero byte
// exactly where the base is not ACGT/acgt; v_dot4_u32_u8 packs the four 2-bit codes (weights
// 1,4,16,64) and the four flags (weights 1,2,4,8 / 16,..,128 on 0x80 bytes) in one instruction each.
__device__ __forceinline__ void encode16(const uint32_t w[4], uint32_t &code, uint32_t &inv)
{
    uint32_t cb[4], fl[4];
#pragma unroll
    for (int d = 0; d < 4; d++) {
        const uint32_t c = (w[d] >> 1) & 0x03030303u;
        const uint32_t letter = __builtin_amdgcn_perm(0u, 0x47544341u, c);          // code -> 'A' 'C' 'T' 'G'
        const uint32_t diff = (w[d] & 0xDFDFDFDFu) ^ letter;
        fl[d] = (((diff & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | diff) & 0x80808080u;       // 0x80 where the byte is not a base
        cb[d] = __builtin_amdgcn_udot4(c, 0x40100401u, 0u, false);
    }
    code = cb[0] | (cb[1] << 8) | (cb[2] << 16) | (cb[3] << 24);
    const uint32_t lo = __builtin_amdgcn_udot4(fl[1], 0x80402010u, __builtin_amdgcn_udot4(fl[0], 0x08040201u, 0u, false), false);
    const uint32_t hi = __builtin_amdgcn_udot4(fl[3], 0x80402010u, __builtin_amdgcn_udot4(fl[2], 0x08040201u, 0u, false), false);
    inv = (lo | (hi << 8)) >> 7;                                                    // sums are 128 x the flag masks
}

// 16 ASCII bytes (4 dwords) -> bit i set where byte i is '\n' (the record boundaries of ss_reads_support: the invalid flags of
// encode16 do not tell '\n' from N)
__device__ __forceinline__ uint32_t newline_mask16(const uint32_t w[4])
{
    uint32_t m = 0;
#pragma unroll
    for (int d = 0; d < 4; d++) {
        const uint32_t x = w[d] ^ 0x0A0A0A0Au;
        const uint32_t z = ~(((x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | x) & 0x80808080u;     // 0x80 where the byte is '\n'
        m |= __builtin_amdgcn_udot4(z, 0x08040201u, 0u, false) >> 7 << (4 * d);
    }
    return m;
}

// 16 bytes at `off` of the base stream; bytes at or beyond n read as '\n'.
template <bool ALIGNED>
__device__ __forceinline__ void load16(const uint8_t *__restrict__ bases, uint64_t off, uint64_t n,
                                       uint32_t w[4])
{
    if (ALIGNED && off + 16 <= n) {
        // non-temporal: the base stream is read exactly once, and 3 GB of it must not push the 4 MB Bloom filter (and the
        // directory / bucket sectors, which do get re-used) out of L2: 3.45 vs 3.50 ms for 20 M reads
        typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
        const u32x4 q = __builtin_nontemporal_load(reinterpret_cast<const u32x4 *>(bases + off));
        const uint4 v = make_uint4(q.x, q.y, q.z, q.w);
        w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w;
    } else {
#pragma unroll
        for (int d = 0; d < 4; d++) {
            uint32_t x = 0;
#pragma unroll
            for (int b = 0; b < 4; b++) {
                uint64_t p = off + d * 4 + b;
                uint32_t c = (p < n) ? bases[p] : 0x0Au;
                x |= c << (8 * b);
            }
            w[d] = x;
        }
    }
}

// ---------------------------------------------------------------------------------------------
// Input layouts of the scan kernels (their IN template parameter):
//   IN_ASCII          bytes, any alignment (load16<false>)
//   IN_ASCII_ALIGNED  bytes, 16-byte aligned block (load16<true>)
//   IN_PACKED         a packed binned slab (ss_reorder.hip): every 8 positions one 3-byte unit -- u16 of 2-bit codes (position
//                     i at bits 2i, the codes encode16 makes) and a u8 of invalid flags.  Group g of 16 positions is the 6 bytes
//                     at 6g: code[0..15] inv[0..7] code[16..31] inv[8..15], exactly encode16 of the ASCII binned slab's
//                     bytes [16g, 16g + 16).  A device allocation: 4-byte aligned, 8 readable bytes behind its last group.
// `n` counts positions in every layout; positions at or beyond n read as '\n' (code 1, invalid).
// ---------------------------------------------------------------------------------------------
enum { IN_ASCII = 0, IN_ASCII_ALIGNED = 1, IN_PACKED = 2 };

// what load_in fetched for 16 positions: ASCII: the 16 bytes; packed: the two dwords around the group's 6 bytes and the
// byte shift of the group in them (0 or 2, as a byte-selector offset in w[2])
template <int IN>
__device__ __forceinline__ void load_in(const uint8_t *__restrict__ bases, uint64_t off, uint64_t n, uint32_t w[4])
{
    if (IN != IN_PACKED) {
        load16<IN == IN_ASCII_ALIGNED>(bases, off, n, w);
    } else if (off + 16 <= n) {
        // one 8-byte load at the 4-byte-aligned address below 6g (6g is 0 or 2 modulo 4)
        const uint64_t g6 = (off >> 4) * 6u;
        typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
        typedef u32x2 u32x2_a4 __attribute__((aligned(4)));
        const u32x2 q = __builtin_nontemporal_load(reinterpret_cast<const u32x2_a4 *>(bases + (g6 & ~3ull)));
        w[0] = q.x; w[1] = q.y; w[2] = (uint32_t)(g6 & 2u) * 0x01010101u;
    } else {                                             // 16 positions of '\n': code 0x5555 / inv 0xFF per 8, at shift 0
        w[0] = 0x55FF5555u; w[1] = 0x0000FF55u; w[2] = 0u;
    }
}

// 16 positions -> 32 bits of 2-bit codes + 16 invalid flags (encode16 for ASCII; two byte permutes for the packed layout)
template <int IN>
__device__ __forceinline__ void decode_in(const uint32_t w[4], uint32_t &code, uint32_t &inv)
{
    if (IN != IN_PACKED) {
        encode16(w, code, inv);
    } else {
        code = __builtin_amdgcn_perm(w[1], w[0], 0x04030100u + w[2]);                 // bytes s, s+1, s+3, s+4
        inv = __builtin_amdgcn_perm(w[1], w[0], 0x0C0C0502u + (w[2] & 0xFFFFu));      // bytes s+2, s+5 (0x0C: zero)
    }
}

// inclusive prefix sum over the 64 lanes of a wave in the VALU (DPP row shifts + row broadcasts):
// no LDS round trips (ds_bpermute) on the critical path of every tile (scan_mini_kernel, scan_minik_kernel)
__device__ __forceinline__ uint32_t wave_inclusive_sum(uint32_t v)
{
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x111, 0xf, 0xf, false);   // row_shr:1
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x112, 0xf, 0xf, false);   // row_shr:2
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x114, 0xf, 0xf, false);   // row_shr:4
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x118, 0xf, 0xf, false);   // row_shr:8
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x142, 0xa, 0xf, false);   // row_bcast:15 -> rows 1, 3
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x143, 0xc, 0xf, false);   // row_bcast:31 -> rows 2, 3
    return v;
}

// Where record i of a slab of n positions stands (the slab's records are rec0 + i in the numbering of the set): a packed slab's
// record fills the first fixed_len positions of slot i, an ASCII slab's start[rec0 + i] .. end[rec0 + i] say (record_spans_kernel,
// ss_select.hip; they come filled with ~0).  ok: the span is not empty and lies inside the slab.  Whoever reads a record's
// positions asks here first, so that a wild span selects nothing, draws nothing, has no class -- and is never read.  The packed
// test is always true on a well-formed slab, which holds n_rec whole slots; it is made all the same, for every caller alike.
struct RecordSpan { uint64_t s, len; bool ok; };
__device__ __forceinline__ RecordSpan record_span(bool packed, uint64_t i, uint64_t rec0, const unsigned long long *__restrict__ start,
                                                  const unsigned long long *__restrict__ end, uint32_t slot, uint32_t fixed_len, uint64_t n)
{
    if (packed) {
        const uint64_t s = i * (uint64_t)slot, len = fixed_len;
        return {s, len, len > 0 && s + len <= n};
    }
    const uint64_t s = start[rec0 + i], e = end[rec0 + i];
    return {s, e - s, s < e && e <= n};
}

// the close of a length pass: cnt records and their bytes, summed over the wave, added to tot[0] and tot[1]
__device__ __forceinline__ void add_selected(unsigned long long cnt, unsigned long long bytes, unsigned long long *__restrict__ tot)
{
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) { cnt += __shfl_xor(cnt, d, 64); bytes += __shfl_xor(bytes, d, 64); }
    if ((threadIdx.x & 63u) == 0 && cnt) { atomicAdd(&tot[0], cnt); atomicAdd(&tot[1], bytes); }
}

// positions [s, s + 16) of a packed slab (s + 16 <= its positions) as the 16 letters its ASCII form holds inside a record: the
// three 3-byte units around them, fetched as twelve bytes from the first unit on (a packed slab has 8 readable bytes behind its
// last group, IN_PACKED, and its last unit but one begins 6 bytes before the end).  ss_select.hip's gather, ss_resample.hip's digest.
__device__ __forceinline__ uint4 packed_letters16(const uint8_t *__restrict__ pk, uint64_t s)
{
    uint32_t t[3];
    __builtin_memcpy(t, pk + (s >> 3) * 3u, 12);
    const uint32_t sh = (uint32_t)s & 7u;
    const uint64_t lo = (uint64_t)t[0] | ((uint64_t)t[1] << 32);
    uint64_t code = (lo & 0xFFFFull) | (((lo >> 24) & 0xFFFFull) << 16) | ((lo >> 48) << 32);      // bytes 0 1, 3 4, 6 7
    uint32_t inv = (uint32_t)((lo >> 16) & 0xFFull) | (uint32_t)(((lo >> 40) & 0xFFull) << 8) | ((t[2] & 0xFFu) << 16);      // bytes 2, 5, 8
    code >>= 2u * sh;
    inv >>= sh;
    uint32_t w[4];
#pragma unroll
    for (int d = 0; d < 4; d++) {
        uint32_t x = 0;
#pragma unroll
        for (int b = 0; b < 4; b++) {
            const int i = 4 * d + b;
            const uint32_t c = (uint32_t)(code >> (2 * i)) & 3u;
            const uint32_t ch = ((inv >> i) & 1u) ? (uint32_t)'N' : (0x47544341u >> (8u * c)) & 0xFFu;      // "ACTG"[code]
            x |= ch << (8 * b);
        }
        w[d] = x;
    }
    return make_uint4(w[0], w[1], w[2], w[3]);
}

// byte offset of position `pos` (a multiple of 16) in a block of the given layout
__host__ __device__ __forceinline__ uint64_t in_bytes(bool packed, uint64_t pos) { return packed ? (pos >> 4) * 6u : pos; }
// the layout a launch instantiates for a block at `p`
inline int input_layout(const void *p, bool packed)
{
    return packed ? IN_PACKED : ((((uintptr_t)p) & 15) == 0 ? IN_ASCII_ALIGNED : IN_ASCII);
}
// ... handed to the launch as a compile-time value: f(std::integral_constant<int, IN_...>()), so that a launch names its kernel
// once -- scan_kernel<decltype(in)::value, ...> -- whatever the layout; with_bool does the same for a template flag
template <class F>
inline void with_input_layout(const void *p, bool packed, F &&f)
{
    switch (input_layout(p, packed)) {
    case IN_PACKED: f(std::integral_constant<int, IN_PACKED>()); break;
    case IN_ASCII_ALIGNED: f(std::integral_constant<int, IN_ASCII_ALIGNED>()); break;
    default: f(std::integral_constant<int, IN_ASCII>()); break;
    }
}
template <class F>
inline void with_bool(bool v, F &&f)
{
    if (v) f(std::true_type()); else f(std::false_type());
}

}}  // namespace ss::dev
