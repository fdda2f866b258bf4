// The piece copy: how sixteen lanes write one record (or one joined fragment) to an unaligned place of a new slab.  The one copy
// scheme of gather_kernel (ss_select.hip), record_gather_kernel (ss_bam_extract.hip), tag_copy_kernel (ss_bam_tag.hip) and the two
// join_kernels (ss_pairs.hip, ss_bam_pairs.hip).  Not part of the C ABI.
//
// The new slab is 16-byte aligned and holds records back to back: record after record begins wherever the one before ended, and
// the sources are unaligned too.  The destination span [D, E) of a record is cut into the 16-byte ALIGNED pieces it touches,
// a = (D & ~15) + 16 c, and lane l of the record's sixteen takes the pieces c = l, l + 16, ...  What the scheme promises:
//   * Which bytes a lane may write.  Of its piece [a, a + 16) a lane owns [lo, hi) = the piece cut to [D, E), and writes nothing
//     else.  A piece that lies wholly in the span (lo == a, hi == a + 16) is one aligned 16-byte store.  An edge piece, which the
//     record shares with the record before or behind it -- written by other lanes, perhaps of another wave, at the same time --
//     stores its own bytes one by one.  So neighbours never race, and the padding behind the last record is never touched.
//   * Why one clamped load suffices.  The source bytes that belong into a piece stand at source positions [base, base + 16),
//     base = (the source position of the span's first byte) + (a - D): any alignment, and at an edge piece partly in front of
//     the record or behind it, even outside the source block.  The bytes the lane owns, though, are the record's and lie inside
//     the block.  So the lane loads the 16 bytes at q = base clamped into [0, n - 16] -- ONE load, inside the block whatever base
//     is -- and shifts them by base - q bytes: every owned byte was fetched, because it stands in the block and within 16 bytes of
//     base; what the shift brings in from outside is zero and is never stored (or is masked away, or replaced by with_byte).
//   * Why n >= 16 is required.  The clamp's upper end is n - 16; a block below 16 bytes has no place for a 16-byte load, and the
//     callers pad such a block (ss_reads_join_pairs_dev) or refuse it.  A slab of a resident set is padded to a multiple of 16.
// All positions are 64-bit.  The arithmetic is plain C++ and compiles with a host compiler as well: tests/piece_copy_check.cpp
// plays the sixteen lanes over a host buffer, for every alignment, under AddressSanitizer and UBSan.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define SS_PIECE_FN __host__ __device__ __forceinline__
#else
#define SS_PIECE_FN inline
#endif

namespace ss { namespace dev {

typedef unsigned __int128 piece_t;      // the 16 bytes of a piece, byte j in bits [8 j, 8 j + 8)

// bytes [j0, j1) of a piece, 0 <= j0 < j1 <= 16
SS_PIECE_FN piece_t piece_mask(uint32_t j0, uint32_t j1)
{
    return (~(piece_t)0 >> (8u * (16u - (j1 - j0)))) << (8u * j0);
}

// byte j of the result is byte j + shift of x; bytes from outside x are 0 (a shift of 16 bytes and more, either way: all of them)
SS_PIECE_FN piece_t shift_into_piece(piece_t x, int64_t shift)
{
    if (shift >= 16 || shift <= -16) return 0;
    return shift >= 0 ? x >> (8u * (uint32_t)shift) : x << (8u * (uint32_t)-shift);
}

// x with c as its byte j < 16
SS_PIECE_FN piece_t with_byte(piece_t x, uint32_t j, char c)
{
    return (x & ~((piece_t)0xFFu << (8u * j))) | ((piece_t)(uint8_t)c << (8u * j));
}

// where the one load of a piece goes: base clamped into a block of n >= 16 positions
SS_PIECE_FN int64_t clamp_base(int64_t base, uint64_t n)
{
    return base < 0 ? 0 : (base > (int64_t)n - 16 ? (int64_t)n - 16 : base);
}

// the 16 bytes that stand at positions [base, base + 16) of an ASCII block of n >= 16 bytes; positions outside the block read as 0
SS_PIECE_FN piece_t fetch16(const uint8_t *src, uint64_t n, int64_t base)
{
    const int64_t q = clamp_base(base, n);
    piece_t x;
    __builtin_memcpy(&x, src + q, 16);
    return shift_into_piece(x, base - q);
}

// The part of the piece at `a` that one source fills: the source's position s stands at destination P and its bytes go to
// [P, Q); of those the piece owns [lo, hi).  0 where the two do not meet.
SS_PIECE_FN piece_t masked_fetch16(const uint8_t *src, uint64_t n, uint64_t s, uint64_t P, uint64_t Q, uint64_t a, uint64_t lo, uint64_t hi)
{
    const uint64_t l = lo > P ? lo : P, h = hi < Q ? hi : Q;
    if (l >= h) return 0;
    return fetch16(src, n, (int64_t)s + ((int64_t)a - (int64_t)P)) & piece_mask((uint32_t)(l - a), (uint32_t)(h - a));
}

// bytes [lo, hi) of the piece at dst + a (16-byte aligned): one aligned 16-byte store when that is the whole piece, else byte stores
SS_PIECE_FN void store_piece(uint8_t *dst, uint64_t a, uint64_t lo, uint64_t hi, piece_t x)
{
    if (lo == a && hi == a + 16u) {
        __builtin_memcpy(__builtin_assume_aligned(dst + a, 16), &x, 16);
    } else {
        const uint64_t xl = (uint64_t)x, xh = (uint64_t)(x >> 64);
#pragma unroll
        for (uint32_t j = 0; j < 16u; j++)
            if (a + j >= lo && a + j < hi) dst[a + j] = (uint8_t)((j < 8u ? xl >> (8u * j) : xh >> (8u * (j - 8u))) & 0xFFu);
    }
}

// The walk of lane `lane16` (0..15) of the sixteen that write the span [D, E) of dst: piece_of(a, lo, hi) says what the piece at
// `a` holds (only its bytes [lo, hi) matter).  The same for every caller.
template <class PieceOf>
SS_PIECE_FN void write_span(uint8_t *dst, uint64_t D, uint64_t E, uint32_t lane16, PieceOf &&piece_of)
{
    const uint64_t A0 = D & ~15ull, n_pieces = (E - A0 + 15u) >> 4;
    for (uint64_t c = lane16; c < n_pieces; c += 16u) {
        const uint64_t a = A0 + 16u * c;
        const uint64_t lo = a > D ? a : D, hi = a + 16u < E ? a + 16u : E;
        store_piece(dst, a, lo, hi, piece_of(a, lo, hi));
    }
}

// write_span for a span that is a copy: [D, E) of dst = the E - D bytes that stand from position S on in src, a block of n >= 16
// bytes that holds them all, as they are
SS_PIECE_FN void copy_span(uint8_t *dst, uint64_t D, uint64_t E, uint32_t lane16, const uint8_t *src, uint64_t n, uint64_t S)
{
    write_span(dst, D, E, lane16, [&](uint64_t a, uint64_t, uint64_t) { return fetch16(src, n, (int64_t)S + ((int64_t)a - (int64_t)D)); });
}

}}  // namespace ss::dev

#if defined(__HIPCC__)
#include "ss_scan_dev.h"

namespace ss { namespace dev {

// fetch16 from a packed slab of n >= 16 positions: the letters its ASCII form holds there (packed_letters16)
__device__ __forceinline__ piece_t fetch16_packed(const uint8_t *__restrict__ src, uint64_t n, int64_t base)
{
    const int64_t q = clamp_base(base, n);
    const uint4 v = packed_letters16(src, (uint64_t)q);
    piece_t x;
    __builtin_memcpy(&x, &v, 16);
    return shift_into_piece(x, base - q);
}

}}  // namespace ss::dev
#endif
