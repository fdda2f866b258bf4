// What `--tag_bam` adds to the piece copy (ss_piece_copy.h): the piece of a TAGGED record, and the walk over a record's aux fields.
// Used by tag_copy_kernel and aux_check_kernel (ss_bam_tag.hip).  Not part of the C ABI.
//
// A tagged record takes the span [D, D + ol + 14) of the new body, ol = 4 + block_size of the record at source position S:
//   [D, D + 4)            block_size + 14, little-endian           (a value held in a register)
//   [D + 4, D + ol)       the record's bytes S + 4 ..                (masked_fetch16: the one clamped load of the piece)
//   [D + ol, D + ol + 14) t0 t1 'i' <int32 value> t2 t3 'i' <int32 score>   (a value held in a register)
// The rules of ss_piece_copy.h hold unchanged: a lane writes only the bytes [lo, hi) of its piece, which write_span cuts to the
// span; the record's bytes come from one load clamped into the block of n >= 16 bytes; the two register values are shifted to
// their place and masked to it, so nothing of them reaches a byte outside [D, D + 4) and [D + ol, D + ol + 14).
// Plain C++: tests/tag_copy_check.cpp plays the sixteen lanes over a host buffer under AddressSanitizer and UBSan.
#pragma once
#include "ss_piece_copy.h"

namespace ss { namespace dev {

constexpr uint32_t TAG_BYTES = 14;      // SS_BAM_TAG_BYTES (strainscan_hip.h)

// the 14 appended bytes, byte j in bits [8 j, 8 j + 8); tags = t0 | t1 << 8 | t2 << 16 | t3 << 24
SS_PIECE_FN piece_t tag_fields(uint32_t tags, int32_t value, uint32_t score)
{
    const uint64_t v = (uint32_t)value;
    const uint64_t lo = (uint64_t)(tags & 0xFFFFu) | (uint64_t)'i' << 16 | v << 24 | (uint64_t)((tags >> 16) & 0xFFu) << 56;
    const uint64_t hi = (uint64_t)((tags >> 24) & 0xFFu) | (uint64_t)'i' << 8 | (uint64_t)score << 16;
    return (piece_t)lo | (piece_t)hi << 64;
}

// The part of the piece at `a` that a value in a register fills: byte 0 of v stands at destination P and its bytes go to [P, Q),
// Q - P <= 16; of those the piece owns [lo, hi).  0 where the two do not meet.
SS_PIECE_FN piece_t masked_value16(piece_t v, uint64_t P, uint64_t Q, uint64_t a, uint64_t lo, uint64_t hi)
{
    const uint64_t l = lo > P ? lo : P, h = hi < Q ? hi : Q;
    if (l >= h) return 0;
    return shift_into_piece(v, (int64_t)a - (int64_t)P) & piece_mask((uint32_t)(l - a), (uint32_t)(h - a));
}

// piece_of for a tagged record (above): src holds n >= 16 bytes, the record [S, S + ol) lies inside them, ol >= 36
SS_PIECE_FN piece_t tagged_piece(const uint8_t *src, uint64_t n, uint64_t S, uint64_t ol, uint64_t D, piece_t tag, uint64_t a, uint64_t lo,
                                 uint64_t hi)
{
    const piece_t size = (piece_t)(uint32_t)(ol - 4u + TAG_BYTES);
    return masked_value16(size, D, D + 4u, a, lo, hi) | masked_fetch16(src, n, S + 4u, D + 4u, D + ol, a, lo, hi) |
           masked_value16(tag, D + ol, D + ol + TAG_BYTES, a, lo, hi);
}

// The aux fields s[p, end) of a record walked by field: tag[2], type[1], then the value -- A c C 1 byte, s S 2, i I f 4, Z H to a
// NUL, B subtype[1] count[4] and count x size(subtype).  -> AUX_OK, AUX_TAGGED (a field is named t0t1 or t2t3) or AUX_DAMAGED (a
// type that is none of these, or a field that runs past `end`; it wins over AUX_TAGGED).  Advances at least 3 bytes per field and
// reads nothing at or behind `end`.
enum { AUX_OK = 0, AUX_TAGGED = 1, AUX_DAMAGED = 2 };
SS_PIECE_FN uint32_t aux_type_size(uint32_t c)
{
    return (c == 'A' || c == 'c' || c == 'C') ? 1u : (c == 's' || c == 'S') ? 2u : (c == 'i' || c == 'I' || c == 'f') ? 4u : 0u;
}
SS_PIECE_FN uint32_t aux_walk(const uint8_t *s, uint64_t p, uint64_t end, uint32_t tags)
{
    const uint32_t ta = tags & 0xFFFFu, tb = tags >> 16;
    uint32_t found = AUX_OK;
    while (p < end) {
        if (end - p < 3u) return AUX_DAMAGED;
        const uint32_t name = (uint32_t)s[p] | (uint32_t)s[p + 1] << 8, type = s[p + 2];
        p += 3u;
        if (name == ta || name == tb) found = AUX_TAGGED;
        const uint32_t fixed = aux_type_size(type);
        if (fixed) {
            if (end - p < fixed) return AUX_DAMAGED;
            p += fixed;
        } else if (type == 'Z' || type == 'H') {
            while (p < end && s[p]) p++;
            if (p >= end) return AUX_DAMAGED;      // no NUL
            p++;
        } else if (type == 'B') {
            if (end - p < 5u) return AUX_DAMAGED;
            const uint64_t size = s[p] == 'A' ? 0u : aux_type_size(s[p]);      // (c C s S i I f: 'A' is no subtype)
            const uint64_t count = (uint64_t)s[p + 1] | (uint64_t)s[p + 2] << 8 | (uint64_t)s[p + 3] << 16 | (uint64_t)s[p + 4] << 24;
            p += 5u;
            if (!size || count * size > end - p) return AUX_DAMAGED;
            p += count * size;
        } else return AUX_DAMAGED;
    }
    return found;
}

}}  // namespace ss::dev
