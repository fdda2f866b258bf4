// ss_minik.hip -- the page index of ss_mini.hip scanned with k at run time: one lane per start position.
#include "ss_common.h"
#include "ss_scan_dev.h"

#include <algorithm>

using namespace ss::dev;

namespace ss {

// ---------------------------------------------------------------------------------------------
// The page index at ANY k from 17 to 30 (round 6; `-k`, StrainScan.py:136,266-271, reaches the layer-2 scans:
// Vote_Strain_L2_Lasso_new_sp.py:359-371).  Until now every k but 31 went through the flat table (ss_scan.hip): one random
// 64-byte sector per k-mer, 0.08 of the HBM peak by SURVEY 8(d)'s bytes.  The index itself never depended on k = 31 -- a
// k-mer has k - 14 m-mers, its flank k - 15 bases (<= 32 bits), offsets 0..k-15 (<= 17 mask bits) -- only scan_mini_kernel
// (ss_mini.hip) does, in every phase (17-m-mer windows split over two lanes, 16-lane candidate checks, the combining table).  This kernel is
// the plain statement of the same lookups with k as a run-time value: ONE LANE PER START POSITION.  The m-mer keys of a
// 1024-position tile go to LDS once; a position takes the minimum of its k - 14 keys (leftmost on ties, as the build),
// mixes the minimizer, reads the head of its page and settles its own k-mer against the slots that match.  Consecutive
// positions of a read share their minimizer for ~(k - 14) / 2 positions and sit in neighbouring lanes: their page loads are
// the same address in one wave instruction -- one sector from L2 / HBM per run, as there, with no run queues at all.
// ~70 lane instructions per position at k = 25 against the tuned kernel's 45 at k = 31.
// ---------------------------------------------------------------------------------------------
constexpr int KT = 64, KPOS = 1024, KW = KPOS / 16 + 3;      // one wave per workgroup; start positions per tile; 16-base code words per tile (tile + 48 bases)
constexpr int KQ = 320;                                       // candidates (positions whose page has a slot with their tag) queued at a time:
                                                              // a round of 256 positions adds at most 256 to fewer than 64
struct KShared {
    uint32_t code[KW + 1];
    alignas(8) uint16_t inv[KW + 5];
    alignas(16) uint32_t key[KPOS + 32];
    uint2 q[KQ];                                              // position | minimizer offset << 10, h
};

// Where a found k-mer goes (the SINK of scan_minik_kernel).  CountSink: 1 to its counter in the table -- the scan.  SupportSink
// (ss_reads_support, ss_support.hip): the bit of its start position in a bitmap of the tile in LDS; the tile's tail walks the
// bitmap beside the record boundaries and adds the hits to rec_hits, one atomic per (lane, record).  LabelSink
// (ss_reads_support_labeled, ss_label.hip): the LABEL of its slot (slot_label[], indexed like the counters; 0 = none) in a 4-bit
// field per position; the tail does the same walk once per label the lane's 16 positions hold, into that label's slice of
// rec_hits.  The lookup itself -- the one statement of the page format with k at run time -- is the same code for all three.
// PER_POS: the bits a position has in the tile's LDS (0: none, no tail).
struct CountSink {
    static constexpr int PER_POS = 0;
    uint32_t *__restrict__ counts;
    uint32_t cbase;
    __device__ __forceinline__ void bucket(uint32_t slot, uint32_t *, uint32_t) const { atomicAdd(&counts[slot], 1u); }
    __device__ __forceinline__ void inline_slot(uint32_t page_slot, uint32_t *, uint32_t) const { atomicAdd(&counts[cbase + page_slot], 1u); }
};
struct SupportSink {
    static constexpr int PER_POS = 1;
    ss::SupportArgs a;
    __device__ __forceinline__ void bucket(uint32_t, uint32_t *bits, uint32_t p) const { atomicOr(&bits[p >> 5], 1u << (p & 31u)); }
    __device__ __forceinline__ void inline_slot(uint32_t, uint32_t *bits, uint32_t p) const { atomicOr(&bits[p >> 5], 1u << (p & 31u)); }
};
struct LabelSink {
    static constexpr int PER_POS = 4;
    ss::SupportArgs a;                          // rec_hits: [n_labels][rec_limit]
    const uint8_t *__restrict__ slot_label;     // [n_slots] 0 or 1..n_labels
    uint32_t cbase, n_labels;
    __device__ __forceinline__ void mark(uint32_t l, uint32_t *bits, uint32_t p) const { if (l) atomicOr(&bits[p >> 3], l << (4u * (p & 7u))); }
    __device__ __forceinline__ void bucket(uint32_t slot, uint32_t *bits, uint32_t p) const { mark(slot_label[slot], bits, p); }
    __device__ __forceinline__ void inline_slot(uint32_t page_slot, uint32_t *bits, uint32_t p) const { mark(slot_label[cbase + page_slot], bits, p); }
};
static_assert(SS_LABELS_MAX <= 15, "a position's label is a 4-bit field");
// ClassSink (ss_reads_classify, ss_classify.hip): the NODE of its slot (slot_node[], indexed like the counters; 0 = none) in a
// 16-bit field per position, a plain LDS store; a hit whose slot has no node sets the bit of its position in a bitmap behind the
// fields.  Its tail knows no records: a lane writes the sixteen fields of the positions it decoded to pos_node[] of the slab (two
// 16-byte stores, every position of every tile written, so the array needs no clearing) and the bitmap's bits go to *hits0.
struct ClassSink {
    static constexpr int PER_POS = 16;
    uint16_t *__restrict__ pos_node;            // [n_tiles * KPOS] node of the hit at each position of the slab, 0 = none
    const uint16_t *__restrict__ slot_node;     // [n_slots] 0 or 1..n_nodes
    unsigned long long *__restrict__ hits0;     // += hits whose slot has node 0
    uint32_t cbase;
    __device__ __forceinline__ void mark(uint32_t v, uint32_t *bits, uint32_t p) const
    {
        if (v) reinterpret_cast<uint16_t *>(bits)[p] = (uint16_t)v;
        else atomicOr(&bits[KPOS / 2 + (p >> 5)], 1u << (p & 31u));
    }
    __device__ __forceinline__ void bucket(uint32_t slot, uint32_t *bits, uint32_t p) const { mark(slot_node[slot], bits, p); }
    __device__ __forceinline__ void inline_slot(uint32_t page_slot, uint32_t *bits, uint32_t p) const { mark(slot_node[cbase + page_slot], bits, p); }
};
static_assert(SS_CLASS_NODES_MAX <= 0xFFFF, "a position's node is a 16-bit field");
static_assert(SS_STRAIN_SET_MAX <= 16, "... or a mask of called strains (ss_strain_sets.hip), a bit per strain");
// WeightSink (ss_scan_reads_resampled, ss_scan_resampled.hip): the counts of up to sixteen bootstrap replicates from one pass.
// A found k-mer adds the WEIGHTS of its record -- a 64-bit word of 4-bit fields, one per replicate -- to the replicates' own
// slot counters, one atomic per field that is not zero.  It needs the record of a hit when the hit is found (the drains keep
// the lanes in position order: the atomics of one replicate land on neighbouring counters, as the scan's do), so the tile's
// head leaves a record directory in LDS instead of hit bits, and there is no tail: ctx[0..1] = the record of the tile's first
// position; packed: ctx[2] = that position's offset in its slot; ASCII: ctx[CTX_REL + l] = record ends in the tile before the 16
// positions of lane l, and the low / high half of ctx[CTX_BND + l / 2] = the bit of each of those positions that is a record end.
constexpr int PER_POS_CTX = 64;             // the PER_POS of a sink that keeps a record directory, not bits per position
constexpr int CTX_REL = 4, CTX_BND = CTX_REL + KT, CTX_WORDS = CTX_BND + KT / 2;
struct WeightSink {
    static constexpr int PER_POS = PER_POS_CTX;
    ss::ResampledArgs a;
    uint32_t cbase;
    __device__ __forceinline__ void add(uint32_t slot, const uint32_t *ctx, uint32_t p) const
    {
        uint64_t rec = (uint64_t)ctx[0] | ((uint64_t)ctx[1] << 32);
        if (a.slot) rec += (ctx[2] + p) / a.slot;
        else rec += ctx[CTX_REL + (p >> 4)] + (uint32_t)__popc((ctx[CTX_BND + (p >> 5)] >> (p & 16u)) & ((1u << (p & 15u)) - 1u));
        if (rec >= a.rec_limit) return;
        uint32_t *__restrict__ c = a.counts + slot;
        for (uint64_t w = a.weights[rec]; w; c += a.stride, w >>= 4)
            if (w & 15u) atomicAdd(c, (uint32_t)(w & 15u));
    }
    __device__ __forceinline__ void bucket(uint32_t slot, uint32_t *ctx, uint32_t p) const { add(slot, ctx, p); }
    __device__ __forceinline__ void inline_slot(uint32_t page_slot, uint32_t *ctx, uint32_t p) const { add(cbase + page_slot, ctx, p); }
};
static_assert(SS_SCAN_REPLICATES_MAX <= 16, "a record's weights are 4-bit fields of one 64-bit word");
// the tile's LDS: the sinks with a tail add the positions' bits and the '\n' flags of the tile's bytes (nl[0]: bit 15 = the byte before the tile)
// (LEAN: no '\n' flags -- the label sink over a packed slab, which has no '\n': the 132 bytes are what keeps the 21st one-wave
// workgroup on a CU)
template <int PER_POS, bool LEAN> struct KSharedT : KShared {
    static constexpr int HIT_WORDS = KPOS * PER_POS / 32;
    uint32_t hit[HIT_WORDS];
    uint16_t nl[KT + 2];
    __device__ __forceinline__ uint32_t *bits() { return hit; }
};
template <> struct KSharedT<4, true> : KShared {
    static constexpr int HIT_WORDS = KPOS * 4 / 32;
    uint32_t hit[HIT_WORDS];
    __device__ __forceinline__ uint32_t *bits() { return hit; }
};
template <bool LEAN> struct KSharedT<16, LEAN> : KShared {      // the class sink: 16-bit fields, then a bit per position; no '\n' flags
    static constexpr int HIT_WORDS = KPOS / 2 + KPOS / 32;
    alignas(16) uint32_t hit[HIT_WORDS];
    __device__ __forceinline__ uint32_t *bits() { return hit; }
};
template <bool LEAN> struct KSharedT<PER_POS_CTX, LEAN> : KShared {      // the weight sink: the tile's record directory
    static constexpr int HIT_WORDS = CTX_WORDS;
    alignas(8) uint32_t hit[HIT_WORDS];
    __device__ __forceinline__ uint32_t *bits() { return hit; }
};
template <bool LEAN> struct KSharedT<0, LEAN> : KShared { __device__ __forceinline__ uint32_t *bits() { return nullptr; } };

// The hits of a lane's 16 positions to their records: h has PER bits per position (the lowest one set where there is a hit), bnd
// a bit per position where the record index steps up, r is the record of the first position.  add(record, hits) once per record
// with hits.
template <int PER, class T, class ADD>
__device__ __forceinline__ void hits_to_records(T h, uint32_t bnd, uint64_t r, const ADD &add)
{
    for (uint32_t b = bnd; h; r++) {
        const uint32_t nb = b ? (b & (0u - b)) : 0x10000u;      // the positions before the next boundary
        T below;
        if constexpr (PER == 1) below = nb - 1u;
        else below = b ? ((T)1 << (PER * ((uint32_t)__ffs(b) - 1u))) - (T)1 : ~(T)0;
        const uint32_t c = sizeof(T) == 8 ? (uint32_t)__popcll(h & below) : (uint32_t)__popc((uint32_t)(h & below));
        if (c) add(r, c);
        h &= ~below;
        b &= ~nb;
    }
}

// How the time of a first version went (4 M reads, k = 25, profiles/r06_ab_log.md): one lane per position, four positions of a
// thread one after the other: 4.0 ms -- 1.9 of it the minimizers (a loop of k - 14 dependent LDS reads per position at five waves
// per SIMD), 0.2 the page sectors, 2.4 the slots: 4 % of the positions hit, so nearly every wave walked the whole hit path, four
// times per tile.  Hence: a lane owns FOUR ADJACENT positions and reads their k - 11 keys once, as five 16-byte LDS loads (the
// four windows share all but three keys on either side); the four page heads are in flight together; positions whose page shows
// their tag (or is full) are compacted into an LDS queue with ballots and settled ONCE per tile, one candidate per lane.
template <int IN, bool BLOOM, class SINK>
__global__ __launch_bounds__(KT) void scan_minik_kernel(const uint8_t *__restrict__ bases, uint64_t n, uint64_t n_tiles, int k,
                                                        const uint64_t *__restrict__ mkeys, const uint4 *__restrict__ pages, uint32_t n_pages,
                                                        const SINK sink, const uint32_t *__restrict__ bloom, uint32_t bloom_shift)
{
    __shared__ KSharedT<SINK::PER_POS, SINK::PER_POS == 4 && IN == IN_PACKED> S;
    const int t = threadIdx.x;
    const uint32_t W = (uint32_t)(k - ss::MINI_M + 1), F = W - 1u;      // m-mers per k-mer (3..17), flank bases
    const uint64_t kmask = (1ull << (2 * k)) - 1ull, vmask = (1ull << k) - 1ull;
    // one k-mer against the slots of its minimizer's page(s): position p of the tile, minimizer offset o, h = mix30(minimizer)
    auto settle = [&](uint32_t p, uint32_t o, uint32_t h, uint32_t page) {
        const uint32_t w0 = p >> 4, sh = 2 * (p & 15);
        const uint32_t lo = __builtin_amdgcn_alignbit(S.code[w0 + 1], S.code[w0], sh), hi = __builtin_amdgcn_alignbit(S.code[w0 + 2], S.code[w0 + 1], sh);
        const uint64_t key = (((uint64_t)hi << 32) | lo) & kmask;      // bases p .. p + k - 1, base i at bits 2 i
        const uint32_t tt = (h & 0xFFu) * 0x01010101u;
        bool full;
        do {
            const uint4 tg = pages[(uint64_t)page * 4u];                        // (in L1 / L2: the lookup has just read it)
            const uint32_t x0 = tg.x ^ tt, x1 = tg.y ^ tt;                      // zero byte = tag8 matches
            const uint32_t z0 = ~(((x0 & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | x0) & 0x80808080u;
            const uint32_t z1 = ~(((x1 & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | x1) & 0x80808080u;
            uint32_t hit = (z0 >> 7) | (z1 >> 3);                               // slot s at bit 8 (s & 3) + 4 (s >> 2)
            const char *pb = reinterpret_cast<const char *>(pages) + (uint64_t)page * 64u;
            while (hit) {
                const uint32_t b = (uint32_t)__ffs(hit) - 1u, sl = (b >> 3) + (b & 4u);
                hit &= hit - 1u;
                const uint32_t hi8 = (((b & 4u) ? tg.w : tg.z) >> (b & 24u)) & 0xFFu;
                if (hi8 & 0x80u) {                                              // bucket reference
                    if ((hi8 ^ (h >> 8)) & 0x3Fu) continue;
                    const uint32_t l32 = reinterpret_cast<const uint32_t *>(pb + 16)[sl];
                    const uint32_t mask = reinterpret_cast<const uint16_t *>(pb + 48)[sl] | ((hi8 & 0x40u) << 10);
                    const uint32_t bstart = l32 & ss::START_MASK;
                    bool found = false;
                    if ((mask >> o) & 1u) {
                        const uint32_t cpos = bstart + 1u + (uint32_t)__popc(mask & ((1u << o) - 1u));
                        if (mkeys[cpos] == key) { sink.bucket(cpos, S.bits(), p); found = true; }
                    }
                    if (!found && (l32 >> 31)) {                                // several k-mers per offset: look through the bucket
                        const uint32_t cnt = (uint32_t)(mkeys[bstart] >> 32);
                        for (uint32_t c = 0; c < cnt; c++)
                            if (mkeys[bstart + 1u + c] == key) { sink.bucket(bstart + 1u + c, S.bits(), p); break; }
                    }
                } else if ((hi8 & 31u) == F - o) {                              // an inline k-mer with this minimizer offset
                    const uint32_t mid = reinterpret_cast<const uint16_t *>(pb + 48)[sl];
                    if ((mid >> 4) == ((h >> 8) & 0xFFFu) && reinterpret_cast<const uint32_t *>(pb + 16)[sl] == ss::flank_of_key_k(key, o, k))
                        sink.inline_slot(page * 8u + sl, S.bits(), p);
                }
            }
            full = (tg.w >> 24) != (uint32_t)ss::PG_EMPTY_HI;
            page++;                                                             // (the build guarantees a non-full page before the array ends)
        } while (full);
    };
    for (uint64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const uint64_t b0 = tile * (uint64_t)KPOS;
        __syncthreads();                                   // (the tile before is done with S)
        // ---- bases -> codes + invalid flags: 16 bases per lane, the 48 behind the tile by lanes 0..2
        {
            uint32_t w[4], code, inv;
            load_in<IN>(bases, b0 + (uint64_t)t * 16, n, w);
            decode_in<IN>(w, code, inv);
            S.code[t] = code;
            S.inv[t] = (uint16_t)inv;
            if constexpr (SINK::PER_POS == PER_POS_CTX) {
                // the record directory of the weight sink (read by the drains, behind the barriers below)
                const ss::ResampledArgs &A = sink.a;
                if constexpr (IN == IN_PACKED) {
                    if (t == 0) {
                        const uint64_t q = b0 / A.slot, r0 = A.rec_base + q;
                        S.hit[0] = (uint32_t)r0;
                        S.hit[1] = (uint32_t)(r0 >> 32);
                        S.hit[2] = (uint32_t)(b0 - q * A.slot);
                    }
                } else {
                    const uint32_t nl = newline_mask16(w), before = (uint32_t)__shfl_up((int)nl, 1, 64) >> 15;
                    const uint32_t prev = t ? (before & 1u) : ((b0 == 0 || bases[b0 - 1] == 0x0Au) ? 1u : 0u);      // (a slab begins behind a boundary)
                    const uint32_t bnd = nl & ~((nl << 1) | prev) & 0xFFFFu, mine = (uint32_t)__popc(bnd);
                    S.hit[CTX_REL + t] = wave_inclusive_sum(mine) - mine;
                    reinterpret_cast<uint16_t *>(&S.hit[CTX_BND])[t] = (uint16_t)bnd;
                    if (t == 0) {
                        const uint64_t r0 = A.rec_base + A.tile_base[tile];
                        S.hit[0] = (uint32_t)r0;
                        S.hit[1] = (uint32_t)(r0 >> 32);
                    }
                }
            } else if constexpr (SINK::PER_POS != 0) {
                for (int i = t; i < S.HIT_WORDS; i += KT) S.hit[i] = 0u;
                if constexpr (IN != IN_PACKED && SINK::PER_POS != 16) {
                    S.nl[t + 1] = (uint16_t)newline_mask16(w);
                    if (t == 0) S.nl[0] = (b0 == 0 || bases[b0 - 1] == 0x0Au) ? 0x8000u : 0u;      // (a slab begins behind a boundary)
                }
            }
            if (t < 3) {
                load_in<IN>(bases, b0 + (uint64_t)(KT + t) * 16, n, w);
                decode_in<IN>(w, code, inv);
                S.code[KT + t] = code;
                S.inv[KT + t] = (uint16_t)inv;
            } else if (t < 8) {
                if (t == 3) S.code[KW] = 0u;
                S.inv[KT + t] = 0xFFFFu;
            }
        }
        __syncthreads();
        // ---- ordering keys of the m-mers that start in the lane's 16 bases (and the 16 behind the tile: lanes 0..15, one each)
        {
            const uint32_t c0 = S.code[t], c1 = S.code[t + 1];
            uint32_t kk[16];
            kk[0] = ss::mmkey(c0) & ss::KEY_MASK;
#pragma unroll
            for (int i = 1; i < 16; i++) kk[i] = ss::mmkey(__builtin_amdgcn_alignbit(c1, c0, 2 * i)) & ss::KEY_MASK;      // (mmkey looks at the low 24 bits only)
#pragma unroll
            for (int i = 0; i < 4; i++) reinterpret_cast<uint4 *>(&S.key[16 * t])[i] = make_uint4(kk[4 * i], kk[4 * i + 1], kk[4 * i + 2], kk[4 * i + 3]);
            if (t < 16) {
                const uint32_t q = (uint32_t)KPOS + (uint32_t)t;
                S.key[q] = ss::mmkey(__builtin_amdgcn_alignbit(S.code[(q >> 4) + 1], S.code[q >> 4], 2 * (q & 15))) & ss::KEY_MASK;
            } else if (t < 32) {
                S.key[KPOS + t] = 0xFFFFFFFFu;
            }
        }
        __syncthreads();
        uint32_t nq = 0;                                   // candidates queued (the same in every lane)
#pragma unroll 1
        for (uint32_t g = 0; g <= (uint32_t)(KPOS / (4 * KT)); g++) {
            if (g < (uint32_t)(KPOS / (4 * KT))) {
            const uint32_t p0 = 4u * ((uint32_t)t + (uint32_t)KT * g);
            // the 20 keys from p0 on, each tagged with its distance from p0 in its five free low bits: ONE v_min decides key
            // and leftmost position.  Window j = keys j .. j + W - 1 = {j..2} + {3..W-1} (common to the four) + {W..W+j-1}
            // (W is the same for the whole launch: the loops below leave through SCALAR branches -- no lane predicate, one v_min per key)
            uint32_t K[20];
#pragma unroll
            for (int i = 0; i < 5; i++) {
                if (i && (uint32_t)(4 * i) >= W) break;
                const uint4 v = reinterpret_cast<const uint4 *>(&S.key[p0])[i];
                K[4 * i] = v.x | (uint32_t)(4 * i); K[4 * i + 1] = v.y | (uint32_t)(4 * i + 1);
                K[4 * i + 2] = v.z | (uint32_t)(4 * i + 2); K[4 * i + 3] = v.w | (uint32_t)(4 * i + 3);
            }
            const uint32_t T0 = S.key[p0 + W] | W, T1 = S.key[p0 + W + 1u] | (W + 1u), T2 = S.key[p0 + W + 2u] | (W + 2u);
            uint32_t common = 0xFFFFFFFFu;
#pragma unroll
            for (int i = 3; i < 17; i++) {
                if ((uint32_t)i >= W) break;
                common = min(common, K[i]);
            }
            uint32_t m_[4];
            m_[0] = min(min(K[0], K[1]), min(K[2], common));
            m_[1] = min(min(K[1], K[2]), min(common, T0));
            m_[2] = min(min(K[2], common), min(T0, T1));
            m_[3] = min(min(common, T0), min(T1, T2));
            uint64_t iv;
            __builtin_memcpy(&iv, &S.inv[p0 >> 4], 8);
            iv >>= (p0 & 15u);
            uint32_t h_[4], page_[4];
            uint4 tg_[4];
            bool go_[4];
#pragma unroll
            for (int j = 0; j < 4; j++) {
                go_[j] = ((iv >> j) & vmask) == 0;          // live: the k bases from p0 + j on are all ACGT (bytes beyond the block read as '\n')
                const uint32_t q = p0 + (m_[j] & 31u);       // tile position of the minimizer
                const uint32_t x = __builtin_amdgcn_alignbit(S.code[(q >> 4) + 1], S.code[q >> 4], 2 * (q & 15)) & ss::M30;
                h_[j] = ss::mix30(x);
                page_[j] = ss::page_of(h_[j], n_pages);
            }
            if (BLOOM) {
                uint32_t bw[4];
#pragma unroll
                for (int j = 0; j < 4; j++) bw[j] = go_[j] ? bloom[h_[j] >> (bloom_shift + 5)] : 0u;
#pragma unroll
                for (int j = 0; j < 4; j++) go_[j] = go_[j] && ((bw[j] >> ((h_[j] >> bloom_shift) & 31u)) & 1u);
            }
#pragma unroll
            for (int j = 0; j < 4; j++) {
                tg_[j] = make_uint4(0xFFFFFFFFu, 0xFFFFFFFFu, 0x7F7F7F7Fu, 0x7F7F7F7Fu);      // (an empty page: nothing matches, not full)
                if (go_[j]) tg_[j] = pages[(uint64_t)page_[j] * 4u];
            }
            bool cand_[4];
#pragma unroll
            for (int j = 0; j < 4; j++) {
                // a candidate: some slot of the page carries the minimizer's tag8 AND is either an inline k-mer with THIS k-mer's
                // minimizer offset (hi8 == e = F - o) or a bucket reference with the minimizer's filter bits (hi8 = 0x80 | mask bit
                // 16 << 6 | h[13:8]) -- all eight slots at once, on the 16 bytes the lookup has read (a read k-mer shares its
                // minimizer with a database k-mer six times as often as it IS one); or the page is full (its slots may go on)
                auto zb = [](uint32_t x) { return ~(((x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | x) & 0x80808080u; };      // 0x80 where a byte is zero
                const uint32_t tt = (h_[j] & 0xFFu) * 0x01010101u;
                const uint32_t e4 = (F + (uint32_t)j - (m_[j] & 31u)) * 0x01010101u, r4 = (0x80u | ((h_[j] >> 8) & 0x3Fu)) * 0x01010101u;
                const uint32_t c0 = zb(tg_[j].x ^ tt) & (zb(tg_[j].z ^ e4) | zb((tg_[j].z ^ r4) & 0xBFBFBFBFu));
                const uint32_t c1 = zb(tg_[j].y ^ tt) & (zb(tg_[j].w ^ e4) | zb((tg_[j].w ^ r4) & 0xBFBFBFBFu));
                cand_[j] = go_[j] && ((c0 | c1) != 0u || (tg_[j].w >> 24) != (uint32_t)ss::PG_EMPTY_HI);
            }
            // The queue is kept in POSITION order (a lane's candidates side by side, the lanes in order: a wave prefix sum of the
            // lanes' counts), so that the lanes of a drain hold neighbouring positions: the k-mers of a run hit neighbouring
            // counters of ONE bucket, and what an atomic costs on this chip is (instruction, 64-byte line) pairs (27 G/s,
            // profiles/r04_atomics_micro_*.txt).  Queued position class by position class (0, 4, 8, ... then 1, 5, 9, ...) a cluster
            // table's 111 hits per read were ~1.5 hits per pair: 18 ms per 8 M reads.
            {
                const uint32_t mine = (uint32_t)cand_[0] + (uint32_t)cand_[1] + (uint32_t)cand_[2] + (uint32_t)cand_[3];
                const uint32_t incl = wave_inclusive_sum(mine);
                uint32_t idx = nq + incl - mine;
#pragma unroll
                for (int j = 0; j < 4; j++)
                    if (cand_[j]) S.q[idx++] = make_uint2((p0 + (uint32_t)j) | (((m_[j] & 31u) - (uint32_t)j) << 10), h_[j]);
                nq += (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
            }
            }
            // ---- the candidates, one per lane, whenever a wave's worth has come together (and at the end of the tile)
            if (nq >= (uint32_t)KT || g == (uint32_t)(KPOS / (4 * KT))) {
                __syncthreads();
                for (uint32_t e = (uint32_t)t; e < nq; e += KT) {
                    const uint2 c = S.q[e];
                    settle(c.x & 1023u, c.x >> 10, c.y, ss::page_of(c.y, n_pages));
                }
                __syncthreads();
                nq = 0;
            }
        }
        // ---- support: the tile's hit bits to the records.  A lane takes the 16 positions it decoded: `bnd` has a bit where the record
        // index steps up (ASCII: a record end, a '\n' behind a byte that is none -- no k-mer starts there; packed: the first
        // position of a slot), r is the record of its first position: the tile's base + the boundaries of the lanes before (a wave
        // prefix sum), or position / slot.  One atomic per (lane, record) with hits: neighbouring lanes, neighbouring words.
        if constexpr (SINK::PER_POS == 16) {
            // ---- classes: the lane's sixteen node fields to the slab's pos_node (32 bytes, the wave's 2 KB in one piece); the hits
            // without a node are counted, one vector atomic per tile that has any
            uint4 *__restrict__ dst = reinterpret_cast<uint4 *>(sink.pos_node + b0 + 16u * (uint32_t)t);
            dst[0] = reinterpret_cast<const uint4 *>(S.hit)[2 * t];
            dst[1] = reinterpret_cast<const uint4 *>(S.hit)[2 * t + 1];
            uint32_t c = t < KPOS / 32 ? (uint32_t)__popc(S.hit[KPOS / 2 + t]) : 0u;
#pragma unroll
            for (int d = 32; d > 0; d >>= 1) c += __shfl_xor(c, d, 64);
            if (t == 0 && c) atomicAdd(sink.hits0, (unsigned long long)c);
        } else if constexpr (SINK::PER_POS != 0 && SINK::PER_POS != PER_POS_CTX) {
            const ss::SupportArgs &A = sink.a;
            uint32_t bnd = 0;
            uint64_t r = A.rec_base;
            if constexpr (IN == IN_PACKED) {
                const uint64_t q = b0 / A.slot;
                const uint32_t rem0 = (uint32_t)(b0 - q * A.slot) + 16u * (uint32_t)t;
                uint32_t rem = rem0 % A.slot;
                r += q + rem0 / A.slot;
#pragma unroll
                for (int i = 1; i < 16; i++)
                    if (++rem == A.slot) { rem = 0; bnd |= 1u << i; }
            } else {
                const uint32_t nl = S.nl[t + 1];
                bnd = nl & ~((nl << 1) | (uint32_t)(S.nl[t] >> 15)) & 0xFFFFu;
                const uint32_t mine = (uint32_t)__popc(bnd);
                r += A.tile_base[tile] + wave_inclusive_sum(mine) - mine;
            }
            if constexpr (SINK::PER_POS == 1) {
                const uint32_t hits = (S.hit[t >> 1] >> (16 * (t & 1))) & 0xFFFFu;
                hits_to_records<1>(hits, bnd, r, [&](uint64_t rec, uint32_t c) { if (rec < A.rec_limit) atomicAdd(&A.rec_hits[rec], c); });
            } else {
                // the lane's sixteen 4-bit labels; label by label (mostly none, or one): the positions that carry it, walked as above
                uint64_t v = (uint64_t)S.hit[2 * t] | ((uint64_t)S.hit[2 * t + 1] << 32);
                while (v) {
                    const uint32_t j = (uint32_t)(v >> (((uint32_t)__ffsll((unsigned long long)v) - 1u) & ~3u)) & 15u;
                    const uint64_t x = v ^ ((uint64_t)j * 0x1111111111111111ull);
                    const uint64_t z = ~(x | (x >> 1) | (x >> 2) | (x >> 3)) & 0x1111111111111111ull;      // bit 4 i: position i has label j
                    if (j <= sink.n_labels) {
                        uint32_t *__restrict__ rh = A.rec_hits + (uint64_t)(j - 1u) * A.rec_limit;
                        hits_to_records<4>(z, bnd, r, [&](uint64_t rec, uint32_t c) { if (rec < A.rec_limit) atomicAdd(&rh[rec], c); });
                    }
                    v &= ~(z * 15ull);
                }
            }
        }
    }
}

// One launch of scan_minik_kernel over a flat block of n positions, with the sink that says where a found k-mer goes.
// (one-wave workgroups, grid stride; 8 K / 32 K / 131 K / 300 K / 600 K of them: 2.56 / 2.37 / 2.31 / 2.30 / 2.29 ms per 4 M reads at k = 25)
template <class SINK>
static int launch_minik(const ss_db *db, const uint8_t *b, uint64_t n, bool packed, const SINK &sink, hipStream_t stream)
{
    const uint64_t n_tiles = (n + KPOS - 1) / KPOS;
    const unsigned blocks = (unsigned)std::min<uint64_t>(n_tiles, (uint64_t)256 * 32 * 16);
    with_input_layout(b, packed, [&](auto in) {
        with_bool(multi_kind(db) == MULTI_BLOOM, [&](auto bloom) {
            hipLaunchKernelGGL((scan_minik_kernel<decltype(in)::value, decltype(bloom)::value, SINK>), dim3(blocks), dim3(KT), 0, stream, b, n, n_tiles,
                               db->k, db->d_mkeys, reinterpret_cast<const uint4 *>(db->d_dir), db->n_dir, sink, db->d_bloom, 30u - db->bloom_bits);
        });
    });
    SS_HIP(hipGetLastError());
    return SS_OK;
}

// the scan: a found k-mer adds 1 to its counter in the table (launch_scan_mini, ss_mini.hip, says when a table comes here)
int launch_scan_minik(ss_db *db, const uint8_t *b, uint64_t n, hipStream_t stream, bool packed)
{
    return launch_minik(db, b, n, packed, CountSink{db->d_counts, (uint32_t)db->n_mslots}, stream);
}

// the same lookups for ss_reads_support: every k from 17 to 31 goes through the per-position kernel, whose sink marks positions
// instead of counting k-mers; the table's counters are not touched
int launch_support_minik(const ss_db *db, const void *bases_dev, uint64_t n, bool packed, const SupportArgs &a, hipStream_t stream)
{
    if (!n || db->layout != 1 || (packed ? a.slot == 0 : a.tile_base == nullptr)) return SS_EINVAL;
    return launch_minik(db, (const uint8_t *)bases_dev, n, packed, SupportSink{a}, stream);
}

// ... and for ss_reads_support_labeled (ss_label.hip): a found k-mer counts for the label of its slot, in that label's slice of
// a.rec_hits ([n_labels][a.rec_limit]); slot_label is indexed like the table's counters
int launch_label_minik(const ss_db *db, const void *bases_dev, uint64_t n, bool packed, const SupportArgs &a, const uint8_t *slot_label,
                       uint32_t n_labels, hipStream_t stream)
{
    if (!n || db->layout != 1 || (packed ? a.slot == 0 : a.tile_base == nullptr)) return SS_EINVAL;
    if (!slot_label || n_labels < 1 || n_labels > SS_LABELS_MAX) return SS_EINVAL;
    return launch_minik(db, (const uint8_t *)bases_dev, n, packed, LabelSink{a, slot_label, (uint32_t)db->n_mslots, n_labels}, stream);
}

// ... and for ss_scan_reads_resampled (ss_scan_resampled.hip): a found k-mer adds its record's weights to the replicates' counters
int launch_resampled_minik(const ss_db *db, const void *bases_dev, uint64_t n, bool packed, const ResampledArgs &a, hipStream_t stream)
{
    if (!n || db->layout != 1 || (packed ? a.slot == 0 : (a.tile_base == nullptr || a.slot != 0))) return SS_EINVAL;
    if (!a.counts || !a.weights || a.stride < db->n_slots) return SS_EINVAL;
    return launch_minik(db, (const uint8_t *)bases_dev, n, packed, WeightSink{a, (uint32_t)db->n_mslots}, stream);
}

// ... and for ss_reads_classify (ss_classify.hip): a found k-mer leaves the node of its slot at its position in pos_node, which
// holds a whole number of tiles: ((n + 1023) / 1024) * 1024 fields
int launch_class_minik(const ss_db *db, const void *bases_dev, uint64_t n, bool packed, uint16_t *pos_node, const uint16_t *slot_node,
                       unsigned long long *hits0, hipStream_t stream)
{
    if (!n || db->layout != 1 || !pos_node || !slot_node || !hits0 || (((uintptr_t)pos_node) & 15)) return SS_EINVAL;
    return launch_minik(db, (const uint8_t *)bases_dev, n, packed, ClassSink{pos_node, slot_node, hits0, (uint32_t)db->n_mslots}, stream);
}

}  // namespace ss
