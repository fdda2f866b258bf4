// ss_mini.hip -- minimizer-paged k-mer index and its scan kernel (k = 31).
//
// Why: with the flat open-address table (ss_scan.hip) every one of the 120 k-mers of a 150-bp
// read costs a random 64-byte HBM sector although ~95 % of them are not in the database
// (profiles/r01a: 213 GB fetched per 22 GB of algorithmic bytes).  Consecutive k-mers of a read
// share their minimizer (the 15-mer with the smallest ordering key inside the k-mer) for ~9 positions
// on average, so a lane probes the index once per RUN of equal minimizers (~13 per read instead of
// 120).  Counting semantics are unchanged and exact: a k-mer is looked up under ITS OWN minimizer,
// which is a function of the k-mer alone, on the database side and on the read side.
//
// What bounds the lookups (scripts/micro/randsec.hip on MI355X): random 64-byte sectors come at
// ~55 G/s = 3.5 TB/s from anything larger than the L2 (the 256 MB Infinity Cache does not help), at
// 250 G/s out of the 4 MB L2 of an XCD, and reading all 64 bytes of a sector costs the same as
// reading 16.  So one run = ONE sector, and that sector answers as much as possible:
//
// Layout in HBM
//   d_pages[n_pages]  64 B  hash-addressed pages of eight 8-byte slots.  A minimizer (the 30-bit m-mer x)
//                         lives in page floor(h * n_pages / 2^30), h = mix30(x) a BIJECTION of the 30 bits, or,
//                         when that page was full at build time, in the next one(s): a lookup goes on to
//                         the next page only if the page it read is full (slot 7 occupied), which at the
//                         build's load (two items per page on average) is one lookup in a thousand.  No
//                         wrap-around (spare pages follow the last home page), and the build grows the table
//                         until every run of full pages is shorter than n_pages / 1024 -- the distance between
//                         the home pages of two minimizers that share their tag bits -- so a lookup can never
//                         reach another minimizer's slots with the same tag.
//                         A slot is 8 bytes spread over four arrays of the page (byte layout: PG_SLOTS below).
//                         inline k-mer:  tag20 | e5 | flank32
//                              the database k-mer itself: tag20 = low 20 bits of h (with the page number they
//                              determine h, hence x, exactly: two minimizers that agree in the low 20 bits of h
//                              lie >= 2^20 apart, i.e. >= n_pages / 1024 pages apart); e = 16 - o, o =
//                              offset of the minimizer inside the k-mer; flank32 = the other 16 bases (those
//                              behind the minimizer in the low bits, then those in front of it).  A read k-mer
//                              equals it iff tag, offset and flank agree: no second load, no key array.  Its
//                              counter is d_counts[n_mslots + 8 * page + slot].
//                         bucket reference:  tag14 | mask17 | multi | start30
//                              minimizers with more than SS_INLINE_MAX database k-mers keep them in a bucket of
//                              d_mkeys (below); the bucket's header travels in the slot.  tag14 is only a
//                              filter: candidates are compared in full.
//   d_mkeys[n_mslots] u64 buckets back to back.  A bucket = 1 header word + its k-mers sorted by
//                         (offset of the minimizer inside the k-mer, rest):
//                           header: bits 0..16 = which offsets occur, bit 17 = some offset occurs more
//                                   than once ("multi"), bits 32..63 = number of k-mers
//                           k-mer : the 62-bit key
//                         With one k-mer per offset (the normal case: a bucket is one super-k-mer)
//                         the k-mer with offset o sits at header + 1 + popcount(mask & ((1 << o) - 1)).
//   d_counts[n_slots] u32 occurrences: [0, n_mslots) parallel to d_mkeys, [n_mslots, n_mslots + 8 n_pages)
//                         parallel to the page slots
//   d_bloom[2^b/32]   u32 bit h >> (30 - b) set for every minimizer -- only built when it is worth its L2
//                         round trip: >= 4 bits per minimizer within 2^25 bits (the 4 MB L2 of an XCD).  A database
//                         of dense node sets (few minimizers, ~9 k-mers each) gets one; a database of sampled
//                         node sets (Build_tree.py:590-591: nearly one minimizer per k-mer) does not -- there
//                         half of a sample's runs find their minimizer anyway.
#include "ss_common.h"
#include "ss_scan_dev.h"

#include <algorithm>
#include <atomic>
#include <mutex>
#include <type_traits>

// HDR_MULTI, page_of, the page layout constants, flank_of_key, mini_of_key: ss_scan_dev.h (shared with ss_mini_build.hip, ss_build_dev.hip
// and ss_minik.hip).  The host build of the index is ss_mini_build.hip, its image on disk ss_mini_image.hip, the one-lane-per-position
// kernel for any k ss_minik.hip.

namespace {

using namespace ss::dev;

// ---------------------------------------------------------------------------------------------
// scan kernel, minimizer layout: dense SIMD for the arithmetic, compacted LDS work queues for
// the memory probes.
//
// Measured on MI355X (profiles/): what bounds this kernel is not HBM bytes but, depending on the
// database, the instructions a wave issues per tile (dense node sets: VALU 100 % busy at 8 waves/SIMD) or the
// number of random 64-byte sectors it asks of the memory system (sampled node sets: 54 G/s, all there is).
// So per tile of 62 x 16 = 992 start positions, ONE wave, no barriers that wait for another wave:
//   phase 0  coalesced 16-byte loads of the bases, 2-bit encode, codes + invalid flags -> LDS
//   phase 1a every lane keys the 16 m-mers that start in its bases (one multiply-add each) and tags
//            them with their index: packed = (key & ~31) | index, kept in registers
//   phase 1b minimizer of the lane's 16 k-mers = suffix minima over the own packed words, prefix
//            minima over the next lane's (read through a DPP wave shift; one v_min_u32 per step
//            decides key AND leftmost position); runs of equal minimizers, merged across lane
//            boundaries, are pushed to LDS queue q1 through a DPP wave prefix sum
//            (one 32-bit entry per run: ~94 per tile instead of 992 positions)
//   phase 2a (databases with a Bloom filter) lanes pull runs from q1: the minimizer m-mer is re-read from the
//            codes, one mix, one probe of the Bloom filter (L2).  The ~10 % that pass are compacted into q1b
//   phase 2b ONE 16-byte load per run (all runs, or the Bloom survivors): the head of the minimizer's page.
//            Inline k-mers are settled here (tag + offset + flank = the whole k-mer -> atomicAdd); bucket
//            references go to q2
//   phase 3  16 lanes per found bucket, one per position: candidate slot from the run's offset mask
//            -> 64-bit compare -> atomicAdd
// Round 4, template switches of the same kernel:
//   COMB     tables that expect hits (ss_db_expect_hits: a layer-2 cluster table) scanned by a BINNED read set: a workgroup
//            takes four consecutive tiles, hits are added up in an LDS table keyed by the bucket (QComb) and flushed with one
//            atomic per non-zero counter; found runs of SOLID buckets (PG_SOLID) are verified by one lane each (phase 3a),
//            the others by 16 lanes (3b)
//   MULTI    up to four tables in one pass (ss_scan_reads_multi): phases 0-1b once per tile, phases 2-3 per table
// ---------------------------------------------------------------------------------------------
// threads per workgroup of this kernel = one wave
constexpr int MT = 64;
static_assert(MT == 64, "one wave per workgroup: phase 2 compacts with ballots and keeps its counters in scalar registers");
#ifndef SS_Q1CAP
#define SS_Q1CAP 160
#endif
constexpr int Q1CAP = SS_Q1CAP;    // runs (q1), Bloom survivors (q1b) and found runs (q2) per tile held in LDS (random
                                   // reads: mean 94 runs, max ~110); overflow is handled inline.  With 160 the
                                   // workgroup needs 4.9 KB: 32 one-wave workgroups per CU.  Test builds shrink it.
static_assert(Q1CAP <= 4096, "q2 keeps a q1b index in 12 bits");
// ... and with k at run time (KK = 0, 17 <= k <= 30): a k-mer of k - 14 m-mers changes its minimizer every (k - 13) / 2 positions, so a
// tile has ~2 x 992 / (k - 13) runs -- 165 at k = 25, 198 at k = 23, 248 at k = 21.  256: the most the combining table's byte-sized run
// indices (QComb::ent / rest) can name; 7.2 KB per workgroup with it (22 one-wave workgroups per CU).
constexpr int Q1CAP_RT = 256;
// SGPRs decide the residency of this kernel: a SIMD admits floor(800 / (ceil(sgprs / 16) * 16 + 16)) waves
// (MI355X_MICROARCH.md, residency), i.e. 8 waves at <= 80, 7 at <= 96, 6 beyond; VGPRs (58) and LDS (4.9 KB per
// one-wave workgroup = 32 per CU) allow 8.
// (the several-tables instantiation behind per-table Bloom filters, <IN, BLOOM, !COMB, 8, MULTI, 31>: 78 SGPRs, 63-64 VGPRs, no
//  scratch, 528 bytes of kernarg -- the same as its filterless twin; the filter pointers and shifts are read from ScanTabs per table)
constexpr int NUM_SGPR = 80;       // amdgpu_num_sgpr of every instantiation
constexpr int RPL = 2;             // phase 2a: runs per lane and round (their Bloom words in flight together)
constexpr int RPL2 = 1;            // phase 2b: page heads in flight per lane
constexpr int U3 = 4;              // phase 3: found runs' worth of positions per lane and round (all candidate loads in flight before any compare)
// A tile is (MT - 2) x 16 start positions: all MT lanes load 16 bases and key the 16 m-mers that
// START in them; lanes 0..MT-3 own 16 k-mers each, whose 17-m-mer windows end in the NEXT lane's
// m-mers, whose last bases lie in the lane after that.  The last two lanes only feed their
// neighbours: 3 % of the lanes idle is cheaper than a separate halo load + encode, which costs a
// full wave instruction stream for one lane.
constexpr int MLANES = MT - 2;
constexpr int MTILE = MLANES * PPT;

template <int CAP>
struct QSharedT {
    uint32_t code_[MT + 3];            // code_[1 + i] = bases 16 i .. 16 i + 15 of the tile; one word of slack in front (the
                                       // window of 16 bases BEFORE a minimizer near the tile start) and two behind
    uint16_t inv[MT + 2];
    uint32_t q1[CAP + 64];             // run:   len << 12 | tile position of its first k-mer (+64 dump slots)
    alignas(16) uint8_t ib[MT * PPT];  // per tile position: index (0..31, counted from the lane's first m-mer) of the minimizer
    uint64_t q2[CAP];                  // found bucket: bucket start << 32 | multi << 31 | aligned offset mask << 12 | run index (q1b with a
                                       // Bloom filter, q1 without)
    uint32_t cnt[4];                   // [1] = found runs
};
// (a __shared__ variable of its own: instantiations without a Bloom filter do not pay its 1.25 KB)
template <int CAP>
struct QBloomT {
    uint64_t q1b[CAP];                 // run that passed the Bloom filter: h << 32 | minimizer offset in the first k-mer << 17 | q1 entry
};

// ---------------------------------------------------------------------------------------------
// Counting where most read k-mers HIT (layer-2 cluster tables hold every k-mer of their strains; Vote_Strain_L2_Lasso_new_sp.py
// :354-372 scans all reads against one per identified cluster).  What a global atomicAdd costs on this chip
// (scripts/micro/atomics.hip, profiles/r04_atomics_micro_*.txt): 27 G (wave instruction, 64-byte line) pairs per second,
// whatever the footprint (2 MB or 40 MB), the scope, the number of lanes on the line (1..16) -- and the kernel's other work does
// not overlap it.  A read's 120 hits fall into ~13 buckets = ~19 lines, a tile of 6.5 reads pays ~100 line requests: 11 of the
// 17 ms of such a scan.  In a BINNED read set (ss_reorder.hip) the neighbours of a read come from the same locus and hit the same
// buckets, so the hits are first added up in LDS: a small open-address table keyed by the bucket, one byte per bucket slot
// (a run adds at most one to a slot, and the table is flushed before 255 runs have gone into it), flushed with one global
// atomic per non-zero counter every few tiles.  A workgroup works through CONSECUTIVE tiles for that.
// ---------------------------------------------------------------------------------------------
constexpr int COMB_NE = 64;            // entries (= lanes of the wave: the flush looks at one entry per lane)
constexpr int COMB_CH = 4;             // consecutive tiles per workgroup
constexpr uint32_t COMB_NONE = 0xFFu;
template <int CAP>
struct QCombT {
    static_assert(CAP <= 256, "run indices in bytes");
    uint32_t key[COMB_NE];             // bucket start + 1, 0 = free
    uint32_t nrun[COMB_NE];            // found runs that took this entry since the last flush (a byte counter holds 255)
    uint32_t acc[COMB_NE][5];          // byte o = occurrences of the bucket's slot o (1..19; slot 0 is the header)
    uint8_t ent[CAP];                  // per found run of the tile: its entry, COMB_NONE = count in global memory
    uint8_t list[COMB_NE];             // flush: the occupied entries
    uint8_t rest[CAP];                 // phase 3: the found runs whose bucket is not solid, from the front; solid runs whose hits
                                       // go straight to the counters, from the back (indices into q2)
};

// the 31-mer starting at tile position pos as two 32-bit halves (funnel shifts; no 64-bit shifts)
// (khi_mask: the 2 k - 32 bits of the upper half: 0x3FFFFFFF at k = 31)
template <class QS>
__device__ __forceinline__ void kmer_at(const QS &S, uint32_t pos, uint32_t &lo, uint32_t &hi, uint32_t khi_mask = 0x3FFFFFFFu)
{
    const uint32_t w = pos >> 4, sh = 2 * (pos & 15);
    const uint32_t a = S.code_[w + 1], b = S.code_[w + 2], c = S.code_[w + 3];
    lo = __builtin_amdgcn_alignbit(b, a, sh);
    hi = __builtin_amdgcn_alignbit(c, b, sh) & khi_mask;
}

// the 15-mer starting at tile position p (one funnel shift over two code words)
template <class QS>
__device__ __forceinline__ uint32_t mmer_at(const QS &S, uint32_t p)
{
    const uint32_t w = p >> 4;
    return __builtin_amdgcn_alignbit(S.code_[w + 2], S.code_[w + 1], 2 * (p & 15)) & ss::M30;
}
// the 16 bases starting at tile position p (p >= -16)
template <class QS>
__device__ __forceinline__ uint32_t win16_at(const QS &S, int32_t p)
{
    const int32_t w = (p >> 4) + 1;
    return __builtin_amdgcn_alignbit(S.code_[w + 1], S.code_[w], 2 * (p & 15));
}

// A found run carries the bucket's offset mask shifted so that the offset of the run's FIRST k-mer
// sits at bit 16: the k-mer q positions further has offset bit 16 - q (the minimizer stands still
// while the k-mer start moves right).  Slot of the database k-mer that k-mer q would be, 0 = none.
// (F = k - 15, the largest minimizer offset: 16 at k = 31, where the comments above are written)
__device__ __forceinline__ uint32_t cand_slot(uint32_t bstart, uint32_t amask, uint32_t q, uint32_t F = 16u)
{
    const uint32_t o = F - q;
    return ((amask >> o) & 1u) ? bstart + 1u + (uint32_t)__popc(amask & ((1u << o) - 1u)) : 0u;
}
__device__ __forceinline__ uint32_t aligned_mask(uint32_t hdr, uint32_t o0, uint32_t F = 16u)
{
    const uint32_t wm = (2u << F) - 1u;
    return ((hdr & wm) << (F - o0)) & wm;
}

// one occurrence of the database k-mer in slot `cpos` of the bucket at `bstart`: into the LDS entry `ent` of the bucket when it
// has one (QComb), else straight to the counter
template <bool COMB>
__device__ __forceinline__ void count_slot(uint32_t cpos, uint32_t bstart, uint32_t ent, uint32_t *__restrict__ acc5,
                                           uint32_t *__restrict__ counts)
{
    const uint32_t off = cpos - bstart;
    if (COMB && ent != COMB_NONE && off < 20u) atomicAdd(&acc5[ent * 5u + (off >> 2)], 1u << ((off & 3u) * 8u));
    else atomicAdd(&counts[cpos], 1u);
}
// compare the candidate (already loaded) with k-mer `pos`; count; fall back to a bucket scan when
// several database k-mers share a minimizer offset (repeated / colliding minimizer)
template <bool COMB, class QS>
__device__ __forceinline__ void settle_item(const QS &S, uint32_t pos, uint32_t bstart, uint32_t multi, uint32_t cpos,
                                            uint64_t cand, const uint64_t *__restrict__ mkeys,
                                            uint32_t *__restrict__ counts, uint32_t ent = COMB_NONE, uint32_t *__restrict__ acc5 = nullptr,
                                            uint32_t khi_mask = 0x3FFFFFFFu)
{
    uint32_t klo, khi;
    kmer_at(S, pos, klo, khi, khi_mask);
    if ((uint32_t)cand == klo && (uint32_t)(cand >> 32) == khi) {
        count_slot<COMB>(cpos, bstart, ent, acc5, counts);
    } else if (multi) {
        const uint64_t km = ((uint64_t)khi << 32) | klo;
        const uint32_t cnt = (uint32_t)(mkeys[bstart] >> 32);
        for (uint32_t q = 0; q < cnt; q++)
            if (mkeys[bstart + 1 + q] == km) { count_slot<COMB>(bstart + 1 + q, bstart, ent, acc5, counts); break; }
    }
}

// v_mad_u32_u24 with the addend as a scalar constant (one SGPR per VOP3 on gfx9)
__device__ __forceinline__ uint32_t mad24s(uint32_t a, uint32_t b, uint32_t c)
{
    uint32_t d;
    asm("v_mad_u32_u24 %0, %1, %2, %3" : "=v"(d) : "v"(a), "v"(b), "s"(c));
    return d;
}
// a_i = min(a_i, p_i of the NEXT lane), eight at a time: the DPP wave shift rides in the v_min itself (the
// compiler keeps a separate v_mov_dpp per word).  s_nop: a DPP read needs two wait states after the VALU
// write of its source, which the hazard recognizer cannot see inside inline assembly.  Lane 63 reads 0.
#define SS_MIN_DPP(i, j) "v_min_u32_dpp %" #i ", %" #j ", %" #i " wave_shl:1 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
__device__ __forceinline__ void min_next_lane8(uint32_t &a0, uint32_t &a1, uint32_t &a2, uint32_t &a3, uint32_t &a4, uint32_t &a5,
                                               uint32_t &a6, uint32_t &a7, uint32_t p0, uint32_t p1, uint32_t p2, uint32_t p3,
                                               uint32_t p4, uint32_t p5, uint32_t p6, uint32_t p7)
{
    asm("s_nop 1\n\t" SS_MIN_DPP(0, 8) SS_MIN_DPP(1, 9) SS_MIN_DPP(2, 10) SS_MIN_DPP(3, 11) SS_MIN_DPP(4, 12) SS_MIN_DPP(5, 13)
        SS_MIN_DPP(6, 14) SS_MIN_DPP(7, 15)
        : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3), "+v"(a4), "+v"(a5), "+v"(a6), "+v"(a7)
        : "v"(p0), "v"(p1), "v"(p2), "v"(p3), "v"(p4), "v"(p5), "v"(p6), "v"(p7));
}
// m = 2 * m + (a != b): builds a bit mask from comparisons, two instructions per bit
__device__ __forceinline__ uint32_t shift_in_ne(uint32_t m, uint32_t a, uint32_t b)
{
    asm("v_cmp_ne_u32 vcc, %1, %2\n\tv_addc_co_u32 %0, vcc, %0, %0, vcc" : "+v"(m) : "v"(a), "v"(b) : "vcc");
    return m;
}

// found runs of a probe launch (choose_comb), 64 words so that the tiles' single atomics do not queue on one address
__device__ uint32_t ss_probe_runs[64];

// the phases of a tile, labelled in the ISA only: a comment line, no instruction (scripts/archive/r4/isa_budget.py reads them)
#define SS_MARK(i) asm volatile("; SSMARK " #i)

// Several tables in ONE pass over the reads (layer 2: the reference re-reads the FASTQ once per identified cluster,
// Vote_Strain_L2_Lasso_new_sp.py:295-296,354-372): bases, codes, minimizers and runs of a tile are made once, the page lookups
// and candidate checks repeat per table.  Up to four tables per launch (the LDS counters keep the table in the two bits above
// a bucket start's thirty).  Tree tables of several databases (strainscan_amd/multi_db.py) go through the BLOOM instantiation:
// phase 2a probes table tb's own filter and compacts that table's survivors into q1b, phases 2b-3 run on them as for one table.
constexpr int MULTI_MAX = 4;
struct ScanTabs {
    const uint64_t *mkeys[MULTI_MAX];
    const uint4 *pages[MULTI_MAX];
    uint32_t *counts[MULTI_MAX];
    const uint32_t *bloom[MULTI_MAX];               // (BLOOM only) table tb's minimizer filter and its 30 - log2(bits)
    uint32_t n_pages[MULTI_MAX], cbase[MULTI_MAX], bloom_shift[MULTI_MAX];
    int n;
};

// Minimizers of a lane's 16 k-mers when a k-mer has W < 17 m-mers (k < 31; the run-time-k instantiations, KK = 0): the window of
// k-mer j = packed keys x[j .. j + W - 1] of the 32 the lane sees (its own 16, the next lane's 16).  A window of 17 is "own suffix +
// neighbour's prefix" (the k = 31 network below); a shorter one may lie inside the lane's own 16, so: minima over 2, 4, 8(, 16)
// consecutive keys by doubling, and every window = two overlapping power-of-two stretches.  W is a template argument here (the indices
// must be constants: the keys live in registers), the kernel switches on it once per tile.
template <int W>
__device__ __forceinline__ void sliding_min(const uint32_t (&x)[32], uint32_t (&out)[PPT])
{
    constexpr int P = W >= 16 ? 16 : W >= 8 ? 8 : W >= 4 ? 4 : 2;
    uint32_t m[32];
#pragma unroll
    for (int i = 0; i < 32; i++) m[i] = x[i];
#pragma unroll
    for (int s2 = 1; s2 < P; s2 <<= 1) {
#pragma unroll
        for (int i = 0; i + s2 < 32; i++) m[i] = min(m[i], m[i + s2]);      // (ascending i: m[i + s2] is still the narrower minimum)
    }
#pragma unroll
    for (int j = 0; j < PPT; j++) out[j] = min(m[j], m[j + W - P]);
}

// KK: 31 = the k this kernel was tuned for, everything about k a constant; 0 = k is the kernel argument k_rt (17 <= k <= 30, round 6)
template <int IN, bool BLOOM, bool COMB, int WAVES_PER_SIMD, bool MULTI = false, int KK = 31>
__global__ __launch_bounds__(MT, WAVES_PER_SIMD) __attribute__((amdgpu_num_sgpr(NUM_SGPR))) void scan_mini_kernel(
    const uint8_t *__restrict__ bases, uint64_t n, uint64_t n_tiles, const uint64_t *__restrict__ mkeys0,
    const uint4 *__restrict__ pages0, uint32_t n_pages0, uint32_t *__restrict__ counts0, uint32_t cbase0,
    const uint32_t *__restrict__ bloom, uint32_t bloom_shift, uint32_t xcd_swizzle, const ScanTabs tabs, int k_rt)
{
    static_assert(!(COMB && BLOOM), "a combining scan is for tables that expect hits: they have no use for the minimizer filter");
    static_assert(KK == 31 || KK == 0, "k = 31, or k at run time");
    // the table of this pass over the tile's runs (MULTI: tabs.* in turn)
    const uint64_t *__restrict__ mkeys = mkeys0;
    const uint4 *__restrict__ pages = pages0;
    uint32_t *__restrict__ counts = counts0;
    uint32_t n_pages = n_pages0, cbase = cbase0, tab_key = 0u;
    const int K = KK ? KK : k_rt;                    // k = 31: 17 m-mers of length 15 per k-mer
    const uint32_t W = (uint32_t)(K - ss::MINI_M + 1), F = W - 1u;      // m-mers per k-mer, largest minimizer offset (= flank bases)
    const uint32_t khi_mask = (1u << (2 * K - 32)) - 1u;                // upper half of a 2 k-bit key
    const uint32_t fmask = F >= 16u ? 0xFFFFFFFFu : (1u << (2u * F)) - 1u;      // a flank's 2 F bits
    static_assert(31 - ss::MINI_M + 1 == PPT + 1, "k = 31: a k-mer window = own m-mers j..15 + neighbour m-mers 0..j");
    constexpr int QC = KK == 31 ? Q1CAP : Q1CAP_RT;  // runs a tile's queues hold
    __shared__ QSharedT<QC> S;
    __shared__ QBloomT<QC> SB;                       // (dropped from the instantiations that never touch it)
    __shared__ QCombT<QC> C;
    const int t = threadIdx.x;
    const uint32_t vc1 = ss::MMK_C1;
    constexpr uint64_t CH = COMB ? COMB_CH : 1;      // consecutive tiles per workgroup

    // the 16 bases of this lane are fetched one tile AHEAD: the HBM
    // round trip of the stream overlaps the previous tile's phases
    // Workgroup b runs on XCD b % 8 (observed; a speed matter only): with the swizzle, XCD x works through the x-th
    // eighth of the TILES in order (its workgroups stride through that eighth), so neighbouring tiles -- reads that a
    // resident set keeps binned by their first minimizer (ss_reorder.hip) and that share their page sectors -- meet in
    // ONE 4 MB L2 instead of eight.  (The grid is a multiple of 8 then; every XCD gets the same number of tiles.)
    // A workgroup takes CH consecutive tiles, then the next CH `stride` chunks further on (CH = 1: a plain grid stride)
    uint64_t tile = (uint64_t)blockIdx.x * CH, tile_end = n_tiles, stride = gridDim.x, tile0 = 0;
    if (xcd_swizzle & 1u) {
        const uint64_t per = (((n_tiles + 7) >> 3) + CH - 1) / CH * CH, x = blockIdx.x & 7u;
        stride = gridDim.x >> 3;
        tile0 = x * per;
        tile = tile0 + (uint64_t)(blockIdx.x >> 3) * CH;
        tile_end = min(n_tiles, (x + 1) * per);
    }
    auto next_tile = [&](uint64_t tl) -> uint64_t {
        if (CH == 1) return tl + stride;
        return ((tl + 1 - tile0) % CH) ? tl + 1 : tl + 1 + (stride - 1) * CH;
    };
    uint32_t comb_runs = 0;                          // found runs added to the LDS counters since their last flush
    if (COMB) {
        C.key[t] = 0u;
        C.nrun[t] = 0u;
#pragma unroll
        for (int w = 0; w < 5; w++) C.acc[t][w] = 0u;
    }
    // the non-zero LDS counters go to global memory (16 lanes per occupied entry: slots 1..16, then a lane per entry for the
    // slots 17..19), the table is emptied
    auto comb_flush = [&]() {
        const uint32_t key = C.key[t];
        const uint64_t occ = __ballot(key != 0u);
        const uint32_t nocc = (uint32_t)__popcll(occ);
        if (key) C.list[__builtin_amdgcn_mbcnt_hi((uint32_t)(occ >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)occ, 0u))] = (uint8_t)t;
        __syncthreads();
        for (uint32_t g0 = 0; g0 < nocc * 16u; g0 += MT) {
            const uint32_t g = g0 + (uint32_t)t;
            if ((g >> 4) < nocc) {
                const uint32_t e = C.list[g >> 4], off = 1u + (g & 15u);
                const uint32_t c = (C.acc[e][off >> 2] >> ((off & 3u) * 8u)) & 0xFFu;
                if (c) {
                    const uint32_t k1 = C.key[e] - 1u;
                    uint32_t *cb = MULTI ? tabs.counts[k1 >> 30] : counts;
                    atomicAdd(&cb[(k1 & ss::START_MASK) + off], c);
                }
            }
        }
        if (key) {
            const uint32_t w = C.acc[t][4] >> 8;
            if (w) {
                uint32_t *cb = MULTI ? tabs.counts[(key - 1u) >> 30] : counts;
#pragma unroll
                for (uint32_t o = 0; o < 3; o++)
                    if ((w >> (8u * o)) & 0xFFu) atomicAdd(&cb[((key - 1u) & ss::START_MASK) + 17u + o], (w >> (8u * o)) & 0xFFu);
            }
        }
        __syncthreads();
        if (key) {
            C.key[t] = 0u;
            C.nrun[t] = 0u;
#pragma unroll
            for (int w = 0; w < 5; w++) C.acc[t][w] = 0u;
        }
        __syncthreads();
        comb_runs = 0;
    };
    uint32_t wn[4];
    if (tile < tile_end) {
        const uint64_t b0 = tile * MTILE;
        load_in<IN>(bases, b0 + (uint64_t)t * 16, n, wn);
    }
    for (; tile < tile_end; tile = next_tile(tile)) {
        SS_MARK(20);
        // ---- phase 0: bases -> 2-bit codes in LDS ------------------------------------------------
        {
            uint32_t code, inv;
            decode_in<IN>(wn, code, inv);
            S.code_[t + 1] = code;
            S.inv[t] = (uint16_t)inv;
            if (t == 1) S.cnt[1] = 0;
            const uint64_t nt = next_tile(tile);
            if (nt < tile_end) {
                const uint64_t nb = nt * (uint64_t)MTILE;
                load_in<IN>(bases, nb + (uint64_t)t * 16, n, wn);
            }
        }
        __syncthreads();
        SS_MARK(0);

        // ---- phase 1a: key the 16 m-mers that start in this lane's 16 bases -----------------------
        uint32_t hm[PPT];
        {
            const uint32_t c0 = S.code_[t + 1], c1 = S.code_[t + 2];
            // low 24 bits of the m-mers 0..15 (bits 2i.. of c1:c0): 15 funnel shifts, then one multiply-add
            // per m-mer; the "+ i" of the packed word rides in the additive constant
            hm[0] = mad24s(c0, vc1, ss::MMK_C0);
#pragma unroll
            for (int i = 1; i < PPT; i++) hm[i] = mad24s(__builtin_amdgcn_alignbit(c1, c0, 2 * i), vc1, ss::MMK_C0 + (uint32_t)i);
        }
        SS_MARK(1);

        // ---- phase 1b: minimizer of the lane's 16 k-mers, runs ------------------------------------
        // k-mer j is live iff none of the bases j..j+30 is invalid: flags of the positions 0..30 in lo
        // (smeared downwards through a bit reversal: shift-left-or is one instruction), 31..46 in hi
        // (smeared upwards; k-mer j sees hi bits 0..j-1)
        uint32_t live = 0;
        if (KK == 31 && t < MLANES) {
            uint32_t lo;
            __builtin_memcpy(&lo, &S.inv[t], 4);
            uint32_t hi = __builtin_amdgcn_alignbit(S.inv[t + 2], lo, 31);
            lo = __builtin_bitreverse32(lo & 0x7FFFFFFFu);
            lo |= lo << 1; lo |= lo << 2; lo |= lo << 4; lo |= lo << 8; lo |= lo << 16;
            hi |= hi << 1; hi |= hi << 2; hi |= hi << 4; hi |= hi << 8;
            live = ~(__builtin_bitreverse32(lo) | (hi << 1)) & 0xFFFFu;
        } else if (KK != 31 && t < MLANES) {
            // any k: a sliding OR of width k over the 48 flags from the lane's first base on = width 16 by doubling, then two
            // stretches of 16 that overlap (17 <= k <= 31)
            uint64_t y = (uint64_t)S.inv[t] | ((uint64_t)S.inv[t + 1] << 16) | ((uint64_t)S.inv[t + 2] << 32);
            y |= y >> 1; y |= y >> 2; y |= y >> 4; y |= y >> 8;
            y |= y >> (K - 16);
            live = ~(uint32_t)y & 0xFFFFu;
        }
        // k-mer j covers m-mers j..j+16 = own m-mers j..15 (index j..15) and the next lane's m-mers 0..j
        // (index 16..16+j): suffix minima over the own packed words, prefix minima over the neighbour's;
        // equal keys resolve to the smaller index = the leftmost m-mer (the database side uses the same
        // rule).  Every lane computes the prefix minima of ITS keys as its left neighbour counts them
        // (index + 16); the neighbour reads them with a DPP wave shift inside the v_min: the keys never
        // go through LDS.  All lanes execute this (a DPP source lane must be enabled).
        uint32_t need = 0;
        uint32_t mh[PPT];
        if (KK == 31) {
            uint32_t pf[PPT];
            pf[0] = hm[0] + 16u;
#pragma unroll
            for (int j = 1; j < PPT; j++) pf[j] = min(pf[j - 1], hm[j] + 16u);
#pragma unroll
            for (int i = PPT - 2; i >= 0; i--) hm[i] = min(hm[i], hm[i + 1]);         // suffix minima, in place
            min_next_lane8(hm[0], hm[1], hm[2], hm[3], hm[4], hm[5], hm[6], hm[7], pf[0], pf[1], pf[2], pf[3], pf[4], pf[5], pf[6], pf[7]);
            min_next_lane8(hm[8], hm[9], hm[10], hm[11], hm[12], hm[13], hm[14], hm[15], pf[8], pf[9], pf[10], pf[11], pf[12], pf[13], pf[14], pf[15]);
#pragma unroll
            for (int j = 0; j < PPT; j++) mh[j] = hm[j];
        } else {
            // any k: the next lane's 16 keys through DPP wave shifts (index + 16, as the left lane counts them), then the window minima
            uint32_t x[32];
#pragma unroll
            for (int i = 0; i < PPT; i++) {
                x[i] = hm[i];
                x[PPT + i] = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)hm[i], 0x130, 0xf, 0xf, false) + 16u;      // wave_shl:1 (lane 63 reads 0: unused)
            }
            switch (W) {
            case 3: sliding_min<3>(x, mh); break;   case 4: sliding_min<4>(x, mh); break;   case 5: sliding_min<5>(x, mh); break;
            case 6: sliding_min<6>(x, mh); break;   case 7: sliding_min<7>(x, mh); break;   case 8: sliding_min<8>(x, mh); break;
            case 9: sliding_min<9>(x, mh); break;   case 10: sliding_min<10>(x, mh); break; case 11: sliding_min<11>(x, mh); break;
            case 12: sliding_min<12>(x, mh); break; case 13: sliding_min<13>(x, mh); break; case 14: sliding_min<14>(x, mh); break;
            case 15: sliding_min<15>(x, mh); break; default: sliding_min<16>(x, mh); break;
            }
        }
        if (live) {
            // run starts as a bit mask: position j starts a run if it is live and (j == 0, or j-1 is
            // not live, or the minimizer changed)
            uint32_t chg = 0u;
#pragma unroll
            for (int j = PPT - 1; j >= 1; j--) chg = shift_in_ne(chg, mh[j], mh[j - 1]);   // bit j-1 <- (mh[j] != mh[j-1])
            chg = (chg << 1) | 1u;
            need = live & (chg | (~live << 1));
            // the minimizer's index (low byte of the packed word) of all 16 positions: one 16-byte store;
            // phase 2 reads the byte of a run's first position (the walk below no longer gathers it)
            uint32_t pk[4];
#pragma unroll
            for (int w = 0; w < 4; w++) {
                const uint32_t lo = __builtin_amdgcn_perm(mh[4 * w + 1], mh[4 * w], 0x0c0c0400u);
                const uint32_t hi = __builtin_amdgcn_perm(mh[4 * w + 3], mh[4 * w + 2], 0x0c0c0400u);
                pk[w] = __builtin_amdgcn_perm(hi, lo, 0x05040100u);
            }
            reinterpret_cast<uint4 *>(S.ib)[t] = make_uint4(pk[0], pk[1], pk[2], pk[3]);
        }
        SS_MARK(6);
        // A run that reaches the end of a lane goes on in the next lane when that lane's first k-mer has
        // the same minimizer (same packed word: the left lane counts the right lane's m-mer i as 16 + i).
        // The left lane then owns the whole run (at most 16 k-mers: phase 3 gives a run 16 lanes; a longer
        // one stays cut) and the right lane drops its first run: a third fewer runs per tile.
        const uint32_t stop = need | (~live & 0xFFFFu) | 0x10000u;
        uint32_t ext12 = 0;                          // k-mers my last run takes over from the next lane, << 12
        {
            const uint32_t first = (uint32_t)__ffs(stop >> 1);                                   // length of the run starting at 0
            const uint32_t ownlast = (live >> 15) ? (uint32_t)__clz(need) - 15u : 0u;            // 16 - start of my last run
            const uint32_t l_mh = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)mh[PPT - 1], 0x138, 0xf, 0xf, false);   // wave_shr:1
            const uint32_t l_own = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)ownlast, 0x138, 0xf, 0xf, false);
            const bool cont = (live & 1u) && l_own && l_mh == mh[0] + 16u && l_own + first <= 16u;
            const uint32_t give = cont ? first << 12 : 0u;
            ext12 = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)give, 0x130, 0xf, 0xf, false);                         // wave_shl:1
            if (cont) need &= ~1u;
        }
        // wave prefix sum of the run counts; then every lane walks ITS runs (about two, at most a handful:
        // the loop is as long as the busiest lane of the wave) instead of testing all 16 positions
        uint32_t ovf = 0;   // runs that did not fit q1 (processed inline below)
        uint32_t n1;
        {
            const uint32_t mine = (uint32_t)__popc(need);
            const uint32_t incl = wave_inclusive_sum(mine);
            n1 = min((uint32_t)__builtin_amdgcn_readlane((int)incl, 63), (uint32_t)QC);
            const uint32_t mybase = incl - mine;
            if (need) {
                const uint32_t dummy = (uint32_t)QC + (uint32_t)t;   // where entries beyond the capacity go
                const uint32_t stop1 = stop >> 1, tbase = (uint32_t)(t * PPT);
                uint32_t idx = mybase;
                for (uint32_t nd = need; nd; idx++) {
                    const uint32_t j = (uint32_t)__ffs(nd) - 1u;
                    nd &= nd - 1u;
                    const uint32_t len = (uint32_t)__ffs(stop1 >> j);                       // until the next run / gap
                    S.q1[min(idx, dummy)] = (len << 12) + (tbase + j + (nd ? 0u : ext12));
                }
                if (mybase + mine > (uint32_t)QC) {                          // rare: which of my runs did not fit
                    uint32_t r = mybase;
                    for (uint32_t nd = need; nd; nd &= nd - 1u, r++)
                        if (r >= (uint32_t)QC) ovf |= nd & (0u - nd);
                }
            }
        }
        __syncthreads();
        SS_MARK(2);

        // minimizer offset (in the run's first k-mer) from the index byte of the run's first position:
        // meta = offset << 17 | len << 12 | position
        auto run_meta = [&](uint32_t e) {
            const uint32_t rpos = e & 0xFFFu;
            return e | ((((uint32_t)S.ib[rpos] & 31u) - (rpos & 15u)) << 17);
        };
        // a bucket reference whose tag bits match becomes a found run in q2 (phase 3 gives it 16 lanes, one per position)
        auto push_found = [&](uint32_t lo, uint32_t mask17, uint32_t meta, uint32_t ridx, bool queued) {
            const uint32_t bstart = lo & ss::START_MASK, multi = lo >> 31;
            const uint32_t amask = aligned_mask(mask17, (meta >> 17) & 31u, F);
            uint32_t i2 = QC;
            if (queued) i2 = atomicAdd(&S.cnt[1], 1u);
            if (i2 < QC) {
                S.q2[i2] = ((uint64_t)(lo & (ss::START_MASK | ss::PG_SOLID)) << 32) | (multi << 31) | (amask << 12) | ridx;      // (bit 62: solid)
            } else {
                // the queue is full (only with floods of tag collisions), or phase 3 is already
                // over (runs that overflowed q1): settle this run here, so that no k-mer is ever dropped
                const uint32_t rpos = meta & 0xFFFu, len = (meta >> 12) & 31u;
                for (uint32_t q = 0; q < len; q++) {
                    const uint32_t cpos = cand_slot(bstart, amask, q, F);
                    if (cpos) settle_item<false>(S, rpos + q, bstart, multi, cpos, mkeys[cpos], mkeys, counts, COMB_NONE, nullptr, khi_mask);
                }
            }
        };
        // One page against one run; tg = the page's first 16 bytes (tag8[8], hi8[8]).  Inline slots are whole database
        // k-mers: the k-mer of the run with minimizer offset o = 16 - e (if the run has one) equals the slot iff the
        // remaining tag bits and the flank agree -- the flank of EVERY k-mer of the run is a bit-select between the 16
        // bases behind the minimizer (fa) and the 16 in front of it (fb).  Returns true when the page is full (the
        // minimizer's slots may go on in the next page).
        auto scan_page = [&](const uint4 tg, uint32_t page, uint32_t meta, uint32_t h, uint32_t ridx, bool queued) -> bool {
            const uint32_t tt = (h & 0xFFu) * 0x01010101u;
            const uint32_t x0 = tg.x ^ tt, x1 = tg.y ^ tt;                      // zero byte = tag8 matches
            const uint32_t z0 = ~(((x0 & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | x0) & 0x80808080u;
            const uint32_t z1 = ~(((x1 & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | x1) & 0x80808080u;
            uint32_t hit = (z0 >> 7) | (z1 >> 3);                               // slot s at bit 8 (s & 3) + 4 (s >> 2)
            if (hit) {
                const uint32_t o0 = (meta >> 17) & 31u, len = (meta >> 12) & 31u;
                const char *pb = reinterpret_cast<const char *>(pages) + (uint64_t)page * 64u;
                do {
                    const uint32_t b = (uint32_t)__ffs(hit) - 1u, sl = (b >> 3) + (b & 4u);
                    hit &= hit - 1u;
                    const uint32_t hi8 = (((b & 4u) ? tg.w : tg.z) >> (b & 24u)) & 0xFFu;
                    const bool ref = hi8 & 0x80u;
                    const uint32_t e = hi8 & 31u, j = o0 + e - F;               // inline: k-mer j of the run has offset o0 - j (e = F - offset)
                    if (ref ? ((hi8 ^ (h >> 8)) & 0x3Fu) == 0u : j < len) {
                        const uint32_t lo = reinterpret_cast<const uint32_t *>(pb + 16)[sl];
                        const uint32_t mid = reinterpret_cast<const uint16_t *>(pb + 48)[sl];
                        if (ref) {
                            push_found(lo, mid | ((hi8 & 0x40u) << 10), meta, ridx, queued);
                        } else if ((mid >> 4) == ((h >> 8) & 0xFFFu)) {
                            const int32_t q = (int32_t)((meta & 0xFFFu) + o0);  // tile position of the minimizer
                            const uint32_t fa = win16_at(S, q + ss::MINI_M), fb = win16_at(S, q - (int32_t)F);      // the bases behind / the F bases in front
                            const uint32_t m = ((1u << e) << e) - 1u;           // low 2 e bits (e = 16: all)
                            if ((((fa & m) | (fb & ~m)) & fmask) == lo) atomicAdd(&counts[cbase + page * 8u + sl], 1u);
                        }
                    }
                } while (hit);
            }
            return (tg.w >> 24) != (uint32_t)ss::PG_EMPTY_HI;
        };
        // the rare continuation: the page was full, the minimizer's slots may go on in the next one(s)
        auto scan_more = [&](uint32_t page, uint32_t meta, uint32_t h, uint32_t ridx, bool queued) {
            uint4 tg;
            do {
                page++;                                   // the build guarantees a non-full page before the array ends
                tg = pages[(uint64_t)page * 4u];
            } while (scan_page(tg, page, meta, h, ridx, queued));
        };

        SS_MARK(7);
        for (int tb = 0; tb < (MULTI ? tabs.n : 1); tb++) {
        if (MULTI) {
            mkeys = tabs.mkeys[tb]; pages = tabs.pages[tb]; counts = tabs.counts[tb];
            n_pages = tabs.n_pages[tb]; cbase = tabs.cbase[tb]; tab_key = (uint32_t)tb << 30;
            if (BLOOM) { bloom = tabs.bloom[tb]; bloom_shift = tabs.bloom_shift[tb]; }
            if (tb) {                                   // the found-run queue of the table before has been worked off
                if (t == 1) S.cnt[1] = 0;
                __syncthreads();
            }
        }
        // ---- phase 2a (databases with a Bloom filter): one probe of an L2-resident bit array kills most of
        // the ~90 % of the runs whose minimizer is not in the database before they cost a random HBM
        // sector each.  Survivors are compacted into q1b (ballot + lane count: one wave per workgroup)
        uint32_t ns = n1;
        if (BLOOM) {
            ns = 0;
            for (uint32_t r0 = 0; r0 < n1; r0 += RPL * MT) {
                SS_MARK(11);
                uint32_t meta[RPL], hs[RPL], bw[RPL];
                bool ok[RPL];
#pragma unroll
                for (int u = 0; u < RPL; u++) {
                    const uint32_t r = r0 + u * MT + t;
                    ok[u] = r < n1;
                    meta[u] = run_meta(S.q1[ok[u] ? r : 0u]);
                    hs[u] = ss::mix30(mmer_at(S, (meta[u] & 0xFFFu) + (meta[u] >> 17)));   // one mix per run: Bloom bit, page, tags
                }
#pragma unroll
                for (int u = 0; u < RPL; u++) bw[u] = bloom[hs[u] >> (bloom_shift + 5)];
#pragma unroll
                for (int u = 0; u < RPL; u++) ok[u] = ok[u] && ((bw[u] >> ((hs[u] >> bloom_shift) & 31u)) & 1u);
#pragma unroll
                for (int u = 0; u < RPL; u++) {
                    const uint64_t pass = __ballot(ok[u]);
                    if (ok[u]) SB.q1b[ns + __builtin_amdgcn_mbcnt_hi((uint32_t)(pass >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)pass, 0u))] =
                        ((uint64_t)hs[u] << 32) | meta[u];
                    ns += (uint32_t)__popcll(pass);
                }
            }
            __syncthreads();
        }
        // ---- phase 2b: ONE sector per run (all runs, or the Bloom survivors), RPL2 page heads in flight per lane ----
        for (uint32_t i0 = 0; i0 < ns; i0 += RPL2 * MT) {
            SS_MARK(12);
            uint32_t meta[RPL2], hs[RPL2], pgi[RPL2];
            uint4 tg[RPL2];
            bool ok[RPL2];
#pragma unroll
            for (int u = 0; u < RPL2; u++) {
                const uint32_t i = i0 + u * MT + t;
                ok[u] = i < ns;
                if (BLOOM) {
                    const uint64_t sv = SB.q1b[ok[u] ? i : 0u];
                    meta[u] = (uint32_t)sv;
                    hs[u] = (uint32_t)(sv >> 32);
                } else {
                    meta[u] = run_meta(S.q1[ok[u] ? i : 0u]);
                    hs[u] = ss::mix30(mmer_at(S, (meta[u] & 0xFFFu) + (meta[u] >> 17)));
                }
                pgi[u] = ss::page_of(hs[u], n_pages);
                if (ok[u]) tg[u] = pages[(uint64_t)pgi[u] * 4u];
            }
            SS_MARK(13);
#pragma unroll
            for (int u = 0; u < RPL2; u++)
                if (ok[u] && scan_page(tg[u], pgi[u], meta[u], hs[u], i0 + u * MT + t, true)) scan_more(pgi[u], meta[u], hs[u], i0 + u * MT + t, true);
            SS_MARK(14);
        }
        __syncthreads();
        SS_MARK(3);

        // ---- phase 3: the k-mers whose minimizer exists in the database -------------------------
        // 16 lanes per found run (one per position of the run), four runs per lane per round: all
        // candidate loads in flight before any compare
        {
            const uint32_t n2 = min(S.cnt[1], (uint32_t)QC);
            // a probe launch (choose_comb: the first tiles of a binned set against a table nobody has flagged) reports its found runs
            if (!COMB && (xcd_swizzle & 2u) && t == 0) atomicAdd(&ss_probe_runs[blockIdx.x & 63u], n2);
            bool comb_full = false;
            if (COMB) {
                // every found run claims the LDS entry of its bucket (the runs of a locus' reads share theirs); a byte
                // counter takes at most one from a run and an ENTRY takes 255 runs between two flushes (round 5: counted per
                // entry -- a bucket sees the ~7 reads of its locus per tile; the bound used to be 255 runs for the whole table,
                // a flush every 2.4 tiles), the run that finds its entry full counts in global memory like one without an entry.
                // The table is flushed when the workgroup leaves its CH consecutive tiles (the next ones are other loci).
                SS_MARK(10);
                comb_runs += n2;
                for (uint32_t r = (uint32_t)t; r < n2; r += MT) {
                    const uint32_t key = (((uint32_t)(S.q2[r] >> 32) & ss::START_MASK) | tab_key) + 1u;
                    uint32_t i = (key * 0x9E3779B1u) >> 26, e = COMB_NONE;
                    static_assert(COMB_NE == 64, "hash: top six bits");
                    for (int pr = 0; pr < 8; pr++) {
                        const uint32_t old = atomicCAS(&C.key[i], 0u, key);
                        if (old == 0u || old == key) { e = atomicAdd(&C.nrun[i], 1u) < 255u ? i : COMB_NONE; break; }
                        i = (i + 1u) & (COMB_NE - 1u);
                    }
                    C.ent[r] = (uint8_t)e;
                    comb_full = comb_full || e == COMB_NONE;
                }
                comb_full = __ballot(comb_full) != 0ull;      // runs without an entry count in global memory; the table is emptied after the tile
                __syncthreads();
                SS_MARK(9);
            }
            uint32_t n_rest = 0, n_hit = 0;                // found runs whose bucket is not solid (S.rest from the front); solid runs with
                                                           // hits for the counters (S.rest from the back: together at most n2 entries)
            // U runs' worth of positions per lane and round: all their candidate loads in flight before any compare
            auto cand_round = [&](auto UC, uint32_t g0) {
                constexpr int U = decltype(UC)::value;
                SS_MARK(15);
                uint32_t pos[U], bst[U], mul[U], cps[U], ent[U];
                uint64_t cnd[U];
#pragma unroll
                for (int u = 0; u < U; u++) {
                    const uint32_t g = g0 + u * MT + t, q = g & 15u;
                    const bool v = (g >> 4) < n_rest;
                    const uint32_t fi = v ? (COMB ? (uint32_t)C.rest[g >> 4] : (g >> 4)) : 0u;      // the found run (index into q2)
                    const uint64_t r = S.q2[fi];
                    const uint32_t run = BLOOM ? (uint32_t)SB.q1b[(uint32_t)r & 0xFFFu] : S.q1[(uint32_t)r & 0xFFFu];
                    pos[u] = (run & 0xFFFu) + q;
                    bst[u] = (uint32_t)(r >> 32) & ss::START_MASK;
                    mul[u] = (uint32_t)r >> 31;
                    cps[u] = (v && q < ((run >> 12) & 31u)) ? cand_slot(bst[u], ((uint32_t)r >> 12) & 0x1FFFFu, q, F) : 0u;
                    cnd[u] = mkeys[cps[u]];
                    ent[u] = COMB ? (uint32_t)C.ent[fi] : COMB_NONE;
                }
#pragma unroll
                for (int u = 0; u < U; u++)
                    if (cps[u]) settle_item<COMB>(S, pos[u], bst[u], mul[u], cps[u], cnd[u], mkeys, counts, ent[u], &C.acc[0][0], khi_mask);
                SS_MARK(16);
            };
            // (only in the combining scans: a tree scan finds ~6 runs per tile, and six lanes walking through this path cost more
            //  than the 16-lanes-per-run check of 96: contiguous node sets 3.37 -> 3.70 ms with it)
            // ---- 3a: runs whose bucket is SOLID (PG_SOLID: its k-mers are one stretch of bases), ONE LANE per run: the
            // stretch is rebuilt from the bucket's first and last candidate key (they overlap), compared with the read's bases
            // in three words, and a mismatching base strikes the k-mers that cover it.  The other runs are compacted into
            // S.rest for the 16-lanes-per-run check below.
            if (!COMB) n_rest = n2;                        // (S.rest is not used: run i is found run i)
            for (uint32_t r0 = 0; COMB && r0 < n2; r0 += MT) {
                const uint32_t r = r0 + (uint32_t)t;
                const bool v = r < n2;
                const uint64_t q = S.q2[v ? r : 0u];
                const bool solid = v && ((q >> 62) & 1ull);
                uint32_t hitmask = 0;                      // this lane's run: its matching k-mers, when they go straight to the counters
                const uint64_t om = __ballot(v && !solid);
                if (v && !solid) C.rest[n_rest + __builtin_amdgcn_mbcnt_hi((uint32_t)(om >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)om, 0u))] = (uint8_t)r;
                n_rest += (uint32_t)__popcll(om);
                if (solid) {
                    const uint32_t bstart = (uint32_t)(q >> 32) & ss::START_MASK, amask = ((uint32_t)q >> 12) & 0x1FFFFu;
                    const uint32_t run = BLOOM ? (uint32_t)SB.q1b[(uint32_t)q & 0xFFFu] : S.q1[(uint32_t)q & 0xFFFu];
                    const uint32_t rpos = run & 0xFFFu, len = (run >> 12) & 31u;
                    // position p of the run has offset F - p (16 - p at k = 31): the candidates are the offsets of amask at or above W - len
                    const uint32_t am = amask & ~((1u << (W - len)) - 1u);
                    if (am) {
                        const uint32_t o_hi = 31u - (uint32_t)__clz(am), o_lo = (uint32_t)__ffs(am) - 1u, d = o_hi - o_lo;
                        const uint32_t slot_a = bstart + 1u + (uint32_t)__popc(amask & ((1u << o_hi) - 1u));      // the first position's k-mer
                        const uint64_t k1 = mkeys[slot_a], k2 = mkeys[slot_a - d];                                // ... and the last one's
                        const int32_t P = (int32_t)(rpos + F - o_hi);
                        const uint64_t lo64 = k1 | (k2 << (2u * d));
                        const uint32_t hi32 = d ? (uint32_t)(k2 >> (64u - 2u * d)) : 0u;
                        uint32_t x0 = win16_at(S, P) ^ (uint32_t)lo64;
                        // the stretch is d + k bases: 16 in x0, the next min(16, d + k - 16) in x1, the d + k - 32 beyond (if any) in x2
                        const uint32_t nb1 = d + (uint32_t)K - 16u, nb2 = d + (uint32_t)K > 32u ? d + (uint32_t)K - 32u : 0u;
                        uint32_t x1 = (win16_at(S, P + 16) ^ (uint32_t)(lo64 >> 32)) & (nb1 >= 16u ? 0xFFFFFFFFu : (1u << (2u * nb1)) - 1u);
                        uint32_t x2 = nb2 ? (win16_at(S, P + 32) ^ hi32) & ((1u << (2u * nb2)) - 1u) : 0u;
                        uint32_t match = (2u << d) - 1u;                                                           // k-mers 0 .. d of the stretch
                        // a base that differs strikes the k-mers covering it: j in [m - 30, m]
                        x0 = (x0 | (x0 >> 1)) & 0x55555555u; x1 = (x1 | (x1 >> 1)) & 0x55555555u; x2 = (x2 | (x2 >> 1)) & 0x55555555u;
                        auto strike = [&](uint32_t xb, uint32_t base0) {
                            while (xb) {
                                const uint32_t m = base0 + (((uint32_t)__ffs(xb) - 1u) >> 1);
                                xb &= xb - 1u;
                                const uint32_t hi = min(m, d), lw = m > (uint32_t)K - 1u ? m - ((uint32_t)K - 1u) : 0u;
                                if (lw <= hi) match &= ~(((2u << hi) - 1u) & ~((1u << lw) - 1u));
                            }
                        };
                        strike(x0, 0u); strike(x1, 16u); strike(x2, 32u);
                        if (match) {
                            const uint32_t w_ = 1u;
                            const uint32_t off_a = slot_a - bstart;                                                // k-mer j sits at slot offset off_a - j
                            const uint32_t e_ = COMB ? (uint32_t)C.ent[r] : COMB_NONE;
                            if (COMB && e_ != COMB_NONE && off_a < 20u) {
                                const uint32_t bits = __brev(match) >> (31u - off_a);                              // bit o = the k-mer at slot offset o
#pragma unroll
                                for (uint32_t wd = 0; wd < 5; wd++) {
                                    const uint32_t nib = (bits >> (4u * wd)) & 15u;
                                    if (nib) atomicAdd(&C.acc[e_][wd], ((nib * 0x00204081u) & 0x01010101u) * w_);
                                }
                            } else {
                                // straight to the counters, but NOT one k-mer after the other from this lane: an atomic costs
                                // per (instruction, line), and a lane's hits share a line -- the run's result goes back into
                                // its q2 entry and 16 lanes count it below (3c)
                                hitmask = match;
                                S.q2[r] = ((uint64_t)slot_a << 32) | match;
                            }
                        }
                    }
                }
                const uint64_t hm = __ballot(hitmask != 0u);
                if (hitmask) C.rest[QC - 1u - (n_hit + __builtin_amdgcn_mbcnt_hi((uint32_t)(hm >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)hm, 0u)))] = (uint8_t)r;
                n_hit += (uint32_t)__popcll(hm);
            }
            if (COMB) __syncthreads();
            // ---- 3c: the solid runs' hits that go straight to the counters, 16 lanes per run (k-mer 16 of a full stretch: lane 0 again)
            for (uint32_t g0 = 0; g0 < n_hit * 16u; g0 += MT) {
                const uint32_t g = g0 + (uint32_t)t;
                if ((g >> 4) < n_hit) {
                    const uint64_t e = S.q2[C.rest[QC - 1u - (g >> 4)]];
                    const uint32_t j = g & 15u, slot_a = (uint32_t)(e >> 32), mt = (uint32_t)e;
                    if ((mt >> j) & 1u) atomicAdd(&counts[slot_a - j], 1u);
                    if (j == 0u && (mt >> 16)) atomicAdd(&counts[slot_a - 16u], 1u);
                }
            }
            // ---- 3b: the other found runs, 16 lanes each
            // (a tree scan finds ~5 runs per tile = 80 of a round's 256 positions; rounds of 64 for the rest were tried in
            //  round 4 and change nothing: the empty quarters of a round are branched over)
            const uint32_t total = n_rest * 16u;
            uint32_t g0 = 0;
            for (; g0 < total; g0 += U3 * MT) cand_round(std::integral_constant<int, U3>(), g0);
            if (COMB && comb_full) { __syncthreads(); SS_MARK(4); comb_flush(); SS_MARK(8); }
        }
        // ---- overflow: runs that did not fit q1 (pathological inputs only) are done in place ------
        if (ovf) {
            for (int j = 0; j < PPT; j++) {
                if (!((ovf >> j) & 1u)) continue;
                const uint32_t len12 = ((uint32_t)__ffs(stop >> (j + 1)) << 12) + ((need >> (j + 1)) ? 0u : ext12);
                const uint32_t meta = run_meta(len12 + (uint32_t)(t * PPT + j));
                const uint32_t h = ss::mix30(mmer_at(S, (meta & 0xFFFu) + (meta >> 17)));
                const uint32_t page = ss::page_of(h, n_pages);
                if (scan_page(pages[(uint64_t)page * 4u], page, meta, h, 0u, false)) scan_more(page, meta, h, 0u, false);
            }
        }
        if (MULTI && tb + 1 < tabs.n) __syncthreads();
        }   // tables
        SS_MARK(4);
        __syncthreads();   // queues and codes are rewritten by the next tile
        SS_MARK(5);
        if (COMB && CH > 1 && comb_runs && ((tile + 1 - tile0) % CH) == 0) { comb_flush(); SS_MARK(8); }      // the chunk ends: other loci next
    }
    if (COMB && comb_runs) comb_flush();
}

}  // namespace

namespace ss {

std::atomic<long long> g_hook_generic_k{0};      // ss_test_hook(4, ...)

// Which kernel scans a BINNED block (ss_reorder.hip: the reads of a locus lie together) against this table: the plain one,
// whose every hit is a global atomic, or the combining one (COMB: the hits of four consecutive tiles are added up in LDS
// first).  With few hits the plain kernel is the faster (tree tables at their usual 5 % of the read k-mers: 3.8 vs 4.5 ms
// per 20 M reads on sampled node sets, 2.7 vs 3.2 on contiguous ones); with many, the same-address atomics of a locus'
// reads queue up and the combining one wins by up to 3x (half of the read k-mers in the table: 17.1 -> 10.6 ms sampled,
// 14.8 -> 4.9 contiguous; file order 14.1 / 10.2; profiles/r05_ab_log.md 1).  The caller's flag (ss_db_expect_hits: the table of
// an identified cluster) is a hint that saves the probe; every other table is asked: its first PROBE_TILES tiles run
// through the plain kernel with the probe bit set -- they count for real, the main launch starts behind them -- and
// report their found runs (minimizers of the reads that have a bucket in the table); at PROBE_RUNS_PER_TILE and above
// the rest of the block, and every later block of the same read set, goes through the combining kernel.  One probe per
// (read set, table): ~40 us and one stream synchronisation on the first scan of a sample against a table.
constexpr uint64_t PROBE_TILES = 8192;          // one wave per tile: one round of the chip's 8192 wave slots
constexpr double PROBE_RUNS_PER_TILE = 8.0;     // measured crossover: 4 (plain wins by 15 %) ... 8-10 (even) ... 16 (COMB by 30 %)
static std::mutex probe_mu;                     // the probe's device words are one set per process

// (the probe's verdict is read and written under probe_mu: two threads may scan the same table)
static bool probe_known(ss_db *db, uint64_t set_id, bool *comb)
{
    std::lock_guard<std::mutex> g(probe_mu);
    if (db->probe_set != set_id) return false;
    *comb = db->probe_comb != 0;
    return true;
}

// The combining kernel or not, for a pass over a block that is `binned` or not, against a table that is flagged (ss_db_expect_hits)
// or not.  SS_COMBINE (A/B runs and tests) is read here and nowhere else; each kind of pass keeps the meaning it has given it:
//   one table, k = 31        unset: binned blocks only -- flagged tables always, the others as the probe says (`verdict`);
//                            0: never; 1: every scan of a flagged table, binned or not; 2: every binned scan, flagged or not
//   several tables, any k    flagged tables only -- unset: binned blocks; 0: never; 1 and above: every pass, binned or not
//   one table, 17 <= k <= 30 flagged tables under binned blocks, whatever the variable says (no probe either)
static bool choose_comb(bool flagged, bool binned, bool several, int k, bool verdict)
{
    static const int env = [] { const char *e = getenv("SS_COMBINE"); return e ? atoi(e) : -1; }();
    if (several) return flagged && (env < 0 ? binned : env != 0);
    if (k != 31 || env < 0) return binned && (flagged || (k == 31 && verdict));
    return env == 2 ? binned : (flagged && env != 0);
}

// The waves-per-SIMD bound of an instantiation.  k at run time: five (its queues of 256 runs); the combining variant six (it needs
// 71-79 VGPRs: at eight it carried scratch); everything else eight.
constexpr int scan_mini_waves(bool comb, int kk) { return kk == 0 ? 5 : (comb ? 6 : 8); }

// ONE launch of scan_mini_kernel: a pass of the block over one table (several = false: the single-table instantiations) or over up
// to MULTI_MAX tables of one k and one filter kind (several = true).  bloom: behind the tables' minimizer filters; comb: the
// combining variant; probe: the first PROBE_TILES tiles only, which report their found runs (launch_scan_mini).  Exactly the
// instantiations a caller can reach exist: no filter in front of a combining scan, none in a several-tables pass with k at run time.
static int launch_scan_mini_pass(ss_db *const *dbs, int n_dbs, bool several, bool bloom, bool comb, bool probe, const uint8_t *b,
                                 uint64_t n, bool packed, hipStream_t stream)
{
    const int k = dbs[0]->k;
    if ((bloom && comb) || (bloom && several && k != 31)) return SS_EINVAL;
    ScanTabs tabs = {};
    for (int i = 0; i < n_dbs; i++) {
        const ss_db *db = dbs[i];
        tabs.mkeys[i] = db->d_mkeys;
        tabs.pages[i] = reinterpret_cast<const uint4 *>(db->d_dir);
        tabs.counts[i] = db->d_counts;
        tabs.n_pages[i] = db->n_dir;
        tabs.cbase[i] = (uint32_t)db->n_mslots;
        tabs.bloom[i] = db->d_bloom;
        tabs.bloom_shift[i] = 30u - db->bloom_bits;
    }
    tabs.n = n_dbs;
    const uint64_t n_tiles = probe ? PROBE_TILES : (n + MTILE - 1) / MTILE;      // (this kernel's tile is 62 x 16 positions)
    // grid-stride over tiles with MANY more blocks than fit the chip: short blocks start at scattered times, so
    // the waves sharing a SIMD stop marching through their ALU and memory phases in step.  Measured with 8 waves
    // per SIMD resident (20 M reads = 3.04 M tiles; blocks = x * 1024): x = 8 (one round of resident blocks)
    // 4.03 ms, 32: 3.76, 128: 3.59, 512: 3.55, 2048 (1.5 tiles per block): 3.50, 4096 (one tile each): 3.51
    const uint64_t units = comb ? (n_tiles + COMB_CH - 1) / COMB_CH : n_tiles;
    unsigned blocks = (unsigned)std::min<uint64_t>(units, (uint64_t)2048 * 256 * (256 / MT));
    blocks = (blocks + 7u) & ~7u;                           // a multiple of 8: the same number of workgroups on every XCD
    const uint32_t swz = 1u | (probe ? 2u : 0u);            // the XCD swizzle, always; bit 1: a probe launch
    with_input_layout(b, packed, [&](auto in) { with_bool(several, [&](auto multi) { with_bool(k == 31, [&](auto k31) {
        with_bool(bloom, [&](auto bl) { with_bool(comb, [&](auto cb) {
            // k = 31: the instantiation with k a constant; any other k (17..30): k at run time
            constexpr int IN = decltype(in)::value, KK = decltype(k31)::value ? 31 : 0;
            constexpr bool MULTI = decltype(multi)::value, BLOOM = decltype(bl)::value, COMB = decltype(cb)::value;
            if constexpr (!(BLOOM && COMB) && !(BLOOM && MULTI && KK == 0))
                hipLaunchKernelGGL((scan_mini_kernel<IN, BLOOM, COMB, scan_mini_waves(COMB, KK), MULTI, KK>), dim3(blocks), dim3(MT), 0,
                                   stream, b, n, n_tiles, tabs.mkeys[0], tabs.pages[0], tabs.n_pages[0], tabs.counts[0], tabs.cbase[0],
                                   tabs.bloom[0], tabs.bloom_shift[0], swz, tabs, k);
        }); });
    }); }); });
    SS_HIP(hipGetLastError());
    return SS_OK;
}

// launches of the several-tables kernel per filter kind (MULTI_BLOOM / MULTI_EXPECT / MULTI_PLAIN), ss_scan_multi_launches
static std::atomic<uint64_t> g_multi_launches[3];

// a table that expects hits (ss_db_expect_hits) skips its Bloom filter: nearly every minimizer of the reads is in it
int multi_kind(const ss_db *db)
{
    return db->expect_hits ? MULTI_EXPECT : db->d_bloom ? MULTI_BLOOM : MULTI_PLAIN;
}

// May this table share a several-tables pass?  Tables of the page index at k = 31, and at k >= SHARE_K_MIN where scan_mini_kernel
// with k at run time serves every table (below it launch_scan_mini sends the flagged ones to the per-position kernel); the Bloom
// kind has a several-tables instantiation at k = 31 only.  ss_scan_reads_multi scans the others table by table.
constexpr int SHARE_K_MIN = 20;
bool may_share_pass(const ss_db *db)
{
    return db->layout == 1 && db->k >= SHARE_K_MIN && (db->k == 31 || multi_kind(db) != MULTI_BLOOM);
}

// one pass of a flat block against up to MULTI_MAX tables that may share it, all of one k and one filter kind (multi_kind)
int launch_scan_mini_multi(ss_db *const *dbs, int n_dbs, const void *bases_dev, uint64_t n, hipStream_t stream, bool binned, bool packed)
{
    if (n_dbs < 1 || n_dbs > MULTI_MAX || !dbs[0]) return SS_EINVAL;
    const int kind = multi_kind(dbs[0]);      // (one k for the tables of a pass: the tile's minimizers are made once)
    for (int i = 0; i < n_dbs; i++)
        if (!dbs[i] || !may_share_pass(dbs[i]) || dbs[i]->k != dbs[0]->k || multi_kind(dbs[i]) != kind) return SS_EINVAL;
    const bool comb = choose_comb(kind == MULTI_EXPECT, binned, true, dbs[0]->k, false);
    int rc = launch_scan_mini_pass(dbs, n_dbs, true, kind == MULTI_BLOOM, comb, false, (const uint8_t *)bases_dev, n, packed, stream);
    if (rc) return rc;
    g_multi_launches[kind]++;
    for (int i = 0; i < n_dbs; i++) dbs[i]->launches++;
    return SS_OK;
}

extern "C" int ss_scan_multi_launches(uint64_t out[3])
{
    if (!out) return SS_EINVAL;
    for (int i = 0; i < 3; i++) out[i] = g_multi_launches[i].load();
    return SS_OK;
}

int launch_scan_mini(ss_db *db, const void *bases_dev, uint64_t n, hipStream_t stream, bool binned, uint64_t set_id, bool packed)
{
    // Which kernel.  k = 31: scan_mini_kernel with k a constant.  17 <= k <= 30: scan_mini_kernel with k at run time
    // (KK = 0, queues of 256 runs) -- measured against the one-lane-per-position kernel scan_minik_kernel (profiles/r06_k_index.json):
    // a table with few hits, 4 M reads, k = 29 / 25 / 21 / 20 / 19 / 17: 1.38 / 1.51 / 1.73 / 1.82 / 2.63 / 3.46 ms against 2.24 / 2.31 /
    // 2.75 / 2.95 / 3.18 / 3.64 (k = 31: 1.34); a cluster table under binned reads (the combining variant), 8 M reads, k = 29 / 25 / 21 /
    // 20: 3.3 / 4.1 / 7.3 / 9.1 against 8.9 / 9.9 / 15.3 / 16.6.  The exception: tables that expect hits below SHARE_K_MIN (k <= 19),
    // where a tile's ~330+ runs overflow the queues and the per-position kernel is as fast or faster (k = 19: 18.5 binned / 18.9 in
    // file order against 17.5 / 22.2) -- which is why may_share_pass stops there: a several-tables pass is always scan_mini_kernel.
    // ss_test_hook 4 (tests: the kernels held to each other on one index): 1 = tables of k = 31 through the per-position kernel,
    // 2 = tables of every k through it, 3 = tables of every k through scan_mini_kernel.
    const uint8_t *b = (const uint8_t *)bases_dev;
    const long long hk = g_hook_generic_k.load();
    if (db->k == 31 ? (hk == 1 || hk == 2) : (hk != 3 && (hk == 2 || (db->k < SHARE_K_MIN && db->expect_hits))))
        return launch_scan_minik(db, b, n, stream, packed);
    auto comb_if = [&](bool verdict) { return choose_comb(db->expect_hits != 0, binned, false, db->k, verdict); };
    auto pass = [&](bool comb, bool probe) {
        return launch_scan_mini_pass(&db, 1, false, !comb && multi_kind(db) == MULTI_BLOOM, comb, probe, b, n, packed, stream);
    };
    bool verdict = false;
    if (comb_if(false) == comb_if(true)) {}                 // the probe has no say
    else if (set_id && probe_known(db, set_id, &verdict)) {}
    else if ((n + MTILE - 1) / MTILE >= 4 * PROBE_TILES) {
        // The first scan of a (read set, table) pair makes ONE stream synchronisation here (~40 us of probe tiles, a memset and a
        // 256-byte copy back): ss_scan_reads is asynchronous from the second scan of the pair on, and this first launch cannot
        // be captured into a hipGraph (include/strainscan_hip.h says so at ss_scan_reads).
        std::lock_guard<std::mutex> g(probe_mu);
        uint32_t runs[64];
        void *sym = nullptr;
        SS_HIP(hipGetSymbolAddress(&sym, HIP_SYMBOL(ss_probe_runs)));
        SS_HIP(hipMemsetAsync(sym, 0, sizeof(runs), stream));
        int rc = pass(false, true);                         // (the whole n: the last probe tile's k-mers reach beyond it)
        if (rc) return rc;
        SS_HIP(hipMemcpyAsync(runs, sym, sizeof(runs), hipMemcpyDeviceToHost, stream));
        SS_HIP(hipStreamSynchronize(stream));
        uint64_t total = 0;
        for (uint32_t r : runs) total += r;
        db->probe_runs_per_tile = (double)total / (double)PROBE_TILES;
        verdict = db->probe_runs_per_tile >= PROBE_RUNS_PER_TILE;
        db->probe_comb = verdict;
        db->probe_set = set_id;
        b += in_bytes(packed, PROBE_TILES * (uint64_t)MTILE);      // (a multiple of 16 bytes / of 8 packed: the alignment of the block is kept)
        n -= PROBE_TILES * (uint64_t)MTILE;
    }
    return pass(comb_if(verdict), false);
}

}  // namespace ss
