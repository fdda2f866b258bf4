// ss_reads_resample: a resident read set resampled with replacement, as a new resident set (`--bootstrap`).
//
// A Poisson bootstrap over reads: every record of the set is drawn w times, w ~ Poisson(1) cut at 13, and w is a pure function
// of (the record's bytes, seed, replicate).  No state, no order: the same read draws the same weight from a set in file order,
// binned or packed, on whichever rank holds it -- so ranks that each resample their shard add up to the counts of one process
// that resampled the whole sample.  Identical reads share a weight.
//
// The weight (strainscan_hip.h states it; tests/boot_model.py restates it in Python):
//   key = the second half of the record's digest, h2 of record_digest (ss_extract.hip, what ss_flat_record_keys returns in
//         keys[2i + 1]): a multiply-rotate hash over the record's flat bytes as little-endian 8-byte words, the tail
//         zero-padded, seeded with the length and closed with the splitmix64 finisher.  From a packed slab the bytes are the
//         letters of its ASCII form (what ss_reads_read_back writes).
//   x   = key + 0x9E3779B97F4A7C15 * (replicate + 1) + 0xD6E8FEB86659FD93 * seed, through the splitmix64 finisher; u = x >> 32
//   w   = the entries T_k <= u of POISSON1_CDF: T_k = floor(2^32 * e^-1 * sum_{i <= k} 1/i!), k = 0..12
//
// The passes are those of ss_reads_select with a multiplicity in the place of its 0/1 choice, and they are the same code
// (ss_support.h): record_index_of numbers the records, record_spans_of finds their spans, resample_len_kernel writes
// out_len[rec] = w * (length + 1), gather_records turns that into offsets, allocates the new slab and copies every record w times.
// resample_weights_kernel is the length pass of ss_scan_reads_resampled (ss_scan_resampled.hip), which adds w per hit and copies
// nothing: the same digest and the same table, taken here so that neither is stated twice (resample_weights_of, ss_support.h).
//
// resample_len_kernel takes a record per lane: the digest is a chain of one multiply-rotate-multiply step per 8 bytes, 19 steps
// for a 150-base read, each depending on the one before, so a record cannot be spread over lanes; the lanes of a wave walk
// neighbouring records and meet in the same cache lines step after step.
#include "ss_scan_dev.h"
#include "ss_support.h"

using namespace ss::dev;

namespace {

// floor(2^32 * e^-1 * sum_{i <= k} 1/i!), k = 0..12 (from 80-digit decimals; tests/test_bootstrap_host.py recomputes them)
__device__ const uint32_t POISSON1_CDF[13] = {1580030168u, 3160060337u, 3950075421u, 4213413783u, 4279248373u, 4292415291u, 4294609777u,
                                              4294923276u, 4294962463u, 4294966817u, 4294967252u, 4294967292u, 4294967295u};

__device__ __forceinline__ uint64_t rotl64(uint64_t x, int r) { return (x << r) | (x >> (64 - r)); }
__device__ __forceinline__ uint64_t digest_step(uint64_t h, uint64_t w)
{
    return rotl64(h ^ (w * 0xFF51AFD7ED558CCDull), 27) * 0xC4CEB9FE1A85EC53ull + 0x52DCE729ull;
}
__device__ __forceinline__ uint64_t splitmix_finish(uint64_t x)
{
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}
__device__ __forceinline__ uint64_t low_bytes(uint64_t w, uint64_t cnt) { return cnt >= 8u ? w : w & ((1ull << (8u * cnt)) - 1ull); }

// h2 of record_digest over bytes [s, s + len) of a slab of n >= 16 positions that holds them
template <bool PACKED>
__device__ __forceinline__ uint64_t record_key(const uint8_t *__restrict__ src, uint64_t n, uint64_t s, uint64_t len)
{
    uint64_t h = 0x9E3779B97F4A7C15ull ^ (len * 0xD6E8FEB86659FD93ull);
    if (PACKED) {
        // sixteen letters at a time, fetched from a position clamped into the slab and shifted into place (as the gather does it)
        for (uint64_t i = 0; i < len; i += 16u) {
            const uint64_t base = s + i, q = base > n - 16u ? n - 16u : base, left = len - i;
            const uint4 v = packed_letters16(src, q);
            unsigned __int128 x;
            __builtin_memcpy(&x, &v, 16);
            x >>= 8u * (uint32_t)(base - q);                            // base < n, so the shift is below 16 bytes
            h = digest_step(h, low_bytes((uint64_t)x, left));
            if (left > 8u) h = digest_step(h, low_bytes((uint64_t)(x >> 64), left - 8u));
        }
    } else {
        uint64_t i = 0;
        for (; i + 8u <= len; i += 8u) {
            uint64_t w;
            __builtin_memcpy(&w, src + s + i, 8);
            h = digest_step(h, w);
        }
        if (i < len) {                                                  // the tail: eight bytes from a position clamped into the slab
            const uint64_t base = s + i, q = base > n - 8u ? n - 8u : base;
            uint64_t w;
            __builtin_memcpy(&w, src + q, 8);
            w >>= 8u * (uint32_t)(base - q);
            h = digest_step(h, low_bytes(w, len - i));
        }
    }
    h ^= len;
    return splitmix_finish(h);
}

// records [rec0, rec0 + n_rec) of one slab, one per lane: out_len = w * (length + 1), the bytes the record's w copies take in the
// new slab; tot[0] += w, tot[1] += those bytes.  mix = 0x9E3779B97F4A7C15 * (replicate + 1) + 0xD6E8FEB86659FD93 * seed.
// PACKED: record r - rec0 at position (r - rec0) * slot, fixed_len letters; else start[] / end[] say where.  A span that does not
// lie inside the slab (record_span) draws nothing.
template <bool PACKED>
__global__ __launch_bounds__(256) void resample_len_kernel(const uint8_t *__restrict__ src, uint64_t n, const unsigned long long *__restrict__ start,
                                                           const unsigned long long *__restrict__ end, uint64_t rec0, uint64_t n_rec, uint32_t slot,
                                                           uint32_t fixed_len, uint64_t mix, unsigned long long *__restrict__ out_len,
                                                           unsigned long long *__restrict__ tot)
{
    unsigned long long cnt = 0, bytes = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x; i < n_rec; i += (uint64_t)gridDim.x * 256u) {
        const RecordSpan sp = record_span(PACKED, i, rec0, start, end, slot, fixed_len, n);
        unsigned long long ol = 0;
        if (sp.ok) {
            const uint32_t u = (uint32_t)(splitmix_finish(record_key<PACKED>(src, n, sp.s, sp.len) + mix) >> 32);
            uint32_t w = 0;
#pragma unroll
            for (int k = 0; k < 13; k++) w += POISSON1_CDF[k] <= u ? 1u : 0u;
            ol = (unsigned long long)w * (sp.len + 1ull);
            cnt += w;
            bytes += ol;
        }
        out_len[rec0 + i] = ol;
    }
    add_selected(cnt, bytes, tot);
}

// The same pass for ss_scan_reads_resampled (ss_scan_resampled.hip), which weighs the hits of a record instead of copying it:
// out_w[rec] = the weights of replicates first .. first + n_rep - 1 as 4-bit fields (w <= 13), replicate first + j at bits 4 j.
// mix0 = the mix of replicate `first`; a step of one replicate adds 0x9E3779B97F4A7C15.  The digest is taken once per record.
template <bool PACKED>
__global__ __launch_bounds__(256) void resample_weights_kernel(const uint8_t *__restrict__ src, uint64_t n, const unsigned long long *__restrict__ start,
                                                               const unsigned long long *__restrict__ end, uint64_t rec0, uint64_t n_rec, uint32_t slot,
                                                               uint32_t fixed_len, uint64_t mix0, uint32_t n_rep, unsigned long long *__restrict__ out_w)
{
    for (uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x; i < n_rec; i += (uint64_t)gridDim.x * 256u) {
        const RecordSpan sp = record_span(PACKED, i, rec0, start, end, slot, fixed_len, n);
        unsigned long long word = 0;
        if (sp.ok) {
            const uint64_t key = record_key<PACKED>(src, n, sp.s, sp.len);
            uint64_t mix = mix0;
            for (uint32_t j = 0; j < n_rep; j++, mix += 0x9E3779B97F4A7C15ull) {
                const uint32_t u = (uint32_t)(splitmix_finish(key + mix) >> 32);
                uint32_t w = 0;
#pragma unroll
                for (int k = 0; k < 13; k++) w += POISSON1_CDF[k] <= u ? 1u : 0u;
                word |= (unsigned long long)w << (4u * j);
            }
        }
        out_w[rec0 + i] = word;
    }
}

std::atomic<uint64_t> g_resample_calls{0};

}  // namespace

// ss_support.h: the weights of n_rep <= 16 replicates from `first` on for every record of the set, into the spans' len[]
int ss::resample_weights_of(RecHits *rh, RecSpans &sp, uint64_t seed, uint32_t first, uint32_t n_rep)
{
    const uint64_t mix0 = 0x9E3779B97F4A7C15ull * ((uint64_t)first + 1ull) + 0xD6E8FEB86659FD93ull * seed;
    for (const auto &pt : rh->parts) {
        if (!pt.n_rec) continue;
        if (pt.n < 16) return SS_EINVAL;                            // (a slab is padded to a multiple of 16)
        const unsigned blocks = (unsigned)std::min<uint64_t>((pt.n_rec + 255) / 256, 65536);
        with_bool(pt.sl->packed, [&](auto packed) {
            hipLaunchKernelGGL(resample_weights_kernel<decltype(packed)::value>, dim3(blocks), dim3(256), 0, ss::l2s::stream(),
                               (const uint8_t *)pt.sl->d, pt.n, sp.d_start, sp.d_end, pt.rec_base, pt.n_rec, pt.sl->slot,
                               pt.sl->packed ? pt.sl->L : 0u, mix0, n_rep, sp.d_len);
        });
        SS_HIP(hipGetLastError());
    }
    return SS_OK;
}

extern "C" {

int ss_reads_resample_calls(uint64_t *n)
{
    if (!n) return SS_EINVAL;
    *n = g_resample_calls.load();
    return SS_OK;
}

int ss_reads_resample(const ss_reads *R, uint64_t seed, uint32_t replicate, ss_reads **out)
{
    if (!R || !out) return SS_EINVAL;
    if (R->has_cut_record) return SS_ERANGE;                        // a cut piece is not a read
    ss::RecHits rh;
    ss::RecSpans sp;
    int rc = ss::record_index_of(R, -1, &rh, &g_resample_calls);
    if (rc) return rc;
    rc = ss::record_spans_of(&rh, &sp);
    if (rc) return rc;
    const uint64_t mix = 0x9E3779B97F4A7C15ull * ((uint64_t)replicate + 1ull) + 0xD6E8FEB86659FD93ull * seed;
    for (const auto &pt : rh.parts) {
        if (!pt.n_rec) continue;
        if (pt.n < 16) return SS_EINVAL;                            // (a slab is padded to a multiple of 16)
        const unsigned blocks = (unsigned)std::min<uint64_t>((pt.n_rec + 255) / 256, 65536);
        with_bool(pt.sl->packed, [&](auto packed) {
            hipLaunchKernelGGL(resample_len_kernel<decltype(packed)::value>, dim3(blocks), dim3(256), 0, ss::l2s::stream(), (const uint8_t *)pt.sl->d,
                               pt.n, sp.d_start, sp.d_end, pt.rec_base, pt.n_rec, pt.sl->slot, pt.sl->packed ? pt.sl->L : 0u, mix, sp.d_len, sp.d_tot);
        });
        SS_HIP(hipGetLastError());
    }
    return ss::gather_records(&rh, sp, "ss_reads_resample", out);
}

}  // extern "C"
