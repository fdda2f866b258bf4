// ss_bam_pairs.hip -- `--pairs` on a BAM sample: the mates of a BAM linked on the device, and its fragments as a resident set.
//
// A paired BAM holds both mates in ONE stream, anywhere in it (a coordinate-sorted file keeps them far apart).  ss_bam_dev.hip
// leaves the start, kept flag and kept ordinal of every record and a flat block whose non-empty record i is kept record i; with
// BamRecords::want_off also where each kept record's letters begin in that block.  What this file adds (the rule is stated in
// strainscan_hip.h, "Read pairs from a BAM"):
//   1  the stream on the device (BamDeviceStream: gpu_gunzip where the loader would use it, else host inflate and upload), the
//      records and the flat block (bam_records_flat_dev: the host walk where the device walk declines)
//   2  key_kernel: one lane per record -> mate[r] = "no mate" / "not kept", and for a kept record with 0x1 set the digest of its
//      name (bam_name_digest, ss_bam.h: the hash of ss_bam_extract.hip), its role and paired[r] = 1
//   3  ExclusiveSum + compact_kernel: (h2, r) of the paired records, in record order.  Two stable hipcub radix sorts, least
//      significant key first: by h2, then -- h1 gathered into that order -- by h1.  The records of one name (both hashes equal) now
//      stand side by side, in record order
//   4  link_kernel: one lane per sorted position looks two neighbours each way, which tells a group of one (an orphan), of two (a
//      pair when the roles are {1, 2}) and of three or more apart without walking the group: O(1) per lane whatever the names.
//      It writes mate[] and counts pairs, orphans and the records of violating groups
//   5  length_kernel: a fragment's LEADER is its earlier record; lead[r] and the fragment's bytes -> two ExclusiveSums (the
//      lengths in 64 bits): each fragment's index and byte offset; leader_list_kernel: fragment -> its leader
//   6  join_kernel: sixteen lanes per fragment write it in 16-byte aligned pieces of the destination (the piece copy,
//      ss_piece_copy.h): per piece a masked fetch for either mate, both from the one flat block, and the 'N' and the '\n' put in.
// Every per-read kernel decides per record from the record's bytes, so all of them run unchanged on the set this makes.
// ss_bam_select_pairs / ss_bam_extract_pairs (ss_bam_extract.hip) take steps 2 to 4 and fragment_len_kernel from here;
// ss_bam_tag.hip takes steps 2 to 4 (bam_mates_dev) and 5 to 6 (bam_join_dev), with the fragment index of every leader.
// Scratch: the stream-ordered pool (PoolScratch) and ss::big_malloc.  Plain launches, no device-wide barrier inside a kernel.  All
// byte offsets are 64-bit; record counts are below 0x7FFFFFF0 (bam_to_flat_dev).
#include "ss_bam.h"
#include "ss_piece_copy.h"

#include <hipcub/hipcub.hpp>

using namespace ss::dev;
using ss::Clock;
using ss::grid_for;
using ss::ms_since;
using ss::NO_MATE;
using ss::NOT_KEPT;

namespace {

__device__ __forceinline__ uint32_t flag_of(const uint8_t *s, uint64_t p) { return (uint32_t)s[p + 18] | (uint32_t)s[p + 19] << 8; }

// One lane per record r <= n_rec (paired[n_rec] = 0 closes the sum)
__global__ __launch_bounds__(256) void key_kernel(const uint8_t *__restrict__ s, const uint64_t *__restrict__ rec, const uint32_t *__restrict__ keep,
                                                  uint64_t n_rec, unsigned long long *__restrict__ h1, unsigned long long *__restrict__ h2,
                                                  uint8_t *__restrict__ role, uint32_t *__restrict__ paired, uint32_t *__restrict__ mate)
{
    const uint64_t r = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (r > n_rec) return;
    if (r == n_rec) { paired[r] = 0u; return; }
    uint32_t pr = 0u, ro = 0u;
    if (keep[r]) {
        const uint64_t p = rec[r];
        const uint32_t f = flag_of(s, p);
        if (f & 0x1u) {
            pr = 1u;
            ro = (f & 0xC0u) == 0x40u ? 1u : (f & 0xC0u) == 0x80u ? 2u : 0u;
            ss::bam_name_digest(s, p, &h1[r], &h2[r]);
        }
    }
    paired[r] = pr;
    role[r] = (uint8_t)ro;
    mate[r] = keep[r] ? NO_MATE : NOT_KEPT;
}

// (h2, r) of the paired records, in record order
__global__ __launch_bounds__(256) void compact_kernel(const uint32_t *__restrict__ paired, const uint32_t *__restrict__ pidx,
                                                      const unsigned long long *__restrict__ h2, uint64_t n_rec,
                                                      unsigned long long *__restrict__ key, uint32_t *__restrict__ idx)
{
    const uint64_t r = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (r >= n_rec || !paired[r]) return;
    key[pidx[r]] = h2[r];
    idx[pidx[r]] = (uint32_t)r;
}

__global__ __launch_bounds__(256) void gather_h1_kernel(const uint32_t *__restrict__ idx, const unsigned long long *__restrict__ h1, uint32_t n_p,
                                                        unsigned long long *__restrict__ key)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i < n_p) key[i] = h1[idx[i]];
}

// One lane per sorted position.  cnt[0] += pairs, cnt[1] += orphans, cnt[2] += records in violating groups
__global__ __launch_bounds__(256) void link_kernel(const uint32_t *__restrict__ idx, const unsigned long long *__restrict__ h1,
                                                   const unsigned long long *__restrict__ h2, const uint8_t *__restrict__ role, uint32_t n_p,
                                                   uint32_t *__restrict__ mate, unsigned long long *__restrict__ cnt)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    unsigned long long pairs = 0, orphans = 0, bad = 0;
    if (i < n_p) {
        const uint32_t r = idx[i];
        const unsigned long long a = h1[r], b = h2[r];
        auto same = [&](uint32_t j) { const uint32_t q = idx[j]; return h1[q] == a && h2[q] == b; };
        const bool p1 = i >= 1u && same(i - 1u), n1 = i + 1u < n_p && same(i + 1u);
        const bool p2 = p1 && i >= 2u && same(i - 2u), n2 = n1 && i + 2u < n_p && same(i + 2u);
        if (!p1 && !n1) orphans = 1;
        else if ((p1 && n1) || p2 || n2) bad = 1;                       // three records and more
        else {
            const uint32_t q = idx[p1 ? i - 1u : i + 1u];
            const uint32_t mine = role[r], other = role[q];
            if (mine && other && mine + other == 3u) {
                mate[r] = q;
                pairs = mine == 1u ? 1 : 0;                             // (a pair is counted by its first mate)
            } else bad = 1;
        }
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        pairs += __shfl_xor(pairs, d, 64);
        orphans += __shfl_xor(orphans, d, 64);
        bad += __shfl_xor(bad, d, 64);
    }
    if ((threadIdx.x & 63u) == 0) {
        if (pairs) atomicAdd(&cnt[0], pairs);
        if (orphans) atomicAdd(&cnt[1], orphans);
        if (bad) atomicAdd(&cnt[2], bad);
    }
}

// the letters of kept record r in the flat block (off: BamRecords::d_off)
__device__ __forceinline__ uint64_t bases_of(const uint64_t *__restrict__ off, uint64_t r) { return off[r + 1] - off[r] - 1u; }

// One lane per record r <= n_rec: lead[r] = 1 and flen[r] = the fragment's bytes when r is the earlier record of its fragment
__global__ __launch_bounds__(256) void length_kernel(const uint32_t *__restrict__ keep, const uint32_t *__restrict__ mate,
                                                     const uint64_t *__restrict__ off, uint64_t n_rec, uint32_t *__restrict__ lead,
                                                     unsigned long long *__restrict__ flen)
{
    const uint64_t r = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (r > n_rec) return;
    uint32_t l = 0;
    unsigned long long len = 0;
    if (r < n_rec && keep[r]) {
        const uint32_t m = mate[r];
        if (m == NO_MATE) { l = 1u; len = bases_of(off, r) + 2u; }
        else if (m > r) { l = 1u; len = bases_of(off, r) + bases_of(off, m) + 2u; }
    }
    lead[r] = l;
    flen[r] = len;
}

__global__ __launch_bounds__(256) void leader_list_kernel(const uint32_t *__restrict__ lead, const uint32_t *__restrict__ fidx, uint64_t n_rec,
                                                          uint32_t *__restrict__ leader)
{
    const uint64_t r = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (r < n_rec && lead[r]) leader[fidx[r]] = (uint32_t)r;
}

// Sixteen lanes per fragment; flat holds n >= 16 bytes, dst is 16-byte aligned.  Fragment g of leader r begins at foff[r]:
// [D, J) mate 1's letters (none for an orphan of role 2), 'N' at J, [M2, E - 1) mate 2's (none for a single and an orphan of role
// 0 or 1), '\n' at E - 1.
__global__ __launch_bounds__(256) void join_kernel(const uint8_t *__restrict__ flat, uint64_t n, const uint64_t *__restrict__ off,
                                                   const uint32_t *__restrict__ leader, const uint32_t *__restrict__ mate,
                                                   const uint8_t *__restrict__ role, const unsigned long long *__restrict__ foff,
                                                   uint64_t n_frag, uint8_t *__restrict__ dst)
{
    const uint64_t g = ((uint64_t)blockIdx.x * 256u + threadIdx.x) >> 4;
    if (g >= n_frag) return;
    const uint32_t r = leader[g], m = mate[r];
    uint64_t s1 = 0, s2 = 0, len1 = 0, len2 = 0;
    if (m != NO_MATE) {
        const uint32_t m1 = role[r] == 1u ? r : m, m2 = role[r] == 1u ? m : r;
        s1 = off[m1], len1 = bases_of(off, m1);
        s2 = off[m2], len2 = bases_of(off, m2);
    } else if (role[r] == 2u) {
        s2 = off[r], len2 = bases_of(off, r);
    } else {
        s1 = off[r], len1 = bases_of(off, r);
    }
    const uint64_t D = foff[r], J = D + len1, M2 = J + 1u, L = M2 + len2, E = L + 1u;      // the fragment: [D, E); '\n' at L
    write_span(dst, D, E, threadIdx.x & 15u, [&](uint64_t a, uint64_t lo, uint64_t hi) {
        piece_t x = masked_fetch16(flat, n, s1, D, J, a, lo, hi) | masked_fetch16(flat, n, s2, M2, L, a, lo, hi);
        if (J >= lo && J < hi) x = with_byte(x, (uint32_t)(J - a), 'N');
        if (L >= lo && L < hi) x = with_byte(x, (uint32_t)(L - a), '\n');
        return x;
    });
}

// One lane per record r <= n_rec: out_len[r] = 4 + block_size when the hits of kept record r's fragment reach min_hits
__global__ __launch_bounds__(256) void fragment_len_kernel(const uint8_t *__restrict__ s, const uint64_t *__restrict__ rec,
                                                           const uint32_t *__restrict__ keep, const uint32_t *__restrict__ kidx,
                                                           const uint32_t *__restrict__ mate, const uint32_t *__restrict__ hits, uint64_t n_rec,
                                                           uint32_t min_hits, unsigned long long *__restrict__ out_len,
                                                           unsigned long long *__restrict__ tot)
{
    const uint64_t r = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    unsigned long long written = 0, frags = 0;
    if (r <= n_rec) {
        unsigned long long len = 0;
        if (r < n_rec && keep[r]) {
            const uint32_t m = mate[r];
            const uint64_t h = (uint64_t)hits[kidx[r]] + (m != NO_MATE ? (uint64_t)hits[kidx[m]] : 0u);
            if (h >= min_hits) {
                const uint64_t p = rec[r];
                len = 4ull + ss::ld32_le(s, p);
                written = 1;
                frags = m == NO_MATE || m > r ? 1 : 0;
            }
        }
        out_len[r] = len;
    }
    add_selected(written, frags, tot);      // (no fragment without a written record)
}

ss::BamTiming g_timing;      // the last ss_reads_load_pairs_bam: ss_bam_pairs_timing

// steps 1 (second half) to 6 on a stream that lies on the device; ms[1..6]
int join_on_device(const ss::BamDeviceStream &ds, int order, ss_reads **out, uint64_t counters[6], double *ms)
{
    auto t0 = Clock::now();
    ss::BamRecords recs;
    recs.want_off = true;
    char *flat = nullptr;
    uint64_t flat_len = 0, flat_cap = 0;
    int rc = ss::bam_records_flat_dev(ds.d, ds.n, ds.h, ds.seg, &flat, &flat_len, &flat_cap, &recs);
    if (rc) return rc;
    const ss::BamFlatOwner owned{recs, flat, flat_cap};
    ms[1] = ms_since(t0);
    ss::PoolScratch scratch;
    uint32_t *d_mate = nullptr;
    uint8_t *d_role = nullptr;
    rc = ss::bam_mates_dev((const uint8_t *)ds.d, recs, scratch, &d_mate, &d_role, counters, ms + 2);
    if (rc) return rc;
    if (counters[5]) return SS_EIO;
    const uint64_t n_frag = recs.kept - counters[2];
    ss_reads *S = nullptr;
    rc = ss::bam_join_dev(flat, flat_len, recs, scratch, d_mate, d_role, n_frag, &S, nullptr, ms + 5);      // steps 5 and 6
    if (rc) return rc;
    t0 = Clock::now();
    if (order) {
        rc = ss_reads_order(S);
        if (rc != SS_OK) { ss_reads_destroy(S); return rc; }
    }
    if (n_frag) ms[6] += ms_since(t0);
    *out = S;
    return SS_OK;
}

}  // namespace

namespace ss {

int bam_join_dev(const char *flat, uint64_t flat_len, const BamRecords &recs, PoolScratch &scratch, const uint32_t *d_mate,
                 const uint8_t *d_role, uint64_t n_frag, ss_reads **out, uint32_t **d_fidx_out, double *ms)
{
    const hipStream_t st = l2s::stream();
    const uint64_t n_rec = recs.n_rec, kept = recs.kept;
    const uint64_t total = (flat_len - kept) + 2u * n_frag;
    const char *const who = "ss_reads_join_pairs_bam";
    ss_reads *S = nullptr;
    uint8_t *slab = nullptr;
    int rc = SS_OK;
    *out = nullptr;
    if (d_fidx_out) *d_fidx_out = nullptr;
    if (n_frag) {
        // 5. leaders, lengths, offsets
        auto t0 = Clock::now();
        uint32_t *d_lead = nullptr, *d_fidx = nullptr, *d_leader = nullptr;
        unsigned long long *d_flen = nullptr, *d_foff = nullptr;
        void *d_tmp = nullptr;
        const int items = (int)(n_rec + 1);
        size_t tb1 = 0, tb2 = 0;
        unsigned long long tot = 0;
        uint32_t nf = 0;
        const ss::HipFail fail{who};
        bool bad = fail(scratch.get((void **)&d_lead, (n_rec + 1) * 4)) || fail(scratch.get((void **)&d_fidx, (n_rec + 1) * 4)) ||
                   fail(scratch.get((void **)&d_flen, (n_rec + 1) * 8)) || fail(scratch.get((void **)&d_foff, (n_rec + 1) * 8)) ||
                   fail(scratch.get((void **)&d_leader, n_frag * 4)) ||
                   fail(hipcub::DeviceScan::ExclusiveSum(nullptr, tb1, d_lead, d_fidx, items, st)) ||
                   fail(hipcub::DeviceScan::ExclusiveSum(nullptr, tb2, d_flen, d_foff, items, st)) ||
                   fail(scratch.get(&d_tmp, std::max(tb1, tb2)));
        if (!bad) {
            hipLaunchKernelGGL(length_kernel, dim3(grid_for(n_rec + 1)), dim3(256), 0, st, (const uint32_t *)recs.d_keep, (const uint32_t *)d_mate,
                               (const uint64_t *)recs.d_off, n_rec, d_lead, d_flen);
            tb1 = tb2 = std::max(tb1, tb2);
            bad = fail(hipGetLastError()) || fail(hipcub::DeviceScan::ExclusiveSum(d_tmp, tb1, d_lead, d_fidx, items, st)) ||
                  fail(hipcub::DeviceScan::ExclusiveSum(d_tmp, tb2, d_flen, d_foff, items, st));
        }
        if (!bad) {
            hipLaunchKernelGGL(leader_list_kernel, dim3(grid_for(n_rec)), dim3(256), 0, st, (const uint32_t *)d_lead, (const uint32_t *)d_fidx, n_rec,
                               d_leader);
            bad = fail(hipGetLastError()) || fail(hipMemcpyAsync(&nf, d_fidx + n_rec, 4, hipMemcpyDeviceToHost, st)) ||
                  fail(ss::l2s::copy(&tot, d_foff + n_rec, 8, hipMemcpyDeviceToHost));
        }
        if (!bad && (nf != n_frag || tot != total)) {
            ss::set_last_error("ss_reads_join_pairs_bam: the leaders are not the fragments", __FILE__, __LINE__, hipErrorUnknown);
            bad = true;
        }
        if (ms) ms[0] = ms_since(t0);
        // 6. the slab
        t0 = Clock::now();
        if (!bad) {
            rc = ss::one_slab_set(n_frag, total, who, &S, &slab);
            if (rc) return rc;
            hipLaunchKernelGGL(join_kernel, dim3(grid_for(n_frag * 16u)), dim3(256), 0, st, (const uint8_t *)flat, ss_reads::padded(flat_len),
                               (const uint64_t *)recs.d_off, (const uint32_t *)d_leader, (const uint32_t *)d_mate, (const uint8_t *)d_role,
                               (const unsigned long long *)d_foff, n_frag, slab);
            bad = fail(hipGetLastError());
        }
        bad = fail(ss::l2s::sync()) || bad;
        if (bad) { ss_reads_destroy(S); return SS_EHIP; }
        if (ms) ms[1] = ms_since(t0);
        if (d_fidx_out) *d_fidx_out = d_fidx;
    } else {
        rc = ss::one_slab_set(0, 0, who, &S, &slab);
        if (rc) return rc;
    }
    *out = S;
    return SS_OK;
}

int bam_mates_dev(const uint8_t *s, const BamRecords &recs, PoolScratch &scratch, uint32_t **d_mate, uint8_t **d_role, uint64_t counters[6],
                  double *ms)
{
    const hipStream_t st = l2s::stream();
    const uint64_t n_rec = recs.n_rec;
    for (int i = 0; i < 6; i++) counters[i] = 0;
    counters[0] = n_rec;
    counters[1] = recs.kept;
    *d_mate = nullptr;
    *d_role = nullptr;
    if (!n_rec) return SS_OK;
    // 2. keys
    auto t0 = Clock::now();
    unsigned long long *d_h1 = nullptr, *d_h2 = nullptr, *d_cnt = nullptr;
    uint32_t *d_paired = nullptr, *d_pidx = nullptr;
    void *d_tmp = nullptr;
    SS_HIP(scratch.get((void **)&d_h1, n_rec * 8));
    SS_HIP(scratch.get((void **)&d_h2, n_rec * 8));
    SS_HIP(scratch.get((void **)d_role, n_rec));
    SS_HIP(scratch.get((void **)d_mate, n_rec * 4));
    SS_HIP(scratch.get((void **)&d_paired, (n_rec + 1) * 4));
    SS_HIP(scratch.get((void **)&d_pidx, (n_rec + 1) * 4));
    SS_HIP(scratch.get((void **)&d_cnt, 24));
    SS_HIP(l2s::set(d_cnt, 0, 24));
    hipLaunchKernelGGL(key_kernel, dim3(grid_for(n_rec + 1)), dim3(256), 0, st, s, (const uint64_t *)recs.d_rec, (const uint32_t *)recs.d_keep, n_rec,
                       d_h1, d_h2, *d_role, d_paired, *d_mate);
    SS_HIP(hipGetLastError());
    size_t tb = 0;
    SS_HIP(hipcub::DeviceScan::ExclusiveSum(nullptr, tb, d_paired, d_pidx, (int)(n_rec + 1), st));
    SS_HIP(scratch.get(&d_tmp, tb));
    SS_HIP(hipcub::DeviceScan::ExclusiveSum(d_tmp, tb, d_paired, d_pidx, (int)(n_rec + 1), st));
    uint32_t n_p = 0;
    SS_HIP(l2s::copy(&n_p, d_pidx + n_rec, 4, hipMemcpyDeviceToHost));
    if (ms) ms[0] = ms_since(t0);
    counters[4] = recs.kept - n_p;
    if (!n_p) return SS_OK;
    // 3. the paired records sorted by (h1, h2), records of one name in record order
    t0 = Clock::now();
    unsigned long long *d_ka = nullptr, *d_kb = nullptr;
    uint32_t *d_ia = nullptr, *d_ib = nullptr;
    void *d_sort = nullptr;
    SS_HIP(scratch.get((void **)&d_ka, (uint64_t)n_p * 8));
    SS_HIP(scratch.get((void **)&d_kb, (uint64_t)n_p * 8));
    SS_HIP(scratch.get((void **)&d_ia, (uint64_t)n_p * 4));
    SS_HIP(scratch.get((void **)&d_ib, (uint64_t)n_p * 4));
    hipLaunchKernelGGL(compact_kernel, dim3(grid_for(n_rec)), dim3(256), 0, st, (const uint32_t *)d_paired, (const uint32_t *)d_pidx,
                       (const unsigned long long *)d_h2, n_rec, d_ka, d_ia);
    SS_HIP(hipGetLastError());
    size_t sb = 0;
    SS_HIP(hipcub::DeviceRadixSort::SortPairs(nullptr, sb, d_ka, d_kb, d_ia, d_ib, (int)n_p, 0, 64, st));
    SS_HIP(scratch.get(&d_sort, sb));
    SS_HIP(hipcub::DeviceRadixSort::SortPairs(d_sort, sb, d_ka, d_kb, d_ia, d_ib, (int)n_p, 0, 64, st));      // by h2 -> d_ib
    hipLaunchKernelGGL(gather_h1_kernel, dim3(grid_for(n_p)), dim3(256), 0, st, (const uint32_t *)d_ib, (const unsigned long long *)d_h1, n_p, d_ka);
    SS_HIP(hipGetLastError());
    SS_HIP(hipcub::DeviceRadixSort::SortPairs(d_sort, sb, d_ka, d_kb, d_ib, d_ia, (int)n_p, 0, 64, st));      // then by h1 -> d_ia
    if (ms) { SS_HIP(l2s::sync()); ms[1] = ms_since(t0); }
    // 4. link
    t0 = Clock::now();
    hipLaunchKernelGGL(link_kernel, dim3(grid_for(n_p)), dim3(256), 0, st, (const uint32_t *)d_ia, (const unsigned long long *)d_h1,
                       (const unsigned long long *)d_h2, (const uint8_t *)*d_role, n_p, *d_mate, d_cnt);
    SS_HIP(hipGetLastError());
    unsigned long long cnt[3] = {0, 0, 0};
    SS_HIP(l2s::copy(cnt, d_cnt, 24, hipMemcpyDeviceToHost));
    counters[2] = cnt[0];
    counters[3] = cnt[1];
    counters[5] = cnt[2];
    if (ms) ms[2] = ms_since(t0);
    return SS_OK;
}

int bam_fragment_out_len(const uint8_t *s, const BamRecords &recs, const uint32_t *d_mate, const uint32_t *d_hits, uint32_t min_hits,
                         unsigned long long *d_out_len, unsigned long long *d_tot)
{
    hipLaunchKernelGGL(fragment_len_kernel, dim3(grid_for(recs.n_rec + 1)), dim3(256), 0, l2s::stream(), s, (const uint64_t *)recs.d_rec,
                       (const uint32_t *)recs.d_keep, (const uint32_t *)recs.d_kidx, d_mate, d_hits, recs.n_rec, min_hits, d_out_len, d_tot);
    SS_HIP(hipGetLastError());
    return SS_OK;
}

}  // namespace ss

extern "C" {

int ss_bam_pairs_timing(double out[8]) { return g_timing.load(out); }

int ss_bam_mates(const void *stream, uint64_t n, uint32_t *mate, uint64_t cap, uint64_t counters[6])
{
    if ((!stream && n) || !counters || (!mate && cap)) return SS_EINVAL;
    for (int i = 0; i < 6; i++) counters[i] = 0;
    ss::BamDeviceStream ds;
    int rc = ds.upload(stream, n);
    if (rc) return rc;
    ss::BamRecords recs;
    char *flat = nullptr;
    uint64_t flat_len = 0, flat_cap = 0;
    rc = ss::bam_records_flat_dev(ds.d, ds.n, ds.h, ds.seg, &flat, &flat_len, &flat_cap, &recs);
    if (rc) return rc;
    ss::big_put(flat, flat_cap);
    {
        ss::PoolScratch scratch;
        uint32_t *d_mate = nullptr;
        uint8_t *d_role = nullptr;
        rc = ss::bam_mates_dev((const uint8_t *)ds.d, recs, scratch, &d_mate, &d_role, counters, nullptr);
        if (rc == SS_OK && recs.n_rec > cap) rc = SS_ERANGE;
        if (rc == SS_OK && recs.n_rec && ss::l2s::copy(mate, d_mate, recs.n_rec * 4, hipMemcpyDeviceToHost) != hipSuccess) rc = SS_EHIP;
    }
    recs.release();
    if (rc == SS_OK && counters[5]) rc = SS_EIO;
    return rc;
}

int ss_reads_join_pairs_bam(const void *stream, uint64_t n, int order, ss_reads **out, uint64_t counters[6])
{
    if (!out) return SS_EINVAL;
    *out = nullptr;
    if ((!stream && n) || !counters) return SS_EINVAL;
    for (int i = 0; i < 6; i++) counters[i] = 0;
    ss::g_join_pairs_calls++;
    ss::BamDeviceStream ds;
    const int rc = ds.upload(stream, n);
    if (rc) return rc;
    double ms[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    return join_on_device(ds, order, out, counters, ms);
}

int ss_reads_load_pairs_bam(const char *path, int order, ss_reads **out, uint64_t counters[6])
{
    if (!out) return SS_EINVAL;
    *out = nullptr;
    if (!path || !counters) return SS_EINVAL;
    for (int i = 0; i < 6; i++) counters[i] = 0;
    ss::BamFileCall call;
    int rc = call.open(path, ss::g_join_pairs_calls);
    if (rc) return rc;
    rc = join_on_device(call.ds, order, out, counters, call.ms);
    if (rc) return rc;
    call.finish(g_timing);
    return SS_OK;
}

}  // extern "C"
