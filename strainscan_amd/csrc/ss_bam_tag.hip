// ss_bam_tag.hip -- `--tag_bam`: a BAM sample written back with the class of every read as two aux tags.
//
// `--classify_reads` says how many reads went to each node, never which.  For a BAM that needs no map back to file order:
// ss_bam_dev.hip leaves the start (d_rec), the kept flag (d_keep) and the kept ordinal (d_kidx) of every record on the device, and
// its flat block holds kept record i as non-empty record i -- so the classes that classify_records (ss_classify.hip) leaves for
// that block are indexed by BAM record.  One path, for ss_bam_tag_stream (a stream in host memory) and ss_bam_tag_file (a file);
// the rule is stated in strainscan_hip.h, "Tagged BAM", and tests/bam_tag_model.py restates it:
//   1  the stream on the device (BamDeviceStream, ss_bam_dev.hip)
//   2  bam_records_flat_dev: walk, list, keep, length, decode
//   3  `pairs`: bam_mates_dev + bam_join_dev (ss_bam_pairs.hip): the fragments as a one-slab set, built from the same flat block,
//      and the fragment index of every leader
//   4  classify_records on that set, or on the one-slab set wrapped around the flat block, with the classes and the scores kept
//   5  aux_check_kernel: one lane per record walks the aux fields of a kept record by field (aux_walk, ss_tag_copy.h) -- a record
//      that already bears one of the two tags, or whose fields do not end with the record, stops the call;
//      record_tag_kernel: record -> (its fragment's leader -> fragment index ->) class and score -> the two values of its tags;
//      tag_copy_kernel: sixteen lanes per record copy it to where it stands in the new body, rec[r] - hdr_end + 14 kidx[r] -- a
//      fixed 14 bytes per kept record, so the prefix the decoder left is the only one -- in 16-byte aligned pieces of the
//      destination (the piece copy, ss_piece_copy.h); a kept record's span is composed from the patched block_size, the record's
//      bytes and the 14 tag bytes (tagged_piece, ss_tag_copy.h)
//   6  the body to the host (bam_download_chunks); ss_bam_tag_file: through the file step and the call frame of ss_bam_out.hip.
// Scratch: the stream-ordered pool (PoolScratch) and ss::big_malloc.  Plain launches, no device-wide barrier inside a kernel.
#include "ss_bam.h"
#include "ss_tag_copy.h"

using namespace ss::dev;
using ss::Clock;
using ss::grid_for;
using ss::ms_since;
using ss::NO_MATE;

namespace {

// where the aux fields of the record at s + p begin (rec_len of ss_bam_dev.hip has checked that this is not behind its end)
__device__ __forceinline__ uint64_t aux_begin(const uint8_t *__restrict__ s, uint64_t p)
{
    const uint64_t lrn = s[p + 12], ncig = (uint64_t)s[p + 16] | (uint64_t)s[p + 17] << 8, lseq = ss::ld32_le(s, p + 20);
    return p + 36u + lrn + 4u * ncig + (lseq + 1u) / 2u + lseq;
}

// One lane per record r <= n_rec: flag[r] = aux_walk of a kept record (0 for the others and for [n_rec]).  cnt[0] += kept records
// that bear one of the tags, cnt[1] += kept records whose aux fields are damaged
__global__ __launch_bounds__(256) void aux_check_kernel(const uint8_t *__restrict__ s, const uint64_t *__restrict__ rec,
                                                        const uint32_t *__restrict__ keep, uint64_t n_rec, uint32_t tags,
                                                        uint8_t *__restrict__ flag, unsigned long long *__restrict__ cnt)
{
    const uint64_t r = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    unsigned long long tagged = 0, damaged = 0;
    if (r <= n_rec) {
        uint32_t f = AUX_OK;
        if (r < n_rec && keep[r]) {
            const uint64_t p = rec[r], end = p + 4u + ss::ld32_le(s, p), b = aux_begin(s, p);
            f = b > end ? (uint32_t)AUX_DAMAGED : aux_walk(s, b, end, tags);
        }
        flag[r] = (uint8_t)f;
        tagged = f == AUX_TAGGED;
        damaged = f == AUX_DAMAGED;
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        tagged += __shfl_xor(tagged, d, 64);
        damaged += __shfl_xor(damaged, d, 64);
    }
    if ((threadIdx.x & 63u) == 0) {
        if (tagged) atomicAdd(&cnt[0], tagged);
        if (damaged) atomicAdd(&cnt[1], damaged);
    }
}

// One lane per record: kept record r -> the record of the classified set it belongs to -- kidx[r], or with `mate` the fragment
// index of its fragment's leader (the earlier record of the two) -- and from there val[r] = node_value[class], sc[r] = the score.
// cnt[2] += kept records of a class != 0
__global__ __launch_bounds__(256) void record_tag_kernel(const uint32_t *__restrict__ keep, const uint32_t *__restrict__ kidx,
                                                         const uint32_t *__restrict__ mate, const uint32_t *__restrict__ fidx,
                                                         const uint32_t *__restrict__ cls, const uint32_t *__restrict__ score,
                                                         const int32_t *__restrict__ node_value, uint64_t n_rec, uint32_t n_nodes,
                                                         uint64_t n_classified, int32_t *__restrict__ val, uint32_t *__restrict__ sc,
                                                         unsigned long long *__restrict__ cnt)
{
    const uint64_t r = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    unsigned long long classified = 0;
    if (r < n_rec && keep[r]) {
        uint64_t i = kidx[r];
        if (mate) {
            const uint32_t m = mate[r];
            i = fidx[(m == NO_MATE || m > r) ? r : m];
        }
        uint32_t c = 0, q = 0;
        if (i < n_classified) { c = cls[i]; q = score[i]; }
        if (c > n_nodes) c = 0;
        val[r] = node_value[c];
        sc[r] = q;
        classified = c != 0u;
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) classified += __shfl_xor(classified, d, 64);
    if ((threadIdx.x & 63u) == 0 && classified) atomicAdd(&cnt[2], classified);
}

// Sixteen lanes per record; src holds n >= 16 bytes and every record lies inside them; dst is 16-byte aligned.  Record r goes to
// D = rec[r] - hdr_end + 14 kidx[r] (kidx: the kept records before it): a record that is not kept as it is, a kept record with its
// block_size raised and the 14 tag bytes behind it (tagged_piece).
__global__ __launch_bounds__(256) void tag_copy_kernel(const uint8_t *__restrict__ src, uint64_t n, const uint64_t *__restrict__ rec,
                                                       const uint32_t *__restrict__ keep, const uint32_t *__restrict__ kidx,
                                                       const int32_t *__restrict__ val, const uint32_t *__restrict__ sc, uint64_t n_rec,
                                                       uint64_t hdr_end, uint32_t tags, uint8_t *__restrict__ dst)
{
    const uint64_t r = ((uint64_t)blockIdx.x * 256u + threadIdx.x) >> 4;
    if (r >= n_rec) return;
    const uint64_t S = rec[r], ol = 4ull + ss::ld32_le(src, S), D = S - hdr_end + (uint64_t)TAG_BYTES * kidx[r];
    if (keep[r]) {
        const piece_t tag = tag_fields(tags, val[r], sc[r]);
        write_span(dst, D, D + ol + TAG_BYTES, threadIdx.x & 15u,
                   [&](uint64_t a, uint64_t lo, uint64_t hi) { return tagged_piece(src, n, S, ol, D, tag, a, lo, hi); });
    } else {
        copy_span(dst, D, D + ol, threadIdx.x & 15u, src, n, S);
    }
}

std::atomic<uint64_t> g_bam_tag_calls{0};
ss::BamTiming g_timing;      // the last ss_bam_tag_file: ss_bam_tag_timing

// What the call asks for, checked once
struct TagArgs {
    const ss_db *db;
    const uint32_t *row_node;
    uint32_t n_nodes;
    const uint32_t *parent;
    uint32_t min_score;
    const int32_t *node_value;
    uint32_t tags;      // t0 | t1 << 8 | t2 << 16 | t3 << 24
    bool pairs;
    uint64_t *direct, *node_hits, *kmers;
};

bool tag_ok(const char *t)
{
    const auto alpha = [](char c) { return (c >= 'A' && c <= 'Z') || (c >= 'a' && c <= 'z'); };
    return alpha(t[0]) && (alpha(t[1]) || (t[1] >= '0' && t[1] <= '9'));
}

int check_args(const ss_db *db, const uint32_t *row_node, uint32_t n_nodes, const uint32_t *parent, uint32_t min_score, const int32_t *node_value,
               const char *tags, int pairs, uint64_t *direct, uint64_t *node_hits, uint64_t *kmers, TagArgs *A)
{
    if (!db || !row_node || !parent || !node_value || !tags || min_score == 0 || n_nodes < 1 || n_nodes > SS_CLASS_NODES_MAX) return SS_EINVAL;
    if (!tag_ok(tags) || !tag_ok(tags + 2) || (tags[0] == tags[2] && tags[1] == tags[3])) return SS_EINVAL;
    if (db->layout != 1) return SS_ERANGE;                          // page-index tables only
    const uint32_t t = (uint32_t)(uint8_t)tags[0] | (uint32_t)(uint8_t)tags[1] << 8 | (uint32_t)(uint8_t)tags[2] << 16 | (uint32_t)(uint8_t)tags[3] << 24;
    *A = TagArgs{db, row_node, n_nodes, parent, min_score, node_value, t, pairs != 0, direct, node_hits, kmers};
    return SS_OK;
}

// What the device leaves: the new body in d_out (big_malloc'ed, out_cap; nullptr when nothing was copied)
struct Tagged {
    char *d_out = nullptr;
    uint64_t out_cap = 0, total = 0, hdr_end = 0;
    uint64_t counters[6] = {0, 0, 0, 0, 0, 0};
    double ms[4] = {0, 0, 0, 0};                   // walk + decode, mate link + join, classify, tag check + copy
    ~Tagged() { if (d_out) ss::big_put(d_out, out_cap); }
};

struct SetOwner {                                  // the fragments' set, destroyed on every way out
    ss_reads *s = nullptr;
    ~SetOwner() { if (s) ss_reads_destroy(s); }
};

// steps 2 to 5 on a stream that lies on the device (h_stream: the same bytes on the host, or nullptr).  cap: the bytes the caller
// has room for -- a body above it is measured and counted, not copied (SS_ERANGE).  SS_EIO with out->counters set: a violating
// name group (`pairs`), a kept record that bears a tag (counters[3]) or has damaged aux fields
int tag_on_device(const char *d_stream, uint64_t n, const uint8_t *h_stream, const std::vector<uint64_t> &seg, const TagArgs &A, uint64_t cap,
                  Tagged *out)
{
    auto t0 = Clock::now();
    // 2. records, kept flags, flat block
    ss::BamRecords recs;
    recs.want_off = A.pairs;
    char *flat = nullptr;
    uint64_t flat_len = 0, flat_cap = 0;
    int rc = ss::bam_records_flat_dev(d_stream, n, h_stream, seg, &flat, &flat_len, &flat_cap, &recs);
    if (rc) return rc;
    const hipStream_t st = ss::l2s::stream();
    const ss::BamFlatOwner owned{recs, flat, flat_cap};
    const uint64_t n_rec = recs.n_rec, kept = recs.kept;
    const uint8_t *s = reinterpret_cast<const uint8_t *>(d_stream);
    out->hdr_end = recs.hdr_end;
    out->counters[0] = n_rec;
    out->counters[1] = kept;
    out->counters[4] = kept;
    out->total = (n - recs.hdr_end) + (uint64_t)TAG_BYTES * kept;
    out->ms[0] = ms_since(t0);
    // 3. `pairs`: the fragments as a set of their own
    t0 = Clock::now();
    SetOwner frags;                                 // (outlives C, whose parts point into its slab)
    ss_reads wrapped;
    ss::Classified C;
    ss::PoolScratch &scratch = C.rh.scratch;
    uint32_t *d_mate = nullptr, *d_fidx = nullptr;
    uint8_t *d_role = nullptr;
    uint64_t n_classified = kept;
    const ss_reads *R = &wrapped;
    if (A.pairs) {
        uint64_t pc[6];
        rc = ss::bam_mates_dev(s, recs, scratch, &d_mate, &d_role, pc, nullptr);
        if (rc) return rc;
        if (pc[5]) return SS_EIO;
        n_classified = kept - pc[2];
        out->counters[4] = n_classified;
        rc = ss::bam_join_dev(flat, flat_len, recs, scratch, d_mate, d_role, n_classified, &frags.s, &d_fidx, nullptr);
        if (rc) return rc;
        R = frags.s;
        out->ms[1] = ms_since(t0);
    } else if (kept) {
        ss::bam_flat_as_set(flat, flat_len, flat_cap, kept, &wrapped);
    }
    // 4. classes and scores
    t0 = Clock::now();
    rc = ss::classify_records(A.db, R, A.row_node, A.n_nodes, A.parent, A.min_score, true, nullptr, &C, true);
    if (rc) return rc;
    uint64_t ties = 0;
    rc = ss::classified_counts(C, A.n_nodes, A.direct, A.node_hits, A.kmers, &ties);
    if (rc) return rc;
    if (C.rh.rec_total != n_classified) {
        ss::set_last_error("ss_bam_tag: the classified records are not the kept records", __FILE__, __LINE__, hipErrorUnknown);
        return SS_EHIP;
    }
    out->counters[5] = ties;
    out->ms[2] = ms_since(t0);
    if (!n_rec) return SS_OK;
    // 5. the aux fields, the values of the tags, the copy
    t0 = Clock::now();
    uint8_t *d_flag = nullptr;
    unsigned long long *d_cnt = nullptr;
    int32_t *d_value = nullptr, *d_val = nullptr;
    uint32_t *d_sc = nullptr;
    SS_HIP(scratch.get((void **)&d_flag, n_rec + 1));
    SS_HIP(scratch.get((void **)&d_cnt, 24));
    SS_HIP(scratch.get((void **)&d_value, ((size_t)A.n_nodes + 1) * 4));
    SS_HIP(scratch.get((void **)&d_val, n_rec * 4));
    SS_HIP(scratch.get((void **)&d_sc, n_rec * 4));
    SS_HIP(ss::l2s::set(d_cnt, 0, 24));
    SS_HIP(ss::l2s::copy(d_value, A.node_value, ((size_t)A.n_nodes + 1) * 4, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(aux_check_kernel, dim3(grid_for(n_rec + 1)), dim3(256), 0, st, s, (const uint64_t *)recs.d_rec, (const uint32_t *)recs.d_keep,
                       n_rec, A.tags, d_flag, d_cnt);
    SS_HIP(hipGetLastError());
    hipLaunchKernelGGL(record_tag_kernel, dim3(grid_for(n_rec)), dim3(256), 0, st, (const uint32_t *)recs.d_keep, (const uint32_t *)recs.d_kidx,
                       (const uint32_t *)(A.pairs ? d_mate : nullptr), (const uint32_t *)d_fidx, (const uint32_t *)C.d_class,
                       (const uint32_t *)C.d_score, (const int32_t *)d_value, n_rec, A.n_nodes, n_classified, d_val, d_sc, d_cnt);
    SS_HIP(hipGetLastError());
    unsigned long long cnt[3] = {0, 0, 0};
    SS_HIP(ss::l2s::copy(cnt, d_cnt, 24, hipMemcpyDeviceToHost));
    out->counters[2] = cnt[2];
    if (cnt[1]) return SS_EIO;                                          // a damaged stream: counters[3] stays 0
    out->counters[3] = cnt[0];
    if (cnt[0]) return SS_EIO;
    if (out->total > cap) return SS_ERANGE;
    if (n < 16) return SS_EHIP;                                         // (a record is 36 bytes and more)
    if (ss::big_malloc((void **)&out->d_out, ss_reads::padded(out->total), &out->out_cap) != hipSuccess) { out->d_out = nullptr; return SS_ENOMEM; }
    hipLaunchKernelGGL(tag_copy_kernel, dim3(grid_for(n_rec * 16u)), dim3(256), 0, st, s, n, (const uint64_t *)recs.d_rec, (const uint32_t *)recs.d_keep,
                       (const uint32_t *)recs.d_kidx, (const int32_t *)d_val, (const uint32_t *)d_sc, n_rec, recs.hdr_end, A.tags,
                       (uint8_t *)out->d_out);
    SS_HIP(hipGetLastError());
    SS_HIP(ss::l2s::sync());
    out->ms[3] = ms_since(t0);
    return SS_OK;
}

}  // namespace

extern "C" {

int ss_bam_tag_calls(uint64_t *n)
{
    if (!n) return SS_EINVAL;
    *n = g_bam_tag_calls.load();
    return SS_OK;
}

int ss_bam_tag_timing(double out[8]) { return g_timing.load(out); }

int ss_bam_tag_stream(const void *stream, uint64_t n, const ss_db *db, const uint32_t *row_node, uint32_t n_nodes, const uint32_t *parent,
                      uint32_t min_score, const int32_t *node_value, const char tags[4], int pairs, void *out, uint64_t cap, uint64_t *out_len,
                      uint64_t counters[6], uint64_t *direct, uint64_t *node_hits, uint64_t *kmers)
{
    if ((!stream && n) || !out_len || !counters || (!out && cap)) return SS_EINVAL;
    TagArgs A;
    int rc = check_args(db, row_node, n_nodes, parent, min_score, node_value, tags, pairs, direct, node_hits, kmers, &A);
    if (rc) return rc;
    g_bam_tag_calls++;
    *out_len = 0;
    for (int i = 0; i < 6; i++) counters[i] = 0;
    ss::BamDeviceStream ds;
    rc = ds.upload(stream, n);
    if (rc) return rc;
    Tagged T;
    rc = tag_on_device(ds.d, n, ds.h, ds.seg, A, cap, &T);
    memcpy(counters, T.counters, sizeof T.counters);
    if (rc == SS_OK || rc == SS_ERANGE) *out_len = T.total;
    if (rc) return rc;
    return ss::bam_download_chunks(T.d_out, T.total, (char *)out);
}

int ss_bam_tag_file(const char *in_path, const ss_db *db, const uint32_t *row_node, uint32_t n_nodes, const uint32_t *parent, uint32_t min_score,
                    const int32_t *node_value, const char tags[4], int pairs, const char *out_path, uint64_t counters[6], uint64_t *direct,
                    uint64_t *node_hits, uint64_t *kmers)
{
    if (!in_path || !out_path || !counters) return SS_EINVAL;
    TagArgs A;
    int rc = check_args(db, row_node, n_nodes, parent, min_score, node_value, tags, pairs, direct, node_hits, kmers, &A);
    if (rc) return rc;
    for (int i = 0; i < 6; i++) counters[i] = 0;
    ss::BamFileCall call;
    rc = call.open(in_path, g_bam_tag_calls);                           // 1. the stream on the device
    if (rc) return rc;
    ss::BamDeviceStream &ds = call.ds;
    Tagged T;
    rc = tag_on_device(ds.d, ds.n, ds.h, ds.seg, A, ~0ull, &T);
    memcpy(counters, T.counters, sizeof T.counters);
    if (rc) return rc;
    // 6. header and body to the host, then the file
    rc = ss::bam_write_file(ds, T.hdr_end, T.d_out, T.total, out_path, &call.ms[5], &call.ms[6]);
    if (rc) return rc;
    for (int i = 0; i < 4; i++) call.ms[1 + i] = T.ms[i];
    call.finish(g_timing);
    return SS_OK;
}

}  // extern "C"
