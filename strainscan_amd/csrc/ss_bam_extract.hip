// ss_bam_extract.hip -- `-x` / `--by_strain` on a BAM sample: the records of the selected templates, copied out of the inflated
// stream on the device, written as a BGZF BAM on the host.
//
// The FASTQ writer (ss_extract.hip) finds reads again by content because a resident set keeps no map back to file order.  A BAM
// needs no such map: ss_bam_dev.hip leaves the start of every record (d_rec), the kept flag (d_keep) and the kept ordinal (d_kidx)
// on the device, and its flat block holds kept record i as non-empty record i -- so the hits of rec_hits_of (ss_support.hip) on
// that block are indexed by BAM record.  One path, for ss_bam_select (a stream in host memory) and ss_bam_extract (a file):
//   1  the stream on the device (BamDeviceStream, ss_bam_dev.hip: gpu_gunzip where the loader would use it; else the host
//      inflaters and an upload)
//   2  bam_records_flat_dev: bam_to_flat_dev (shard_world 1) with BamRecords: walk, list, keep, length, decode; the record starts
//      from the host walk when the device walk declines
//   3  the flat block wrapped as a one-slab ASCII set -> rec_hits_of (with slot labels: the hits of one label), rec_total == kept
//   4  name_digest_kernel: one lane per record; a kept record's read name (the bytes before the first NUL) -> two independent
//      64-bit hashes over the bytes and the length, and sel[r] = hits >= N.  ExclusiveSum + compact_kernel + hipcub SortPairs: the
//      digests of the selected records, sorted by the first hash.  template_len_kernel: a kept record is written when it is
//      selected or a binary search finds its digest (both hashes) among them; out_len[r] = 4 + block_size, else 0
//   5  a 64-bit ExclusiveSum of out_len -> offsets; record_gather_kernel: sixteen lanes per written record copy it in 16-byte
//      aligned pieces of the destination (the piece copy, ss_piece_copy.h: copy_span)
//   6  the result to the host (bam_download_chunks); ss_bam_extract: through the file step and the call frame of ss_bam_out.hip.
// Records that the loader does not keep (0x100, 0x800, no bases) are never written, whatever their name.
// ss_bam_select_pairs / ss_bam_extract_pairs (`--pairs`): the same path with the mate link of ss_bam_pairs.hip in the place of step
// 4 -- a kept record is written iff its hits and its mate's together reach N, and nothing is joined by name after that.
// Scratch: the stream-ordered pool (PoolScratch) and ss::big_malloc.  No device-wide barrier inside a kernel.
#include "ss_bam.h"
#include "ss_piece_copy.h"

#include <hipcub/hipcub.hpp>

using namespace ss::dev;
using ss::Clock;
using ss::grid_for;
using ss::ms_since;

namespace {

// One lane per record r <= n_rec (entry n_rec closes the sums).  A kept record: (h1, h2) = the digest of its name (bam_name_digest,
// ss_bam.h); sel = its hits reach min_hits.  A record that is not kept: sel = 0 and a digest nobody asks for.
__global__ __launch_bounds__(256) void name_digest_kernel(const uint8_t *__restrict__ s, const uint64_t *__restrict__ rec,
                                                          const uint32_t *__restrict__ keep, const uint32_t *__restrict__ kidx,
                                                          const uint32_t *__restrict__ hits, uint64_t n_rec, uint32_t min_hits,
                                                          unsigned long long *__restrict__ h1, unsigned long long *__restrict__ h2,
                                                          uint32_t *__restrict__ sel)
{
    const uint64_t r = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (r > n_rec) return;
    if (r == n_rec || !keep[r]) { sel[r] = 0u; return; }
    ss::bam_name_digest(s, rec[r], &h1[r], &h2[r]);
    sel[r] = hits[kidx[r]] >= min_hits ? 1u : 0u;
}

// the digests of the selected records, in record order: (k1, k2)[sidx[r]]
__global__ __launch_bounds__(256) void compact_kernel(const uint32_t *__restrict__ sel, const uint32_t *__restrict__ sidx,
                                                      const unsigned long long *__restrict__ h1, const unsigned long long *__restrict__ h2,
                                                      uint64_t n_rec, unsigned long long *__restrict__ k1, unsigned long long *__restrict__ k2)
{
    const uint64_t r = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (r >= n_rec || !sel[r]) return;
    k1[sidx[r]] = h1[r];
    k2[sidx[r]] = h2[r];
}

// out_len[r] (r <= n_rec; [n_rec] = 0) = 4 + block_size when kept record r is selected or shares its name's digest with a selected
// record (k1 ascending, k2 beside it: every entry of the run of equal k1 is looked at, so a true match is never missed), else 0.
// tot[0] += records written
__global__ __launch_bounds__(256) void template_len_kernel(const uint8_t *__restrict__ s, const uint64_t *__restrict__ rec,
                                                           const uint32_t *__restrict__ keep, const uint32_t *__restrict__ sel,
                                                           const unsigned long long *__restrict__ h1, const unsigned long long *__restrict__ h2,
                                                           uint64_t n_rec, const unsigned long long *__restrict__ k1,
                                                           const unsigned long long *__restrict__ k2, uint32_t n_sel,
                                                           unsigned long long *__restrict__ out_len, unsigned long long *__restrict__ tot)
{
    const uint64_t r = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    unsigned long long cnt = 0;
    if (r <= n_rec) {
        unsigned long long len = 0;
        if (r < n_rec && keep[r]) {
            bool w = sel[r] != 0u;
            if (!w && n_sel) {
                const unsigned long long a = h1[r], b = h2[r];
                uint32_t lo = 0, hi = n_sel;
                while (lo < hi) {
                    const uint32_t mid = lo + ((hi - lo) >> 1);
                    if (k1[mid] < a) lo = mid + 1u;
                    else hi = mid;
                }
                for (; lo < n_sel && k1[lo] == a && !w; lo++) w = k2[lo] == b;
            }
            if (w) { len = 4ull + ss::ld32_le(s, rec[r]); cnt = 1; }
        }
        out_len[r] = len;
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) cnt += __shfl_xor(cnt, d, 64);
    if ((threadIdx.x & 63u) == 0 && cnt) atomicAdd(&tot[0], cnt);
}

// Sixteen lanes per record; src holds n >= 16 bytes and every written record lies inside them; dst is 16-byte aligned.  The piece
// copy of ss_piece_copy.h, the record's bytes as they are (copy_span).
__global__ __launch_bounds__(256) void record_gather_kernel(const uint8_t *__restrict__ src, uint64_t n, const uint64_t *__restrict__ rec,
                                                            const unsigned long long *__restrict__ out_len,
                                                            const unsigned long long *__restrict__ out_off, uint64_t n_rec,
                                                            uint8_t *__restrict__ dst)
{
    const uint64_t r = ((uint64_t)blockIdx.x * 256u + threadIdx.x) >> 4;
    if (r >= n_rec) return;
    const uint64_t ol = out_len[r];
    if (!ol) return;                                                    // not written
    const uint64_t D = out_off[r], S = rec[r];
    copy_span(dst, D, D + ol, threadIdx.x & 15u, src, n, S);
}

std::atomic<uint64_t> g_bam_extract_calls{0};
ss::BamTiming g_timing;      // the last ss_bam_extract: ss_bam_extract_timing

// What the selection leaves: the written records back to back in d_out (big_malloc'ed, out_cap; nullptr when nothing is written)
struct Selection {
    char *d_out = nullptr;
    uint64_t out_cap = 0, total = 0, hdr_end = 0;
    uint64_t counters[4] = {0, 0, 0, 0};
    uint64_t pair_counters[6] = {0, 0, 0, 0, 0, 0};      // `pairs`: what the mate link counted
    double ms[4] = {0, 0, 0, 0};                   // walk + decode, hits, join, gather
    ~Selection() { if (d_out) ss::big_put(d_out, out_cap); }
};

// steps 2 to 5 on a stream that lies on the device (h_stream: the same bytes on the host, or nullptr)
// pairs (ss_bam_select_pairs, ss_bam_extract_pairs): step 4 is the mate link of ss_bam_pairs.hip in the place of the template join
// -- a kept record is written iff the hits of its fragment reach min_hits; counters[2] = fragments selected; SS_EIO (and
// pair_counters filled) when a name is not one first and one second mate
int select_on_device(const char *d_stream, uint64_t n, const uint8_t *h_stream, const std::vector<uint64_t> &seg, const ss_db *db,
                     const uint8_t *row_labels, uint32_t n_labels, uint32_t label, uint32_t min_hits, Selection *out, bool pairs = false)
{
    auto t0 = Clock::now();
    // 2. records, kept flags, flat block
    ss::BamRecords recs;
    char *flat = nullptr;
    uint64_t flat_len = 0, flat_cap = 0;
    int rc = ss::bam_records_flat_dev(d_stream, n, h_stream, seg, &flat, &flat_len, &flat_cap, &recs);
    if (rc) return rc;
    const hipStream_t st = ss::l2s::stream();
    const ss::BamFlatOwner owned{recs, flat, flat_cap};
    const uint64_t n_rec = recs.n_rec, kept = recs.kept;
    out->hdr_end = recs.hdr_end;
    out->counters[0] = n_rec;
    out->counters[1] = kept;
    out->ms[0] = ms_since(t0);
    if (!kept) return SS_OK;
    // 3. hits per kept record
    t0 = Clock::now();
    ss_reads R;
    ss::bam_flat_as_set(flat, flat_len, flat_cap, kept, &R);
    ss::RecHits rh;
    uint8_t *d_lab = nullptr;
    if (row_labels) {
        rc = ss::slot_labels_for(db, row_labels, n_labels, label, rh.scratch, &d_lab);
        if (rc) return rc;
    }
    rc = ss::rec_hits_of(db, &R, &rh, nullptr, d_lab, 1);
    if (rc) return rc;
    SS_HIP(ss::l2s::sync());
    if (rh.rec_total != kept) {
        ss::set_last_error("ss_bam_select: the flat block's records are not the kept records", __FILE__, __LINE__, hipErrorUnknown);
        return SS_EHIP;
    }
    out->ms[1] = ms_since(t0);
    // 4. template join; with `pairs` the mate link
    t0 = Clock::now();
    const uint8_t *s = reinterpret_cast<const uint8_t *>(d_stream);
    ss::PoolScratch &scratch = rh.scratch;
    unsigned long long *d_h1 = nullptr, *d_h2 = nullptr, *d_k1 = nullptr, *d_k2 = nullptr, *d_s1 = nullptr, *d_s2 = nullptr;
    unsigned long long *d_len = nullptr, *d_off = nullptr, *d_tot = nullptr;
    uint32_t *d_sel = nullptr, *d_sidx = nullptr;
    void *d_tmp = nullptr;
    const int items = (int)(n_rec + 1);                                 // (n_rec < 0x7FFFFFF0: bam_to_flat_dev)
    const unsigned g1 = grid_for(n_rec + 1);
    SS_HIP(scratch.get((void **)&d_sel, (n_rec + 1) * 4));
    SS_HIP(scratch.get((void **)&d_sidx, (n_rec + 1) * 4));
    SS_HIP(scratch.get((void **)&d_len, (n_rec + 1) * 8));
    SS_HIP(scratch.get((void **)&d_off, (n_rec + 1) * 8));
    SS_HIP(scratch.get((void **)&d_tot, 16));
    SS_HIP(ss::l2s::set(d_tot, 0, 16));
    size_t tb1 = 0, tb2 = 0;
    SS_HIP(hipcub::DeviceScan::ExclusiveSum(nullptr, tb1, d_sel, d_sidx, items, st));
    SS_HIP(hipcub::DeviceScan::ExclusiveSum(nullptr, tb2, d_len, d_off, items, st));
    const size_t tmp_bytes = std::max(tb1, tb2);
    SS_HIP(scratch.get(&d_tmp, tmp_bytes));
    if (pairs) {
        uint32_t *d_mate = nullptr;
        uint8_t *d_role = nullptr;
        rc = ss::bam_mates_dev(s, recs, scratch, &d_mate, &d_role, out->pair_counters, nullptr);
        if (rc) return rc;
        if (out->pair_counters[5]) return SS_EIO;
        rc = ss::bam_fragment_out_len(s, recs, d_mate, rh.d_rec_hits, min_hits, d_len, d_tot);
        if (rc) return rc;
    } else {
        SS_HIP(scratch.get((void **)&d_h1, n_rec * 8));
        SS_HIP(scratch.get((void **)&d_h2, n_rec * 8));
        hipLaunchKernelGGL(name_digest_kernel, dim3(g1), dim3(256), 0, st, s, (const uint64_t *)recs.d_rec, (const uint32_t *)recs.d_keep,
                           (const uint32_t *)recs.d_kidx, (const uint32_t *)rh.d_rec_hits, n_rec, min_hits, d_h1, d_h2, d_sel);
        SS_HIP(hipGetLastError());
        tb1 = tmp_bytes;
        SS_HIP(hipcub::DeviceScan::ExclusiveSum(d_tmp, tb1, d_sel, d_sidx, items, st));
        uint32_t n_sel = 0;
        SS_HIP(ss::l2s::copy(&n_sel, d_sidx + n_rec, 4, hipMemcpyDeviceToHost));
        out->counters[2] = n_sel;
        if (n_sel) {
            SS_HIP(scratch.get((void **)&d_k1, (uint64_t)n_sel * 8));
            SS_HIP(scratch.get((void **)&d_k2, (uint64_t)n_sel * 8));
            SS_HIP(scratch.get((void **)&d_s1, (uint64_t)n_sel * 8));
            SS_HIP(scratch.get((void **)&d_s2, (uint64_t)n_sel * 8));
            hipLaunchKernelGGL(compact_kernel, dim3(g1), dim3(256), 0, st, (const uint32_t *)d_sel, (const uint32_t *)d_sidx,
                               (const unsigned long long *)d_h1, (const unsigned long long *)d_h2, n_rec, d_k1, d_k2);
            SS_HIP(hipGetLastError());
            size_t sb = 0;
            void *d_sort = nullptr;
            SS_HIP(hipcub::DeviceRadixSort::SortPairs(nullptr, sb, d_k1, d_s1, d_k2, d_s2, (int)n_sel, 0, 64, st));
            SS_HIP(scratch.get(&d_sort, sb));
            SS_HIP(hipcub::DeviceRadixSort::SortPairs(d_sort, sb, d_k1, d_s1, d_k2, d_s2, (int)n_sel, 0, 64, st));
        }
        hipLaunchKernelGGL(template_len_kernel, dim3(g1), dim3(256), 0, st, s, (const uint64_t *)recs.d_rec, (const uint32_t *)recs.d_keep,
                           (const uint32_t *)d_sel, (const unsigned long long *)d_h1, (const unsigned long long *)d_h2, n_rec,
                           (const unsigned long long *)d_s1, (const unsigned long long *)d_s2, n_sel, d_len, d_tot);
        SS_HIP(hipGetLastError());
    }
    // 5. offsets and copy
    tb2 = tmp_bytes;
    SS_HIP(hipcub::DeviceScan::ExclusiveSum(d_tmp, tb2, d_len, d_off, items, st));
    unsigned long long total = 0, tot[2] = {0, 0};
    SS_HIP(hipMemcpyAsync(&total, d_off + n_rec, 8, hipMemcpyDeviceToHost, st));
    SS_HIP(ss::l2s::copy(tot, d_tot, 16, hipMemcpyDeviceToHost));
    out->counters[3] = tot[0];
    if (pairs) out->counters[2] = tot[1];
    out->total = total;
    out->ms[2] = ms_since(t0);
    if (!total) return SS_OK;
    t0 = Clock::now();
    if (n < 16 || total > n) return SS_EHIP;                            // (a record is 36 bytes and more; the records are the stream's)
    if (ss::big_malloc((void **)&out->d_out, ss_reads::padded(total), &out->out_cap) != hipSuccess) { out->d_out = nullptr; return SS_ENOMEM; }
    hipLaunchKernelGGL(record_gather_kernel, dim3(grid_for(n_rec * 16u)), dim3(256), 0, st, s, n, (const uint64_t *)recs.d_rec,
                       (const unsigned long long *)d_len, (const unsigned long long *)d_off, n_rec, (uint8_t *)out->d_out);
    SS_HIP(hipGetLastError());
    SS_HIP(ss::l2s::sync());
    out->ms[3] = ms_since(t0);
    return SS_OK;
}

int check_args(const ss_db *db, const uint8_t *row_labels, uint32_t n_labels, uint32_t label, uint32_t min_hits)
{
    if (!db || min_hits == 0) return SS_EINVAL;
    if (row_labels && (n_labels < 1 || n_labels > SS_LABELS_MAX || label < 1 || label > n_labels)) return SS_EINVAL;
    if (db->layout != 1) return SS_ERANGE;                          // page-index tables only
    return SS_OK;
}

}  // namespace

extern "C" {

int ss_bam_extract_calls(uint64_t *n)
{
    if (!n) return SS_EINVAL;
    *n = g_bam_extract_calls.load();
    return SS_OK;
}

int ss_bam_extract_timing(double out[8]) { return g_timing.load(out); }

static int select_stream(const void *stream, uint64_t n, const ss_db *db, const uint8_t *row_labels, uint32_t n_labels, uint32_t label,
                         uint32_t min_hits, void *out, uint64_t cap, uint64_t *out_len, uint64_t counters[4], bool pairs)
{
    if ((!stream && n) || !out_len || !counters || (!out && cap)) return SS_EINVAL;
    int rc = check_args(db, row_labels, n_labels, label, min_hits);
    if (rc) return rc;
    g_bam_extract_calls++;
    ss::BamDeviceStream ds;
    rc = ds.upload(stream, n);
    if (rc) return rc;
    Selection sel;
    rc = select_on_device(ds.d, n, ds.h, ds.seg, db, row_labels, n_labels, label, min_hits, &sel, pairs);
    if (rc) return rc;
    memcpy(counters, sel.counters, sizeof sel.counters);
    *out_len = sel.total;
    if (sel.total > cap) return SS_ERANGE;
    return ss::bam_download_chunks(sel.d_out, sel.total, (char *)out);
}

static int extract_file(const char *in_path, const ss_db *db, const uint8_t *row_labels, uint32_t n_labels, uint32_t label,
                        uint32_t min_hits, const char *out_path, uint64_t counters[4], bool pairs)
{
    if (!in_path || !out_path || !counters) return SS_EINVAL;
    int rc = check_args(db, row_labels, n_labels, label, min_hits);
    if (rc) return rc;
    ss::BamFileCall call;
    rc = call.open(in_path, g_bam_extract_calls);                       // 1. the stream on the device
    if (rc) return rc;
    ss::BamDeviceStream &ds = call.ds;
    Selection sel;
    rc = select_on_device(ds.d, ds.n, ds.h, ds.seg, db, row_labels, n_labels, label, min_hits, &sel, pairs);
    if (rc) return rc;
    // 6. header and records to the host, then the file
    rc = ss::bam_write_file(ds, sel.hdr_end, sel.d_out, sel.total, out_path, &call.ms[5], &call.ms[6]);
    if (rc) return rc;
    memcpy(counters, sel.counters, sizeof sel.counters);
    for (int i = 0; i < 4; i++) call.ms[1 + i] = sel.ms[i];
    call.finish(g_timing);
    return SS_OK;
}

int ss_bam_select(const void *stream, uint64_t n, const ss_db *db, const uint8_t *row_labels, uint32_t n_labels, uint32_t label,
                  uint32_t min_hits, void *out, uint64_t cap, uint64_t *out_len, uint64_t counters[4])
{
    return select_stream(stream, n, db, row_labels, n_labels, label, min_hits, out, cap, out_len, counters, false);
}

int ss_bam_select_pairs(const void *stream, uint64_t n, const ss_db *db, const uint8_t *row_labels, uint32_t n_labels, uint32_t label,
                        uint32_t min_hits, void *out, uint64_t cap, uint64_t *out_len, uint64_t counters[4])
{
    return select_stream(stream, n, db, row_labels, n_labels, label, min_hits, out, cap, out_len, counters, true);
}

int ss_bam_extract(const char *in_path, const ss_db *db, const uint8_t *row_labels, uint32_t n_labels, uint32_t label,
                   uint32_t min_hits, const char *out_path, uint64_t counters[4])
{
    return extract_file(in_path, db, row_labels, n_labels, label, min_hits, out_path, counters, false);
}

int ss_bam_extract_pairs(const char *in_path, const ss_db *db, const uint8_t *row_labels, uint32_t n_labels, uint32_t label,
                         uint32_t min_hits, const char *out_path, uint64_t counters[4])
{
    return extract_file(in_path, db, row_labels, n_labels, label, min_hits, out_path, counters, true);
}

}  // extern "C"
