// ss_reads_select: the records of a resident read set with at least min_hits hits against a table, as a new resident set
// (`--extract_reads`).
//
// ss_reads_support reduces rec_hits[] to a histogram and throws it away; this keeps it and acts on it.  A record and a hit mean
// what they mean there, so the selection depends on a record's bytes only: the same records are chosen from a set in file
// order, binned or packed, and the caller finds them in the input files again BY CONTENT (ss_extract.hip) -- nothing here knows
// where a record stood in a file.
//
// Four passes, each a plain launch; the scratch comes from the stream-ordered pool and goes back before the call returns:
//   1. rec_hits_of (ss_support.hip): the record base of every tile and rec_hits[], exactly as ss_reads_support makes them.
//      Passes 2-4 are select_records, which works on whichever slice of rec_hits[] it is given: ss_reads_select_labeled
//      (ss_label.hip) hands it the hits of one label.
//   2. record_spans_kernel (ASCII slabs): start[rec] and end[rec].  A lane takes 16 bytes; a record START is a byte other than
//      '\n' behind a '\n' (or at the slab's first byte), a record END a '\n' behind a byte that is none (and the slab's end behind
//      such a byte).  Starts and ends alternate, so the record a start belongs to is the number of ends before it: the tile's
//      base + the ends of the lanes before (a wave prefix sum of popcounts) + the ends below it in the lane.  A record that spans
//      tiles gets its start from the tile where it begins and its end from the tile where it ends; empty lines between records
//      belong to no record.  A packed slab needs no kernel: start = rec * slot, length = L.
//   3. select_len_kernel: out_len[rec] = hits >= min_hits ? length + 1 : 0, the selected records counted on the way; hipcub's
//      64-bit ExclusiveSum turns the lengths into byte offsets in the new slab, which is allocated once (ss::big_malloc).
//   4. gather_kernel: sixteen lanes per selected record copy its bytes and a '\n' to its offset, in 16-byte aligned pieces of
//      the destination (the piece copy, ss_piece_copy.h).  From a packed slab a piece is three 3-byte units turned back into
//      letters ("ACTG"[code], 'N' where invalid: what ss_reads_read_back writes).
// select_records is three steps (ss_support.h): record_spans_of (pass 2 and the scratch of pass 3), the length pass, and
// gather_records (the prefix sum, the new slab, pass 4).  out_len[rec] may be any multiple of length + 1: the gather writes that
// many copies of the record back to back.  ss_reads_resample (ss_resample.hip) is the same three steps with its own length pass,
// a Poisson multiplicity in the place of the 0/1 choice.
#include "ss_piece_copy.h"
#include "ss_support.h"

#include <hipcub/hipcub.hpp>

using namespace ss::dev;
using ss::SUP_TILE;

namespace {

// one wave per tile, 16 bytes per lane (the shape of record_ends_kernel, ss_support.hip); records at or beyond rec_limit are
// never written
template <bool ALIGNED>
__global__ __launch_bounds__(256) void record_spans_kernel(const uint8_t *__restrict__ bases, uint64_t n, uint64_t n_tiles,
                                                           const uint32_t *__restrict__ tile_base, uint64_t rec_base, uint64_t rec_limit,
                                                           unsigned long long *__restrict__ start, unsigned long long *__restrict__ end)
{
    const uint64_t tile = (uint64_t)blockIdx.x * 4u + (threadIdx.x >> 6);
    if (tile >= n_tiles) return;                                        // (the same for the whole wave)
    const uint64_t off = tile * (uint64_t)SUP_TILE + (uint64_t)(threadIdx.x & 63u) * 16u;
    uint32_t ends = 0, starts = 0, last = 0;
    if (off < n) {
        uint32_t w[4];
        load16<ALIGNED>(bases, off, n, w);
        const uint32_t nl = newline_mask16(w);
        const uint32_t prev = (off == 0 || bases[off - 1] == 0x0Au) ? 1u : 0u;
        const uint32_t behind_nl = (nl << 1) | prev;                    // bit i: the byte before byte i is '\n'
        ends = nl & ~behind_nl & 0xFFFFu;
        starts = ~nl & behind_nl & 0xFFFFu;
        if (n - off < 16u) {                                            // positions below n only
            const uint32_t m = (1u << (uint32_t)(n - off)) - 1u;
            ends &= m;
            starts &= m;
        }
        if (n - off <= 16u) last = ((nl >> (uint32_t)(n - 1u - off)) & 1u) ^ 1u;      // the slab ends inside a record
    }
    const uint32_t mine = (uint32_t)__popc(ends) + last;
    uint64_t r = rec_base + tile_base[tile] + wave_inclusive_sum(mine) - mine;
    for (uint32_t ev = starts | ends; ev; ev &= ev - 1u) {
        const uint32_t b = (uint32_t)__ffs(ev) - 1u;
        if ((starts >> b) & 1u) {
            if (r < rec_limit) start[r] = off + b;
        } else {
            if (r < rec_limit) end[r] = off + b;
            r++;
        }
    }
    if (last && r < rec_limit) end[r] = n;
}

// records [rec0, rec0 + n_rec) of one slab: out_len = the bytes a record takes in the new slab (its length + '\n', 0 when it is
// not selected); tot[0] += selected records, tot[1] += their bytes.  fixed_len != 0: a packed slab, every record that long in a
// slot of `slot` positions.  A span that does not lie inside the slab (record_span) selects nothing, so that the gather never reads
// outside the slab.
__global__ __launch_bounds__(256) void select_len_kernel(const uint32_t *__restrict__ rec_hits, const unsigned long long *__restrict__ start,
                                                         const unsigned long long *__restrict__ end, uint64_t rec0, uint64_t n_rec, uint64_t n,
                                                         uint32_t slot, uint32_t fixed_len, uint32_t min_hits, unsigned long long *__restrict__ out_len,
                                                         unsigned long long *__restrict__ tot)
{
    unsigned long long cnt = 0, bytes = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x; i < n_rec; i += (uint64_t)gridDim.x * 256u) {
        unsigned long long len = 0;
        if (rec_hits[rec0 + i] >= min_hits) {
            const RecordSpan sp = record_span(fixed_len != 0u, i, rec0, start, end, slot, fixed_len, n);
            if (sp.ok) { len = sp.len + 1ull; cnt++; bytes += len; }
        }
        out_len[rec0 + i] = len;
    }
    add_selected(cnt, bytes, tot);
}

// Sixteen lanes per record of one slab of n >= 16 positions (records [rec0, rec0 + n_rec)) copy it and a '\n' behind it to dst,
// 16-byte aligned, by the piece copy of ss_piece_copy.h.  PACKED: src is a packed slab, record r - rec0 at position
// (r - rec0) * slot, and a piece is its letters (fetch16_packed); else src is an ASCII slab and start[] says where.
// out_len[r] is a multiple of the record's length + 1: that many copies of it stand back to back from out_off[r] on (one for
// ss_reads_select, 0..13 for ss_reads_resample), and the sixteen lanes write one after the other.
template <bool PACKED>
__global__ __launch_bounds__(256) void gather_kernel(const uint8_t *__restrict__ src, uint64_t n, const unsigned long long *__restrict__ start,
                                                     const unsigned long long *__restrict__ end, const unsigned long long *__restrict__ out_len,
                                                     const unsigned long long *__restrict__ out_off, uint64_t rec0, uint64_t n_rec, uint32_t slot,
                                                     uint32_t fixed_len, uint8_t *__restrict__ dst)
{
    const uint64_t g = ((uint64_t)blockIdx.x * 256u + threadIdx.x) >> 4;
    if (g >= n_rec) return;
    const uint64_t r = rec0 + g;
    const uint64_t all = out_len[r];
    if (!all) return;                                                   // not selected
    const uint64_t S = PACKED ? g * (uint64_t)slot : (uint64_t)start[r];
    const uint64_t len = PACKED ? (uint64_t)fixed_len : (uint64_t)end[r] - S, ol = len + 1u, D_end = out_off[r] + all;
    for (uint64_t D = out_off[r]; D + ol <= D_end; D += ol)
        write_span(dst, D, D + ol, threadIdx.x & 15u, [&](uint64_t a, uint64_t, uint64_t) {
            const int64_t base = (int64_t)S + ((int64_t)a - (int64_t)D);    // source position of the piece's byte 0
            const piece_t x = PACKED ? fetch16_packed(src, n, base) : fetch16(src, n, base);
            return D + len < a + 16u ? with_byte(x, (uint32_t)(D + len - a), '\n') : x;      // the byte behind the record
        });
}

std::atomic<uint64_t> g_select_calls{0};

}  // namespace

extern "C" {

int ss_reads_select_calls(uint64_t *n)
{
    if (!n) return SS_EINVAL;
    *n = g_select_calls.load();
    return SS_OK;
}

int ss_reads_select(const ss_db *db, const ss_reads *R, uint32_t min_hits, ss_reads **out)
{
    if (!db || !R || !out || min_hits == 0) return SS_EINVAL;
    if (db->layout != 1) return SS_ERANGE;                          // page-index tables only
    if (R->has_cut_record) return SS_ERANGE;                        // at any k: a cut piece is not a read
    ss::RecHits rh;
    // 1. hits per record
    const int rc = ss::rec_hits_of(db, R, &rh, &g_select_calls);
    if (rc) return rc;
    return ss::select_records(&rh, rh.d_rec_hits, min_hits, out);
}

}  // extern "C"

int ss::select_records(RecHits *rhp, const uint32_t *d_rec_hits, uint32_t min_hits, ss_reads **out)
{
    RecHits &rh = *rhp;
    RecSpans sp;
    // 2. record spans
    const int rc = ss::record_spans_of(&rh, &sp);
    if (rc) return rc;
    // 3. select: bytes per record
    for (const auto &pt : rh.parts) {
        if (!pt.n_rec) continue;
        const unsigned blocks = (unsigned)std::min<uint64_t>((pt.n_rec + 256 * 4 - 1) / (256 * 4), 4096);
        hipLaunchKernelGGL(select_len_kernel, dim3(blocks), dim3(256), 0, ss::l2s::stream(), d_rec_hits, sp.d_start, sp.d_end, pt.rec_base, pt.n_rec,
                           pt.n, pt.sl->packed ? pt.sl->slot : 0u, pt.sl->packed ? pt.sl->L : 0u, min_hits, sp.d_len, sp.d_tot);
        SS_HIP(hipGetLastError());
    }
    return ss::gather_records(&rh, sp, "ss_reads_select", out);
}

int ss::record_spans_of(RecHits *rhp, RecSpans *sp)
{
    RecHits &rh = *rhp;
    if (rh.rec_total > 0x7FFFFFFFull) return SS_ERANGE;             // hipcub counts its items in an int
    const hipStream_t st = ss::l2s::stream();
    const uint64_t rec_total = rh.rec_total;
    if (!rec_total) return SS_OK;
    bool any_ascii = false;
    for (const auto &pt : rh.parts) any_ascii = any_ascii || (!pt.sl->packed && pt.n_rec);
    if (any_ascii) {
        SS_HIP(rh.scratch.get((void **)&sp->d_start, rec_total * 8));
        SS_HIP(rh.scratch.get((void **)&sp->d_end, rec_total * 8));
        SS_HIP(ss::l2s::set(sp->d_start, 0xFF, rec_total * 8));
        SS_HIP(ss::l2s::set(sp->d_end, 0xFF, rec_total * 8));
    }
    for (const auto &pt : rh.parts) {
        if (pt.sl->packed || !pt.n_rec) continue;
        const uint8_t *b = (const uint8_t *)pt.sl->d;
        const dim3 grid((unsigned)((pt.n_tiles + 3) / 4));
        with_bool((((uintptr_t)b) & 15) == 0, [&](auto aligned) {
            hipLaunchKernelGGL(record_spans_kernel<decltype(aligned)::value>, grid, dim3(256), 0, st, b, pt.n, pt.n_tiles,
                               rh.d_tile_base + pt.tile_off, pt.rec_base, pt.rec_base + pt.n_rec, sp->d_start, sp->d_end);
        });
        SS_HIP(hipGetLastError());
    }
    SS_HIP(rh.scratch.get((void **)&sp->d_len, rec_total * 8));
    SS_HIP(rh.scratch.get((void **)&sp->d_tot, 16));
    SS_HIP(ss::l2s::set(sp->d_tot, 0, 16));
    return SS_OK;
}

int ss::gather_records(RecHits *rhp, RecSpans &sp, const char *who, ss_reads **out)
{
    RecHits &rh = *rhp;
    const hipStream_t st = ss::l2s::stream();
    const uint64_t rec_total = rh.rec_total;
    unsigned long long tot[2] = {0, 0};
    if (rec_total) {
        // the exclusive sum of the bytes per record: where each record's copies begin in the new slab
        if (!sp.d_off) {
            SS_HIP(rh.scratch.get((void **)&sp.d_off, rec_total * 8));
            SS_HIP(hipcub::DeviceScan::ExclusiveSum(nullptr, sp.tmp_bytes, sp.d_len, sp.d_off, (int)rec_total, st));
            SS_HIP(rh.scratch.get(&sp.d_tmp, sp.tmp_bytes));
        }
        size_t tmp_bytes = sp.tmp_bytes;
        SS_HIP(hipcub::DeviceScan::ExclusiveSum(sp.d_tmp, tmp_bytes, sp.d_len, sp.d_off, (int)rec_total, st));
        SS_HIP(ss::l2s::copy(tot, sp.d_tot, 16, hipMemcpyDeviceToHost));
    }
    unsigned long long *const d_off = sp.d_off;
    // the new slab, allocated once from the total
    ss_reads *S = nullptr;
    uint8_t *slab = nullptr;
    const int rc = ss::one_slab_set(tot[0], tot[1], who, &S, &slab);
    if (rc) return rc;
    if (slab) {
        // 4. gather
        const ss::HipFail fail{who};
        bool bad = false;
        for (const auto &pt : rh.parts) {
            if (bad || !pt.n_rec) continue;
            if (pt.n < 16) { bad = fail(hipErrorInvalidValue); continue; }      // (a slab is padded to a multiple of 16)
            const dim3 grid((unsigned)((pt.n_rec * 16u + 255u) / 256u));
            with_bool(pt.sl->packed, [&](auto packed) {
                hipLaunchKernelGGL(gather_kernel<decltype(packed)::value>, grid, dim3(256), 0, st, (const uint8_t *)pt.sl->d, pt.n, sp.d_start, sp.d_end,
                                   sp.d_len, d_off, pt.rec_base, pt.n_rec, pt.sl->slot, pt.sl->packed ? pt.sl->L : 0u, slab);
            });
            bad = fail(hipGetLastError());
        }
        bad = fail(ss::l2s::sync()) || bad;
        if (bad) { ss_reads_destroy(S); return SS_EHIP; }
    }
    *out = S;
    return SS_OK;
}

int ss::one_slab_set(uint64_t n_records, uint64_t total, const char *who, ss_reads **out, uint8_t **slab)
{
    *out = nullptr;
    *slab = nullptr;
    ss_reads *S = new (std::nothrow) ss_reads();
    if (!S) return SS_ENOMEM;
    S->n_records = n_records;
    S->n_bases = total - n_records;
    if (total) {
        ss_reads::Slab sl;
        sl.used = ss_reads::padded(total);
        if (ss::big_malloc((void **)&sl.d, sl.used, &sl.cap) != hipSuccess) { delete S; return SS_ENOMEM; }
        S->slabs.push_back(sl);
        S->device_bytes = sl.cap;
        S->n_blocks = 1;
        S->first_slab = sl.cap;
        if (HipFail{who}(ss::l2s::set(sl.d + total, '\n', sl.used - total))) { ss_reads_destroy(S); return SS_EHIP; }
        *slab = (uint8_t *)sl.d;
    }
    *out = S;
    return SS_OK;
}
