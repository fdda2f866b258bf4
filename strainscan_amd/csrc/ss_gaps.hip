// ss_reads_gaps: the runs of missing k-mers inside the records of a resident set, against the k-mers of the called strains
// (`--divergence`).  strainscan_hip.h has the rule, tests/gap_model.py restates it.  Nothing here depends on the order of the records.
//
// The passes, each a plain launch; all scratch comes from the stream-ordered pool and goes back before the call returns:
//   1. slot_called_kernel: one thread per row, atomicOr of 2 (a called row) or 1 (any other) into its slot; slot_called_finish_kernel:
//      one thread per slot, 2 where a called row was seen, else 1 where any row was, else 0 -- the UNION of the rows, not the
//      agree-or-zero rule of the label and mask folds.  kmers and kmers_called are counted on the way, a ballot each.
//   2. per slab: scan_minik_kernel<.., ClassSink> (ss_minik.hip), unchanged, with these slot values in the place of the slot nodes:
//      pos[p] = 2 (C), 1 (T) or 0 (no k-mer of the table starts at p: a miss, or no window at all), 16 bits per position.  No slot
//      of the table has the value 0, so the sink's count of hits without a node stays 0.  Record spans are those of
//      ss_reads_select (record_spans_of).
//   3. gap_walk_kernel<IN, false>: one lane per record walks its fields, eight per aligned 16-byte load.  A field that is not 0
//      says that the window is valid; a field of 0 does not tell a miss from a window that an N cuts, so the lane looks at the
//      slab's own invalid flags (load_in / decode_in, sixteen per load, the word kept until the walk leaves it).  It has to look at
//      ONE base per miss: the lane keeps `scanned`, the end of the bases that are known to be valid from the window's start on,
//      and a window behind a valid one adds its last base only.  An invalid base at b makes the windows up to b invalid at once
//      (`skip`).  The state machine: the previous window (I, C, inside a run that began behind a C, inside one that did not), the
//      open run's length and whether it is all T, the stretch's first and last C.  Eight fields that are all C behind a C are
//      one step.  A wave's sums are taken with shuffles, added to the workgroup's in LDS, and the workgroup issues one set of
//      64-bit atomics when it ends: no device-wide barrier, no per-record global atomics.  A record above GAP_LONG positions is
//      put on a list, so that one long record does not hold up the 63 others of its wave.
//   4. gap_walk_kernel<IN, true>: the listed records, one lane each, through the same walk (its counters are 32 bits: a record is
//      shorter than a block).  A sample of long reads is listed whole and walked at the rate of pass 3; a single long record among
//      short ones costs one lane's serial walk of it.
#include "ss_scan_dev.h"
#include "ss_support.h"

using namespace ss::dev;

namespace {

constexpr uint32_t GAP_LONG = 4095;         // positions a record may have in pass 3
constexpr uint32_t GAP_SUMS = 16;           // what a wave adds up: out[0..14], and the listed records (out[17])
constexpr uint32_t GAP_LONG_WGS = 256;      // workgroups of pass 4
static_assert(SS_GAPS_OUT == 18, "out[]: fifteen sums of the walk, kmers, kmers_called, the listed records");

// the records of one slab and where their results go
struct GapArgs {
    const uint16_t *pos;                        // the slab's fields
    const uint8_t *bases;                       // the slab itself, for its invalid flags
    const unsigned long long *start, *end;      // ASCII slab: spans by record of the set; packed: unused
    uint64_t rec0, n_rec, n;                    // the slab's first record, its records, its positions
    uint32_t slot, fixed_len;                   // packed slab: positions per slot, bases per record; else 0
    uint32_t k, min_hits;
    unsigned long long *out;                    // [SS_GAPS_OUT]
    unsigned long long *n_long;                 // records of this slab on the list
    uint32_t *long_list;                        // [n_rec] records of this slab (slab-relative) left to pass 4
    uint4 *rec_out;                             // [records of the set] or nullptr
};

__global__ __launch_bounds__(256) void slot_called_kernel(const uint8_t *__restrict__ row_called, const uint32_t *__restrict__ slot_of_row,
                                                          uint64_t n_rows, uint64_t n_slots, uint32_t *__restrict__ any)
{
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= n_rows) return;
    const uint32_t sl = slot_of_row[i];
    if (sl == SS_NO_SLOT || sl >= n_slots) return;
    atomicOr(&any[sl], !row_called || row_called[i] ? 2u : 1u);
}

// out[slot] = 2 (a called row), 1 (rows, none of them called) or 0 (no row); n_with[0] += occupied slots, n_with[1] += called ones
__global__ __launch_bounds__(256) void slot_called_finish_kernel(const uint32_t *__restrict__ any, uint64_t n_slots, uint16_t *__restrict__ out,
                                                                 unsigned long long *__restrict__ n_with)
{
    unsigned long long occ = 0, called = 0;     // (lane 0 keeps the wave's)
    for (uint64_t s0 = (uint64_t)blockIdx.x * 256u; s0 < n_slots; s0 += (uint64_t)gridDim.x * 256u) {
        const uint64_t s = s0 + threadIdx.x;
        uint32_t v = 0;
        if (s < n_slots) {
            const uint32_t a = any[s];
            v = (a & 2u) ? 2u : (a & 1u);
            out[s] = (uint16_t)v;
        }
        occ += (unsigned long long)__popcll(__ballot(v != 0u));
        called += (unsigned long long)__popcll(__ballot(v == 2u));
    }
    if ((threadIdx.x & 63u) == 0u) {
        if (occ) atomicAdd(&n_with[0], occ);
        if (called) atomicAdd(&n_with[1], called);
    }
}

// what the walk of one record leaves
struct GapRec { uint32_t hc, ht, mx, gap[5], incl, sites, det; };

enum { ST_I = 0, ST_C = 1, ST_RUN = 2, ST_OPEN = 3 };      // the previous window: invalid or none, C, in a run behind a C, in a run behind no C

// the invalid flags of positions [16 blk, 16 blk + 16) of the slab, a bit each (positions at or beyond n are invalid)
template <int IN>
__device__ __forceinline__ uint32_t invalid16(const uint8_t *__restrict__ bases, uint64_t blk, uint64_t n)
{
    uint32_t w[4], code, inv;
    load_in<IN>(bases, blk * 16u, n, w);
    decode_in<IN>(w, code, inv);
    return inv & 0xFFFFu;
}

// The record at positions [s, s + len) of the slab (s + len <= n).  pos holds a whole number of tiles, so the aligned 16-byte
// loads around the record's windows stay inside it.
template <int IN>
__device__ __forceinline__ void walk_record(const uint16_t *__restrict__ pos, const uint8_t *__restrict__ bases, uint64_t n, uint64_t s, uint64_t len,
                                            uint32_t k, GapRec &R)
{
    if (len < k) return;
    const uint64_t e = s + (len - k + 1u);      // the record's windows start in [s, e)
    uint32_t state = ST_I, run = 0, first = 0, last = 0;
    bool all_t = false, has_c = false;
    uint64_t skip = s;                          // windows before it are done (an invalid base makes a row of them invalid at once)
    uint64_t scanned = s;                       // no invalid base in [the window at hand, scanned)
    uint64_t flag_blk = ~0ull;
    uint32_t flags = 0;
    auto close_stretch = [&]() {
        if (has_c && last - first > k) R.det += last - first - k;
        has_c = false;
    };
    for (uint64_t c = s & ~7ull; c < e; c += 8u) {
        if (c + 8u <= skip) continue;
        const uint4 q = *reinterpret_cast<const uint4 *>(pos + c);
        if (state == ST_C && c + 8u <= e && q.x == 0x00020002u && q.y == 0x00020002u && q.z == 0x00020002u && q.w == 0x00020002u) {
            R.hc += 8u;                         // (behind a C: c > s, and skip <= c)
            last = (uint32_t)(c + 7u - s);
            scanned = c + 7u + k;
            continue;
        }
        const uint64_t lo = (uint64_t)q.x | ((uint64_t)q.y << 32), hi = (uint64_t)q.z | ((uint64_t)q.w << 32);
        for (uint32_t i = 0; i < 8u; i++) {
            const uint64_t a = c + i;
            if (a < skip || a >= e) continue;
            const uint32_t v = (uint32_t)(((i & 4u) ? hi : lo) >> (16u * (i & 3u))) & 0xFFFFu;
            const uint32_t p = (uint32_t)(a - s);
            if (v == 2u) {
                if (state == ST_RUN) {
                    R.gap[run < k - 1u ? 0 : run == k - 1u ? 1 : run == k ? 2 : run < 2u * k ? 3 : 4]++;
                    if (all_t) R.incl++;
                    else if (run >= k - 1u && run < 2u * k) R.sites++;
                }
                state = ST_C;
                R.hc++;
                if (!has_c) { first = p; has_c = true; }
                last = p;
                scanned = a + k;
                continue;
            }
            if (v == 0u) {
                // a miss, or not a window: the first invalid base of [scanned, a + k)
                if (scanned < a) scanned = a;
                uint64_t bad = ~0ull;
                for (uint64_t b = scanned; b < a + k;) {
                    const uint64_t blk = b >> 4;
                    if (blk != flag_blk) { flags = invalid16<IN>(bases, blk, n); flag_blk = blk; }
                    const uint64_t upto = a + k - blk * 16u;      // >= 1
                    const uint32_t m = flags & (0xFFFFu << (uint32_t)(b & 15u)) & (upto < 16u ? (1u << (uint32_t)upto) - 1u : 0xFFFFu);
                    if (m) { bad = blk * 16u + (uint32_t)__ffs((int)m) - 1u; break; }
                    b = blk * 16u + 16u;
                }
                if (bad != ~0ull) {             // the windows a .. bad are invalid
                    close_stretch();
                    state = ST_I;
                    skip = scanned = bad + 1u;
                    continue;
                }
            }
            scanned = a + k;
            if (v) R.ht++; else R.mx++;
            if (state == ST_C) { state = ST_RUN; run = 1u; all_t = v != 0u; }
            else if (state == ST_RUN) { run++; all_t = all_t && v != 0u; }
            else state = ST_OPEN;
        }
    }
    close_stretch();
}

// pass 3 (LISTED == false: every record of the slab, the long ones to the list) and pass 4 (LISTED == true: the listed ones)
template <int IN, bool LISTED>
__global__ __launch_bounds__(256) void gap_walk_kernel(const GapArgs A)
{
    __shared__ unsigned long long acc[GAP_SUMS];
    const uint32_t t = threadIdx.x, lane = t & 63u;
    if (t < GAP_SUMS) acc[t] = 0ull;
    __syncthreads();
    const uint64_t n_items = LISTED ? (uint64_t)*A.n_long : A.n_rec;
    for (uint64_t g0 = (uint64_t)blockIdx.x * 256u; g0 < n_items; g0 += (uint64_t)gridDim.x * 256u) {      // (the same for the workgroup)
        const uint64_t it = g0 + t;
        GapRec R{};
        bool valid = false, listed = false;
        uint64_t g = 0;
        if (it < n_items) {
            g = LISTED ? (uint64_t)A.long_list[it] : it;
            const RecordSpan sp = record_span(A.slot != 0u, g, A.rec0, A.start, A.end, A.slot, A.fixed_len, A.n);
            if (sp.ok && !LISTED && sp.len > GAP_LONG) {
                A.long_list[atomicAdd(A.n_long, 1ull)] = (uint32_t)g;
                listed = true;
            } else if (sp.ok) {
                valid = true;
                walk_record<IN>(A.pos, A.bases, A.n, sp.s, sp.len, A.k, R);
            }
        }
        const uint32_t gaps = R.gap[0] + R.gap[1] + R.gap[2] + R.gap[3] + R.gap[4];
        if (valid && A.rec_out) A.rec_out[A.rec0 + g] = make_uint4(R.hc, gaps, R.sites, R.det);
        const bool assessed = valid && R.hc >= A.min_hits;
        if (!assessed) R = GapRec{};
        unsigned long long v[GAP_SUMS] = {valid ? 1ull : 0ull, assessed ? 1ull : 0ull, (unsigned long long)R.hc + R.ht + R.mx, R.hc, R.ht, R.mx,
                                          R.gap[0], R.gap[1], R.gap[2], R.gap[3], R.gap[4], R.incl, R.sites, R.sites ? 1ull : 0ull, R.det,
                                          listed ? 1ull : 0ull};
#pragma unroll
        for (uint32_t j = 0; j < GAP_SUMS; j++) {
#pragma unroll
            for (int d = 32; d > 0; d >>= 1) v[j] += __shfl_xor(v[j], d, 64);
            if (lane == 0u && v[j]) atomicAdd(&acc[j], v[j]);
        }
    }
    __syncthreads();
    if (t < GAP_SUMS && acc[t]) atomicAdd(&A.out[t < 15u ? t : 17u], acc[t]);
}

std::atomic<uint64_t> g_gaps_calls{0};

}  // namespace

extern "C" {

int ss_reads_gaps_calls(uint64_t *n)
{
    if (!n) return SS_EINVAL;
    *n = g_gaps_calls.load();
    return SS_OK;
}

int ss_reads_gaps(const ss_db *db, const ss_reads *R, const uint8_t *row_called, uint32_t min_hits, uint64_t out[SS_GAPS_OUT], uint32_t *rec_out)
{
    if (!db || !R || !out || min_hits == 0) return SS_EINVAL;
    if (db->layout != 1) return SS_ERANGE;                          // page-index tables only
    if (R->has_cut_record) return SS_ERANGE;                        // at any k: a cut piece is not a read
    const uint64_t n_rows = db->n_rows, n_slots = db->n_slots;

    ss::RecHits rh;
    ss::RecSpans sp;
    int rc = ss::record_index_of(R, db->device, &rh, &g_gaps_calls);
    if (rc) return rc;
    rc = ss::record_spans_of(&rh, &sp);
    if (rc) return rc;
    const hipStream_t st = ss::l2s::stream();
    ss::PoolScratch &scratch = rh.scratch;
    const uint64_t rec_total = rh.rec_total;

    unsigned long long *d_out = nullptr;        // out[SS_GAPS_OUT], the slab's listed records, the sink's hits without a node
    SS_HIP(scratch.get((void **)&d_out, (SS_GAPS_OUT + 2) * 8));
    SS_HIP(ss::l2s::set(d_out, 0, (SS_GAPS_OUT + 2) * 8));
    unsigned long long *d_long = d_out + SS_GAPS_OUT, *d_hits0 = d_out + SS_GAPS_OUT + 1;

    // 1. C / T per slot
    uint8_t *d_rows = nullptr;
    uint32_t *d_any = nullptr;
    uint16_t *d_slot_val = nullptr;
    SS_HIP(scratch.get((void **)&d_any, n_slots * 4));
    SS_HIP(scratch.get((void **)&d_slot_val, n_slots * 2));
    SS_HIP(ss::l2s::set(d_any, 0, std::max<uint64_t>(n_slots * 4, 16)));
    if (n_rows) {
        if (row_called) {
            SS_HIP(scratch.get((void **)&d_rows, n_rows));
            SS_HIP(ss::l2s::copy(d_rows, row_called, n_rows, hipMemcpyHostToDevice));
        }
        hipLaunchKernelGGL(slot_called_kernel, dim3(ss::grid_for(n_rows)), dim3(256), 0, st, d_rows, db->d_slot_of_row, n_rows, n_slots, d_any);
        SS_HIP(hipGetLastError());
    }
    if (n_slots) {
        const unsigned blocks = (unsigned)std::min<uint64_t>((n_slots + 256 * 8 - 1) / (256 * 8), 4096);
        hipLaunchKernelGGL(slot_called_finish_kernel, dim3(blocks), dim3(256), 0, st, d_any, n_slots, d_slot_val, d_out + 15);
        SS_HIP(hipGetLastError());
    }

    // 2.-4. slab by slab
    uint64_t max_fields = 0, max_rec = 0;
    for (const auto &pt : rh.parts)
        if (pt.n_rec) { max_fields = std::max(max_fields, pt.n_tiles * (uint64_t)ss::SUP_TILE); max_rec = std::max(max_rec, pt.n_rec); }
    uint16_t *d_pos = nullptr;
    uint32_t *d_list = nullptr, *d_rec = nullptr;
    if (max_fields) {
        SS_HIP(scratch.get((void **)&d_pos, max_fields * 2));
        SS_HIP(scratch.get((void **)&d_list, max_rec * 4));
    }
    if (rec_out && rec_total) {
        SS_HIP(scratch.get((void **)&d_rec, rec_total * 16));
        SS_HIP(ss::l2s::set(d_rec, 0, rec_total * 16));
    }
    for (const auto &pt : rh.parts) {
        if (!pt.n_rec) continue;
        if (pt.n >= (uint64_t)db->k) {
            rc = ss::launch_class_minik(db, pt.sl->d, pt.n, pt.sl->packed, d_pos, d_slot_val, d_hits0, st);
            if (rc) return rc;
        } else {
            SS_HIP(ss::l2s::set(d_pos, 0, pt.n_tiles * (uint64_t)ss::SUP_TILE * 2));      // too short for a k-mer: records without windows
        }
        SS_HIP(ss::l2s::set(d_long, 0, 8));
        const GapArgs A{d_pos, (const uint8_t *)pt.sl->d, sp.d_start, sp.d_end, pt.rec_base, pt.n_rec, pt.n, pt.sl->packed ? pt.sl->slot : 0u,
                        pt.sl->packed ? pt.sl->L : 0u, (uint32_t)db->k, min_hits, d_out, d_long, d_list, reinterpret_cast<uint4 *>(d_rec)};
        const unsigned blocks = (unsigned)std::min<uint64_t>((pt.n_rec + 256 * 4 - 1) / (256 * 4), 8192);
        const unsigned long_blocks = (unsigned)std::min<uint64_t>(ss::grid_for(pt.n_rec), GAP_LONG_WGS);
        with_input_layout(pt.sl->d, pt.sl->packed, [&](auto in) {
            hipLaunchKernelGGL((gap_walk_kernel<decltype(in)::value, false>), dim3(blocks), dim3(256), 0, st, A);
            hipLaunchKernelGGL((gap_walk_kernel<decltype(in)::value, true>), dim3(long_blocks), dim3(256), 0, st, A);
        });
        SS_HIP(hipGetLastError());
    }
    unsigned long long host[SS_GAPS_OUT];
    SS_HIP(ss::l2s::copy(host, d_out, sizeof(host), hipMemcpyDeviceToHost));
    for (uint32_t j = 0; j < SS_GAPS_OUT; j++) out[j] = host[j];
    if (d_rec) SS_HIP(ss::l2s::copy(rec_out, d_rec, rec_total * 16, hipMemcpyDeviceToHost));
    return SS_OK;
}

}  // extern "C"
