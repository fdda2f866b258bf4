// ss_reads_calls: what ss_reads_classify decides, record by record (`--read_calls`): the class and the best score of every record
// of a resident set and the record's HIT LIST -- every node v >= 1 with h[v] > 0 in ascending v, with h[v] -- as one CSR over the
// records: the list of record i is entries rec_first[i] .. rec_first[i + 1] - 1 of list_node / list_hits.
//
// The classification is classify_records (ss_classify.hip), unchanged; the classes and scores are its keep_class / keep_score.  The
// lists are made slab by slab, right behind classify_long_kernel of the slab, because pos_node -- the node of every position --
// is sized by the largest slab and reused by the next one.  Of the two designs that fit there, this file takes the fixed-stride
// staging with a compaction, and handles the listed records apart:
//   a. classify_kernel, which holds a short record's distinct nodes in LDS anyway, leaves them as they are -- up to CLS_CAP = 8
//      words node << 16 | hits, unsorted -- in stage[8 * record] and their number in cnt[record]: two 16-byte stores per record and
//      no second walk over the record's 2 bytes per position (a 150-base read: 32 bytes written and read again beside 300 bytes
//      read again, and the search of every hit among the kept nodes not repeated).  Counting first and filling in a second pass
//      over the positions would need no staging (32 bytes per record of the largest slab) but pays that walk twice.
//   b. list_long_kernel<false>: a record that classify_kernel left to the general pass (more than 8 nodes, or more than CLS_LONG
//      positions, where a count may pass 16 bits) is counted from the dense h[] of its workgroup: the positions add their nodes up
//      and take them away again, and the first to take a node's count away counts the node.
//   c. hipcub's exclusive sum over cnt[] (64-bit) gives every record's offset in the slab; the slab's total comes back to the host,
//      which knows the entries of the slabs before (`base`) and whether this slab's lists still fit `cap`.
//   d. list_fill_kernel: one thread per record writes rec_first and, for a record of the fast path, sorts its eight staged words in
//      registers (a fixed network: nodes are distinct, so the words sort by node) and writes them out.
//   e. list_long_kernel<true>: the listed records once more: h[] is added up again and then walked in node order, 256 nodes at a
//      time, a ballot and four wave totals giving every non-zero node its place -- ascending v for free, 32-bit hits -- and the
//      walk clears h[] behind itself.
// Where the lists do not fit (cap == 0 among them) only a.-c. run, without the staging: *n_list is what the caller has to bring.
// Offsets are 64-bit throughout; the record count is limited as ss_reads_select limits it (record_spans_of).  All scratch comes
// from the call's PoolScratch and goes back before the call returns.
//
// ss_reads_load_ordered (the single-file load in FILE ORDER that `--read_calls` classifies) is in ss_pairs.hip, beside
// file_to_flat_dev, which it shares with ss_reads_load_pairs.
#include "ss_scan_dev.h"
#include "ss_support.h"

#include <hipcub/hipcub.hpp>

using namespace ss::dev;

namespace {

using ss::ClassArgs;
using ss::HitLists;

constexpr uint32_t LIST_STRIDE = 8;      // CLS_CAP of ss_classify.hip: the words classify_kernel stages per record

__device__ __forceinline__ RecordSpan span_of(const ClassArgs &A, uint64_t g)
{
    return record_span(A.slot != 0u, g, A.rec0, A.start, A.end, A.slot, A.fixed_len, A.n);
}

__device__ __forceinline__ void order2(uint32_t &a, uint32_t &b)
{
    const uint32_t lo = min(a, b), hi = max(a, b);
    a = lo;
    b = hi;
}

// One thread per record of the slab: rec_first, and the list of a record of the fast path from its staged words.
// off[i]: the entries of the slab's records before i; base: those of the slabs before; fill: the lists are written.
__global__ __launch_bounds__(256) void list_fill_kernel(const unsigned long long *__restrict__ cnt, const unsigned long long *__restrict__ off,
                                                        const uint32_t *__restrict__ stage, uint64_t rec0, uint64_t n_rec, uint64_t base, bool fill,
                                                        uint64_t cap, unsigned long long *__restrict__ first, uint32_t *__restrict__ list_node,
                                                        uint32_t *__restrict__ list_hits)
{
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= n_rec) return;
    const uint64_t o = base + off[i];
    first[rec0 + i] = o;
    const uint64_t c = cnt[i];
    if (!fill || c == 0 || c > LIST_STRIDE) return;
    const uint4 a = *reinterpret_cast<const uint4 *>(stage + i * LIST_STRIDE);
    if (a.x == 0u) return;                                              // (a listed record: list_long_kernel writes it)
    const uint4 b = *reinterpret_cast<const uint4 *>(stage + i * LIST_STRIDE + 4);
    uint32_t x0 = a.x, x1 = a.y, x2 = a.z, x3 = a.w, x4 = b.x, x5 = b.y, x6 = b.z, x7 = b.w;      // (unused words are 0xFFFFFFFF: last)
    // Batcher's odd-even merge sort of eight: 19 exchanges
    order2(x0, x1); order2(x2, x3); order2(x4, x5); order2(x6, x7);
    order2(x0, x2); order2(x1, x3); order2(x4, x6); order2(x5, x7);
    order2(x1, x2); order2(x5, x6);
    order2(x0, x4); order2(x1, x5); order2(x2, x6); order2(x3, x7);
    order2(x2, x4); order2(x3, x5);
    order2(x1, x2); order2(x3, x4); order2(x5, x6);
    const uint32_t x[LIST_STRIDE] = {x0, x1, x2, x3, x4, x5, x6, x7};
#pragma unroll
    for (uint32_t j = 0; j < LIST_STRIDE; j++) {
        if (j < c && o + j < cap) {
            list_node[o + j] = x[j] >> 16;
            list_hits[o + j] = x[j] & 0xFFFFu;
        }
    }
}

// The listed records of one slab, one workgroup each at a time; h: [gridDim.x][n_nodes + 1], all zero before and after (the
// arrays of classify_long_kernel, which has finished).  FILL == false: cnt[g] = the record's nodes.  FILL == true: its list, at
// base + off[g].  h[] is written with atomics and read with atomic exchanges: both go to the L2.
template <bool FILL>
__global__ __launch_bounds__(256) void list_long_kernel(const ClassArgs A, uint32_t *__restrict__ h_all, const unsigned long long *__restrict__ off,
                                                        uint64_t base, uint64_t cap, uint32_t *__restrict__ list_node, uint32_t *__restrict__ list_hits)
{
    __shared__ uint32_t n_dist, wave_sum[4];
    const uint32_t t = threadIdx.x;
    uint32_t *h = h_all + (uint64_t)blockIdx.x * ((uint64_t)A.n_nodes + 1u);
    const uint64_t n_list = A.tot[1];
    for (uint64_t li = blockIdx.x; li < n_list; li += gridDim.x) {
        const uint64_t g = A.long_list[li];
        if (g >= A.n_rec) continue;                    // (never: the list holds records of this slab; uniform over the workgroup)
        const RecordSpan sp = span_of(A, g);
        if (!sp.ok) continue;
        const uint64_t want = FILL ? A.cnt[g] : 0u;
        if (FILL && want == 0u) continue;
        const uint64_t s = sp.s, e = sp.s + sp.len;
        if (t == 0) n_dist = 0u;
        for (uint64_t p = s + t; p < e; p += 256u) {
            const uint32_t v = A.pos_node[p];
            if (v) atomicAdd(&h[v], 1u);
        }
        __syncthreads();
        if (!FILL) {
            for (uint64_t p = s + t; p < e; p += 256u) {
                const uint32_t v = A.pos_node[p];
                if (v && atomicExch(&h[v], 0u)) atomicAdd(&n_dist, 1u);
            }
            __syncthreads();
            if (t == 0) A.cnt[g] = n_dist;
        } else {
            const uint64_t o = base + off[g];
            uint64_t run = 0;
            for (uint32_t v0 = 1u; v0 <= A.n_nodes; v0 += 256u) {
                const uint32_t v = v0 + t;
                const uint32_t c = v <= A.n_nodes ? atomicExch(&h[v], 0u) : 0u;
                const unsigned long long m = __ballot(c != 0u);
                if ((t & 63u) == 0u) wave_sum[t >> 6] = (uint32_t)__popcll(m);
                __syncthreads();
                uint32_t before = (uint32_t)__popcll(m & ((1ull << (t & 63u)) - 1ull)), all = 0;
#pragma unroll
                for (uint32_t w = 0; w < 4u; w++) {
                    if (w < (t >> 6)) before += wave_sum[w];
                    all += wave_sum[w];
                }
                const uint64_t at = run + before;
                if (c && at < want && o + at < cap) {
                    list_node[o + at] = v;
                    list_hits[o + at] = c;
                }
                run += all;
                __syncthreads();                           // (wave_sum[] is free for the next 256 nodes)
            }
        }
        __syncthreads();                                   // (n_dist and h[] are free for the next record)
    }
}

std::atomic<uint64_t> g_calls_calls{0};

}  // namespace

int ss::hit_lists_begin(HitLists *H, PoolScratch &scratch, uint64_t rec_total, uint64_t max_rec, uint64_t positions)
{
    H->n_list = 0;
    H->cap = std::min(H->cap, positions);                   // (a listed node has a hit, a hit a position)
    H->fill = H->cap > 0;
    SS_HIP(scratch.get((void **)&H->d_first, (rec_total + 1) * 8));
    SS_HIP(ss::l2s::set(H->d_first, 0, (rec_total + 1) * 8));
    if (!max_rec) return SS_OK;
    if (max_rec + 1 >= 0x7FFFFFFFull) return SS_ERANGE;     // hipcub counts its items in an int
    SS_HIP(scratch.get((void **)&H->d_cnt, (max_rec + 1) * 8));
    SS_HIP(scratch.get((void **)&H->d_off, (max_rec + 1) * 8));
    SS_HIP(hipcub::DeviceScan::ExclusiveSum(nullptr, H->tmp_bytes, H->d_cnt, H->d_off, (int)(max_rec + 1), ss::l2s::stream()));
    SS_HIP(scratch.get(&H->d_tmp, H->tmp_bytes));
    if (H->fill) {
        SS_HIP(scratch.get((void **)&H->d_stage, max_rec * LIST_STRIDE * 4));
        SS_HIP(scratch.get((void **)&H->d_node, H->cap * 4));
        SS_HIP(scratch.get((void **)&H->d_hits, H->cap * 4));
    }
    return SS_OK;
}

int ss::hit_lists_slab(HitLists *H, const ClassArgs &A, uint32_t *d_h, uint32_t long_wgs)
{
    const hipStream_t st = ss::l2s::stream();
    // b. the listed records' counts; c. the offsets and the slab's total
    hipLaunchKernelGGL(list_long_kernel<false>, dim3(long_wgs), dim3(256), 0, st, A, d_h, H->d_off, (uint64_t)0, (uint64_t)0, (uint32_t *)nullptr,
                       (uint32_t *)nullptr);
    SS_HIP(hipGetLastError());
    size_t tmp_bytes = H->tmp_bytes;
    SS_HIP(hipcub::DeviceScan::ExclusiveSum(H->d_tmp, tmp_bytes, H->d_cnt, H->d_off, (int)(A.n_rec + 1), st));
    unsigned long long total = 0;
    SS_HIP(ss::l2s::copy(&total, H->d_off + A.n_rec, 8, hipMemcpyDeviceToHost));
    const uint64_t base = H->n_list;
    const bool fill = H->fill && A.stage != nullptr && base + total <= H->cap;
    H->fill = fill;                                         // (once a slab's lists do not fit, nothing more is written)
    // d., e.
    hipLaunchKernelGGL(list_fill_kernel, dim3(ss::grid_for(A.n_rec)), dim3(256), 0, st, H->d_cnt, H->d_off, A.stage, A.rec0, A.n_rec, base, fill,
                       H->cap, H->d_first, H->d_node, H->d_hits);
    SS_HIP(hipGetLastError());
    if (fill && total) {
        hipLaunchKernelGGL(list_long_kernel<true>, dim3(long_wgs), dim3(256), 0, st, A, d_h, H->d_off, base, H->cap, H->d_node, H->d_hits);
        SS_HIP(hipGetLastError());
    }
    H->n_list = base + total;
    return SS_OK;
}

extern "C" {

int ss_reads_calls_calls(uint64_t *n)
{
    if (!n) return SS_EINVAL;
    *n = g_calls_calls.load();
    return SS_OK;
}

int ss_reads_calls(const ss_db *db, const ss_reads *R, const uint32_t *row_node, uint32_t n_nodes, const uint32_t *parent, uint32_t min_score,
                   uint32_t *rec_class, uint32_t *rec_score, uint64_t *rec_first, uint32_t *list_node, uint32_t *list_hits, uint64_t cap,
                   uint64_t *n_list, uint64_t *direct, uint64_t *node_hits, uint64_t *kmers)
{
    if (!rec_class || !rec_score || !rec_first || !n_list) return SS_EINVAL;
    if (cap && (!list_node || !list_hits)) return SS_EINVAL;
    *n_list = 0;
    ss::HitLists H;
    H.cap = cap;
    ss::Classified C;
    C.lists = &H;
    int rc = ss::classify_records(db, R, row_node, n_nodes, parent, min_score, true, &g_calls_calls, &C, true);
    if (rc) return rc;
    SS_HIP(ss::l2s::sync());
    *n_list = H.n_list;
    if (H.n_list > cap || (H.n_list && !H.fill)) return SS_ERANGE;
    rc = ss::classified_counts(C, n_nodes, direct, node_hits, kmers, nullptr);
    if (rc) return rc;
    const uint64_t records = C.rh.rec_total;
    if (records) {
        SS_HIP(ss::l2s::copy(rec_class, C.d_class, records * 4, hipMemcpyDeviceToHost));
        SS_HIP(ss::l2s::copy(rec_score, C.d_score, records * 4, hipMemcpyDeviceToHost));
        SS_HIP(ss::l2s::copy(rec_first, H.d_first, records * 8, hipMemcpyDeviceToHost));
    }
    rec_first[records] = H.n_list;
    if (H.n_list) {
        SS_HIP(ss::l2s::copy(list_node, H.d_node, H.n_list * 4, hipMemcpyDeviceToHost));
        SS_HIP(ss::l2s::copy(list_hits, H.d_hits, H.n_list * 4, hipMemcpyDeviceToHost));
    }
    return SS_OK;
}

}  // extern "C"
