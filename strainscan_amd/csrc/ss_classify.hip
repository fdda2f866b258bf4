// ss_reads_classify: every record of a resident read set assigned to a node of a tree over the table's k-mers (`--classify_reads`).
//
// The caller says which node each ROW of the table belongs to and gives the forest's parents; a hit of a record (ss_reads_support's
// hit) then points at a node, and the record goes to the node whose root path collects the most hits (strainscan_hip.h has the
// definition, tests/class_model.py restates it).  Nothing here depends on the order of the records.
//
// The passes, each a plain launch; all scratch comes from the stream-ordered pool and goes back before the call returns:
//   0. host: the forest is checked (a parent above n_nodes, a cycle: SS_EINVAL) and walked once: depth[v] (a root has 1), and the
//      Euler-tour interval tin[v] .. tout[v] of v's subtree, so that "u is v or an ancestor of v" is tin[u] <= tin[v] < tout[u].
//   1. slot_nodes_kernel: one thread per row, atomicMin / atomicMax of the row's node + 1 into its slot; slot_nodes_finish_kernel:
//      one thread per slot, min == max -> that node, else 0 (no rows, or rows that disagree: label_model's slot rule with 16-bit
//      nodes).  kmers[v] is counted on the way.
//   2. per slab: scan_minik_kernel<.., ClassSink> (ss_minik.hip) leaves pos_node[p], the node of the k-mer found at position p, 16
//      bits per position of the slab; hits without a node are only counted (node_hits[0]).  The array is sized by the largest slab
//      and reused slab by slab.  Record spans of ASCII slabs are those of ss_reads_select (record_spans_of); a packed slab's
//      record g is positions [g * slot, g * slot + L).
//   3. classify_kernel: one thread per record walks its fields, eight per 16-byte load, and keeps the distinct nodes it meets with
//      their hit counts in LDS -- up to CLS_CAP of them.  score(v) = the hits of the kept nodes whose interval holds tin[v]; the
//      best score wins, tied nodes fold to their lowest common ancestor (parents and depths; 0 across trees).  A record with more
//      distinct nodes, or longer than CLS_LONG positions, adds nothing and is put on a list instead.
//   4. classify_long_kernel: one workgroup per listed record, any length, any number of nodes: the record's hits are added up in
//      a dense h[n_nodes + 1] of the workgroup in global memory, every hit position then sums h[] along its node's root path,
//      the workgroup reduces (score, node) with the same tie fold, and h[] is cleared by the positions that filled it.
//   direct[] and node_hits[] are added up in LDS per workgroup where n_nodes + 1 <= CLS_LDS, with 64-bit global atomics otherwise.
// All of this is classify_records, which leaves its results -- the classes of the records among them -- on the device, in the
// scratch of the call.  ss_reads_classify copies them back.  ss_bam_tag.hip (`--tag_bam`) calls it through ss_support.h and asks
// for the best score of every record as well (ClassArgs::rec_score, written only where it is not null: nobody here asks).
// ss_calls.hip (`--read_calls`, ss_reads_calls) asks for both and for every record's list of (node, hits): classify_kernel then
// leaves its kept nodes in ClassArgs::stage and their number in ClassArgs::cnt, again behind a null test, and hit_lists_slab makes
// the lists behind classify_long_kernel of each slab, while pos_node still holds that slab's fields.
//
// ss_reads_select_class (`--extract_class`) runs classify_records once and then, per listed clade:
//   5. select_class_len_kernel: one thread per record, out_len[rec] = the record's class lies in the clade ? length + 1 : 0 --
//      select_len_kernel (ss_select.hip) with the Euler interval of the clade's node in the place of the hit threshold, the span
//      rule and the totals shared with it (record_span, add_selected: ss_scan_dev.h); clade 0 is class 0.  gather_records (ss_select.hip) then makes the new set from out_len[], which is reset for the next clade.
// The classes never leave the device, and a second clade costs a length pass, a prefix sum and a gather.
#include "ss_scan_dev.h"
#include "ss_support.h"

using namespace ss::dev;

namespace {

constexpr uint32_t CLS_CAP = 8;          // distinct nodes a record may hold on the fast path
constexpr uint32_t CLS_LONG = 4096;      // positions a record may have there
constexpr uint32_t CLS_LDS = 4096;       // nodes (+ 1) whose direct[] / node_hits[] a workgroup adds up in LDS
constexpr uint32_t CLS_LONG_WGS = 64;    // workgroups (and dense h[] arrays) of the general pass

using ss::ClassArgs;
using ss::Classified;
using ss::Forest;

__global__ __launch_bounds__(256) void slot_nodes_kernel(const uint16_t *__restrict__ row_node, const uint32_t *__restrict__ slot_of_row,
                                                         uint64_t n_rows, uint64_t n_slots, uint32_t *__restrict__ lo, uint32_t *__restrict__ hi)
{
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= n_rows) return;
    const uint32_t sl = slot_of_row[i];
    if (sl == SS_NO_SLOT || sl >= n_slots) return;
    const uint32_t v = (uint32_t)row_node[i] + 1u;
    atomicMin(&lo[sl], v);
    atomicMax(&hi[sl], v);
}

// out[slot] = the common node of its rows; n_with[v] += slots of node v (v >= 1)
__global__ __launch_bounds__(256) void slot_nodes_finish_kernel(const uint32_t *__restrict__ lo, const uint32_t *__restrict__ hi, uint64_t n_slots,
                                                                uint32_t n_nodes, uint16_t *__restrict__ out, unsigned long long *__restrict__ n_with)
{
    __shared__ uint32_t cnt[CLS_LDS];
    const bool in_lds = n_nodes < CLS_LDS;
    if (in_lds) {
        for (uint32_t v = threadIdx.x; v <= n_nodes; v += 256u) cnt[v] = 0u;
        __syncthreads();
    }
    for (uint64_t s = (uint64_t)blockIdx.x * 256u + threadIdx.x; s < n_slots; s += (uint64_t)gridDim.x * 256u) {
        const uint32_t a = lo[s], b = hi[s];
        const uint32_t v = (b && a == b && b - 1u <= n_nodes) ? b - 1u : 0u;
        out[s] = (uint16_t)v;
        if (v) {
            if (in_lds) atomicAdd(&cnt[v], 1u);
            else atomicAdd(&n_with[v], 1ull);
        }
    }
    if (in_lds) {
        __syncthreads();
        for (uint32_t v = 1u + threadIdx.x; v <= n_nodes; v += 256u)
            if (cnt[v]) atomicAdd(&n_with[v], (unsigned long long)cnt[v]);
    }
}

// the lowest common ancestor of two nodes; 0 when they stand in different trees (or either is 0)
__device__ __forceinline__ uint32_t lca_of(const Forest &f, uint32_t a, uint32_t b)
{
    uint32_t da = f.depth[a], db = f.depth[b];
    while (da > db) { a = f.parent[a]; da--; }
    while (db > da) { b = f.parent[b]; db--; }
    while (a != b) { a = f.parent[a]; b = f.parent[b]; }
    return a;
}

// record g of the slab (every record has a span; one that has none, or a wild one, reads nothing)
__device__ __forceinline__ RecordSpan span_of(const ClassArgs &A, uint64_t g)
{
    return record_span(A.slot != 0u, g, A.rec0, A.start, A.end, A.slot, A.fixed_len, A.n);
}

__global__ __launch_bounds__(256) void classify_kernel(const ClassArgs A, const Forest F)
{
    __shared__ uint32_t acc_direct[CLS_LDS], acc_hits[CLS_LDS];
    __shared__ uint32_t kept[CLS_CAP][256];      // node << 16 | hits (at most CLS_LONG), a column per thread
    const bool in_lds = A.n_nodes < CLS_LDS;
    const uint32_t t = threadIdx.x;
    if (in_lds) {
        for (uint32_t v = t; v <= A.n_nodes; v += 256u) { acc_direct[v] = 0u; acc_hits[v] = 0u; }
        __syncthreads();
    }
    unsigned long long ties = 0;
    for (uint64_t g = (uint64_t)blockIdx.x * 256u + t; g < A.n_rec; g += (uint64_t)gridDim.x * 256u) {
        const RecordSpan sp = span_of(A, g);
        const uint64_t s = sp.s, e = sp.s + sp.len;
        const bool ok = sp.ok;
        bool over = ok && sp.len > CLS_LONG;
        uint32_t d = 0, cur = 0;                  // kept nodes; the one met last
        if (ok && !over) {
            for (uint64_t c = s & ~7ull; c < e && !over; c += 8u) {
                const uint4 q = *reinterpret_cast<const uint4 *>(A.pos_node + c);
                if (!(q.x | q.y | q.z | q.w)) continue;
                const uint32_t w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
                for (uint32_t i = 0; i < 8u; i++) {
                    const uint32_t v = (w[i >> 1] >> (16u * (i & 1u))) & 0xFFFFu;
                    if (!v || c + i < s || c + i >= e || over) continue;
                    if (!(d && (kept[cur][t] >> 16) == v)) {
                        for (cur = 0; cur < d && (kept[cur][t] >> 16) != v; cur++) {}
                        if (cur == d) {
                            if (d == CLS_CAP) { over = true; continue; }
                            kept[d++][t] = v << 16;
                        }
                    }
                    kept[cur][t]++;
                }
            }
        }
        if (over) {
            A.long_list[atomicAdd(&A.tot[1], 1ull)] = (uint32_t)g;
            if (A.stage) A.stage[g * CLS_CAP] = 0u;      // (no kept node is 0: the general pass lists this record)
            continue;
        }
        if (!ok) continue;
        if (A.cnt) {                                 // ss_reads_calls: the kept nodes are the record's list, still unsorted
            A.cnt[g] = d;
            if (A.stage) {
                uint32_t x[CLS_CAP];
#pragma unroll
                for (uint32_t i = 0; i < CLS_CAP; i++) x[i] = i < d ? kept[i][t] : 0xFFFFFFFFu;
                uint4 *dst = reinterpret_cast<uint4 *>(A.stage + g * CLS_CAP);
                dst[0] = make_uint4(x[0], x[1], x[2], x[3]);
                dst[1] = make_uint4(x[4], x[5], x[6], x[7]);
            }
        }
        // scores: the kept nodes on v's root path, v itself among them
        uint32_t best = 0, cls = 0;
        bool tie = false;
        for (uint32_t i = 0; i < d; i++) {
            const uint32_t v = kept[i][t] >> 16;
            uint32_t sc = kept[i][t] & 0xFFFFu;
            if (d > 1) {
                const uint32_t tv = F.tin[v];
                for (uint32_t j = 0; j < d; j++) {
                    const uint32_t u = kept[j][t] >> 16;
                    if (j != i && F.tin[u] <= tv && tv < F.tout[u]) sc += kept[j][t] & 0xFFFFu;
                }
            }
            if (sc > best) { best = sc; cls = v; tie = false; }
            else if (sc == best) { cls = lca_of(F, cls, v); tie = true; }
        }
        if (A.rec_score) A.rec_score[A.rec0 + g] = best;
        if (best < A.min_score) { cls = 0; tie = false; }
        ties += tie;
        if (A.rec_class) A.rec_class[A.rec0 + g] = cls;
        if (in_lds) {
            atomicAdd(&acc_direct[cls], 1u);
            for (uint32_t i = 0; i < d; i++) atomicAdd(&acc_hits[kept[i][t] >> 16], kept[i][t] & 0xFFFFu);
        } else {
            atomicAdd(&A.direct[cls], 1ull);
            for (uint32_t i = 0; i < d; i++) atomicAdd(&A.node_hits[kept[i][t] >> 16], (unsigned long long)(kept[i][t] & 0xFFFFu));
        }
    }
#pragma unroll
    for (int dd = 32; dd > 0; dd >>= 1) ties += __shfl_xor(ties, dd, 64);
    if ((t & 63u) == 0 && ties) atomicAdd(&A.tot[0], ties);
    if (in_lds) {
        __syncthreads();
        for (uint32_t v = t; v <= A.n_nodes; v += 256u) {
            if (acc_direct[v]) atomicAdd(&A.direct[v], (unsigned long long)acc_direct[v]);
            if (acc_hits[v]) atomicAdd(&A.node_hits[v], (unsigned long long)acc_hits[v]);
        }
    }
}

// what a thread, then the workgroup, knows of a record: the best score, the fold of the nodes that reach it, whether there were two
struct Best { uint32_t score, node, tie; };
__device__ __forceinline__ void best_add(const Forest &F, Best &b, uint32_t score, uint32_t node, uint32_t tie)
{
    if (!score || score < b.score) return;
    if (score > b.score) { b.score = score; b.node = node; b.tie = tie; }
    else if (node != b.node || tie || b.tie) { b.node = lca_of(F, b.node, node); b.tie = 1u; }
}

// the listed records of one slab, one workgroup each at a time; h: [gridDim.x][n_nodes + 1], all zero before and after.
// h[] is written with atomics and read with atomic loads: both go to the L2, so no stale line of a CU's L1 is ever read.
__global__ __launch_bounds__(256) void classify_long_kernel(const ClassArgs A, const Forest F, uint32_t *__restrict__ h_all)
{
    __shared__ Best red[256];
    const uint32_t t = threadIdx.x;
    uint32_t *h = h_all + (uint64_t)blockIdx.x * ((uint64_t)A.n_nodes + 1u);
    const uint64_t n_list = A.tot[1];
    for (uint64_t li = blockIdx.x; li < n_list; li += gridDim.x) {
        const uint64_t g = A.long_list[li];
        const RecordSpan sp = span_of(A, g);
        if (!sp.ok) continue;                      // (uniform over the workgroup)
        const uint64_t s = sp.s, e = sp.s + sp.len;
        for (uint64_t p = s + t; p < e; p += 256u) {
            const uint32_t v = A.pos_node[p];
            if (v) atomicAdd(&h[v], 1u);
        }
        __syncthreads();
        Best b{0u, 0u, 0u};
        for (uint64_t p = s + t; p < e; p += 256u) {
            const uint32_t v = A.pos_node[p];
            if (!v) continue;
            uint32_t sc = 0;
            for (uint32_t u = v; u; u = F.parent[u]) sc += __hip_atomic_load(&h[u], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            best_add(F, b, sc, v, 0u);
        }
        red[t] = b;
        __syncthreads();
        for (uint32_t w = 128u; w > 0u; w >>= 1) {
            if (t < w) {
                Best x = red[t];
                const Best y = red[t + w];
                best_add(F, x, y.score, y.node, y.tie);
                red[t] = x;
            }
            __syncthreads();
        }
        // node_hits, and h[] back to zero: the first position to take a node's count away adds it
        for (uint64_t p = s + t; p < e; p += 256u) {
            const uint32_t v = A.pos_node[p];
            if (!v) continue;
            const uint32_t c = atomicExch(&h[v], 0u);
            if (c) atomicAdd(&A.node_hits[v], (unsigned long long)c);
        }
        if (t == 0) {
            Best r = red[0];
            if (A.rec_score) A.rec_score[A.rec0 + g] = r.score;
            if (r.score < A.min_score) { r.node = 0u; r.tie = 0u; }
            if (r.tie) atomicAdd(&A.tot[0], 1ull);
            atomicAdd(&A.direct[r.node], 1ull);
            if (A.rec_class) A.rec_class[A.rec0 + g] = r.node;
        }
        __syncthreads();                             // (red[] and h[] are free for the next record)
    }
}

// records [rec0, rec0 + n_rec) of one slab: out_len = the bytes a record takes in the new slab (its length + '\n'; 0 when its
// class is not in the clade), tot[0] += selected records, tot[1] += their bytes.  The clade of node c > 0 is the classes whose tin
// lies in [lo, hi) = [tin[c], tout[c]); unclassified == true is the clade 0: class 0 alone.  fixed_len != 0: a packed slab, every record
// that long.  A span that does not lie inside the slab (record_span) selects nothing: classify_kernel gave such a record no class,
// and the gather must not read outside the slab.
__global__ __launch_bounds__(256) void select_class_len_kernel(const uint32_t *__restrict__ rec_class, const uint32_t *__restrict__ tin,
                                                               const unsigned long long *__restrict__ start, const unsigned long long *__restrict__ end,
                                                               uint64_t rec0, uint64_t n_rec, uint64_t n, uint32_t slot, uint32_t fixed_len,
                                                               uint32_t n_nodes, bool unclassified, uint32_t lo, uint32_t hi, unsigned long long *__restrict__ out_len,
                                                               unsigned long long *__restrict__ tot)
{
    unsigned long long cnt = 0, bytes = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x; i < n_rec; i += (uint64_t)gridDim.x * 256u) {
        const uint32_t c = rec_class[rec0 + i];
        unsigned long long len = 0;
        bool in = unclassified ? c == 0u : false;
        if (!unclassified && c != 0u && c <= n_nodes) {
            const uint32_t t = tin[c];
            in = lo <= t && t < hi;
        }
        if (in) {
            const RecordSpan sp = record_span(fixed_len != 0u, i, rec0, start, end, slot, fixed_len, n);
            if (sp.ok) { len = sp.len + 1ull; cnt++; bytes += len; }
        }
        out_len[rec0 + i] = len;
    }
    add_selected(cnt, bytes, tot);
}

std::atomic<uint64_t> g_classify_calls{0}, g_select_class_calls{0};
thread_local uint64_t t_last_ties = 0;

// parent[1..n_nodes] (0 = a root) -> par / depth / tin / tout [n_nodes + 1]; false: a parent above n_nodes, or a cycle
bool walk_forest(const uint32_t *parent, uint32_t n_nodes, std::vector<uint32_t> &par, std::vector<uint32_t> &depth, std::vector<uint32_t> &tin,
                 std::vector<uint32_t> &tout)
{
    const size_t n1 = (size_t)n_nodes + 1;
    par.assign(n1, 0);
    for (uint32_t v = 1; v <= n_nodes; v++) {
        if (parent[v] > n_nodes) return false;
        par[v] = parent[v];
    }
    // children as a CSR; a forest is reached whole from its roots, a cycle never
    std::vector<uint32_t> first(n1 + 1, 0), kids(n_nodes);
    for (uint32_t v = 1; v <= n_nodes; v++) first[par[v] + 1]++;
    for (size_t i = 1; i <= n1; i++) first[i] += first[i - 1];
    {
        std::vector<uint32_t> at(first.begin(), first.end() - 1);
        for (uint32_t v = 1; v <= n_nodes; v++) kids[at[par[v]]++] = v;
    }
    depth.assign(n1, 0);
    tin.assign(n1, 0);
    tout.assign(n1, 0);
    std::vector<uint32_t> stack, next(first.begin(), first.end() - 1);
    uint32_t clock = 0, seen = 0;
    stack.push_back(0);                              // 0 stands above the roots
    while (!stack.empty()) {
        const uint32_t v = stack.back();
        if (next[v] < first[v + 1]) {
            const uint32_t c = kids[next[v]++];
            depth[c] = depth[v] + 1;
            tin[c] = clock++;
            seen++;
            stack.push_back(c);
        } else {
            tout[v] = clock;
            stack.pop_back();
        }
    }
    tout[0] = 0;                                     // (0 is nobody's ancestor)
    return seen == n_nodes;
}

}  // namespace

// The whole of ss_reads_classify but the copy back (the passes 0-4 above; declared in ss_support.h: ss_bam_tag.hip calls it too).
// *calls (or nullptr) is counted once the arguments have passed.
int ss::classify_records(const ss_db *db, const ss_reads *R, const uint32_t *row_node, uint32_t n_nodes, const uint32_t *parent, uint32_t min_score,
                         bool keep_class, std::atomic<uint64_t> *calls, Classified *C, bool keep_score)
{
    if (!db || !R || !row_node || !parent || min_score == 0 || n_nodes < 1 || n_nodes > SS_CLASS_NODES_MAX) return SS_EINVAL;
    if (db->layout != 1) return SS_ERANGE;                          // page-index tables only
    if (R->has_cut_record) return SS_ERANGE;                        // at any k: a cut piece is not a read
    const uint64_t n_rows = db->n_rows, n_slots = db->n_slots;
    const size_t n1 = (size_t)n_nodes + 1;
    std::vector<uint16_t> rows16(std::max<uint64_t>(n_rows, 1));
    uint32_t top = 0;
    for (uint64_t i = 0; i < n_rows; i++) { top = std::max(top, row_node[i]); rows16[i] = (uint16_t)row_node[i]; }
    if (top > n_nodes) return SS_EINVAL;
    std::vector<uint32_t> par, depth;
    std::vector<uint32_t> &tin = C->tin, &tout = C->tout;
    if (!walk_forest(parent, n_nodes, par, depth, tin, tout)) return SS_EINVAL;

    ss::RecHits &rh = C->rh;
    ss::RecSpans &sp = C->sp;
    int rc = ss::record_index_of(R, db->device, &rh, calls);
    if (rc) return rc;
    rc = ss::record_spans_of(&rh, &sp);
    if (rc) return rc;
    const hipStream_t st = ss::l2s::stream();
    ss::PoolScratch &scratch = rh.scratch;
    const uint64_t rec_total = rh.rec_total;

    // the forest, the results
    uint32_t *d_forest = nullptr;
    unsigned long long *&d_out = C->d_out;
    SS_HIP(scratch.get((void **)&d_forest, 4 * n1 * 4));
    SS_HIP(scratch.get((void **)&d_out, (3 * n1 + 2) * 8));
    {
        std::vector<uint32_t> all(4 * n1);
        std::copy(par.begin(), par.end(), all.begin());
        std::copy(depth.begin(), depth.end(), all.begin() + n1);
        std::copy(tin.begin(), tin.end(), all.begin() + 2 * n1);
        std::copy(tout.begin(), tout.end(), all.begin() + 3 * n1);
        SS_HIP(ss::l2s::copy(d_forest, all.data(), all.size() * 4, hipMemcpyHostToDevice));
    }
    SS_HIP(ss::l2s::set(d_out, 0, (3 * n1 + 2) * 8));
    const Forest F{d_forest, d_forest + n1, d_forest + 2 * n1, d_forest + 3 * n1};
    C->F = F;
    unsigned long long *d_direct = d_out, *d_hits = d_out + n1, *d_kmers = d_out + 2 * n1, *d_tot = d_out + 3 * n1;

    // 1. nodes per slot
    uint16_t *d_rows = nullptr, *d_slot_node = nullptr;
    uint32_t *d_lo = nullptr, *d_hi = nullptr;
    SS_HIP(scratch.get((void **)&d_rows, n_rows * 2));
    SS_HIP(scratch.get((void **)&d_lo, n_slots * 4));
    SS_HIP(scratch.get((void **)&d_hi, n_slots * 4));
    SS_HIP(scratch.get((void **)&d_slot_node, n_slots * 2));
    SS_HIP(ss::l2s::set(d_lo, 0xFF, std::max<uint64_t>(n_slots * 4, 16)));
    SS_HIP(ss::l2s::set(d_hi, 0, std::max<uint64_t>(n_slots * 4, 16)));
    if (n_rows) {
        SS_HIP(ss::l2s::copy(d_rows, rows16.data(), n_rows * 2, hipMemcpyHostToDevice));
        hipLaunchKernelGGL(slot_nodes_kernel, dim3((unsigned)((n_rows + 255) / 256)), dim3(256), 0, st, d_rows, db->d_slot_of_row, n_rows, n_slots, d_lo, d_hi);
        SS_HIP(hipGetLastError());
    }
    if (n_slots) {
        const unsigned blocks = (unsigned)std::min<uint64_t>((n_slots + 256 * 8 - 1) / (256 * 8), 4096);
        hipLaunchKernelGGL(slot_nodes_finish_kernel, dim3(blocks), dim3(256), 0, st, d_lo, d_hi, n_slots, n_nodes, d_slot_node, d_kmers);
        SS_HIP(hipGetLastError());
    }

    // 2.-4. slab by slab
    uint64_t max_fields = 0, max_rec = 0;
    for (const auto &pt : rh.parts)
        if (pt.n_rec) { max_fields = std::max(max_fields, pt.n_tiles * (uint64_t)ss::SUP_TILE); max_rec = std::max(max_rec, pt.n_rec); }
    uint16_t *d_pos = nullptr;
    uint32_t *&d_class = C->d_class;
    uint32_t *d_list = nullptr, *d_h = nullptr;
    if (max_fields) {
        SS_HIP(scratch.get((void **)&d_pos, max_fields * 2));
        SS_HIP(scratch.get((void **)&d_list, max_rec * 4));
        SS_HIP(scratch.get((void **)&d_h, (uint64_t)CLS_LONG_WGS * n1 * 4));
        SS_HIP(ss::l2s::set(d_h, 0, (uint64_t)CLS_LONG_WGS * n1 * 4));
    }
    if (keep_class && rec_total) {
        SS_HIP(scratch.get((void **)&d_class, rec_total * 4));
        SS_HIP(ss::l2s::set(d_class, 0, rec_total * 4));
    }
    if (keep_score && rec_total) {
        SS_HIP(scratch.get((void **)&C->d_score, rec_total * 4));
        SS_HIP(ss::l2s::set(C->d_score, 0, rec_total * 4));
    }
    ss::HitLists *const H = C->lists;
    if (H) {
        uint64_t positions = 0;
        for (const auto &pt : rh.parts) positions += pt.n_rec ? pt.n : 0;
        rc = ss::hit_lists_begin(H, scratch, rec_total, max_rec, positions);
        if (rc) return rc;
    }
    for (const auto &pt : rh.parts) {
        if (!pt.n_rec) continue;
        if (pt.n >= (uint64_t)db->k) {
            rc = ss::launch_class_minik(db, pt.sl->d, pt.n, pt.sl->packed, d_pos, d_slot_node, d_hits, st);
            if (rc) return rc;
        } else {
            SS_HIP(ss::l2s::set(d_pos, 0, pt.n_tiles * (uint64_t)ss::SUP_TILE * 2));      // too short for a k-mer: records without hits
        }
        SS_HIP(ss::l2s::set(d_tot + 1, 0, 8));
        const ClassArgs A{d_pos, sp.d_start, sp.d_end, pt.rec_base, pt.n_rec, pt.n, pt.sl->packed ? pt.sl->slot : 0u, pt.sl->packed ? pt.sl->L : 0u,
                          n_nodes, min_score, d_direct, d_hits, d_tot, d_class, C->d_score, d_list, H ? H->d_cnt : nullptr,
                          H && H->fill ? H->d_stage : nullptr};
        if (H) SS_HIP(ss::l2s::set(H->d_cnt, 0, (pt.n_rec + 1) * 8));
        const unsigned blocks = (unsigned)std::min<uint64_t>((pt.n_rec + 256 * 4 - 1) / (256 * 4), 8192);
        hipLaunchKernelGGL(classify_kernel, dim3(blocks), dim3(256), 0, st, A, F);
        SS_HIP(hipGetLastError());
        hipLaunchKernelGGL(classify_long_kernel, dim3(CLS_LONG_WGS), dim3(256), 0, st, A, F, d_h);
        SS_HIP(hipGetLastError());
        if (H) {
            rc = ss::hit_lists_slab(H, A, d_h, CLS_LONG_WGS);
            if (rc) return rc;
        }
    }
    return SS_OK;
}

namespace {

using ss::classify_records;

// direct / node_hits / kmers [n1] (each nullptr to skip) and the calling thread's ties from what classify_records left; synchronous
int classify_results(const Classified &C, size_t n1, uint64_t *direct, uint64_t *node_hits, uint64_t *kmers)
{
    std::vector<unsigned long long> out(3 * n1 + 2);
    SS_HIP(ss::l2s::copy(out.data(), C.d_out, out.size() * 8, hipMemcpyDeviceToHost));
    for (size_t v = 0; v < n1; v++) {
        if (direct) direct[v] = out[v];
        if (node_hits) node_hits[v] = out[n1 + v];
        if (kmers) kmers[v] = v ? out[2 * n1 + v] : 0;
    }
    t_last_ties = out[3 * n1];
    return SS_OK;
}

// the sets of ss_reads_select_class, one per clade, from the classes on the device; out[i] is set as it is made
int select_clades(Classified &C, uint32_t n_nodes, const uint32_t *clades, uint32_t n_clades, ss_reads **out)
{
    const hipStream_t st = ss::l2s::stream();
    for (uint32_t i = 0; i < n_clades; i++) {
        const uint32_t c = clades[i];
        if (i && C.sp.d_tot) SS_HIP(ss::l2s::set(C.sp.d_tot, 0, 16));      // (d_len is written whole by every pass)
        for (const auto &pt : C.rh.parts) {
            if (!pt.n_rec) continue;
            const unsigned blocks = (unsigned)std::min<uint64_t>((pt.n_rec + 256 * 4 - 1) / (256 * 4), 4096);
            hipLaunchKernelGGL(select_class_len_kernel, dim3(blocks), dim3(256), 0, st, C.d_class, C.F.tin, C.sp.d_start, C.sp.d_end, pt.rec_base,
                               pt.n_rec, pt.n, pt.sl->packed ? pt.sl->slot : 0u, pt.sl->packed ? pt.sl->L : 0u, n_nodes, c == 0u, c ? C.tin[c] : 0u,
                               c ? C.tout[c] : 0u, C.sp.d_len, C.sp.d_tot);
            SS_HIP(hipGetLastError());
        }
        const int rc = ss::gather_records(&C.rh, C.sp, "ss_reads_select_class", &out[i]);
        if (rc) return rc;
    }
    return SS_OK;
}

}  // namespace

int ss::classified_counts(const Classified &C, uint32_t n_nodes, uint64_t *direct, uint64_t *node_hits, uint64_t *kmers, uint64_t *ties)
{
    const int rc = classify_results(C, (size_t)n_nodes + 1, direct, node_hits, kmers);
    if (rc == SS_OK && ties) *ties = t_last_ties;
    return rc;
}

extern "C" {

int ss_reads_classify_calls(uint64_t *n)
{
    if (!n) return SS_EINVAL;
    *n = g_classify_calls.load();
    return SS_OK;
}

int ss_reads_select_class_calls(uint64_t *n)
{
    if (!n) return SS_EINVAL;
    *n = g_select_class_calls.load();
    return SS_OK;
}

int ss_reads_classify_ties(uint64_t *n)
{
    if (!n) return SS_EINVAL;
    *n = t_last_ties;
    return SS_OK;
}

int ss_reads_classify(const ss_db *db, const ss_reads *R, const uint32_t *row_node, uint32_t n_nodes, const uint32_t *parent, uint32_t min_score,
                      uint64_t *direct, uint64_t *node_hits, uint64_t *kmers, uint32_t *rec_class)
{
    if (!direct || !node_hits || !kmers) return SS_EINVAL;
    Classified C;
    int rc = classify_records(db, R, row_node, n_nodes, parent, min_score, rec_class != nullptr, &g_classify_calls, &C);
    if (rc) return rc;
    rc = classify_results(C, (size_t)n_nodes + 1, direct, node_hits, kmers);
    if (rc) return rc;
    if (C.d_class) SS_HIP(ss::l2s::copy(rec_class, C.d_class, C.rh.rec_total * 4, hipMemcpyDeviceToHost));
    return SS_OK;
}

int ss_reads_select_class(const ss_db *db, const ss_reads *R, const uint32_t *row_node, uint32_t n_nodes, const uint32_t *parent, uint32_t min_score,
                          const uint32_t *clades, uint32_t n_clades, ss_reads **out, uint64_t *direct, uint64_t *node_hits, uint64_t *kmers)
{
    if (!out) return SS_EINVAL;
    if (n_clades >= 1 && n_clades <= SS_SELECT_CLADES_MAX)
        for (uint32_t i = 0; i < n_clades; i++) out[i] = nullptr;
    if (!clades || n_clades < 1 || n_clades > SS_SELECT_CLADES_MAX) return SS_EINVAL;
    for (uint32_t i = 0; i < n_clades; i++)
        if (clades[i] > n_nodes) return SS_EINVAL;
    int rc;
    {
        Classified C;
        rc = classify_records(db, R, row_node, n_nodes, parent, min_score, true, &g_select_class_calls, &C);
        if (!rc) rc = classify_results(C, (size_t)n_nodes + 1, direct, node_hits, kmers);
        if (!rc) rc = select_clades(C, n_nodes, clades, n_clades, out);
    }
    if (rc)
        for (uint32_t i = 0; i < n_clades; i++)
            if (out[i]) { ss_reads_destroy(out[i]); out[i] = nullptr; }
    return rc;
}

}  // extern "C"
