// ss_reads_classify_strains: every record of a resident read set assigned to the SET of called strains that explain it best
// (`--classify_strains`); ss_reads_select_strains: the records of chosen sets as new resident sets (`--extract_strains`).
//
// The caller gives every ROW of the table a 16-bit mask: bit j - 1 says that called strain j has the row's k-mer.  A hit of a
// record (ss_reads_support's hit) then votes for every strain of its k-mer's mask, h[j] counts the votes of strain j, and the
// record's set is the strains with the most votes (strainscan_hip.h has the definition, tests/strain_set_model.py restates it).
// Nothing here depends on the order of the records.
//
// The passes, each a plain launch; all scratch comes from the stream-ordered pool and goes back before the call returns:
//   1. slot_sets_kernel: one thread per row, atomicAnd / atomicOr of the row's mask into its slot; slot_sets_finish_kernel: one
//      thread per slot, and == or -> that mask, else 0 (no rows, or rows that disagree: label_model's slot rule with masks).
//      kmers[j] is counted on the way, a ballot per strain.
//   2. per slab: scan_minik_kernel<.., ClassSink> (ss_minik.hip), unchanged, with the slot masks in the place of the slot nodes:
//      pos_set[p] = the mask of the k-mer found at position p, 16 bits per position; a hit of mask 0 is only counted
//      (strain_hits[0]).  Record spans are those of ss_reads_select (record_spans_of).
//   3. vote_kernel: one thread per record walks its fields, eight per 16-byte load.  The sixteen counters are BIT-SLICED: plane b
//      holds bit b of all sixteen counts, so a run of r equal masks is one ripple add of r x mask over the planes (a full adder
//      per plane: five logic operations), and the argmax set falls out of one pass from the top plane down (cand = plane & cand
//      wherever that is not empty).  SET_PLANES = 12 planes count to 4095, which is the longest record the pass takes; a longer
//      one is put on a list.  The totals need no per-lane extraction either: the count of strain j over a wave's 64 records is
//      the sum over the planes of popcount(ballot(bit j of plane b)) << b, which lane j + 1 keeps; unique[] and tied[] are
//      ballots too.  A wave adds its numbers to the workgroup's in LDS, the workgroup adds them to global memory when it ends.
//      set_reads[]: an LDS histogram while 1 << n_strains <= SET_LDS entries; above that equal sets are folded within the wave,
//      one global atomic per distinct set of a wave's 64 records.
//   4. vote_long_kernel: one workgroup per listed record, any length: every thread walks pieces of SET_CHUNK positions with the
//      same planes, the wave sums go to sixteen 64-bit counts in LDS, and one thread takes the maximum and the set from them.
// All of this is strain_sets_records, which leaves its results -- the sets of the records among them -- on the device.
//
// ss_reads_select_strains runs it once and then, per listed entry:
//   5. select_strains_len_kernel: out_len[rec] = the record's set equals / intersects the wanted one ? length + 1 : 0 --
//      select_class_len_kernel (ss_classify.hip) with a mask test in the place of the Euler interval; gather_records
//      (ss_select.hip) then makes the new set from out_len[], which is written whole again for the next entry.
//
// ss_reads_strain_sets_resampled (`--em_strains`) runs it once too, keeps the sets, and then:
//   6. resample_weights_of (ss_resample.hip): the weights every record draws in up to sixteen bootstrap replicates, 4-bit fields
//      of one word per record, in the spans' len[] under the record's number -- the numbering of the sets.
//   7. set_weights_kernel: a lane per record adds every field that is not zero to hist[replicate][set].  While the
//      n_replicates << n_strains counters fit SETW_LDS 32-bit words a workgroup keeps them in LDS and adds its non-zero entries
//      to the 64-bit ones in global memory when it ends; above that equal sets are folded within the wave as in pass 3, a
//      replicate's weights over the lanes of one set summed by four ballots (a bit of the field each), and lane j issues
//      replicate j's atomic: one per distinct (replicate, set) of a wave.
#include "ss_scan_dev.h"
#include "ss_support.h"

using namespace ss::dev;

namespace {

constexpr uint32_t SET_PLANES = 12;                        // planes of the bit-sliced counters: counts below 4096
constexpr uint32_t SET_LONG = (1u << SET_PLANES) - 1u;     // positions a record may have on the per-thread path
constexpr uint32_t SET_CHUNK = 4088;                       // positions of one piece of the general pass (<= SET_LONG, a multiple of 8)
constexpr uint32_t SET_LDS_BITS = 12;                      // strains whose set_reads[] a workgroup adds up in LDS
constexpr uint32_t SET_LDS = 1u << SET_LDS_BITS;
constexpr uint32_t SET_LONG_WGS = 64;                      // workgroups of the general pass
constexpr uint32_t N1 = SS_STRAIN_SET_MAX + 1;             // entries of unique / tied / strain_hits / kmers on the device
static_assert(SET_CHUNK <= SET_LONG && SET_CHUNK % 8 == 0, "a piece fits the planes and keeps the 16-byte loads aligned");
static_assert(SS_STRAIN_SET_MAX == 16, "a set is a 16-bit mask, and lanes 0..16 of a wave keep its totals");

// the records of one slab and where their results go
struct SetArgs {
    const uint16_t *pos_set;                    // the slab's fields
    const unsigned long long *start, *end;      // ASCII slab: spans by record of the set; packed: unused
    uint64_t rec0, n_rec, n;                    // the slab's first record, its records, its positions
    uint32_t slot, fixed_len;                   // packed slab: positions per slot, bases per record; else 0
    uint32_t n_strains, min_score;
    unsigned long long *uniq, *tied, *hits;     // [N1]
    unsigned long long *set_reads;              // [1 << n_strains] or nullptr
    unsigned long long *n_long;                 // records of this slab on the list
    uint16_t *rec_set;                          // [records of the set] or nullptr
    uint32_t *rec_score;                        // [records of the set] or nullptr
    uint32_t *long_list;                        // [n_rec] records of this slab (slab-relative) left to the general pass
};

__global__ __launch_bounds__(256) void slot_sets_kernel(const uint16_t *__restrict__ row_set, const uint32_t *__restrict__ slot_of_row,
                                                        uint64_t n_rows, uint64_t n_slots, uint32_t *__restrict__ all, uint32_t *__restrict__ any)
{
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= n_rows) return;
    const uint32_t sl = slot_of_row[i];
    if (sl == SS_NO_SLOT || sl >= n_slots) return;
    const uint32_t m = row_set[i];
    atomicAnd(&all[sl], m);
    atomicOr(&any[sl], m);
}

// out[slot] = the common mask of its rows (all[] comes filled with ones: a slot without rows keeps them and gets 0);
// n_with[j] += slots whose mask has bit j - 1
__global__ __launch_bounds__(256) void slot_sets_finish_kernel(const uint32_t *__restrict__ all, const uint32_t *__restrict__ any, uint64_t n_slots,
                                                               uint32_t n_strains, uint16_t *__restrict__ out, unsigned long long *__restrict__ n_with)
{
    const uint32_t lane = threadIdx.x & 63u;
    unsigned long long mine = 0;                // lane j: slots with strain j (j >= 1) of this wave
    for (uint64_t s0 = (uint64_t)blockIdx.x * 256u; s0 < n_slots; s0 += (uint64_t)gridDim.x * 256u) {
        const uint64_t s = s0 + threadIdx.x;
        uint32_t m = 0;
        if (s < n_slots) {
            const uint32_t a = all[s], b = any[s];
            m = a == b ? b & 0xFFFFu : 0u;
            out[s] = (uint16_t)m;
        }
        for (uint32_t j = 0; j < n_strains; j++) {
            const uint32_t c = (uint32_t)__popcll(__ballot((m >> j) & 1u));
            if (lane == j + 1u) mine += c;
        }
    }
    if (lane >= 1u && lane <= n_strains && mine) atomicAdd(&n_with[lane], mine);
}

struct Planes { uint32_t p[SET_PLANES]; };

// every counter of `mask` += run (run <= SET_LONG; the counters stay below 1 << SET_PLANES, which the callers see to)
__device__ __forceinline__ void planes_add(Planes &P, uint32_t mask, uint32_t run)
{
    uint32_t carry = 0;
#pragma unroll
    for (uint32_t b = 0; b < SET_PLANES; b++) {
        const uint32_t a = (0u - ((run >> b) & 1u)) & mask;
        const uint32_t x = P.p[b];
        P.p[b] = x ^ a ^ carry;
        carry = (x & a) | (carry & (x ^ a));
    }
}

// the fields of positions [s, e), e - s <= SET_LONG, added to the planes; pos holds a whole number of tiles, so the aligned
// 16-byte loads around [s, e) stay inside it
__device__ __forceinline__ void walk_fields(const uint16_t *__restrict__ pos, uint64_t s, uint64_t e, Planes &P)
{
    uint32_t cur = 0, run = 0;                  // the mask of the run at hand, its length
    for (uint64_t c = s & ~7ull; c < e; c += 8u) {
        const uint4 q = *reinterpret_cast<const uint4 *>(pos + c);
        if (!(q.x | q.y | q.z | q.w)) {
            if (cur) { planes_add(P, cur, run); cur = 0; }
            continue;
        }
        const uint32_t w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
        for (uint32_t i = 0; i < 8u; i++) {
            uint32_t v = (w[i >> 1] >> (16u * (i & 1u))) & 0xFFFFu;
            if (c + i < s || c + i >= e) v = 0u;
            if (v != cur) {
                if (cur) planes_add(P, cur, run);
                cur = v;
                run = 0u;
            }
            run++;
        }
    }
    if (cur) planes_add(P, cur, run);
}

// the count of strain j + 1 summed over the wave's lanes (the same value in every lane)
__device__ __forceinline__ unsigned long long wave_count(const Planes &P, uint32_t j)
{
    unsigned long long h = 0;
#pragma unroll
    for (uint32_t b = 0; b < SET_PLANES; b++) h += (unsigned long long)__popcll(__ballot((P.p[b] >> j) & 1u)) << b;
    return h;
}

__device__ __forceinline__ RecordSpan span_of(const SetArgs &A, uint64_t g)
{
    return record_span(A.slot != 0u, g, A.rec0, A.start, A.end, A.slot, A.fixed_len, A.n);
}

__global__ __launch_bounds__(256) void vote_kernel(const SetArgs A)
{
    __shared__ uint32_t hist[SET_LDS];
    __shared__ uint32_t acc_u[N1], acc_t[N1];
    __shared__ unsigned long long acc_h[N1];
    const uint32_t t = threadIdx.x, lane = t & 63u;
    const bool lds_hist = A.set_reads && A.n_strains <= SET_LDS_BITS;
    if (lds_hist)
        for (uint32_t m = t; m < (1u << A.n_strains); m += 256u) hist[m] = 0u;
    if (t < N1) { acc_u[t] = 0u; acc_t[t] = 0u; acc_h[t] = 0ull; }
    __syncthreads();
    for (uint64_t g0 = (uint64_t)blockIdx.x * 256u; g0 < A.n_rec; g0 += (uint64_t)gridDim.x * 256u) {      // (the same for the workgroup)
        const uint64_t g = g0 + t;
        Planes P;
#pragma unroll
        for (uint32_t b = 0; b < SET_PLANES; b++) P.p[b] = 0u;
        bool valid = false;
        if (g < A.n_rec) {
            const RecordSpan sp = span_of(A, g);
            if (sp.ok && sp.len > SET_LONG) A.long_list[atomicAdd(A.n_long, 1ull)] = (uint32_t)g;
            else if (sp.ok) { valid = true; walk_fields(A.pos_set, sp.s, sp.s + sp.len, P); }
        }
        // the largest count and who has it: from the top plane down
        uint32_t cand = 0xFFFFu, score = 0;
#pragma unroll
        for (int b = (int)SET_PLANES - 1; b >= 0; b--) {
            const uint32_t x = P.p[b] & cand;
            if (x) { cand = x; score |= 1u << b; }
        }
        const uint32_t set = score >= A.min_score && score ? cand : 0u;
        if (valid) {
            if (A.rec_score) A.rec_score[A.rec0 + g] = score;
            if (A.rec_set) A.rec_set[A.rec0 + g] = (uint16_t)set;
        }
        // the wave's totals: lane 0 the empty and the tied sets, lane j the numbers of strain j
        const bool multi = valid && (set & (set - 1u)) != 0u;
        uint32_t uq = 0, td = 0;
        unsigned long long hs = 0;
        {
            const uint32_t none = (uint32_t)__popcll(__ballot(valid && set == 0u)), many = (uint32_t)__popcll(__ballot(multi));
            if (lane == 0u) { uq = none; td = many; }
        }
        for (uint32_t j = 0; j < A.n_strains; j++) {
            const uint32_t u = (uint32_t)__popcll(__ballot(valid && set == (1u << j)));
            const uint32_t m = (uint32_t)__popcll(__ballot(multi && ((set >> j) & 1u)));
            const unsigned long long h = wave_count(P, j);
            if (lane == j + 1u) { uq = u; td = m; hs = h; }
        }
        if (lane <= A.n_strains) {
            if (uq) atomicAdd(&acc_u[lane], uq);
            if (td) atomicAdd(&acc_t[lane], td);
            if (hs) atomicAdd(&acc_h[lane], hs);
        }
        if (lds_hist) {
            if (valid) atomicAdd(&hist[set], 1u);
        } else if (A.set_reads) {
            // equal sets of the wave's records folded before they go to global memory
            for (unsigned long long rem = __ballot(valid); rem;) {
                const int src = __ffsll((long long)rem) - 1;
                const uint32_t key = (uint32_t)__shfl((int)set, src, 64);
                const unsigned long long same = __ballot(valid && set == key);
                if ((int)lane == src) atomicAdd(&A.set_reads[key], (unsigned long long)__popcll(same));
                rem &= ~same;
            }
        }
    }
    __syncthreads();
    if (t < N1) {
        if (acc_u[t]) atomicAdd(&A.uniq[t], (unsigned long long)acc_u[t]);
        if (acc_t[t]) atomicAdd(&A.tied[t], (unsigned long long)acc_t[t]);
        if (t && acc_h[t]) atomicAdd(&A.hits[t], acc_h[t]);
    }
    if (lds_hist)
        for (uint32_t m = t; m < (1u << A.n_strains); m += 256u)
            if (hist[m]) atomicAdd(&A.set_reads[m], (unsigned long long)hist[m]);
}

// the listed records of one slab, one workgroup each at a time
__global__ __launch_bounds__(256) void vote_long_kernel(const SetArgs A)
{
    __shared__ unsigned long long h[SS_STRAIN_SET_MAX];
    const uint32_t t = threadIdx.x, lane = t & 63u;
    const uint64_t n_list = *A.n_long;
    for (uint64_t li = blockIdx.x; li < n_list; li += gridDim.x) {
        const uint64_t g = A.long_list[li];
        const RecordSpan sp = span_of(A, g);
        if (!sp.ok) continue;                      // (uniform over the workgroup)
        if (t < SS_STRAIN_SET_MAX) h[t] = 0ull;
        __syncthreads();
        const uint64_t e = sp.s + sp.len;
        for (uint64_t r0 = sp.s; r0 < e; r0 += 256ull * SET_CHUNK) {      // (uniform too)
            Planes P;
#pragma unroll
            for (uint32_t b = 0; b < SET_PLANES; b++) P.p[b] = 0u;
            const uint64_t a = r0 + (uint64_t)t * SET_CHUNK;
            if (a < e) walk_fields(A.pos_set, a, a + SET_CHUNK < e ? a + SET_CHUNK : e, P);
            unsigned long long mine = 0;
            for (uint32_t j = 0; j < A.n_strains; j++) {
                const unsigned long long c = wave_count(P, j);
                if (lane == j) mine = c;
            }
            if (lane < A.n_strains && mine) atomicAdd(&h[lane], mine);
        }
        __syncthreads();
        if (t == 0) {
            unsigned long long best = 0;
            for (uint32_t j = 0; j < A.n_strains; j++) best = h[j] > best ? h[j] : best;
            uint32_t set = 0;
            for (uint32_t j = 0; j < A.n_strains; j++) {
                if (best && h[j] == best) set |= 1u << j;
                if (h[j]) atomicAdd(&A.hits[j + 1u], h[j]);
            }
            if (best < A.min_score) set = 0u;
            if (A.rec_score) A.rec_score[A.rec0 + g] = (uint32_t)best;
            if (A.rec_set) A.rec_set[A.rec0 + g] = (uint16_t)set;
            if (!set) atomicAdd(&A.uniq[0], 1ull);
            else if (!(set & (set - 1u))) atomicAdd(&A.uniq[__ffs((int)set)], 1ull);
            else {
                atomicAdd(&A.tied[0], 1ull);
                for (uint32_t j = 0; j < A.n_strains; j++)
                    if ((set >> j) & 1u) atomicAdd(&A.tied[j + 1u], 1ull);
            }
            if (A.set_reads) atomicAdd(&A.set_reads[set], 1ull);
        }
        __syncthreads();                             // (h[] is free for the next record)
    }
}

// records [rec0, rec0 + n_rec) of one slab: out_len = the bytes a record takes in the new slab (its length + '\n'; 0 when its set
// is not wanted), tot[0] += selected records, tot[1] += their bytes.  intersects == false: the sets equal to `want`, the empty
// one for want == 0; true: the sets that share a strain with it.  A span that does not lie inside the slab (record_span) selects
// nothing: vote_kernel gave such a record no set, and the gather must not read outside the slab.
__global__ __launch_bounds__(256) void select_strains_len_kernel(const uint16_t *__restrict__ rec_set, const unsigned long long *__restrict__ start,
                                                                 const unsigned long long *__restrict__ end, uint64_t rec0, uint64_t n_rec, uint64_t n,
                                                                 uint32_t slot, uint32_t fixed_len, uint32_t want, bool intersects,
                                                                 unsigned long long *__restrict__ out_len, unsigned long long *__restrict__ tot)
{
    unsigned long long cnt = 0, bytes = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x; i < n_rec; i += (uint64_t)gridDim.x * 256u) {
        const uint32_t st = rec_set[rec0 + i];
        unsigned long long len = 0;
        if (intersects ? (st & want) != 0u : st == want) {
            const RecordSpan sp = record_span(fixed_len != 0u, i, rec0, start, end, slot, fixed_len, n);
            if (sp.ok) { len = sp.len + 1ull; cnt++; bytes += len; }
        }
        out_len[rec0 + i] = len;
    }
    add_selected(cnt, bytes, tot);
}

// hist[j << n_strains | set] += the weight of replicate j, over every record of the set: w[rec] holds the weights as 4-bit fields
// (resample_weights_kernel; 0 for a record without a span), rec_set[rec] the record's set.  lds: the counters fit SETW_LDS words.
constexpr uint32_t SETW_LDS = 1u << 14;
__global__ __launch_bounds__(256) void set_weights_kernel(const uint16_t *__restrict__ rec_set, const unsigned long long *__restrict__ w, uint64_t n_rec,
                                                          uint32_t n_strains, uint32_t n_rep, bool lds, unsigned long long *__restrict__ hist)
{
    __shared__ uint32_t acc[SETW_LDS];
    const uint32_t t = threadIdx.x, lane = t & 63u, cells = n_rep << n_strains;
    if (lds) {
        for (uint32_t c = t; c < cells; c += 256u) acc[c] = 0u;
        __syncthreads();
    }
    for (uint64_t g0 = (uint64_t)blockIdx.x * 256u; g0 < n_rec; g0 += (uint64_t)gridDim.x * 256u) {      // (the same for the workgroup)
        const uint64_t g = g0 + t;
        const unsigned long long word = g < n_rec ? w[g] : 0ull;
        const uint32_t set = word ? rec_set[g] : 0u;
        if (lds) {
            for (unsigned long long rest = word; rest;) {
                const uint32_t j = (uint32_t)(__ffsll((long long)rest) - 1) >> 2;
                atomicAdd(&acc[(j << n_strains) | set], (uint32_t)(word >> (4u * j)) & 15u);
                rest &= ~(15ull << (4u * j));
            }
            continue;
        }
        for (unsigned long long rem = __ballot(word != 0ull); rem;) {
            const int src = __ffsll((long long)rem) - 1;
            const uint32_t key = (uint32_t)__shfl((int)set, src, 64);
            const bool in = word != 0ull && set == key;
            unsigned long long mine = 0;                // lane j: replicate j's weights over the lanes of this set
            for (uint32_t j = 0; j < n_rep; j++) {
                const uint32_t f = in ? (uint32_t)(word >> (4u * j)) & 15u : 0u;
                unsigned long long c = 0;
#pragma unroll
                for (uint32_t b = 0; b < 4u; b++) c += (unsigned long long)__popcll(__ballot((f >> b) & 1u)) << b;
                if (lane == j) mine = c;
            }
            if (lane < n_rep && mine) atomicAdd(&hist[((size_t)lane << n_strains) | key], mine);
            rem &= ~__ballot(in);
        }
    }
    if (lds) {
        __syncthreads();
        for (uint32_t c = t; c < cells; c += 256u)
            if (acc[c]) atomicAdd(&hist[c], (unsigned long long)acc[c]);
    }
}

std::atomic<uint64_t> g_classify_strains_calls{0}, g_select_strains_calls{0}, g_sets_resampled_calls{0};
thread_local uint64_t t_last_set_ties = 0;

// what strain_sets_records leaves behind: everything on the device lives in rh.scratch and is enqueued on ss::l2s::stream()
struct StrainSets {
    ss::RecHits rh;
    ss::RecSpans sp;
    unsigned long long *d_out = nullptr;        // unique[N1], tied[N1], strain_hits[N1], kmers[N1], the slab's listed records
    unsigned long long *d_set_reads = nullptr;  // [1 << n_strains] (keep_sets)
    uint16_t *d_set = nullptr;                  // [rh.rec_total] the set of every record (keep_set; nullptr for a set without records)
    uint32_t *d_score = nullptr;                // [rh.rec_total] the largest count of every record (keep_score)
};

// The whole of ss_reads_classify_strains but the copy back (the passes 1-4 above).  *calls is counted once the arguments have passed.
int strain_sets_records(const ss_db *db, const ss_reads *R, const uint16_t *row_sets, uint32_t n_strains, uint32_t min_score, bool keep_sets,
                        bool keep_set, bool keep_score, std::atomic<uint64_t> *calls, StrainSets *S)
{
    if (!db || !R || !row_sets || min_score == 0 || n_strains < 1 || n_strains > SS_STRAIN_SET_MAX) return SS_EINVAL;
    if (db->layout != 1) return SS_ERANGE;                          // page-index tables only
    if (R->has_cut_record) return SS_ERANGE;                        // at any k: a cut piece is not a read
    const uint64_t n_rows = db->n_rows, n_slots = db->n_slots;
    uint32_t seen = 0;
    for (uint64_t i = 0; i < n_rows; i++) seen |= row_sets[i];
    if (seen >> n_strains) return SS_EINVAL;

    ss::RecHits &rh = S->rh;
    ss::RecSpans &sp = S->sp;
    int rc = ss::record_index_of(R, db->device, &rh, calls);
    if (rc) return rc;
    rc = ss::record_spans_of(&rh, &sp);
    if (rc) return rc;
    const hipStream_t st = ss::l2s::stream();
    ss::PoolScratch &scratch = rh.scratch;
    const uint64_t rec_total = rh.rec_total;

    unsigned long long *&d_out = S->d_out;
    SS_HIP(scratch.get((void **)&d_out, (4 * N1 + 2) * 8));
    SS_HIP(ss::l2s::set(d_out, 0, (4 * N1 + 2) * 8));
    unsigned long long *d_uniq = d_out, *d_tied = d_out + N1, *d_hits = d_out + 2 * N1, *d_kmers = d_out + 3 * N1, *d_long = d_out + 4 * N1;
    if (keep_sets) {
        SS_HIP(scratch.get((void **)&S->d_set_reads, (8ull << n_strains)));
        SS_HIP(ss::l2s::set(S->d_set_reads, 0, std::max<uint64_t>(8ull << n_strains, 16)));
    }

    // 1. masks per slot
    uint16_t *d_rows = nullptr, *d_slot_set = nullptr;
    uint32_t *d_all = nullptr, *d_any = nullptr;
    SS_HIP(scratch.get((void **)&d_rows, n_rows * 2));
    SS_HIP(scratch.get((void **)&d_all, n_slots * 4));
    SS_HIP(scratch.get((void **)&d_any, n_slots * 4));
    SS_HIP(scratch.get((void **)&d_slot_set, n_slots * 2));
    SS_HIP(ss::l2s::set(d_all, 0xFF, std::max<uint64_t>(n_slots * 4, 16)));
    SS_HIP(ss::l2s::set(d_any, 0, std::max<uint64_t>(n_slots * 4, 16)));
    if (n_rows) {
        SS_HIP(ss::l2s::copy(d_rows, row_sets, n_rows * 2, hipMemcpyHostToDevice));
        hipLaunchKernelGGL(slot_sets_kernel, dim3(ss::grid_for(n_rows)), dim3(256), 0, st, d_rows, db->d_slot_of_row, n_rows, n_slots, d_all, d_any);
        SS_HIP(hipGetLastError());
    }
    if (n_slots) {
        const unsigned blocks = (unsigned)std::min<uint64_t>((n_slots + 256 * 8 - 1) / (256 * 8), 4096);
        hipLaunchKernelGGL(slot_sets_finish_kernel, dim3(blocks), dim3(256), 0, st, d_all, d_any, n_slots, n_strains, d_slot_set, d_kmers);
        SS_HIP(hipGetLastError());
    }

    // 2.-4. slab by slab
    uint64_t max_fields = 0, max_rec = 0;
    for (const auto &pt : rh.parts)
        if (pt.n_rec) { max_fields = std::max(max_fields, pt.n_tiles * (uint64_t)ss::SUP_TILE); max_rec = std::max(max_rec, pt.n_rec); }
    uint16_t *d_pos = nullptr;
    uint32_t *d_list = nullptr;
    if (max_fields) {
        SS_HIP(scratch.get((void **)&d_pos, max_fields * 2));
        SS_HIP(scratch.get((void **)&d_list, max_rec * 4));
    }
    if (keep_set && rec_total) {
        SS_HIP(scratch.get((void **)&S->d_set, rec_total * 2));
        SS_HIP(ss::l2s::set(S->d_set, 0, std::max<uint64_t>(rec_total * 2, 16)));
    }
    if (keep_score && rec_total) {
        SS_HIP(scratch.get((void **)&S->d_score, rec_total * 4));
        SS_HIP(ss::l2s::set(S->d_score, 0, std::max<uint64_t>(rec_total * 4, 16)));
    }
    for (const auto &pt : rh.parts) {
        if (!pt.n_rec) continue;
        if (pt.n >= (uint64_t)db->k) {
            rc = ss::launch_class_minik(db, pt.sl->d, pt.n, pt.sl->packed, d_pos, d_slot_set, d_hits, st);
            if (rc) return rc;
        } else {
            SS_HIP(ss::l2s::set(d_pos, 0, pt.n_tiles * (uint64_t)ss::SUP_TILE * 2));      // too short for a k-mer: records without hits
        }
        SS_HIP(ss::l2s::set(d_long, 0, 8));
        const SetArgs A{d_pos, sp.d_start, sp.d_end, pt.rec_base, pt.n_rec, pt.n, pt.sl->packed ? pt.sl->slot : 0u, pt.sl->packed ? pt.sl->L : 0u,
                        n_strains, min_score, d_uniq, d_tied, d_hits, S->d_set_reads, d_long, S->d_set, S->d_score, d_list};
        const unsigned blocks = (unsigned)std::min<uint64_t>((pt.n_rec + 256 * 4 - 1) / (256 * 4), 8192);
        hipLaunchKernelGGL(vote_kernel, dim3(blocks), dim3(256), 0, st, A);
        SS_HIP(hipGetLastError());
        hipLaunchKernelGGL(vote_long_kernel, dim3(SET_LONG_WGS), dim3(256), 0, st, A);
        SS_HIP(hipGetLastError());
    }
    return SS_OK;
}

// unique / tied / strain_hits / kmers [n_strains + 1] (each nullptr to skip) and the calling thread's ties; synchronous
int strain_sets_results(const StrainSets &S, uint32_t n_strains, uint64_t *uniq, uint64_t *tied, uint64_t *hits, uint64_t *kmers)
{
    unsigned long long out[4 * N1];
    SS_HIP(ss::l2s::copy(out, S.d_out, sizeof(out), hipMemcpyDeviceToHost));
    for (uint32_t j = 0; j <= n_strains; j++) {
        if (uniq) uniq[j] = out[j];
        if (tied) tied[j] = out[N1 + j];
        if (hits) hits[j] = out[2 * N1 + j];
        if (kmers) kmers[j] = j ? out[3 * N1 + j] : 0;
    }
    t_last_set_ties = out[N1];
    return SS_OK;
}

}  // namespace

extern "C" {

int ss_reads_classify_strains_calls(uint64_t *n)
{
    if (!n) return SS_EINVAL;
    *n = g_classify_strains_calls.load();
    return SS_OK;
}

int ss_reads_select_strains_calls(uint64_t *n)
{
    if (!n) return SS_EINVAL;
    *n = g_select_strains_calls.load();
    return SS_OK;
}

int ss_reads_classify_strains_ties(uint64_t *n)
{
    if (!n) return SS_EINVAL;
    *n = t_last_set_ties;
    return SS_OK;
}

int ss_reads_classify_strains(const ss_db *db, const ss_reads *R, const uint16_t *row_sets, uint32_t n_strains, uint32_t min_score, uint64_t *uniq,
                              uint64_t *tied, uint64_t *strain_hits, uint64_t *kmers, uint64_t *set_reads, uint16_t *rec_set, uint32_t *rec_score)
{
    if (!uniq || !tied || !strain_hits || !kmers) return SS_EINVAL;
    StrainSets S;
    int rc = strain_sets_records(db, R, row_sets, n_strains, min_score, set_reads != nullptr, rec_set != nullptr, rec_score != nullptr,
                                 &g_classify_strains_calls, &S);
    if (rc) return rc;
    rc = strain_sets_results(S, n_strains, uniq, tied, strain_hits, kmers);
    if (rc) return rc;
    if (set_reads) SS_HIP(ss::l2s::copy(set_reads, S.d_set_reads, 8ull << n_strains, hipMemcpyDeviceToHost));
    if (S.d_set) SS_HIP(ss::l2s::copy(rec_set, S.d_set, S.rh.rec_total * 2, hipMemcpyDeviceToHost));
    if (S.d_score) SS_HIP(ss::l2s::copy(rec_score, S.d_score, S.rh.rec_total * 4, hipMemcpyDeviceToHost));
    return SS_OK;
}

int ss_reads_strain_sets_resampled_calls(uint64_t *n)
{
    if (!n) return SS_EINVAL;
    *n = g_sets_resampled_calls.load();
    return SS_OK;
}

int ss_reads_strain_sets_resampled(const ss_db *db, const ss_reads *R, const uint16_t *row_sets, uint32_t n_strains, uint32_t min_score, uint64_t seed,
                                   uint32_t first_replicate, uint32_t n_replicates, uint64_t *set_reads)
{
    if (!set_reads || n_replicates < 1 || n_replicates > SS_SCAN_REPLICATES_MAX) return SS_EINVAL;
    StrainSets S;
    int rc = strain_sets_records(db, R, row_sets, n_strains, min_score, false, true, false, &g_sets_resampled_calls, &S);
    if (rc) return rc;
    const size_t cells = (size_t)n_replicates << n_strains;
    unsigned long long *d_hist = nullptr;
    SS_HIP(S.rh.scratch.get((void **)&d_hist, cells * 8));
    SS_HIP(ss::l2s::set(d_hist, 0, std::max<size_t>(cells * 8, 16)));
    if (S.rh.rec_total && S.d_set) {
        rc = ss::resample_weights_of(&S.rh, S.sp, seed, first_replicate, n_replicates);      // (in the spans' len[], by record of the set)
        if (rc) return rc;
        const unsigned blocks = (unsigned)std::min<uint64_t>((S.rh.rec_total + 256 * 4 - 1) / (256 * 4), 512);
        hipLaunchKernelGGL(set_weights_kernel, dim3(blocks), dim3(256), 0, ss::l2s::stream(), S.d_set, S.sp.d_len, S.rh.rec_total, n_strains,
                           n_replicates, cells <= SETW_LDS, d_hist);
        SS_HIP(hipGetLastError());
    }
    SS_HIP(ss::l2s::copy(set_reads, d_hist, cells * 8, hipMemcpyDeviceToHost));
    return SS_OK;
}

int ss_reads_select_strains(const ss_db *db, const ss_reads *R, const uint16_t *row_sets, uint32_t n_strains, uint32_t min_score, const uint16_t *want,
                            const uint8_t *how, uint32_t n_want, ss_reads **out, uint64_t *uniq, uint64_t *tied, uint64_t *strain_hits, uint64_t *kmers)
{
    if (!out) return SS_EINVAL;
    if (n_want >= 1 && n_want <= SS_SELECT_STRAINS_MAX)
        for (uint32_t i = 0; i < n_want; i++) out[i] = nullptr;
    if (!want || !how || n_want < 1 || n_want > SS_SELECT_STRAINS_MAX || n_strains < 1 || n_strains > SS_STRAIN_SET_MAX) return SS_EINVAL;
    for (uint32_t i = 0; i < n_want; i++)
        if (((uint32_t)want[i] >> n_strains) || how[i] > 1) return SS_EINVAL;
    int rc;
    {
        StrainSets S;
        rc = strain_sets_records(db, R, row_sets, n_strains, min_score, false, true, false, &g_select_strains_calls, &S);
        if (!rc) rc = strain_sets_results(S, n_strains, uniq, tied, strain_hits, kmers);
        const hipStream_t st = ss::l2s::stream();
        for (uint32_t i = 0; i < n_want && !rc; i++) {
            if (i && S.sp.d_tot) rc = ss::HipFail{"ss_reads_select_strains"}(ss::l2s::set(S.sp.d_tot, 0, 16)) ? SS_EHIP : SS_OK;      // (d_len is written whole by every pass)
            for (const auto &pt : S.rh.parts) {
                if (rc || !pt.n_rec) continue;
                const unsigned blocks = (unsigned)std::min<uint64_t>((pt.n_rec + 256 * 4 - 1) / (256 * 4), 4096);
                hipLaunchKernelGGL(select_strains_len_kernel, dim3(blocks), dim3(256), 0, st, S.d_set, S.sp.d_start, S.sp.d_end, pt.rec_base, pt.n_rec,
                                   pt.n, pt.sl->packed ? pt.sl->slot : 0u, pt.sl->packed ? pt.sl->L : 0u, (uint32_t)want[i], how[i] != 0,
                                   S.sp.d_len, S.sp.d_tot);
                if (ss::HipFail{"ss_reads_select_strains"}(hipGetLastError())) rc = SS_EHIP;
            }
            if (!rc) rc = ss::gather_records(&S.rh, S.sp, "ss_reads_select_strains", &out[i]);
        }
    }
    if (rc)
        for (uint32_t i = 0; i < n_want; i++)
            if (out[i]) { ss_reads_destroy(out[i]); out[i] = nullptr; }
    return rc;
}

}  // extern "C"
