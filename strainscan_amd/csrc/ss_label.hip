// ss_reads_support_labeled / ss_reads_select_labeled: read support and read selection per LABEL of a table's rows (`--by_strain`).
//
// A cluster table holds every k-mer of all strains of its cluster, so the hits of a read against it say nothing about which of the
// called strains the read belongs to.  The caller labels the table's ROWS (0 = nobody's, j = strain j's alone); this file turns
// the row labels into SLOT labels -- the scan kernel finds slots, not rows -- and runs the passes of ss_reads_support with the
// label sink of scan_minik_kernel (ss_minik.hip), which keeps a hit apart by the label of its slot.
//
//   1. slot_labels_kernel: one thread per row, atomicOr(1 << label) into a 16-bit set per slot (two slots per word).  Rows
//      without a slot are skipped.  OR is commutative: nothing depends on the order in which the rows arrive.
//      slot_labels_finish_kernel: one thread per slot, the set -> the label: the one label of a set with one member, 0 for an
//      empty set and for a set with several (the rows that share the slot disagree: it counts for nobody).  The distinct slots per
//      label are counted on the way (LDS, then one 64-bit atomic per label and workgroup).
//   2. rec_hits_of (ss_support.hip) with the slot labels: passes 1 and 2 of ss_reads_support, rec_hits[n_labels][rec_total].
//   3. per label: rec_hits_histogram (ss_support.hip) or select_records (ss_select.hip) on that label's slice.
// ss_reads_select_labeled needs one label's hits only: it folds the row labels to {0, 1} (1 = `label`) before pass 1 -- a slot
// whose rows disagree is still in conflict after the fold -- and runs everything with a single slice.
// The scratch (2 + 1 bytes per slot, 1 per row, 4 per record and label) comes from the stream-ordered pool.
#include "ss_scan_dev.h"
#include "ss_support.h"

namespace {

__global__ __launch_bounds__(256) void slot_labels_kernel(const uint8_t *__restrict__ row_label, const uint32_t *__restrict__ slot_of_row,
                                                          uint64_t n_rows, uint64_t n_slots, uint32_t *__restrict__ sets)
{
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= n_rows) return;
    const uint32_t sl = slot_of_row[i];
    if (sl == SS_NO_SLOT || sl >= n_slots) return;
    atomicOr(&sets[sl >> 1], 1u << ((uint32_t)(row_label[i] & 15u) + 16u * (sl & 1u)));
}

// sets[] holds n_slots 16-bit sets; out[slot] = its label; n_with[j] += slots of label j (j >= 1)
__global__ __launch_bounds__(256) void slot_labels_finish_kernel(const uint32_t *__restrict__ sets, uint64_t n_slots, uint8_t *__restrict__ out,
                                                                 unsigned long long *__restrict__ n_with)
{
    __shared__ uint32_t cnt[16];
    if (threadIdx.x < 16) cnt[threadIdx.x] = 0u;
    __syncthreads();
    for (uint64_t s = (uint64_t)blockIdx.x * 256u + threadIdx.x; s < n_slots; s += (uint64_t)gridDim.x * 256u) {
        const uint32_t m = (sets[s >> 1] >> (16u * ((uint32_t)s & 1u))) & 0xFFFFu;
        const uint32_t l = (m && !(m & (m - 1u))) ? (uint32_t)__ffs(m) - 1u : 0u;
        out[s] = (uint8_t)l;
        if (l) atomicAdd(&cnt[l], 1u);
    }
    __syncthreads();
    if (threadIdx.x >= 1 && threadIdx.x < 16 && cnt[threadIdx.x]) atomicAdd(&n_with[threadIdx.x], (unsigned long long)cnt[threadIdx.x]);
}

std::atomic<uint64_t> g_labeled_calls{0};

// row labels (host, db->n_rows of them, each <= n_labels; only == `only` kept as 1 when only != 0) -> *d_slot_label [db->n_slots]
// in `scratch`; kmers[j - 1] = slots of label j (may be null)
int slot_labels_of(const ss_db *db, const uint8_t *row_labels, uint32_t n_labels, uint32_t only, ss::PoolScratch &scratch,
                   uint8_t **d_slot_label, uint64_t *kmers)
{
    const uint64_t n_rows = db->n_rows, n_slots = db->n_slots;
    std::vector<uint8_t> folded;
    uint8_t top = 0;
    for (uint64_t i = 0; i < n_rows; i++) top = std::max(top, row_labels[i]);      // (no early exit: the loop vectorises)
    if (top > n_labels) return SS_EINVAL;
    if (only) {
        folded.resize(n_rows);
        for (uint64_t i = 0; i < n_rows; i++) folded[i] = row_labels[i] == only ? 1u : 0u;
        row_labels = folded.data();
    }
    const hipStream_t st = ss::l2s::stream();
    uint8_t *d_rows = nullptr, *d_lab = nullptr;
    uint32_t *d_sets = nullptr;
    unsigned long long *d_with = nullptr;
    const uint64_t set_bytes = ((n_slots + 1) / 2) * 4;
    SS_HIP(scratch.get((void **)&d_rows, n_rows));
    SS_HIP(scratch.get((void **)&d_sets, set_bytes));
    SS_HIP(scratch.get((void **)&d_lab, n_slots));
    SS_HIP(scratch.get((void **)&d_with, 16 * 8));
    SS_HIP(ss::l2s::set(d_sets, 0, std::max<uint64_t>(set_bytes, 16)));
    SS_HIP(ss::l2s::set(d_with, 0, 16 * 8));
    if (n_rows) {
        SS_HIP(ss::l2s::copy(d_rows, row_labels, n_rows, hipMemcpyHostToDevice));
        hipLaunchKernelGGL(slot_labels_kernel, dim3((unsigned)((n_rows + 255) / 256)), dim3(256), 0, st, d_rows, db->d_slot_of_row, n_rows, n_slots, d_sets);
        SS_HIP(hipGetLastError());
    }
    if (n_slots) {
        const unsigned blocks = (unsigned)std::min<uint64_t>((n_slots + 256 * 8 - 1) / (256 * 8), 4096);
        hipLaunchKernelGGL(slot_labels_finish_kernel, dim3(blocks), dim3(256), 0, st, d_sets, n_slots, d_lab, d_with);
        SS_HIP(hipGetLastError());
    }
    unsigned long long with[16];
    SS_HIP(ss::l2s::copy(with, d_with, sizeof with, hipMemcpyDeviceToHost));
    if (kmers)
        for (uint32_t j = 1; j <= n_labels; j++) kmers[j - 1] = with[j];
    *d_slot_label = d_lab;
    return SS_OK;
}

}  // namespace

// (ss_support.h: ss_bam_select obtains its slot labels here, as ss_reads_select_labeled does)
int ss::slot_labels_for(const ss_db *db, const uint8_t *row_labels, uint32_t n_labels, uint32_t only, PoolScratch &scratch, uint8_t **d_slot_label)
{
    return slot_labels_of(db, row_labels, n_labels, only, scratch, d_slot_label, nullptr);
}

extern "C" {

int ss_reads_labeled_calls(uint64_t *n)
{
    if (!n) return SS_EINVAL;
    *n = g_labeled_calls.load();
    return SS_OK;
}

int ss_reads_support_labeled(const ss_db *db, const ss_reads *R, const uint8_t *row_labels, uint32_t n_labels, uint32_t n_bins,
                             uint64_t *hist, uint64_t *hits, uint64_t *kmers)
{
    if (!db || !R || !row_labels || !hist || !hits || !kmers || n_bins < 2 || n_labels < 1 || n_labels > SS_LABELS_MAX) return SS_EINVAL;
    if (db->layout != 1) return SS_ERANGE;                          // page-index tables only
    if (R->has_cut_record && db->k != 31) return SS_ERANGE;         // (as ss_reads_support)
    ss::RecHits rh;
    uint8_t *d_lab = nullptr;
    int rc = slot_labels_of(db, row_labels, n_labels, 0, rh.scratch, &d_lab, kmers);
    if (rc) return rc;
    rc = ss::rec_hits_of(db, R, &rh, &g_labeled_calls, d_lab, n_labels);
    for (uint32_t j = 0; j < n_labels && !rc; j++)
        rc = ss::rec_hits_histogram(&rh, rh.d_rec_hits + (uint64_t)j * rh.rec_total, n_bins, hist + (uint64_t)j * n_bins, hits + j);
    return rc;
}

int ss_reads_select_labeled(const ss_db *db, const ss_reads *R, const uint8_t *row_labels, uint32_t n_labels, uint32_t label,
                            uint32_t min_hits, ss_reads **out)
{
    if (!db || !R || !row_labels || !out || min_hits == 0 || n_labels < 1 || n_labels > SS_LABELS_MAX || label < 1 || label > n_labels)
        return SS_EINVAL;
    if (db->layout != 1) return SS_ERANGE;                          // page-index tables only
    if (R->has_cut_record) return SS_ERANGE;                        // (as ss_reads_select)
    ss::RecHits rh;
    uint8_t *d_lab = nullptr;
    int rc = slot_labels_of(db, row_labels, n_labels, label, rh.scratch, &d_lab, nullptr);
    if (rc) return rc;
    rc = ss::rec_hits_of(db, R, &rh, &g_labeled_calls, d_lab, 1);
    if (rc) return rc;
    return ss::select_records(&rh, rh.d_rec_hits, min_hits, out);
}

}  // extern "C"
