// ss_scan_reads_resampled: the counts of several bootstrap replicates from one pass over a resident set (`--bootstrap_clusters`).
//
// ss_reads_resample materialises a replicate: every record copied w times into a new set, which is then binned and scanned.  The
// scan never needed the copies -- a replicate's count for a k-mer is the sum of the weights of the records that carry it -- so
// here the reads are fetched ONCE and a hit adds its record's weight to the counters of up to sixteen replicates.
//
// The passes, each a plain launch on the calling thread's stream:
//   1. record_index_of, record_spans_of (ss_support.h): the records numbered and their spans, as ss_reads_resample has them.
//   2. resample_weights_of (ss_resample.hip) -- a record per lane, beside resample_len_kernel and with its digest and table: one
//      64-bit word per record, the weight of replicate first + j in bits 4 j .. 4 j + 3 (w <= 13).
//   3. scan_minik_kernel<.., WeightSink> (ss_minik.hip): the lookups of the per-position scan kernel.  The sink finds the record
//      of a hit from the tile's record directory, loads its word and issues one atomicAdd per field that is not zero into
//      slot counters of the replicates' own, [n][n_slots] of scratch.
//   4. replicate_rows_kernel: every replicate's slot counters to its row vector, as ss_counts_rows_dev does for the table's.
// The table's own counters are never read or written.
#include "ss_scan_dev.h"
#include "ss_support.h"

using namespace ss::dev;

namespace {

// out[j * n_rows + i] = replicate j's count of row i: gather_rows_kernel (ss_scan.hip) over n_rep slices of slot counters
__global__ __launch_bounds__(256) void replicate_rows_kernel(const uint32_t *__restrict__ counts, uint64_t stride, const uint32_t *__restrict__ slot_of_row,
                                                             const uint8_t *__restrict__ row_valid, uint64_t n_rows, uint32_t n_rep,
                                                             uint32_t *__restrict__ out)
{
    for (uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x; i < n_rows; i += (uint64_t)gridDim.x * 256u) {
        const bool valid = row_valid[i] != 0;
        const uint64_t s = valid ? slot_of_row[i] : 0u;
        for (uint32_t j = 0; j < n_rep; j++) out[(uint64_t)j * n_rows + i] = valid ? counts[(uint64_t)j * stride + s] : 0u;
    }
}

std::atomic<uint64_t> g_scan_resampled_calls{0};

}  // namespace

extern "C" {

int ss_scan_reads_resampled_calls(uint64_t *n)
{
    if (!n) return SS_EINVAL;
    *n = g_scan_resampled_calls.load();
    return SS_OK;
}

int ss_scan_reads_resampled(const ss_db *db, const ss_reads *R, uint64_t seed, uint32_t first_replicate, uint32_t n_replicates,
                            uint32_t *counts_rows_dev)
{
    if (!db || !R || !counts_rows_dev || n_replicates < 1 || n_replicates > SS_SCAN_REPLICATES_MAX) return SS_EINVAL;
    if (db->layout != 1) return SS_ERANGE;                          // page-index tables only
    if (R->has_cut_record) return SS_ERANGE;                        // a cut piece is not a read
    ss::RecHits rh;
    ss::RecSpans sp;
    int rc = ss::record_index_of(R, db->device, &rh, &g_scan_resampled_calls);
    if (rc) return rc;
    rc = ss::record_spans_of(&rh, &sp);
    if (rc) return rc;
    const hipStream_t st = ss::l2s::stream();
    const uint64_t stride = db->n_slots, n_rows = db->n_rows;
    if (!n_rows) return SS_OK;
    if (!rh.rec_total) {                                            // no records: every count is zero
        SS_HIP(ss::l2s::set(counts_rows_dev, 0, (size_t)n_replicates * n_rows * 4));
        SS_HIP(ss::l2s::sync());
        return SS_OK;
    }
    // 2. the weights (in the spans' len[], one 64-bit word per record)
    rc = ss::resample_weights_of(&rh, sp, seed, first_replicate, n_replicates);
    if (rc) return rc;
    const unsigned long long *d_w = sp.d_len;
    // 3. the hits, weighted, into the replicates' slot counters
    uint32_t *d_counts = nullptr;
    const size_t counts_bytes = (size_t)n_replicates * stride * 4;
    SS_HIP(rh.scratch.get((void **)&d_counts, counts_bytes));
    SS_HIP(ss::l2s::set(d_counts, 0, std::max<size_t>(counts_bytes, 16)));
    for (const auto &pt : rh.parts) {
        if (pt.n < (uint64_t)db->k || !pt.n_rec) continue;
        const ss::ResampledArgs a{d_counts, stride, (const uint64_t *)d_w, pt.sl->packed ? nullptr : rh.d_tile_base + pt.tile_off,
                                  pt.rec_base, rh.rec_total, pt.sl->packed ? pt.sl->slot : 0u};
        rc = ss::launch_resampled_minik(db, pt.sl->d, pt.n, pt.sl->packed, a, st);
        if (rc) return rc;
    }
    // 4. slots -> rows, replicate after replicate
    const unsigned blocks = (unsigned)std::min<uint64_t>((n_rows + 255) / 256, 65536);
    hipLaunchKernelGGL(replicate_rows_kernel, dim3(blocks), dim3(256), 0, st, d_counts, stride, db->d_slot_of_row, db->d_row_valid, n_rows,
                       n_replicates, counts_rows_dev);
    SS_HIP(hipGetLastError());
    SS_HIP(ss::l2s::sync());
    return SS_OK;
}

}  // extern "C"
