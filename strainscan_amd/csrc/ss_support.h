// What the per-read passes over a resident set share: the hits of every record against a page-index table, left on the device
// (the first two passes of ss_reads_support, ss_support.hip), the records' spans and the gather of a selection into a new set
// (ss_select.hip), the classification (ss_classify.hip) and the slot labels (ss_label.hip).  Not part of the C ABI.
#pragma once
#include "ss_common.h"

#include <algorithm>
#include <chrono>

namespace ss {

constexpr int SUP_TILE = 1024;      // positions per tile: KPOS of scan_minik_kernel (ss_minik.hip), one wave each

// pool allocations of one call, given back on every way out
struct PoolScratch {
    std::vector<void *> p;
    hipError_t get(void **q, size_t bytes)
    {
        const hipError_t e = ss::l2s::dmalloc(q, std::max<size_t>(bytes, 16));
        if (e == hipSuccess) p.push_back(*q);
        return e;
    }
    ~PoolScratch()
    {
        for (void *q : p) (void)ss::l2s::dfree(q);
        if (!p.empty()) (void)ss::l2s::sync();
    }
};

// What rec_hits_of leaves behind.  The records of the set are numbered slab after slab (a slab's records from rec_base on, in
// the order of their ends); rec_hits[i] = hits of record i.  An ASCII slab's tiles begin at tile_base[tile_off + tile]: the
// record ends before the tile, and tile_base[tile_off + n_tiles] = the slab's records.  Everything lives in `scratch` and is
// enqueued on ss::l2s::stream() when the call returns.
struct RecHits {
    struct Part { const ss_reads::Slab *sl; uint64_t n, n_tiles, tile_off, n_rec, rec_base; };
    std::vector<Part> parts;             // the set's slabs that hold positions
    uint64_t tiles_total = 0, rec_total = 0;
    uint32_t *d_tile_base = nullptr;     // [tiles_total], ASCII slabs only
    uint32_t *d_rec_hits = nullptr;      // [n_labels][rec_total] (the plain form: one slice)
    PoolScratch scratch;
};
// SS_ERANGE / SS_EINVAL as ss_reads_support states them; *calls is counted once the arguments have passed.
// The labelled form (d_slot_label != nullptr: [db->n_slots] labels 0..n_labels, ss_label.hip): slice j - 1 of d_rec_hits holds the
// hits whose k-mer has label j.
int rec_hits_of(const ss_db *db, const ss_reads *R, RecHits *out, std::atomic<uint64_t> *calls, const uint8_t *d_slot_label = nullptr,
                uint32_t n_labels = 1);
// pass 1 of rec_hits_of alone: parts, tile bases and the record numbering (d_rec_hits stays nullptr); device < 0: any device
int record_index_of(const ss_reads *R, int device, RecHits *out, std::atomic<uint64_t> *calls);
// pass 3 of ss_reads_support on one slice of rec_hits: hist[n_bins] and *hits (scratch from rh)
int rec_hits_histogram(RecHits *rh, const uint32_t *d_rec_hits, uint32_t n_bins, uint64_t *hist, uint64_t *hits);
// passes 2-4 of ss_reads_select (ss_select.hip) on one slice of rec_hits: the records with at least min_hits there, as a new set
int select_records(RecHits *rh, const uint32_t *d_rec_hits, uint32_t min_hits, ss_reads **out);
// The halves of select_records, which ss_reads_resample (ss_resample.hip) shares.  record_spans_of is pass 2 and the scratch of
// pass 3: start[] / end[] of the records of the ASCII slabs (nullptr when the set has none), len[] and tot[2] = {0, 0}; SS_ERANGE
// for more records than hipcub's int item count holds.  The caller fills len[rec] = copies * (length + 1), the bytes a record
// takes in the new slab, and adds the copies and their bytes to tot[0] and tot[1]; a record whose span does not lie in its slab
// gets 0.  gather_records is the exclusive sum of len[], the new slab and pass 4: every record copied len / (length + 1) times.
// It may be called again on the same spans after len[] and tot[] have been filled anew (ss_reads_select_class, a set per clade):
// the offsets and hipcub's scratch (d_off, d_tmp) are allocated by the first call and kept.
struct RecSpans {
    unsigned long long *d_start = nullptr, *d_end = nullptr, *d_len = nullptr, *d_tot = nullptr;
    unsigned long long *d_off = nullptr;
    void *d_tmp = nullptr;
    size_t tmp_bytes = 0;
};
int record_spans_of(RecHits *rh, RecSpans *sp);
int gather_records(RecHits *rh, RecSpans &sp, const char *who, ss_reads **out);
// The length pass of ss_scan_reads_resampled (ss_resample.hip, beside resample_len_kernel and with its digest and Poisson table):
// len[rec] = the weights the record draws in replicates first .. first + n_rep - 1 of `seed` as 4-bit fields, replicate first + j
// at bits 4 j (n_rep <= 16); a record whose span does not lie in its slab gets 0.  Enqueued on ss::l2s::stream().
int resample_weights_of(RecHits *rh, RecSpans &sp, uint64_t seed, uint32_t first, uint32_t n_rep);
// The resident set that a gather or a join fills (ss_select.hip): n_records records, `total` bytes, in ONE slab allocated from the
// total and padded to a multiple of 16, the '\n' of the padding enqueued.  *slab: where the caller writes the `total` bytes;
// nullptr for total == 0, the valid empty set without a slab.  SS_ENOMEM: no memory; SS_EHIP: the fill failed.  Nothing is left then.
int one_slab_set(uint64_t n_records, uint64_t total, const char *who, ss_reads **out, uint8_t **slab);
// ... and what the calls that fill it do with a HIP error: fail(e) is true, and ss_last_error names `who`, when e is one
struct HipFail {
    const char *who;
    bool operator()(hipError_t e) const
    {
        if (e != hipSuccess) set_last_error(who, __FILE__, __LINE__, e);
        return e != hipSuccess;
    }
};
// the host clock around a step that ends with the stream synchronised
using Clock = std::chrono::steady_clock;
inline double ms_since(Clock::time_point t0) { return std::chrono::duration<double, std::milli>(Clock::now() - t0).count(); }
inline unsigned grid_for(uint64_t items) { return (unsigned)((items + 255u) / 256u); }      // workgroups of 256 threads, one item each

extern std::atomic<uint64_t> g_join_pairs_calls;      // ss_reads_join_pairs_calls (ss_pairs.hip)

// The classification of ss_reads_classify left on the device (ss_classify.hip), which ss_bam_tag.hip runs on the one-slab set
// wrapped around a BAM's flat block.  Forest: device arrays [n_nodes + 1]; entry 0: parent 0, depth 0, an empty interval.
struct Forest {
    const uint32_t *parent, *depth, *tin, *tout;
};
// the records of one slab and where their results go (classify_kernel, classify_long_kernel; the list kernels of ss_calls.hip)
struct ClassArgs {
    const uint16_t *pos_node;                   // the slab's fields
    const unsigned long long *start, *end;      // ASCII slab: spans by record of the set; packed: unused
    uint64_t rec0, n_rec, n;                    // the slab's first record, its records, its positions
    uint32_t slot, fixed_len;                   // packed slab: positions per slot, bases per record; else 0
    uint32_t n_nodes, min_score;
    unsigned long long *direct, *node_hits;     // [n_nodes + 1]
    unsigned long long *tot;                    // [0] records whose class came from a tie, [1] records on the list
    uint32_t *rec_class;                        // [records of the set] or nullptr
    uint32_t *rec_score;                        // [records of the set] or nullptr: the largest score of the record, below min_score too
    uint32_t *long_list;                        // [n_rec] records of this slab (slab-relative) left to the general pass
    unsigned long long *cnt;                    // [n_rec + 1] or nullptr: the listed nodes of every record of this slab (ss_reads_calls)
    uint32_t *stage;                            // [8 * n_rec] or nullptr: the kept nodes of a record of the fast path, node << 16 | hits
};
// The per-record hit lists of ss_reads_calls (ss_calls.hip), which classify_records fills slab by slab while a slab's fields are
// there.  cap: the entries d_node / d_hits hold; n_list: the entries of all records, counted also where they were not written.
struct HitLists {
    uint64_t cap = 0, n_list = 0;
    bool fill = false;                          // the lists are written (until one slab's do not fit any more)
    uint32_t *d_node = nullptr, *d_hits = nullptr;
    unsigned long long *d_first = nullptr;      // [rec_total + 1]
    unsigned long long *d_cnt = nullptr, *d_off = nullptr;      // [max_rec + 1]: of the slab at work
    uint32_t *d_stage = nullptr;                // [8 * max_rec]
    void *d_tmp = nullptr;
    size_t tmp_bytes = 0;
};
// scratch for a set of rec_total records in slabs of at most max_rec records and `positions` positions in all
int hit_lists_begin(HitLists *H, PoolScratch &scratch, uint64_t rec_total, uint64_t max_rec, uint64_t positions);
// behind classify_long_kernel of the slab A, whose pos_node, long_list and tot[1] are still there; d_h: the dense h[] arrays, all zero
int hit_lists_slab(HitLists *H, const ClassArgs &A, uint32_t *d_h, uint32_t long_wgs);
// What classify_records leaves behind: everything on the device lives in rh.scratch and is enqueued on ss::l2s::stream() when
// the call returns.
struct Classified {
    HitLists *lists = nullptr;                // in: where ss_reads_calls wants the hit lists (nobody else asks)
    RecHits rh;
    RecSpans sp;
    Forest F{nullptr, nullptr, nullptr, nullptr};
    unsigned long long *d_out = nullptr;      // direct[n1], node_hits[n1], kmers[n1], tot[2]
    uint32_t *d_class = nullptr;              // [rh.rec_total] the class of every record (keep_class; nullptr for a set without records)
    uint32_t *d_score = nullptr;              // [rh.rec_total] the largest score of every record, below min_score too (keep_score)
    std::vector<uint32_t> tin, tout;          // the host's copy of the Euler intervals
};
// SS_EINVAL / SS_ERANGE as ss_reads_classify states them; *calls (or nullptr) is counted once the arguments have passed.
int classify_records(const ss_db *db, const ss_reads *R, const uint32_t *row_node, uint32_t n_nodes, const uint32_t *parent, uint32_t min_score,
                     bool keep_class, std::atomic<uint64_t> *calls, Classified *C, bool keep_score = false);
// direct / node_hits / kmers [n_nodes + 1] (each nullptr to skip) and *ties (or nullptr) from what classify_records left; synchronous
int classified_counts(const Classified &C, uint32_t n_nodes, uint64_t *direct, uint64_t *node_hits, uint64_t *kmers, uint64_t *ties);

// row labels (host, db->n_rows of them; only != 0: folded to 1 = `only`, 0 = the rest) -> *d_slot_label [db->n_slots] in `scratch`
// (ss_label.hip); SS_EINVAL for a label above n_labels
int slot_labels_for(const ss_db *db, const uint8_t *row_labels, uint32_t n_labels, uint32_t only, PoolScratch &scratch, uint8_t **d_slot_label);

}  // namespace ss
