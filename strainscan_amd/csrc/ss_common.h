// Internal helpers shared by the gfx950 translation units.  Not part of the C ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <atomic>
#include <functional>
#include <vector>
#include <string.h>

#include "strainscan_hip.h"

namespace ss {

void set_last_error(const char *what, const char *file, int line, hipError_t e);

#define SS_HIP(call)                                               \
    do {                                                           \
        hipError_t _e = (call);                                    \
        if (_e != hipSuccess) {                                    \
            ss::set_last_error(#call, __FILE__, __LINE__, _e);     \
            return (_e == hipErrorOutOfMemory) ? SS_ENOMEM         \
                   : (_e == hipErrorNoDevice)  ? SS_ENODEV         \
                                               : SS_EHIP;          \
        }                                                          \
    } while (0)

constexpr uint64_t EMPTY_KEY = ~0ull;

// Table hash.  Two odd multipliers with a fold in between: the keys are overlapping windows of
// genomes (key[p+1] = key[p] >> 2 | base << 2(k-1)), so a single multiplicative hash would map
// neighbouring windows to related slots.
__host__ __device__ __forceinline__ uint64_t mix64(uint64_t x)
{
    x *= 0x9E3779B97F4A7C15ull;
    x ^= x >> 32;
    x *= 0xD6E8FEB86659FD93ull;
    x ^= x >> 29;
    return x;
}

__host__ __device__ __forceinline__ uint32_t slot_of(uint64_t key, uint32_t log2cap)
{
    return (uint32_t)(mix64(key) >> (64 - log2cap));
}
// flat layout's Bloom filter (ss_scan.hip): bit index from the LOW half of the same mix (the table slot takes the top bits)
__host__ __device__ __forceinline__ uint32_t bloom_bit_of(uint64_t mixed, uint32_t bloom_bits)
{
    return (uint32_t)(mixed & 0xFFFFFFFFull) >> (32 - bloom_bits);
}

// ascii -> 2-bit code ((c >> 1) & 3: A0 C1 T2 G3) or -1
__host__ __device__ __forceinline__ int base_code(unsigned char c)
{
    unsigned char u = c & 0xDF;
    if (u == 'A' || u == 'C' || u == 'G' || u == 'T') return (c >> 1) & 3;
    return -1;
}

inline hipStream_t as_stream(void *s) { return (hipStream_t)s; }

// CPUs this process may really use: hardware threads, capped by the cgroup's CPU quota (v2 cpu.max, v1 cfs quota).
// A container with 16 CPUs of quota on a 256-thread host runs 64 busy threads SLOWER than 16 (CFS throttles the
// whole group once the quota of a period is spent).
unsigned host_cpus();
extern std::atomic<long long> g_hook_generic_k;      // ss_test_hook 4 (ss_mini.hip)
unsigned ingest_threads();      // FASTQ parse threads of this process: its share of host_cpus() (LOCAL_WORLD_SIZE), at most 20 (ss_ingest.hip)
// The base-quality mask (ss_set_min_base_qual, ss_host.hip): a base whose Phred quality is below the threshold becomes 'N' in
// whichever decoder turns its file into bases.  0 = off.  mask_count adds to the process-wide counters of ss_mask_counters.
int min_base_qual();
void mask_count(uint64_t bases, uint64_t records_without_qual = 0);

}  // namespace ss

// The opaque database handle.
struct ss_db {
    int k = 0;
    int device = 0;
    uint64_t n_rows = 0;
    uint64_t n_distinct = 0;
    uint32_t log2cap = 0;
    uint64_t capacity = 0;
    int layout = 0;                    // 0 = flat open-address table, 1 = minimizer pages (17 <= k <= 31)
    uint64_t n_slots = 0;              // length of d_counts: capacity (flat) or n_mslots + 8 * n_dir (pages)
    uint64_t n_mslots = 0;             // pages: length of d_mkeys (bucket headers + k-mers)
    uint64_t n_inline = 0;             // pages: database k-mers held inline in page slots
    uint64_t *d_keys = nullptr;        // flat: [capacity] table keys, EMPTY_KEY where free
    uint64_t *d_mkeys = nullptr;       // pages: [n_mslots] buckets of the minimizers with many k-mers (ss_mini.hip)
    uint64_t *d_dir = nullptr;         // pages: [n_dir][8] 64-byte pages of slots (inline k-mers, bucket references)
    uint32_t dirbits = 0;
    uint32_t n_dir = 0;                // pages: number of home pages (range of page_of)
    uint32_t n_dir_alloc = 0;          // pages: home pages + spare pages behind them (overflow never wraps)
    uint32_t *d_bloom = nullptr;       // buckets: one-probe Bloom filter over the minimizers (L2 resident), or null
    uint32_t bloom_bits = 0;           // log2 of its size in bits
    uint64_t n_buckets = 0;
    uint32_t *d_counts = nullptr;      // [n_slots] occurrences per slot (accumulated by scans)
    int expect_hits = 0;               // ss_db_expect_hits: most read k-mers are in the table (a layer-2 cluster table)
    uint64_t probe_set = 0;            // the resident read set (ss_reads::serial) whose first tiles were last probed against this
    int probe_comb = 0;                // table, and what they said: add the hits up in LDS (ss_mini.hip launch_scan_mini)
    double probe_runs_per_tile = 0;    // found runs per tile of that probe (ss_db_info_ex)
    uint32_t *d_slot_of_row = nullptr; // [n_rows]   slot owning row i, SS_NO_SLOT if none
    uint8_t *d_row_valid = nullptr;    // [n_rows]   1 iff row i is a key of match_results
    // pinned staging for host-resident base blocks
    char *h_stage[2] = {nullptr, nullptr};
    char *d_stage[2] = {nullptr, nullptr};
    uint64_t stage_bytes = 0;
    hipStream_t streams[2] = {nullptr, nullptr};
    hipEvent_t stage_free[2] = {nullptr, nullptr};
    std::atomic<uint64_t> launches{0};
    // per-worker resources of the parallel ingest path (allocated on first use, kept for the handle's life)
    struct Worker { char *h_buf = nullptr; char *d_buf = nullptr; hipEvent_t done = nullptr; uint64_t cap = 0;
                    char *t_buf = nullptr; uint64_t t_cap = 0; };   // t_buf: private copy of the text chunk being parsed;
                                                                    // done: this worker's last copy/kernel has finished
    static constexpr int MAX_WORKERS = 64;
    Worker workers[MAX_WORKERS];
    static void free_workers(Worker *w, int n);
    uint64_t device_bytes = 0;
};

#include <chrono>
#include <mutex>

// A sample's reads resident in HBM (ss_ingest.hip loads them, ss_reorder.hip orders them for locality).
namespace ss { hipError_t big_malloc(void **p, uint64_t bytes, uint64_t *got = nullptr); void big_put(void *p, uint64_t cap); bool ingest_trace(); }      // (below)
struct ss_reads {
    // Blocks live back to back in a few large device slabs; every block is followed by at least one '\n'
    // and padded with '\n' to a multiple of 16 bytes, so a slab is itself one flat base block: one scan
    // launch per slab (one in all for a typical sample) instead of one per 12 MB block, and no device
    // allocation per block while loading.
    // binned: ss_reorder.hip has ordered its records.  packed: ... and holds them as 2-bit codes + invalid flags, 3 bytes per 8
    // positions (ss_scan_dev.h IN_PACKED): n_pos positions (a multiple of 16) in `used` bytes, every record L bases in a slot of
    // `slot` positions, the slots back to back from position 0.  Scans take positions(): the length of the block in bases, whichever the layout.
    struct Slab {
        char *d = nullptr; uint64_t cap = 0, used = 0; bool binned = false;
        bool packed = false; uint64_t n_pos = 0; uint32_t L = 0, slot = 0;
        uint64_t positions() const { return packed ? n_pos : used; }
    };
    std::vector<Slab> slabs;
    std::mutex mu;
    uint64_t n_records = 0, n_bases = 0, device_bytes = 0, n_blocks = 0;
    bool records_counted = true;      // false: made from a flat block (ss_reads_from_flat_dev); ss_reads_info counts the records when asked
    bool has_cut_record = false;      // a record longer than a block was cut with a 30-base overlap (k = 31 only)
    uint64_t first_slab = 0;          // size of the first slab (estimate from the file sizes)
    uint64_t serial = next_serial();  // names this set: a table remembers which set it was last probed with
    static uint64_t next_serial() { static std::atomic<uint64_t> c{0}; return ++c; }

    static uint64_t padded(uint64_t len) { return (len + 1 + 15) & ~15ull; }
    // a flat block that is already on the device (hipMalloc'ed, padded as above) becomes a slab of its own
    void adopt(char *d, uint64_t cap, uint64_t len)
    {
        std::lock_guard<std::mutex> g(mu);
        Slab sl;
        sl.d = d; sl.cap = cap; sl.used = padded(len);
        if (!slabs.empty() && slabs.back().used < slabs.back().cap) slabs.insert(slabs.end() - 1, sl);      // the open slab stays last
        else slabs.push_back(sl);
        device_bytes += cap;
        n_blocks++;
    }
    // room for a block of `len` bytes (+ padding); nullptr when the device is out of memory
    char *reserve(uint64_t len)
    {
        const uint64_t need = padded(len);
        std::lock_guard<std::mutex> g(mu);
        if (slabs.empty() || slabs.back().used + need > slabs.back().cap) {
            Slab sl;
            sl.cap = std::max<uint64_t>(need, slabs.empty() ? std::max<uint64_t>(first_slab, 64ull << 20) : 512ull << 20);
            const auto t0 = std::chrono::steady_clock::now();
            if (ss::big_malloc((void **)&sl.d, sl.cap, &sl.cap) != hipSuccess) return nullptr;
            if (ss::ingest_trace())
                fprintf(stderr, "[ingest] slab of %.0f MB: %.4f s\n", sl.cap / 1e6,
                        std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count());
            slabs.push_back(sl);
        }
        Slab &sl = slabs.back();
        char *p = sl.d + sl.used;
        sl.used += need;
        device_bytes += need;
        n_blocks++;
        return p;
    }
};


namespace ss {
// Records of every slab re-ordered by the minimizer of their first k-mer (ss_reorder.hip); `force`: ignore SS_READS_ORDER
int reads_order_for_locality(ss_reads *R, bool force = false);
// src[0, n) -> *out: a new binned slab (d, cap, used, binned, packed, n_pos, L); packed where its records may be (ss_test_hook 5)
int order_flat_dev(const char *src, uint64_t n, ss_reads::Slab *out);
extern std::atomic<long long> g_hook_ascii_slabs;      // ss_test_hook 5 (ss_reorder.hip): 1 = binned slabs stay ASCII
extern std::atomic<long long> g_hook_atomic_binning;   // ss_test_hook 6 (ss_reorder.hip): 1 = one-length slabs take the count + atomic placement
void reorder_release();
void reorder_counters(uint64_t out[2]);      // slabs binned by the one-length passes / by the general ones, in this process
void reorder_timing(double out[3]);      // the last binning call (ms): key + sort, slab allocation, gather + tail (the sorted one-length path); else count + prefix, slab allocation, place      // the binning scratch kept between calls goes back to the device (ss_gz_gpu_release)
// the page index built on the host (ss_mini_build.hip), after the device build has had its turn
int build_mini(ss_db *db, const uint64_t *keys, const uint8_t *flags, uint64_t n_rows, int upper_keys);
// the same index built on the device (ss_build_dev.hip); anything but SS_OK / SS_EKEY: nothing was built, use the host build
int build_mini_dev(ss_db *db, const uint64_t *keys, const uint8_t *flags, uint64_t n_rows, int upper_keys);
int mark_solid(ss_db *db);      // PG_SOLID flags of the bucket references, after either build (ss_mini_build.hip)
struct InflatedText { char *p = nullptr; uint64_t n = 0; };
bool inflate_whole(const char *path, uint64_t budget, char **text, uint64_t *len, int mode, unsigned threads);
uint64_t inflate_budget_bytes();
// gzip member header -> offset of the deflate data, 0 = not a header this code handles (ss_pgz.hip)
uint64_t gzip_header_len(const uint8_t *p, uint64_t n);
hipStream_t ingest_stream(unsigned i);   // a few process-wide non-blocking streams (creating one costs ~13 ms)
void free_later(char *p);
bool ingest_trace();                     // SS_INGEST_TRACE, read once: the "[ingest]" stage lines of ss_ingest.hip and ss_scan.hip
// the gzip inputs `gz` (indices into paths) inflated whole on the host, all at once: texts[i] where it worked, left empty where not
void inflate_gz_inputs(const char *const *paths, const std::vector<int> &gz, std::vector<InflatedText> &texts);
// unless SS_GZ_GPU=0: .gz inputs are inflated on the device (ss_ginflate.hip) and strict four-line FASTQ is turned into the flat
// base block there (ss_fastq_dev.hip)
bool gz_on_gpu();
int gz_policy();                         // ss_gz_set_policy: 0 device then host, 1 device or SS_EAGAIN, 2 host
bool gpu_gunzip(const uint8_t *in, uint64_t in_n, char **text_dev, uint64_t *len, void **lease, int fd);      // the text is lent until ...
void gpu_gunzip_done(void *lease);                          // (ss_gz_scratch.hip: the lease is the call's scratch arena)
// a non-blocking stream for the length of a call, from a small pool (making and destroying one is ~0.6 ms); handed back synchronised
hipStream_t call_stream_get();
void call_stream_put(hipStream_t s);
// range mode (ss_gz_set_range, ss_gz_range.hip): this rank's slices of a member.  text[at, at + len) is a slice's text, its first `keep` bytes
// end with the last record that is complete in it, `carry` holds the bytes of the record that began in the slice before
struct GzPiece { uint64_t at, len, keep; std::vector<uint8_t> carry; };
bool gz_range_active();
extern std::atomic<long long> g_hook_entry, g_hook_decline, g_hook_skip_chain;      // ss_test_hook 1, 2 (ss_ginflate.hip), 3 (ss_gz_range.hip)
// The files of a load go down the chain in the order of their paths (the messages of one pair of ranks are matched in order): a
// file draws a ticket (in path order, before its thread starts), its first chain call waits for the files before it to have
// finished THEIR chain traffic, and gz_range_pass hands the turn on (idempotent; waits for the turn itself if the file never
// used it).  What a file does before its first chain call -- upload, search, the inflation of its first slice -- runs beside
// the chain of the file in front of it: both mates of a pair are in flight on every rank.
uint64_t gz_range_ticket();
void gz_range_pass(uint64_t ticket);
bool gpu_gunzip_range(const uint8_t *in, uint64_t in_n, char **text_dev, void **lease, int fd, std::vector<GzPiece> *pieces,
                      uint64_t ticket, bool decline = false);      // decline: test hook -- plan the slices, serve the chain, hand nothing back
int gz_fastq_pieces_dev(const char *path, uint64_t ticket, const std::function<int(char *, uint64_t, uint64_t, uint64_t)> &flat);
int gz_fastq_to_flat_dev(const char *path, int shard_rank, int shard_world, char **d_flat, uint64_t *flat_len, uint64_t *flat_cap,
                         uint64_t *n_records, char **text, uint64_t *text_len);
// the gzip inputs `gz` (indices into paths) through gz_fastq_to_flat_dev, one host thread per file (range mode:
// gz_fastq_pieces_dev): `flat(d_flat, len, cap, n_records)` takes over a device buffer (called from that file's thread; returns
// an SS_* code); inputs that were only inflated come back as host texts in `texts`; done[i] = 1 for the inputs that need nothing
// more.  Nothing happens under SS_GZ_GPU=0.  SS_EAGAIN: strict policy and the device declined one (every chain has been served).
int gz_inputs_on_device(const char *const *paths, const std::vector<int> &gz, int shard_rank, int shard_world,
                        const std::function<int(char *, uint64_t, uint64_t, uint64_t)> &flat, std::vector<InflatedText> &texts,
                        std::vector<char> &done);
// What an input path holds (ss_ingest.hip), from ONE look at its first 64 KB: the magic, and for a gzip file the start of its
// first member ("BAM\1": BGZF or any gzip around a BAM stream).  "" is the absent second mate; a path that cannot be read counts
// as text (the reader reports it).  Values up to INPUT_CRAM are those of ss_input_kind.
enum InputKind { INPUT_TEXT = 0, INPUT_BAM_GZ = 1, INPUT_BAM_RAW = 2, INPUT_CRAM = 3, INPUT_GZ = 4, INPUT_EMPTY = 5 };
int input_kind(const char *path);
// What a consumer of input files does with their flat base blocks: ss_scan_files_shard scans them into a table, ss_reads_load
// keeps them.  ingest_inputs sends every input down the ladder -- BAM, .gz on the device, .gz inflated on the host, the chunked
// parse, the sequential reader -- and hands each block to the entry of the rung it came from.  `records` / `bases` add up what
// was handed over (the reader entry counts its own blocks).
struct InputSink {
    std::atomic<uint64_t> records{0}, bases{0};
    // chunked parse (parse_text_parallel): the workers whose pinned buffers it uses; copy: it copies each block to the worker's
    // device buffer before parsed_block sees it
    ss_db::Worker *workers = nullptr;
    bool copy = true;
    // sequential reader: records longer than a block are cut with this overlap into blocks of reader_cap bytes; block b of file f
    // is the rank's own when (b + (reader_shard_by_file ? f : 0)) % shard_world == shard_rank; one thread per file, or one file
    // after the other
    int reader_overlap = 30;
    uint64_t reader_cap = 32ull << 20;
    bool reader_shard_by_file = false, reader_threads = false;
    // a flat block already on the device, padded like a block of ss_reads (a BAM: big_malloc'ed; a .gz reduced to its sequence
    // lines: hipMalloc'ed): the sink owns it from here (ss_reads::adopt takes either: big_put, which lets a set's slabs go, frees
    // what it does not keep with hipFree).  May be called from several threads at once.
    virtual int device_block(int kind, char *d, uint64_t len, uint64_t cap) = 0;
    // a parse worker's block: h_buf pinned (64 bytes of slack behind len), d_buf its copy when `copy`, enqueued on `stream`
    virtual int parsed_block(const char *h_buf, char *d_buf, uint64_t len, hipStream_t stream) = 0;
    // where the reader of `file` puts its next block (room for reader_cap bytes), then that block: every block of the file is
    // shown, `mine` says whether it is this rank's
    virtual int reader_buffer(int file, char **buf) = 0;
    virtual int reader_block(int file, char *buf, uint64_t len, uint64_t n_records, bool mine) = 0;
    virtual ~InputSink() = default;
};
int ingest_inputs(const char *const *paths, int n_paths, int shard_rank, int shard_world, InputSink &sink);
// (packed: the block is a packed binned slab, n counts its positions -- ss_scan_dev.h IN_PACKED)
int launch_scan_mini(ss_db *db, const void *bases_dev, uint64_t n, hipStream_t stream, bool binned = false, uint64_t set_id = 0,
                     bool packed = false);
int launch_scan_mini_multi(ss_db *const *dbs, int n_dbs, const void *bases_dev, uint64_t n, hipStream_t stream, bool binned,
                           bool packed = false);
// ss_reads_support (ss_support.hip): the lookups of one slab with the per-record sink of scan_minik_kernel (ss_minik.hip).  A found
// k-mer adds 1 to rec_hits[rec_base + record of its start position]; records at or beyond rec_limit are never written.
struct SupportArgs {
    uint32_t *rec_hits;             // [rec_limit] hits per record of the set
    const uint32_t *tile_base;      // ASCII slab: record ends before each 1024-position tile of the slab; packed: unused
    uint64_t rec_base, rec_limit;   // records of the slabs before this one; records of the set
    uint32_t slot;                  // packed slab: positions per record
};
int launch_support_minik(const ss_db *db, const void *bases_dev, uint64_t n, bool packed, const SupportArgs &a, hipStream_t stream);
// ss_reads_support_labeled (ss_label.hip): the same with the label sink.  slot_label[n_slots] (indexed like d_counts) is 0 or
// 1..n_labels; a found k-mer of label j adds 1 to a.rec_hits[(j - 1) * a.rec_limit + record]; label 0 counts nowhere.
int launch_label_minik(const ss_db *db, const void *bases_dev, uint64_t n, bool packed, const SupportArgs &a, const uint8_t *slot_label,
                       uint32_t n_labels, hipStream_t stream);
// ss_reads_classify (ss_classify.hip): the same with the class sink.  slot_node[n_slots] (indexed like d_counts) is 0 or
// 1..n_nodes; pos_node[p] = the node of the k-mer found at position p of the slab (0: no hit, or a hit without a node), written for
// every position of every tile: room for ((n + 1023) / 1024) * 1024 fields, 16-byte aligned.  *hits0 += the hits without a node.
int launch_class_minik(const ss_db *db, const void *bases_dev, uint64_t n, bool packed, uint16_t *pos_node, const uint16_t *slot_node,
                       unsigned long long *hits0, hipStream_t stream);
// ss_scan_reads_resampled (ss_scan_resampled.hip): the same with the weight sink.  A found k-mer adds the weights of its record,
// one per replicate, to the replicates' slot counters: counts[j * stride + slot] += (weights[record] >> 4 j) & 15, slot indexed like
// d_counts.  The record of a position is found as the support sink finds it; records at or beyond rec_limit add nothing.
struct ResampledArgs {
    uint32_t *counts;               // [n_replicates][stride] slot counters of the replicates, cleared by the caller
    uint64_t stride;                // >= the table's n_slots
    const uint64_t *weights;        // [rec_limit] sixteen 4-bit weights per record of the set, replicate j at bits 4 j
    const uint32_t *tile_base;      // ASCII slab: record ends before each 1024-position tile of the slab; packed: unused
    uint64_t rec_base, rec_limit;   // records of the slabs before this one; records of the set
    uint32_t slot;                  // packed slab: positions per record
};
int launch_resampled_minik(const ss_db *db, const void *bases_dev, uint64_t n, bool packed, const ResampledArgs &a, hipStream_t stream);
// the scan of one table through the same kernel (ss_minik.hip): launch_scan_mini sends it the tables it does not take itself
int launch_scan_minik(ss_db *db, const uint8_t *bases_dev, uint64_t n, hipStream_t stream, bool packed);
// the filter kind of a table in a several-tables pass: its own Bloom filter (a tree table), none because it expects hits (a cluster
// table: the combining variant under binned reads), or none at all.  One launch takes tables of one kind (ss_scan_multi_launches).
enum { MULTI_BLOOM = 0, MULTI_EXPECT = 1, MULTI_PLAIN = 2 };
int multi_kind(const ss_db *db);
bool may_share_pass(const ss_db *db);      // may go through launch_scan_mini_multi, with tables of its k and kind (ss_mini.hip)
// Layer 2 (ss_l2.hip, ss_enet.hip) works on the CALLING THREAD's own stream and takes its temporaries from the stream-ordered
// pool (round 5): the clusters of a sample are solved on several host threads at once, and on the legacy default stream every
// synchronous copy of one thread waited for the kernels of all the others, every hipFree for the whole device (four 5 M-row
// clusters: 36 ms each in the O(K) vector pass that takes 5.5 ms alone).  Buffers that live in a handle stay with hipMalloc.
// the stream-ordered pool keeps at least `bytes` of what its users free (raised, never lowered: ss_host.hip)
void pool_keep_at_least(uint64_t bytes);
namespace l2s {
inline hipStream_t stream() { return hipStreamPerThread; }
hipError_t dmalloc(void **p, size_t n);          // (ss_host.hip: sets the pool's release threshold once)
inline hipError_t dfree(void *p) { return p ? hipFreeAsync(p, stream()) : hipSuccess; }
inline hipError_t copy(void *d, const void *s_, size_t n, hipMemcpyKind k)
{
    const hipError_t e = hipMemcpyAsync(d, s_, n, k, stream());
    return e != hipSuccess ? e : hipStreamSynchronize(stream());
}
inline hipError_t set(void *d, int v, size_t n) { return hipMemsetAsync(d, v, n, stream()); }
inline hipError_t sync() { return hipStreamSynchronize(stream()); }
}  // namespace l2s
// Large device blocks a load is done with (the text of a big .gz, the file-order slab that binning has replaced) are kept for
// the next large request of the same process instead of going back to the driver: a fresh process is handed device memory at
// ~25 GB/s and a 50 M-read .gz pair asked for ~47 GB of it, a third of that for blocks that replace each other (ss_host.hip).
// big_take: a kept block of at least `bytes` (and at most 2.5 x), or nullptr; the caller owns it and gives it back with
// big_put or hipFree.  big_put keeps blocks of 256 MB and more, at most three and 24 GB, and frees what it does not keep.
constexpr uint64_t BIG_KEEP_MIN = 256ull << 20;           // blocks big_put keeps (smaller ones go back to the driver)
void *big_take(uint64_t bytes, uint64_t *cap = nullptr);      // *cap: what the block really holds (the caller keeps that, for the next big_put)
void big_put(void *p, uint64_t cap);
void big_release();                                      // everything kept goes back to the driver (ss_gz_gpu_release)
hipError_t big_malloc(void **p, uint64_t bytes, uint64_t *got);      // big_take, else hipMalloc (which, failing, is tried again after big_release); *got >= bytes
// a whole file into device memory through the pinned upload buffers of the .gz path (ss_gz_scratch.hip)
bool upload_file_to_device(int fd, uint64_t n, uint8_t *d_dst);
// ss_scan_flat_dev for a block whose records ss_reorder.hip has binned by locus (the scan may add hits up in LDS first)
// (set_id: ss_reads::serial of the resident set the block belongs to, 0 = none)
// (packed: a packed binned slab of n positions, ss_scan_dev.h IN_PACKED)
int scan_flat_dev(ss_db *db, const void *bases_dev, uint64_t n, void *stream, bool binned, uint64_t set_id = 0, bool packed = false);
}  // namespace ss
