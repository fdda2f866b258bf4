// What the BAM translation units share: the decode path of ss_bam_dev.hip that the loader enters through bam_input (ss_ingest.hip),
// the record-level steps that ss_bam_extract.hip, ss_bam_pairs.hip and ss_bam_tag.hip take from each other, and the output path of
// ss_bam_out.hip.  Not part of the C ABI.
#pragma once
#include "ss_support.h"

namespace ss {

// one BAM input (INPUT_BAM_GZ or INPUT_BAM_RAW) of a load or a scan (ss_bam_dev.hip): on the device unless SS_GZ_GPU=0 or policy
// 2, on the host for what the device declines (policy 0 and 2; policy 1: SS_EAGAIN).  on_dev takes over a big_malloc'ed device
// block (len, cap, n_records), on_host a malloc'ed host block padded like a block of ss_reads (len, n_records; the callee frees
// it).  SS_EIO: damaged.
int bam_input(const char *path, int kind, int shard_rank, int shard_world, const std::function<int(char *, uint64_t, uint64_t, uint64_t)> &on_dev,
              const std::function<int(char *, uint64_t, uint64_t)> &on_host);
// The steps of that path that the other BAM files take on their own (ss_bam_dev.hip).  BamRecords: what a caller of bam_to_flat_dev
// may keep -- record r of the stream starts at d_rec[r] (n_rec of them), d_keep[r] says whether the loader keeps it and d_kidx[r] is
// its ordinal among the kept ones, so kept record i is non-empty record i of the flat block (shard_world 1); the three come from
// the stream-ordered pool (hipFreeAsync on any stream).  host_rec / host_n_rec (in): record starts from bam_host_records, for a
// stream whose device walk declined.  want_off (in): d_off [n_rec + 1] stays too -- kept record r's letters begin at byte
// d_off[r] of the flat block and d_off[r + 1] - d_off[r] is their number + 1, 0 for a record that is not kept.
struct BamRecords {
    uint64_t *d_rec = nullptr;
    uint32_t *d_keep = nullptr, *d_kidx = nullptr;
    uint64_t n_rec = 0, kept = 0, hdr_end = 0;
    const uint64_t *host_rec = nullptr;
    uint64_t host_n_rec = 0;
    bool want_off = false;
    uint64_t *d_off = nullptr;
    void release();      // the device arrays back to the pool (synchronises)
};
int bam_to_flat_dev(const char *d_stream, uint64_t n, const std::vector<uint64_t> &seg, int shard_rank, int shard_world, char **d_flat,
                    uint64_t *flat_len, uint64_t *flat_cap, uint64_t *n_records, BamRecords *recs = nullptr);
// bam_to_flat_dev for one rank with `recs` kept, and the host walk (bam_host_records) where the device walk declines.  h_stream:
// the same bytes on the host, or nullptr (they are copied back then).  SS_ERANGE: more records than hipcub's int item count holds.
int bam_records_flat_dev(const char *d_stream, uint64_t n, const uint8_t *h_stream, const std::vector<uint64_t> &seg, char **d_flat,
                         uint64_t *flat_len, uint64_t *flat_cap, BamRecords *recs);
std::vector<uint64_t> bam_segments(const uint8_t *in, uint64_t in_n, uint64_t n);      // in = NULL: 64 KB pieces
struct BamHostStream {                   // the inflated stream on the host: s[0, n), released with the object
    const uint8_t *s = nullptr;
    uint64_t n = 0;
    char *text = nullptr;
    void *map = nullptr;
    uint64_t map_n = 0;
    ~BamHostStream();
};
int bam_host_stream(const char *path, int kind, BamHostStream *out);
int bam_host_records(const uint8_t *s, uint64_t n, std::vector<uint64_t> *rec, uint64_t *hdr_end);
// The inflated stream of a BAM on the device, d[0, n): a file inflated there where the loader would do that (gpu_gunzip: 1 MB and
// more, not under SS_GZ_GPU=0; `inflated_on_device`), else inflated on the host and uploaded; or a copy of a stream in host memory.
// h: the same bytes on the host where they are there; seg: bam_segments.  release() (and the destructor) gives everything back.
struct BamDeviceStream {
    char *d = nullptr;
    uint64_t n = 0;
    const uint8_t *h = nullptr;
    std::vector<uint64_t> seg;
    bool inflated_on_device = false;
    int open_file(const char *path, int kind);
    int upload(const void *stream, uint64_t n_bytes);
    void release();
    ~BamDeviceStream() { release(); }
private:
    void *lease = nullptr;
    char *copy = nullptr;
    uint64_t copy_cap = 0;
    BamHostStream hs;
};
extern std::atomic<uint64_t> g_bam_dev_files, g_bam_host_files;
extern std::atomic<long long> g_hook_bam_walk_decline;      // ss_test_hook 7 (ss_bam_dev.hip)

// What bam_records_flat_dev handed over, given back on every way out.
struct BamFlatOwner {
    BamRecords &recs;
    char *&flat;
    uint64_t &cap;
    ~BamFlatOwner()
    {
        recs.release();
        if (flat) big_put(flat, cap);
    }
};
// That flat block (flat_len bytes, `kept` records) as the one ASCII slab of *R, which the per-read passes take like any resident
// set.  The block stays the caller's: *R goes out of scope, it is never destroyed.
inline void bam_flat_as_set(char *flat, uint64_t flat_len, uint64_t flat_cap, uint64_t kept, ss_reads *R)
{
    R->adopt(flat, flat_cap, flat_len);
    R->n_records = kept;
    R->n_bases = flat_len - kept;
}
// the little-endian 32-bit field at s + p (any alignment): a BAM record's block_size stands at its start
__device__ __forceinline__ uint32_t ld32_le(const uint8_t *__restrict__ s, uint64_t p)
{
    return (uint32_t)s[p] | (uint32_t)s[p + 1] << 8 | (uint32_t)s[p + 2] << 16 | (uint32_t)s[p + 3] << 24;
}
// The 128-bit digest of the read name of the BAM record at s + p (the bytes before the first NUL; l_read_name >= 1 and the bytes
// lie inside the record: rec_len of ss_bam_dev.hip): *h1 = FNV-1a (64-bit) over the name's bytes and the eight bytes of its length,
// *h2 = a rotate-xor-multiply hash over the same bytes, closed with the length and the splitmix64 finisher.  The one hash of
// ss_bam_extract.hip (the template join) and ss_bam_pairs.hip (the mate link).
__device__ __forceinline__ void bam_name_digest(const uint8_t *__restrict__ s, uint64_t p, unsigned long long *h1, unsigned long long *h2)
{
    const uint32_t lrn = s[p + 12];
    unsigned long long a = 0xCBF29CE484222325ull, b = 0x243F6A8885A308D3ull;
    uint32_t len = 0;
    for (; len + 1u < lrn; len++) {
        const uint32_t c = s[p + 36 + len];
        if (!c) break;
        a = (a ^ c) * 0x100000001B3ull;
        b = (((b << 7) | (b >> 57)) ^ c) * 0x9E3779B97F4A7C15ull;
    }
    for (int i = 0; i < 8; i++) a = (a ^ (i == 0 ? len : 0u)) * 0x100000001B3ull;
    b ^= (unsigned long long)len * 0xD6E8FEB86659FD93ull;
    b = (b ^ (b >> 30)) * 0xBF58476D1CE4E5B9ull;
    b = (b ^ (b >> 27)) * 0x94D049BB133111EBull;
    b ^= b >> 31;
    *h1 = a;
    *h2 = b;
}

// The mate link of a BAM stream's records (ss_bam_pairs.hip; the rule: strainscan_hip.h, "Read pairs from a BAM").  recs: what
// bam_to_flat_dev left.  *d_mate [n_rec] and *d_role [n_rec] (0, 1 or 2; kept 0x1 records only) come from `scratch`; mate[r] is
// the record of kept record r's mate, NO_MATE for a kept record without one, NOT_KEPT for the others (the values are the ABI's:
// ss_bam_mates hands them out).  counters: records, kept, pairs, orphans, singles, records in violating groups; ms (or nullptr):
// keys, sort, link, each synchronised.  SS_OK also with violations (counters[5] says so).  n_rec == 0: nothing is allocated.
constexpr uint32_t NO_MATE = 0xFFFFFFFEu, NOT_KEPT = 0xFFFFFFFFu;
int bam_mates_dev(const uint8_t *d_stream, const BamRecords &recs, PoolScratch &scratch, uint32_t **d_mate, uint8_t **d_role,
                  uint64_t counters[6], double *ms);
// out_len[r] (r <= n_rec; [n_rec] = 0) = 4 + block_size when kept record r's FRAGMENT -- its own hits plus its mate's -- reaches
// min_hits, else 0 (d_hits: per kept record, by d_kidx); tot[0] += records written, tot[1] += fragments selected.  Enqueued.
int bam_fragment_out_len(const uint8_t *d_stream, const BamRecords &recs, const uint32_t *d_mate, const uint32_t *d_hits,
                         uint32_t min_hits, unsigned long long *d_out_len, unsigned long long *d_tot);
// Steps 5 and 6 of ss_bam_pairs.hip on the linked records of a stream (recs with want_off, flat: its flat block of flat_len
// bytes): the fragments joined into *out, one ASCII slab in fragment order.  n_frag = kept - pairs.  *d_fidx (or nullptr to skip;
// [n_rec + 1], from `scratch`, nullptr when n_frag == 0): the fragment index of every LEADER -- the earlier record of a fragment;
// what it holds for other records is the exclusive count of leaders before them.  ms (or nullptr): [0] lengths + scan, [1] join.
int bam_join_dev(const char *flat, uint64_t flat_len, const BamRecords &recs, PoolScratch &scratch, const uint32_t *d_mate,
                 const uint8_t *d_role, uint64_t n_frag, ss_reads **out, uint32_t **d_fidx, double *ms);

// The output path (ss_bam_out.hip).  d_src[0, total) -> dst (host, pageable) through two pinned buffers, chunk by chunk; synchronous
int bam_download_chunks(const char *d_src, uint64_t total, char *dst);
// The file step of a writer: the header ds.d[0, hdr_end) and the new body d_body[0, total) to the host (*ms_download), `ds`
// released before the host compresses, then a BGZF BAM through ss_bgzf_write at zlib level 1 (SS_BAM_OUT_LEVEL=0..9 changes it),
// written to <out_path>.tmp and moved to out_path (*ms_write).  SS_ENOMEM, SS_EHIP, SS_EIO: nothing is left behind then.
int bam_write_file(BamDeviceStream &ds, uint64_t hdr_end, const char *d_body, uint64_t total, const char *out_path, double *ms_download,
                   double *ms_write);
// The eight timing slots of a feature's last file call (ms), behind its ss_bam_*_timing entry point
struct BamTiming {
    std::mutex mu;
    double last[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    void store(const double ms[8])
    {
        std::lock_guard<std::mutex> g(mu);
        memcpy(last, ms, sizeof last);
    }
    int load(double out[8])
    {
        if (!out) return SS_EINVAL;
        std::lock_guard<std::mutex> g(mu);
        memcpy(out, last, sizeof last);
        return SS_OK;
    }
};
// The frame of the entry points that take a BAM FILE (ss_bam_extract, ss_bam_tag_file, ss_reads_load_pairs_bam): open() refuses
// a path that is no BAM (SS_EINVAL, nothing counted), counts the call, starts the clock and brings the stream to the device
// (ms[0]); the caller fills ms[1..6] as strainscan_hip.h states them; finish(), after a call that succeeded, counts the file
// under the route its inflation took, closes ms[7] and publishes the eight slots.
struct BamFileCall {
    BamDeviceStream ds;
    double ms[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    Clock::time_point t_all;
    int open(const char *path, std::atomic<uint64_t> &calls);
    void finish(BamTiming &timing);
};

}  // namespace ss
