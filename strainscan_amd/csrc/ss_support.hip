// ss_reads_support: how many records of a resident read set carry k-mers of a table (`--read_support`).
//
// The scans add a hit to the counter of its k-mer and forget the read it came from; this is the other projection: hits per RECORD,
// reduced on the device to a histogram (records with exactly b hits) and the total.  A record is a maximal run of bytes other
// than '\n' in a slab (a slot's L bases in a packed slab); a hit is a start position at which ss_scan_reads would count.  Nothing
// here depends on the order of the records, so the result is the same for a set in file order, binned, or packed.
//
// Three passes, each a plain launch (no device-wide barrier inside a kernel):
//   1. record_ends_kernel (ASCII slabs only): record ends per 1024-position tile, from the raw bytes -- a record end is a '\n'
//      behind a byte that is none; a slab that does not end in '\n' ends its last record all the same.  hipcub's ExclusiveSum
//      turns them into the record index at which every tile begins.  A packed slab needs neither: record = position / slot.
//   2. scan_minik_kernel<.., SupportSink> (ss_minik.hip): the lookups of the per-position scan kernel, k at run time, all three
//      input layouts, behind the table's Bloom filter where it has one.  A found k-mer sets the bit of its position in a bitmap
//      of the tile in LDS; the tile's tail adds the bits up per record and issues one atomicAdd per (lane, record) into
//      rec_hits[] -- about two per lane for 150-base reads, neighbouring lanes on neighbouring words.  Records that straddle
//      tiles, or span many, meet in that array; record indices run on from slab to slab.
//   3. support_hist_kernel: rec_hits -> bins in LDS per workgroup -> a few global 64-bit atomics.
// The scratch (4 bytes per record, 4 per tile) comes from the stream-ordered pool and goes back before the call returns.
// Passes 1 and 2 are rec_hits_of (ss_support.h), which ss_reads_select (ss_select.hip) calls too; with slot labels (ss_label.hip)
// pass 2 runs the label sink and rec_hits[] has a slice per label.  Pass 3 is rec_hits_histogram, on one slice.
#include "ss_scan_dev.h"
#include "ss_support.h"

#include <hipcub/hipcub.hpp>

using namespace ss::dev;
using ss::SUP_TILE;

namespace {

// one wave per tile, 16 bytes per lane; tile_ends[tile] = record ends at positions [tile * 1024, tile * 1024 + 1024) below n, and
// in the tile of byte n - 1 one more if that byte is not '\n'
template <bool ALIGNED>
__global__ __launch_bounds__(256) void record_ends_kernel(const uint8_t *__restrict__ bases, uint64_t n, uint64_t n_tiles,
                                                          uint32_t *__restrict__ tile_ends)
{
    const uint64_t tile = (uint64_t)blockIdx.x * 4u + (threadIdx.x >> 6);
    if (tile >= n_tiles) return;                                        // (the same for the whole wave)
    const uint64_t off = tile * (uint64_t)SUP_TILE + (uint64_t)(threadIdx.x & 63u) * 16u;
    uint32_t c = 0;
    if (off < n) {
        uint32_t w[4];
        load16<ALIGNED>(bases, off, n, w);
        const uint32_t nl = newline_mask16(w);
        const uint32_t prev = (off == 0 || bases[off - 1] == 0x0Au) ? 1u : 0u;
        uint32_t ends = nl & ~((nl << 1) | prev) & 0xFFFFu;
        if (n - off < 16u) ends &= (1u << (uint32_t)(n - off)) - 1u;    // positions below n only
        c = (uint32_t)__popc(ends);
        if (n - off <= 16u) c += ((nl >> (uint32_t)(n - 1u - off)) & 1u) ^ 1u;
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) c += __shfl_xor(c, d, 64);
    if ((threadIdx.x & 63u) == 0) tile_ends[tile] = c;
}

constexpr uint32_t HIST_LDS = 1024;      // bins a workgroup adds up in LDS; higher bins (n_bins above that) go to global memory

// out[b], b < n_bins: records with min(hits, n_bins - 1) == b; out[n_bins]: the hits of all records
__global__ __launch_bounds__(256) void support_hist_kernel(const uint32_t *__restrict__ rec_hits, uint64_t n_rec, uint32_t n_bins,
                                                           unsigned long long *__restrict__ out)
{
    __shared__ uint32_t bins[HIST_LDS];
    for (uint32_t b = threadIdx.x; b < HIST_LDS; b += 256u) bins[b] = 0u;
    __syncthreads();
    unsigned long long sum = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x; i < n_rec; i += (uint64_t)gridDim.x * 256u) {
        const uint32_t h = rec_hits[i], b = min(h, n_bins - 1u);
        sum += h;
        if (b < HIST_LDS) atomicAdd(&bins[b], 1u);
        else atomicAdd(&out[b], 1ull);
    }
    __syncthreads();
    for (uint32_t b = threadIdx.x; b < min(n_bins, HIST_LDS); b += 256u)
        if (bins[b]) atomicAdd(&out[b], (unsigned long long)bins[b]);
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) sum += __shfl_xor(sum, d, 64);
    if ((threadIdx.x & 63u) == 0 && sum) atomicAdd(&out[n_bins], sum);
}

std::atomic<uint64_t> g_support_calls{0};

}  // namespace

// passes 1 and 2 (ss_support.h): ss_reads_support reduces rec_hits to a histogram, ss_reads_select (ss_select.hip) acts on it;
// pass 1 alone is record_index_of, all that ss_reads_resample (ss_resample.hip) needs of a set
int ss::rec_hits_of(const ss_db *db, const ss_reads *R, RecHits *out, std::atomic<uint64_t> *calls, const uint8_t *d_slot_label, uint32_t n_labels)
{
    if (db->layout != 1) return SS_ERANGE;                          // page-index tables only
    if (R->has_cut_record && db->k != 31) return SS_ERANGE;         // cut records carry a 30-base overlap (as ss_scan_reads)
    const int rc0 = ss::record_index_of(R, db->device, out, calls);
    if (rc0) return rc0;
    const hipStream_t st = ss::l2s::stream();
    PoolScratch &scratch = out->scratch;
    const uint64_t rec_total = out->rec_total;
    uint32_t *d_base = out->d_tile_base, *d_rec = nullptr;
    // 2. hits per record (the labelled form: a slice per label)
    SS_HIP(scratch.get((void **)&d_rec, rec_total * 4 * n_labels));
    SS_HIP(ss::l2s::set(d_rec, 0, std::max<uint64_t>(rec_total * 4 * n_labels, 16)));
    for (const RecHits::Part &pt : out->parts) {
        if (pt.n >= (uint64_t)db->k && pt.n_rec) {
            const ss::SupportArgs a{d_rec, pt.sl->packed ? nullptr : d_base + pt.tile_off, pt.rec_base, rec_total, pt.sl->packed ? pt.sl->slot : 0u};
            const int rc = d_slot_label ? ss::launch_label_minik(db, pt.sl->d, pt.n, pt.sl->packed, a, d_slot_label, n_labels, st)
                                        : ss::launch_support_minik(db, pt.sl->d, pt.n, pt.sl->packed, a, st);
            if (rc) return rc;
        }
    }
    out->d_rec_hits = d_rec;
    return SS_OK;
}

// pass 1 (ss_support.h): the set's slabs that hold positions, their records numbered slab after slab
int ss::record_index_of(const ss_reads *R, int device, RecHits *out, std::atomic<uint64_t> *calls)
{
    using Part = RecHits::Part;
    std::vector<Part> &parts = out->parts;
    uint64_t tiles_total = 0;
    for (const auto &sl : R->slabs) {
        if (!sl.used || !sl.positions()) continue;
        hipPointerAttribute_t at;
        if (hipPointerGetAttributes(&at, sl.d) != hipSuccess || (device >= 0 && at.device != device)) { (void)hipGetLastError(); return SS_EINVAL; }
        Part pt{&sl, sl.positions(), 0, tiles_total, 0, 0};
        pt.n_tiles = (pt.n + SUP_TILE - 1) / SUP_TILE;
        if (sl.packed) {
            if (!sl.slot) return SS_EINVAL;
            pt.n_rec = pt.n / sl.slot;
        } else {
            if (pt.n_tiles + 1 > 0x7FFFFFFFull) return SS_ERANGE;   // hipcub counts its items in an int
            tiles_total += pt.n_tiles + 1;
        }
        parts.push_back(pt);
    }
    if (calls) (*calls)++;
    const hipStream_t st = ss::l2s::stream();
    PoolScratch &scratch = out->scratch;
    uint32_t *d_ends = nullptr, *d_base = nullptr;
    // 1. ASCII slabs: record ends per tile -> the record index at which each tile begins; [n_tiles] of a slab = its records
    if (tiles_total) {
        SS_HIP(scratch.get((void **)&d_ends, tiles_total * 4));
        SS_HIP(scratch.get((void **)&d_base, tiles_total * 4));
        SS_HIP(ss::l2s::set(d_ends, 0, tiles_total * 4));
        size_t tmp_bytes = 0;
        for (const Part &pt : parts)
            if (!pt.sl->packed) {
                size_t tb = 0;
                SS_HIP(hipcub::DeviceScan::ExclusiveSum(nullptr, tb, d_ends, d_base, (int)(pt.n_tiles + 1), st));
                tmp_bytes = std::max(tmp_bytes, tb);
            }
        void *d_tmp = nullptr;
        SS_HIP(scratch.get(&d_tmp, tmp_bytes));
        std::vector<uint32_t> n_rec(parts.size(), 0);
        for (size_t i = 0; i < parts.size(); i++) {
            const Part &pt = parts[i];
            if (pt.sl->packed) continue;
            const uint8_t *b = (const uint8_t *)pt.sl->d;
            const dim3 grid((unsigned)((pt.n_tiles + 3) / 4));
            if ((((uintptr_t)b) & 15) == 0) hipLaunchKernelGGL(record_ends_kernel<true>, grid, dim3(256), 0, st, b, pt.n, pt.n_tiles, d_ends + pt.tile_off);
            else hipLaunchKernelGGL(record_ends_kernel<false>, grid, dim3(256), 0, st, b, pt.n, pt.n_tiles, d_ends + pt.tile_off);
            SS_HIP(hipGetLastError());
            size_t tb = tmp_bytes;
            SS_HIP(hipcub::DeviceScan::ExclusiveSum(d_tmp, tb, d_ends + pt.tile_off, d_base + pt.tile_off, (int)(pt.n_tiles + 1), st));
            SS_HIP(hipMemcpyAsync(&n_rec[i], d_base + pt.tile_off + pt.n_tiles, 4, hipMemcpyDeviceToHost, st));
        }
        SS_HIP(ss::l2s::sync());
        for (size_t i = 0; i < parts.size(); i++)
            if (!parts[i].sl->packed) parts[i].n_rec = n_rec[i];
    }
    uint64_t rec_total = 0;
    for (Part &pt : parts) { pt.rec_base = rec_total; rec_total += pt.n_rec; }
    out->tiles_total = tiles_total;
    out->rec_total = rec_total;
    out->d_tile_base = d_base;
    return SS_OK;
}

// 3. histogram and total
int ss::rec_hits_histogram(RecHits *rh, const uint32_t *d_rec, uint32_t n_bins, uint64_t *hist, uint64_t *hits)
{
    const hipStream_t st = ss::l2s::stream();
    const uint64_t rec_total = rh->rec_total;
    unsigned long long *d_out = nullptr;
    SS_HIP(rh->scratch.get((void **)&d_out, ((size_t)n_bins + 1) * 8));
    SS_HIP(ss::l2s::set(d_out, 0, ((size_t)n_bins + 1) * 8));
    if (rec_total) {
        const unsigned blocks = (unsigned)std::min<uint64_t>((rec_total + 256 * 8 - 1) / (256 * 8), 2048);
        hipLaunchKernelGGL(support_hist_kernel, dim3(blocks), dim3(256), 0, st, d_rec, rec_total, n_bins, d_out);
        SS_HIP(hipGetLastError());
    }
    std::vector<unsigned long long> out((size_t)n_bins + 1);
    SS_HIP(ss::l2s::copy(out.data(), d_out, out.size() * 8, hipMemcpyDeviceToHost));
    for (uint32_t b = 0; b < n_bins; b++) hist[b] = out[b];
    *hits = out[n_bins];
    return SS_OK;
}

extern "C" {

int ss_reads_support_calls(uint64_t *n)
{
    if (!n) return SS_EINVAL;
    *n = g_support_calls.load();
    return SS_OK;
}

int ss_reads_support(const ss_db *db, const ss_reads *R, uint32_t n_bins, uint64_t *hist, uint64_t *hits)
{
    if (!db || !R || !hist || !hits || n_bins < 2) return SS_EINVAL;
    ss::RecHits rh;
    const int rc = ss::rec_hits_of(db, R, &rh, &g_support_calls);
    if (rc) return rc;
    return ss::rec_hits_histogram(&rh, rh.d_rec_hits, n_bins, hist, hits);
}

}  // extern "C"
