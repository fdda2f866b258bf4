// ss_mini_image.hip -- the index image on disk: the built page index of ss_mini.hip (device arrays) dumped verbatim, so that
// a database is indexed once, not at every run (device image cache).
#include "ss_common.h"
#include "ss_scan_dev.h"

#include <fcntl.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <atomic>
#include <thread>
#include <vector>

namespace {
// An imported image is checked before it is used: every index that the scan or gather kernels will follow must stay
// inside its array (a truncated-and-padded or overwritten cache file must fail here, not read out of bounds later).
__global__ void validate_image_kernel(const uint32_t *__restrict__ slot_of_row, uint64_t n_rows, uint64_t n_slots,
                                      const uint8_t *__restrict__ pages, uint64_t n_pages, const uint64_t *__restrict__ mkeys,
                                      uint64_t n_mslots, uint32_t e_max /* k - 15 */, uint32_t *__restrict__ bad)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n_rows) {
        const uint32_t sl = slot_of_row[i];
        if (sl != SS_NO_SLOT && sl >= n_slots) atomicAdd(bad, 1u);
    }
    if (i < n_pages * 8) {
        const uint8_t *pp = pages + (i >> 3) * 64;
        const uint32_t sl = (uint32_t)(i & 7), hi8 = pp[8 + sl];
        if (hi8 & 0x80u) {                       // bucket reference: header + candidates inside d_mkeys
            uint32_t lo;
            memcpy(&lo, pp + 16 + 4 * sl, 4);
            const uint64_t start = lo & ss::START_MASK;
            if (start + 1 >= n_mslots) atomicAdd(bad, 1u);
            else {
                const uint64_t cnt = mkeys[start] >> 32;          // header at start, k-mers at start + 1 .. start + cnt
                if (cnt < 1 || cnt > n_mslots || start + cnt >= n_mslots) atomicAdd(bad, 1u);
            }
        } else if (hi8 != ss::PG_EMPTY_HI && (hi8 & 31u) > e_max) atomicAdd(bad, 1u);
    }
}

struct ImageHeader {
    char magic[8];          // "SSIDX10\0" (10: PG_SOLID flags in the bucket references)
    int32_t k, layout;
    uint64_t n_rows, n_distinct, n_slots, n_buckets, n_mslots, n_inline;
    uint32_t n_dir, bloom_bits, n_dir_alloc, reserved;
};

bool write_dev(FILE *f, const void *d, uint64_t bytes)
{
    std::vector<char> buf(std::min<uint64_t>(bytes, 64ull << 20));
    for (uint64_t off = 0; off < bytes; off += buf.size()) {
        const uint64_t n = std::min<uint64_t>(buf.size(), bytes - off);
        if (hipMemcpy(buf.data(), (const char *)d + off, n, hipMemcpyDeviceToHost) != hipSuccess) return false;
        if (fwrite(buf.data(), 1, n, f) != n) return false;
    }
    return true;
}

// A file range straight to device memory: four threads pread() 16 MB pieces into pinned buffers and copy them on
// the shared ingest streams (one pageable 64 MB bounce buffer moved the 0.54 GB image of an E. coli database in
// 0.09 s: more than reading the sample).
struct PinnedReaders {
    static constexpr int T = 4;
    static constexpr uint64_t PIECE = 16ull << 20;
    char *buf[T] = {nullptr, nullptr, nullptr, nullptr};
    bool ok = true;
    PinnedReaders()
    {
        std::vector<std::thread> pool;
        for (int t = 0; t < T; t++) pool.emplace_back([this, t] { if (hipHostMalloc((void **)&buf[t], PIECE, hipHostMallocDefault) != hipSuccess) buf[t] = nullptr; });
        for (auto &th : pool) th.join();
        for (int t = 0; t < T; t++) ok = ok && buf[t] && ss::ingest_stream((unsigned)t);
    }
    ~PinnedReaders() { for (int t = 0; t < T; t++) if (buf[t]) hipHostFree(buf[t]); }
    bool read(int fd, uint64_t file_off, void *d, uint64_t bytes)
    {
        if (!ok) return false;
        int device = 0;
        hipGetDevice(&device);
        std::atomic<bool> good(true);
        std::atomic<uint64_t> next(0);
        const uint64_t pieces = (bytes + PIECE - 1) / PIECE;
        std::vector<std::thread> pool;
        for (int t = 0; t < T && (uint64_t)t < pieces; t++)
            pool.emplace_back([&, t] {
                hipSetDevice(device);
                hipStream_t st = ss::ingest_stream((unsigned)t);
                for (uint64_t c; good && (c = next.fetch_add(1)) < pieces;) {
                    const uint64_t off = c * PIECE, n = std::min<uint64_t>(PIECE, bytes - off);
                    uint64_t got = 0;
                    while (got < n) {
                        const ssize_t r = pread(fd, buf[t] + got, n - got, (off_t)(file_off + off + got));
                        if (r <= 0) break;
                        got += (uint64_t)r;
                    }
                    if (got != n || hipMemcpyAsync((char *)d + off, buf[t], n, hipMemcpyHostToDevice, st) != hipSuccess ||
                        hipStreamSynchronize(st) != hipSuccess)
                        good = false;
                }
            });
        for (auto &th : pool) th.join();
        return good;
    }
};
}  // namespace

extern "C" {

int ss_db_export(const ss_db *db, const char *path)
{
    if (!db || !path) return SS_EINVAL;
    if (db->layout != 1) return SS_ERANGE;          // only the minimizer layout has a build worth caching
    FILE *f = fopen(path, "wb");
    if (!f) return SS_EIO;
    ImageHeader h;
    memset(&h, 0, sizeof(h));
    memcpy(h.magic, "SSIDX10", 8);
    h.k = db->k; h.layout = db->layout;
    h.n_rows = db->n_rows; h.n_distinct = db->n_distinct; h.n_slots = db->n_slots; h.n_buckets = db->n_buckets;
    h.n_mslots = db->n_mslots; h.n_inline = db->n_inline;
    h.n_dir = db->n_dir; h.n_dir_alloc = db->n_dir_alloc;
    h.bloom_bits = db->d_bloom ? db->bloom_bits : 0;
    const uint64_t nr = std::max<uint64_t>(1, db->n_rows);
    bool ok = fwrite(&h, sizeof(h), 1, f) == 1 && write_dev(f, db->d_mkeys, db->n_mslots * 8) &&
              write_dev(f, db->d_dir, (uint64_t)db->n_dir_alloc * 64) && write_dev(f, db->d_slot_of_row, nr * 4) &&
              write_dev(f, db->d_row_valid, nr) &&
              (!h.bloom_bits || write_dev(f, db->d_bloom, (1ull << h.bloom_bits) / 8));
    ok = (fclose(f) == 0) && ok;
    if (!ok) { remove(path); return SS_EIO; }
    return SS_OK;
}

int ss_db_import(const char *path, ss_db **out)
{
    if (!path || !out) return SS_EINVAL;
    const int fd = open(path, O_RDONLY);
    if (fd < 0) return SS_EIO;
    ImageHeader h;
    struct stat st;
    if (fstat(fd, &st) != 0 || pread(fd, &h, sizeof(h), 0) != (ssize_t)sizeof(h) || memcmp(h.magic, "SSIDX10", 8) != 0 ||
        h.layout != 1 || h.k < ss::MINI_K_MIN || h.k > 31 || h.n_mslots == 0 || h.n_dir < ss::PG_MIN_PAGES || h.n_dir_alloc != h.n_dir + h.n_dir / 1024 || h.n_slots != h.n_mslots + (uint64_t)h.n_dir_alloc * 8 ||
        h.n_slots >= 0xFFFFFFF0ull || h.n_mslots >= (uint64_t)ss::START_MASK || (h.bloom_bits && (h.bloom_bits < 10 || h.bloom_bits > 30))) {
        close(fd);
        return SS_EINVAL;
    }
    const uint64_t nr = std::max<uint64_t>(1, h.n_rows);
    const uint64_t sizes[5] = {h.n_mslots * 8, (uint64_t)h.n_dir_alloc * 64, nr * 4, nr, h.bloom_bits ? (1ull << h.bloom_bits) / 8 : 0};
    uint64_t offs[6] = {sizeof(h), 0, 0, 0, 0, 0};
    for (int i = 0; i < 5; i++) offs[i + 1] = offs[i] + sizes[i];
    if ((uint64_t)st.st_size != offs[5]) { close(fd); return SS_EIO; }     // the file must be exactly the image
    ss_db *db = new (std::nothrow) ss_db();
    if (!db) { close(fd); return SS_ENOMEM; }
    db->k = h.k; db->layout = 1;
    db->n_rows = h.n_rows; db->n_distinct = h.n_distinct; db->n_slots = h.n_slots; db->capacity = h.n_slots;
    db->n_mslots = h.n_mslots; db->n_inline = h.n_inline;
    db->n_buckets = h.n_buckets; db->n_dir = h.n_dir; db->n_dir_alloc = h.n_dir_alloc;
    hipGetDevice(&db->device);
    bool ok = hipMalloc((void **)&db->d_mkeys, sizes[0]) == hipSuccess && hipMalloc((void **)&db->d_dir, sizes[1]) == hipSuccess &&
              hipMalloc((void **)&db->d_counts, db->n_slots * 4) == hipSuccess &&
              hipMalloc((void **)&db->d_slot_of_row, sizes[2]) == hipSuccess && hipMalloc((void **)&db->d_row_valid, sizes[3]) == hipSuccess &&
              (!h.bloom_bits || hipMalloc((void **)&db->d_bloom, sizes[4]) == hipSuccess);
    if (ok) {
        PinnedReaders rd;
        ok = rd.read(fd, offs[0], db->d_mkeys, sizes[0]) && rd.read(fd, offs[1], db->d_dir, sizes[1]) &&
             rd.read(fd, offs[2], db->d_slot_of_row, sizes[2]) && rd.read(fd, offs[3], db->d_row_valid, sizes[3]) &&
             (!h.bloom_bits || rd.read(fd, offs[4], db->d_bloom, sizes[4])) &&
             hipMemset(db->d_counts, 0, db->n_slots * 4) == hipSuccess;
    }
    close(fd);
    if (ok) {
        uint32_t *d_bad = nullptr, bad = 1;
        const uint64_t nchk = std::max<uint64_t>(h.n_rows, (uint64_t)h.n_dir_alloc * 8);
        ok = hipMalloc((void **)&d_bad, 4) == hipSuccess && hipMemset(d_bad, 0, 4) == hipSuccess;
        if (ok) {
            hipLaunchKernelGGL(validate_image_kernel, dim3((unsigned)((nchk + 255) / 256)), dim3(256), 0, 0, db->d_slot_of_row, h.n_rows,
                               h.n_slots, (const uint8_t *)db->d_dir, (uint64_t)h.n_dir_alloc, db->d_mkeys, h.n_mslots, (uint32_t)(h.k - ss::MINI_M), d_bad);
            ok = hipMemcpy(&bad, d_bad, 4, hipMemcpyDeviceToHost) == hipSuccess && bad == 0;
        }
        hipFree(d_bad);
    }
    if (ok && h.bloom_bits) db->bloom_bits = h.bloom_bits;
    if (!ok) { ss_db_destroy(db); return SS_EIO; }
    db->device_bytes = db->n_mslots * 8 + db->n_slots * 4 + (uint64_t)db->n_dir_alloc * 64 + nr * 5 + sizes[4];
    *out = db;
    return SS_OK;
}

}  // extern "C"
