// ss_npz_dev.hip -- layer 2's matrix import (ss_l2.hip): members of an .npz archive brought to the device.  A deflated member
// goes through the device gunzip (ss::gpu_gunzip, ss_ginflate.hip), which this file only calls.
#include "ss_common.h"

#include <fcntl.h>
#include <sys/stat.h>
#include <unistd.h>
#include <zlib.h>

#include <algorithm>
#include <atomic>
#include <memory>
#include <thread>
#include <vector>

// A deflated member of a ZIP archive (a .npy array of scipy.sparse.save_npz: all_strains_re.npz, Recls_withR_new.py:110-112)
// inflated on the device and LEFT there: raw deflate data at [off, off + comp_n) of the file, CRC-32 and length of the content
// as the archive's directory states them.  The member is dressed as a gzip member (10-byte header in front, CRC-32 + ISIZE
// behind: the inflater checks both) and goes through gpu_gunzip.  *d_data is lent until ss_npz_member_done(*lease).
// SS_ERANGE: not handled here (no dynamic blocks to enter, too small, an absurd ratio): the caller reads it on the host.
namespace {
struct NpzLease { void *gz = nullptr; void *d_buf = nullptr; };
}
extern "C" int ss_npz_member_dev(const char *path, uint64_t off, uint64_t comp_n, uint32_t crc, uint64_t usize, int method, void **d_data,
                                 uint64_t *n, void **lease)
{
    if (!path || !d_data || !n || !lease || (method != 0 && method != 8) || (method == 8 && comp_n < 64) || (method == 0 && comp_n != usize)) return SS_EINVAL;
    const int fd = open(path, O_RDONLY);
    if (fd < 0) return SS_EIO;
    struct stat st;
    if (fstat(fd, &st) != 0 || (uint64_t)st.st_size < off + comp_n) { close(fd); return SS_EIO; }
    NpzLease *L = new (std::nothrow) NpzLease();
    if (!L) { close(fd); return SS_ENOMEM; }
    if (method == 0) {
        // STORED (scipy.sparse.save_npz(..., compressed=False)): the bytes go to the device as they are, through pinned pieces;
        // every piece's CRC-32 is taken on its way (zipfile's single thread spends 7 ms per million non-zeros on exactly this)
        // and the pieces' CRCs are combined in order
        constexpr uint64_t PIECE = 16ull << 20;
        constexpr int T = 8;
        const uint64_t pieces = (usize + PIECE - 1) / PIECE;
        int device = 0;
        hipGetDevice(&device);
        if (hipMalloc(&L->d_buf, std::max<uint64_t>(usize, 64)) != hipSuccess) { (void)hipGetLastError(); delete L; close(fd); return SS_ENOMEM; }
        std::vector<uint32_t> pcrc((size_t)pieces, 0);
        std::atomic<bool> good(true);
        std::atomic<uint64_t> next(0);
        std::vector<std::thread> pool;
        for (int t = 0; t < T && (uint64_t)t < pieces; t++)
            pool.emplace_back([&, t] {
                hipSetDevice(device);
                char *pin = nullptr;
                if (hipHostMalloc((void **)&pin, PIECE, hipHostMallocDefault) != hipSuccess) { good = false; return; }
                hipStream_t sx = ss::ingest_stream((unsigned)t);
                for (uint64_t c; good && (c = next.fetch_add(1)) < pieces;) {
                    const uint64_t o = c * PIECE, m = std::min<uint64_t>(PIECE, usize - o);
                    uint64_t got = 0;
                    while (got < m) {
                        const ssize_t r = pread(fd, pin + got, m - got, (off_t)(off + o + got));
                        if (r <= 0) break;
                        got += (uint64_t)r;
                    }
                    if (got != m) { good = false; break; }
                    pcrc[(size_t)c] = (uint32_t)crc32(crc32(0L, Z_NULL, 0), (const Bytef *)pin, (uInt)m);
                    if (hipMemcpyAsync((char *)L->d_buf + o, pin, m, hipMemcpyHostToDevice, sx) != hipSuccess || hipStreamSynchronize(sx) != hipSuccess) good = false;
                }
                hipHostFree(pin);
            });
        for (auto &th : pool) th.join();
        close(fd);
        uLong all = crc32(0L, Z_NULL, 0);
        for (uint64_t c = 0; c < pieces; c++) all = crc32_combine(all, pcrc[(size_t)c], (z_off_t)std::min<uint64_t>(PIECE, usize - c * PIECE));
        if (!good || (uint32_t)all != crc) { hipFree(L->d_buf); delete L; return good ? SS_EIO : SS_EHIP; }
        *d_data = L->d_buf; *n = usize; *lease = L;
        return SS_OK;
    }
    const uint64_t in_n = 10 + comp_n + 8;
    std::unique_ptr<uint8_t[]> img(new (std::nothrow) uint8_t[in_n]);
    if (!img) { close(fd); delete L; return SS_ENOMEM; }
    static const uint8_t hdr[10] = {0x1f, 0x8b, 8, 0, 0, 0, 0, 0, 0, 0xff};
    memcpy(img.get(), hdr, 10);
    {   // the compressed bytes, by a few threads (the page cache hands a single pread ~3 GB/s)
        const unsigned T = (unsigned)std::max<uint64_t>(1, std::min<uint64_t>(8, comp_n >> 24));
        std::atomic<bool> ok(true);
        std::vector<std::thread> pool;
        for (unsigned w = 0; w < T; w++)
            pool.emplace_back([&, w] {
                uint64_t a = comp_n * w / T;
                const uint64_t e = comp_n * (w + 1) / T;
                while (a < e) {
                    const ssize_t r = pread(fd, img.get() + 10 + a, (size_t)std::min<uint64_t>(e - a, 1u << 30), (off_t)(off + a));
                    if (r <= 0) { ok = false; return; }
                    a += (uint64_t)r;
                }
            });
        for (auto &th : pool) th.join();
        close(fd);
        if (!ok) { delete L; return SS_EIO; }
    }
    uint8_t *t8 = img.get() + 10 + comp_n;
    for (int q = 0; q < 4; q++) { t8[q] = (uint8_t)(crc >> (8 * q)); t8[4 + q] = (uint8_t)(usize >> (8 * q)); }
    char *d = nullptr;
    uint64_t len = 0;
    if (!ss::gpu_gunzip(img.get(), in_n, &d, &len, &L->gz, -1)) { delete L; return SS_ERANGE; }
    if (len != usize) { ss::gpu_gunzip_done(L->gz); delete L; return SS_EIO; }
    *d_data = d; *n = len; *lease = L;
    return SS_OK;
}
extern "C" int ss_npz_member_done(void *lease)
{
    NpzLease *L = static_cast<NpzLease *>(lease);
    if (!L) return SS_OK;
    if (L->gz) ss::gpu_gunzip_done(L->gz);
    if (L->d_buf) hipFree(L->d_buf);
    delete L;
    return SS_OK;
}

// CRC-32 (zlib's) of `prefix` followed by n copies of one byte, from the prefix's CRC: O(log n) crc32_combine steps.  What
// the `data.npy` member of a binary matrix must have -- a few header bytes, then nnz ones -- so that 630 MB of ones need not
// be inflated to know that they are ones (the archive's directory carries the content's CRC-32 and length).
extern "C" int ss_crc32_repeat(uint32_t prefix_crc, int byte, uint64_t n, uint32_t *out)
{
    if (!out || byte < 0 || byte > 255) return SS_EINVAL;
    const unsigned char b = (unsigned char)byte;
    uLong pw = crc32(crc32(0L, Z_NULL, 0), &b, 1);       // CRC of 2^i copies
    uLong acc = prefix_crc;
    uint64_t len = 1;
    for (uint64_t m = n; m; m >>= 1, len <<= 1) {
        if (m & 1) acc = crc32_combine(acc, pw, (z_off_t)len);
        if (m >> 1) pw = crc32_combine(pw, pw, (z_off_t)len);
    }
    *out = (uint32_t)acc;
    return SS_OK;
}
