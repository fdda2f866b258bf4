// ss_bam_out.hip -- the output path of the calls that write a BAM (`-x` on a BAM sample, `--tag_bam`) and the frame of the entry
// points that take a BAM file (BamFileCall); ss_bam.h states each.  Host code only: a writer adds the selection, which bytes make
// the new body, and nothing else.
#include "ss_bam.h"

#include <zlib.h>

#include <fcntl.h>
#include <unistd.h>

#include <cerrno>
#include <string>
#include <thread>

namespace {

unsigned bgzf_threads()
{
    unsigned t = ss::host_cpus();
    if (const char *e = getenv("SS_HOST_THREADS")) t = (unsigned)std::max(1, atoi(e));
    return std::max(1u, std::min(16u, t));
}

constexpr uint32_t BGZF_BLOCK = 0xff00;
const uint8_t BGZF_EOF[28] = {0x1f, 0x8b, 0x08, 0x04, 0, 0, 0, 0, 0, 0xff, 0x06, 0, 0x42, 0x43, 0x02, 0, 0x1b, 0, 0x03, 0, 0, 0, 0, 0, 0, 0, 0, 0};

// one member behind `out`: the 18-byte header with the "BC" field, raw deflate, CRC-32, ISIZE.  zs: a raw-deflate stream at the
// caller's level; a member that would pass 64 KB (bytes that do not compress) is stored instead, as htslib does
bool bgzf_member(z_stream *zs, const uint8_t *src, uint32_t len, std::vector<uint8_t> *out)
{
    const size_t at = out->size();
    const size_t room = (size_t)len + (len >> 8) + 1024;
    for (int attempt = 0; attempt < 2; attempt++) {
        out->resize(at + 18 + room + 8);
        z_stream stored;
        z_stream *z = zs;
        if (attempt == 1) {
            memset(&stored, 0, sizeof stored);
            if (deflateInit2(&stored, 0, Z_DEFLATED, -15, 8, Z_DEFAULT_STRATEGY) != Z_OK) return false;
            z = &stored;
        } else if (deflateReset(z) != Z_OK) return false;
        z->next_in = const_cast<Bytef *>(src);
        z->avail_in = len;
        z->next_out = out->data() + at + 18;
        z->avail_out = (uInt)room;
        const int r = deflate(z, Z_FINISH);
        const size_t clen = room - z->avail_out;
        if (attempt == 1) deflateEnd(&stored);
        if (r != Z_STREAM_END) return false;
        const size_t bsize = 18 + clen + 8;
        if (bsize > 65536) continue;
        uint8_t *h = out->data() + at;
        const uint8_t head[16] = {0x1f, 0x8b, 0x08, 0x04, 0, 0, 0, 0, 0, 0xff, 0x06, 0, 'B', 'C', 0x02, 0};
        memcpy(h, head, 16);
        h[16] = (uint8_t)((bsize - 1) & 0xFF);
        h[17] = (uint8_t)((bsize - 1) >> 8);
        const uint32_t crc = (uint32_t)crc32(crc32(0L, Z_NULL, 0), src, len);
        uint8_t *t = h + 18 + clen;
        for (int i = 0; i < 4; i++) { t[i] = (uint8_t)(crc >> (8 * i)); t[4 + i] = (uint8_t)(len >> (8 * i)); }
        out->resize(at + bsize);
        return true;
    }
    return false;
}

bool write_all(int fd, const uint8_t *p, size_t n)
{
    while (n) {
        const ssize_t w = write(fd, p, std::min<size_t>(n, 1u << 30));
        if (w < 0) { if (errno == EINTR) continue; return false; }
        p += w;
        n -= (size_t)w;
    }
    return true;
}

}  // namespace

namespace ss {

// (the copy of a chunk runs beside the host's memcpy of the one before)
int bam_download_chunks(const char *d_src, uint64_t total, char *dst)
{
    if (!total) return SS_OK;
    const hipStream_t st = ss::l2s::stream();
    const uint64_t CH = std::min<uint64_t>(total, 16ull << 20);
    char *buf[2] = {nullptr, nullptr};
    hipEvent_t ev[2] = {nullptr, nullptr};
    bool ok = true;
    for (int i = 0; i < 2 && ok; i++)
        ok = hipHostMalloc((void **)&buf[i], CH, hipHostMallocDefault) == hipSuccess && hipEventCreateWithFlags(&ev[i], hipEventDisableTiming) == hipSuccess;
    const uint64_t n_ch = (total + CH - 1) / CH;
    for (uint64_t i = 0; i <= n_ch && ok; i++) {
        if (i < n_ch) {
            const uint64_t o = i * CH, l = std::min(CH, total - o);
            ok = hipMemcpyAsync(buf[i & 1], d_src + o, l, hipMemcpyDeviceToHost, st) == hipSuccess && hipEventRecord(ev[i & 1], st) == hipSuccess;
        }
        if (i > 0 && ok) {
            const uint64_t o = (i - 1) * CH, l = std::min(CH, total - o);
            ok = hipEventSynchronize(ev[(i - 1) & 1]) == hipSuccess;
            if (ok) memcpy(dst + o, buf[(i - 1) & 1], l);
        }
    }
    (void)hipStreamSynchronize(st);
    for (int i = 0; i < 2; i++) {
        if (ev[i]) (void)hipEventDestroy(ev[i]);
        if (buf[i]) (void)hipHostFree(buf[i]);
    }
    if (!ok) { (void)hipGetLastError(); return SS_EHIP; }
    return SS_OK;
}

int bam_write_file(BamDeviceStream &ds, uint64_t hdr_end, const char *d_body, uint64_t total, const char *out_path, double *ms_download,
                   double *ms_write)
{
    int rc = SS_OK;
    std::vector<uint8_t> head;
    char *body = nullptr;
    auto t0 = Clock::now();
    try { head.resize(hdr_end); } catch (const std::bad_alloc &) { rc = SS_ENOMEM; }
    if (rc == SS_OK && hdr_end && hipMemcpy(head.data(), ds.d, hdr_end, hipMemcpyDeviceToHost) != hipSuccess) rc = SS_EHIP;
    if (rc == SS_OK && total) {
        body = (char *)malloc(total);
        rc = body ? bam_download_chunks(d_body, total, body) : SS_ENOMEM;
    }
    ds.release();
    *ms_download = ms_since(t0);
    if (rc == SS_OK) {
        t0 = Clock::now();
        int level = 1;
        if (const char *e = getenv("SS_BAM_OUT_LEVEL")) level = std::max(0, std::min(9, atoi(e)));
        const std::string tmp = std::string(out_path) + ".tmp";
        rc = ss_bgzf_write(tmp.c_str(), head.data(), head.size(), body, total, level);
        if (rc == SS_OK && rename(tmp.c_str(), out_path) != 0) { unlink(tmp.c_str()); rc = SS_EIO; }
        *ms_write = ms_since(t0);
    }
    free(body);
    return rc;
}

int BamFileCall::open(const char *path, std::atomic<uint64_t> &calls)
{
    const int kind = input_kind(path);
    if (kind != INPUT_BAM_GZ && kind != INPUT_BAM_RAW) return SS_EINVAL;
    calls++;
    t_all = Clock::now();
    // the stream on the device: inflated there where the loader would do that, else inflated on the host and uploaded
    const int rc = ds.open_file(path, kind);
    if (rc) return rc;
    ms[0] = ms_since(t_all);
    return SS_OK;
}

void BamFileCall::finish(BamTiming &timing)
{
    (ds.inflated_on_device ? g_bam_dev_files : g_bam_host_files)++;
    ms[7] = ms_since(t_all);
    timing.store(ms);
}

}  // namespace ss

extern "C" int ss_bgzf_write(const char *path, const void *head, uint64_t head_n, const void *body, uint64_t body_n, int level)
{
    if (!path || (!head && head_n) || (!body && body_n) || level < 0 || level > 9) return SS_EINVAL;
    const int fd = open(path, O_WRONLY | O_CREAT | O_TRUNC, 0644);
    if (fd < 0) return SS_EIO;
    // the members: the header's, then the body's (a member never holds bytes of both, so the first record starts a member)
    struct Piece { const uint8_t *p; uint32_t n; };
    std::vector<Piece> pieces;
    for (uint64_t o = 0; o < head_n; o += BGZF_BLOCK) pieces.push_back({(const uint8_t *)head + o, (uint32_t)std::min<uint64_t>(BGZF_BLOCK, head_n - o)});
    for (uint64_t o = 0; o < body_n; o += BGZF_BLOCK) pieces.push_back({(const uint8_t *)body + o, (uint32_t)std::min<uint64_t>(BGZF_BLOCK, body_n - o)});
    const uint64_t M = pieces.size();
    const unsigned T = (unsigned)std::max<uint64_t>(1, std::min<uint64_t>(bgzf_threads(), (M + 63) / 64));
    std::vector<std::vector<uint8_t>> outs(T);
    std::vector<char> good(T, 1);
    auto work = [&](unsigned t) {
        z_stream zs;
        memset(&zs, 0, sizeof zs);
        if (deflateInit2(&zs, level, Z_DEFLATED, -15, 8, Z_DEFAULT_STRATEGY) != Z_OK) { good[t] = 0; return; }
        try {
            for (uint64_t m = M * t / T; m < M * (t + 1) / T && good[t]; m++)
                if (!bgzf_member(&zs, pieces[m].p, pieces[m].n, &outs[t])) good[t] = 0;
        } catch (const std::bad_alloc &) { good[t] = 0; }
        deflateEnd(&zs);
    };
    if (T == 1) work(0);
    else {
        std::vector<std::thread> pool;
        for (unsigned t = 0; t < T; t++) pool.emplace_back(work, t);
        for (auto &th : pool) th.join();
    }
    bool ok = true;
    for (unsigned t = 0; t < T; t++) ok = ok && good[t];
    for (unsigned t = 0; t < T && ok; t++) ok = write_all(fd, outs[t].data(), outs[t].size());
    ok = ok && write_all(fd, BGZF_EOF, sizeof BGZF_EOF);
    ok = (close(fd) == 0) && ok;
    if (!ok) { unlink(path); return SS_EIO; }
    return SS_OK;
}
