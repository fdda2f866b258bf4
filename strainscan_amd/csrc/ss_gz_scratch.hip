// ss_gz_scratch.hip -- what the device gunzip (ss_ginflate.hip) keeps between its calls, process-wide: the scratch arenas, the
// pinned upload buffers with their streams, and the calls' streams.  One mutex guards the three free lists.
// ss_gz_gpu_release hands all of it back, ss_gz_warm_up makes the upload buffers ahead of time.
#include "ss_ginflate.h"

#include <unistd.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <functional>
#include <mutex>
#include <thread>
#include <vector>

namespace ss {

namespace {

struct PinSet;
std::mutex g_arena_mu;
std::vector<Arena *> g_arena_free;                            // (the struct: ss_ginflate.h)
std::vector<PinSet *> g_pin_free;
std::vector<hipStream_t> g_stream_free;

void arena_destroy(Arena *a)
{
    if (!a) return;
    void *q[] = {a->sym, a->map[0], a->map[1], a->meta, a->status, a->win, a->gwin, a->prev, a->todo, a->text};
    for (void *x : q) if (x) hipFree(x);
    for (void *x : a->late_free) if (x) hipFreeAsync(x, nullptr);
    delete a;
}
Arena *arena_get(uint64_t cap_chunks, uint64_t sym_elems)
{
    Arena *a = nullptr;
    {
        std::lock_guard<std::mutex> g(g_arena_mu);
        if (!g_arena_free.empty()) { a = g_arena_free.back(); g_arena_free.pop_back(); }
    }
    if (a && a->cap_chunks >= cap_chunks && a->sym_elems >= sym_elems) return a;
    uint8_t *text = nullptr;
    uint64_t text_cap = 0;
    if (a) { text = a->text; text_cap = a->text_cap; a->text = nullptr; }      // (the text buffer moves to the new arena)
    arena_destroy(a);
    a = new (std::nothrow) Arena();
    if (a) { a->text = text; a->text_cap = text_cap; } else if (text) hipFree(text);
    if (!a) return nullptr;
    a->cap_chunks = cap_chunks;
    a->sym_elems = sym_elems;
    const uint64_t n_groups = cap_chunks / 8 + 2;
    const bool ok = hipMalloc((void **)&a->sym, sym_elems * 2) == hipSuccess && hipMalloc((void **)&a->map[0], cap_chunks * WSIZE * 2) == hipSuccess &&
                    hipMalloc((void **)&a->map[1], cap_chunks * WSIZE * 2) == hipSuccess && hipMalloc((void **)&a->meta, cap_chunks * 8 * 8) == hipSuccess &&
                    hipMalloc((void **)&a->status, cap_chunks * 4) == hipSuccess && hipMalloc((void **)&a->win, cap_chunks * WSIZE) == hipSuccess &&
                    hipMalloc((void **)&a->gwin, n_groups * WSIZE) == hipSuccess && hipMalloc((void **)&a->prev, WSIZE) == hipSuccess &&
                    hipMalloc((void **)&a->todo, cap_chunks * 4) == hipSuccess;
    if (!ok) { arena_destroy(a); return nullptr; }
    return a;
}
// a waiting arena that needs no allocation for this call (then nothing has to ask the driver how much memory is left: 1-2 ms)
Arena *arena_take_if_fits(uint64_t cap_chunks, uint64_t sym_elems, uint64_t text_cap)
{
    std::lock_guard<std::mutex> g(g_arena_mu);
    for (size_t i = g_arena_free.size(); i-- > 0;) {
        Arena *a = g_arena_free[i];
        if (a->cap_chunks >= cap_chunks && a->sym_elems >= sym_elems && a->text_cap >= text_cap) {
            g_arena_free.erase(g_arena_free.begin() + (long)i);
            return a;
        }
    }
    return nullptr;
}

}  // namespace

void arena_put(Arena *a)
{
    if (!a) return;
    if (a->text_cap > (6ull << 30)) { ss::big_put(a->text, a->text_cap); a->text = nullptr; a->text_cap = 0; }      // (not kept here: the text of a very large file
                                                                                                                      //  becomes a slab of the read set, ss::big_take)
    {
        std::lock_guard<std::mutex> g(g_arena_mu);
        if (g_arena_free.size() < 2) { g_arena_free.push_back(a); return; }
    }
    arena_destroy(a);
}

// A large file image on its way to the device: copied out of a mapping of the page cache the runtime faults the pages in
// one by one (8 GB/s); eight threads that pread() blocks of a few MB into pinned buffers of their own and ship them on streams
// of their own do ~25 GB/s.  The pinned buffers (128 MB a set, at most two sets) are kept like the arenas.
namespace {

constexpr uint64_t PIN_BYTES = 16ull << 20;
constexpr int PIN_N = 8;      // threads = buffers of a set (128 MB a set); each with a stream and two events of its own, made
                              // with the set (a stream costs 2-3 ms to make: as much as the upload of 30 MB)
struct PinSet
{
    uint8_t *b[PIN_N] = {};
    hipStream_t s[PIN_N] = {};
    hipEvent_t ev[PIN_N][2] = {};
};
void pin_destroy(PinSet *p)
{
    if (!p) return;
    for (int i = 0; i < PIN_N; i++) {
        if (p->s[i]) { hipStreamSynchronize(p->s[i]); hipStreamDestroy(p->s[i]); }
        for (int q = 0; q < 2; q++) if (p->ev[i][q]) hipEventDestroy(p->ev[i][q]);
        if (p->b[i]) hipHostFree(p->b[i]);
    }
    delete p;
}
PinSet *pin_get()
{
    {
        std::lock_guard<std::mutex> g(g_arena_mu);
        if (!g_pin_free.empty()) { PinSet *p = g_pin_free.back(); g_pin_free.pop_back(); return p; }
    }
    PinSet *p = new (std::nothrow) PinSet();
    if (!p) return nullptr;
    int device = 0;
    hipGetDevice(&device);
    std::atomic<int> bad(0);
    std::vector<std::thread> th;                              // (~10 ms a buffer, ~3-13 ms a stream: all at the same time)
    for (int i = 0; i < PIN_N; i++)
        th.emplace_back([p, i, device, &bad] {
            if (hipSetDevice(device) != hipSuccess || hipHostMalloc((void **)&p->b[i], PIN_BYTES, hipHostMallocDefault) != hipSuccess ||
                hipStreamCreateWithFlags(&p->s[i], hipStreamNonBlocking) != hipSuccess ||
                hipEventCreateWithFlags(&p->ev[i][0], hipEventDisableTiming) != hipSuccess || hipEventCreateWithFlags(&p->ev[i][1], hipEventDisableTiming) != hipSuccess)
                bad = 1;
        });
    for (auto &t : th) t.join();
    if (bad) { pin_destroy(p); return nullptr; }
    return p;
}
void pin_put(PinSet *p)
{
    if (!p) return;
    {
        std::lock_guard<std::mutex> g(g_arena_mu);
        if (g_pin_free.size() < 2) { g_pin_free.push_back(p); return; }
    }
    pin_destroy(p);
}

}  // namespace

bool pin_waiting()
{
    std::lock_guard<std::mutex> g(g_arena_mu);
    return !g_pin_free.empty();
}
// (`ready`: ss_ginflate.h)
bool upload_file(int fd, uint64_t n, uint8_t *d_in, const std::function<void(uint64_t)> &ready)
{
    static const bool trace = getenv("SS_INGEST_TRACE") != nullptr;
    const auto t_begin = std::chrono::steady_clock::now();
    auto since = [&] { return std::chrono::duration<double>(std::chrono::steady_clock::now() - t_begin).count() * 1e3; };
    // one file at a time on the link: the files of a call would otherwise arrive together, late, and their searches start together;
    // in turn the first one is searched while the second one travels
    static std::mutex link;
    std::lock_guard<std::mutex> my_turn(link);
    PinSet *pins = pin_get();
    if (!pins) return false;
    const double t_pins = since();
    std::atomic<int> streams_up(0);
    double t_streams = 0, t_first = 0;
    int device = 0;
    hipGetDevice(&device);
    std::atomic<uint64_t> next(0);
    std::atomic<int> failed(0);
    // every thread's pinned buffer is used in two halves: the copy of one block travels while the next is read.  Blocks
    // of 1/16 of the file (2 MB .. half a buffer), handed out in order, so that the prefix grows steadily
    const uint64_t half = PIN_BYTES / 2;
    const uint64_t blk = std::min<uint64_t>(half, std::max<uint64_t>(2ull << 20, ((n / 16) + (1ull << 20) - 1) & ~((1ull << 20) - 1)));
    const uint64_t n_blocks = (n + blk - 1) / blk;
    std::vector<uint8_t> done((size_t)n_blocks, 0);
    std::mutex mu;
    uint64_t prefix = 0;                                     // blocks [0, prefix) are on the device
    auto finished = [&](uint64_t b) {
        std::lock_guard<std::mutex> g(mu);
        done[(size_t)b] = 1;
        const uint64_t before = prefix;
        while (prefix < n_blocks && done[(size_t)prefix]) prefix++;
        if (trace && before == 0 && prefix) t_first = since();
        if (prefix != before && ready) ready(std::min(n, prefix * blk));
    };
    std::vector<std::thread> pool;
    const int n_threads = PIN_N;
    for (int t = 0; t < n_threads; t++)
        pool.emplace_back([&, t] {
            hipStream_t s2 = pins->s[t];
            hipEvent_t *ev = pins->ev[t];
            if (hipSetDevice(device) != hipSuccess) failed = 1;
            if (trace && streams_up.fetch_add(1) + 1 == n_threads) t_streams = since();
            int64_t in_flight[2] = {-1, -1};                  // the block whose copy was last issued from each half
            int h = 0;
            for (uint64_t b; !failed && (b = next.fetch_add(1)) < n_blocks; h ^= 1) {
                if (in_flight[h] >= 0) {                      // this half's earlier copy must have left it
                    if (hipEventSynchronize(ev[h]) != hipSuccess) { failed = 1; break; }
                    finished((uint64_t)in_flight[h]);
                    in_flight[h] = -1;
                }
                if (in_flight[h ^ 1] >= 0 && hipEventQuery(ev[h ^ 1]) == hipSuccess) {      // (the other half's: reported as soon as it is seen,
                    finished((uint64_t)in_flight[h ^ 1]);                                     //  the caller works on the prefix that has arrived)
                    in_flight[h ^ 1] = -1;
                }
                const uint64_t a = b * blk, len = std::min<uint64_t>(blk, n - a);
                uint8_t *buf = pins->b[t] + (uint64_t)h * half;
                uint64_t got = 0;
                while (got < len) {
                    const ssize_t r = pread(fd, buf + got, len - got, (off_t)(a + got));
                    if (r <= 0) break;
                    got += (uint64_t)r;
                }
                if (got != len || hipMemcpyAsync(d_in + a, buf, len, hipMemcpyHostToDevice, s2) != hipSuccess ||
                    hipEventRecord(ev[h], s2) != hipSuccess) { failed = 1; break; }
                in_flight[h] = (int64_t)b;
            }
            for (int q = 0; q < 2; q++) {
                const int hh = (h + q) & 1;                   // the older copy first
                if (in_flight[hh] >= 0 && !failed) {
                    if (hipEventSynchronize(ev[hh]) != hipSuccess) failed = 1;
                    else finished((uint64_t)in_flight[hh]);
                }
            }
            hipStreamSynchronize(s2);                       // (a failure may leave a copy in flight: the buffers go back to the pool)
        });
    for (auto &th : pool) th.join();
    pin_put(pins);
    if (trace)
        fprintf(stderr, "[ginflate] upload: %llu blocks of %.1f MB; buffers %.2f ms, threads up %.2f, first block %.2f, all %.2f\n", (unsigned long long)n_blocks,
                blk / 1048576.0, t_pins, t_streams, t_first, since());
    return !failed;
}

// the scratch of a call (ss_ginflate.h)
Arena *acquire_scratch(Arena *a, uint64_t cap_chunks, uint64_t sym_elems, uint64_t text_cap, uint64_t beside, Why *why)
{
    if (!a) a = arena_take_if_fits(cap_chunks, sym_elems, text_cap);
    if (!a) {
        size_t mem_free = 0, mem_total = 0;
        if (hipMemGetInfo(&mem_free, &mem_total) != hipSuccess) { *why = Why{"hipMemGetInfo"}; return nullptr; }
        const uint64_t need = 2 * text_cap + sym_elems * 2 + cap_chunks * WSIZE * 5 + (256ull << 20);
        if (need + beside > mem_free / 2) { *why = Why{"device memory", (long long)(need >> 20)}; return nullptr; }
        a = arena_get(cap_chunks, sym_elems);
        if (!a) { *why = Why{"scratch"}; return nullptr; }
    }
    if (a->text_cap < text_cap) {
        if (a->text) hipFree(a->text);
        a->text = nullptr;
        a->text_cap = 0;
        uint64_t got = text_cap;
        if (ss::big_malloc((void **)&a->text, text_cap, &got) != hipSuccess) { arena_put(a); *why = Why{"text buffer", (long long)(text_cap >> 20)}; return nullptr; }
        a->text_cap = got;
    }
    return a;
}

// (the same way in for other whole files: ss_l2_import's cluster images)
bool upload_file_to_device(int fd, uint64_t n, uint8_t *d_dst) { return upload_file(fd, n, d_dst); }

void gpu_gunzip_done(void *lease)
{
    Arena *a = static_cast<Arena *>(lease);
    if (a)
        for (void *&q : a->late_free) {
            if (q) hipFreeAsync(q, nullptr);                 // (last used on the call's stream, which was synchronised before the text was handed out)
            q = nullptr;
        }
    arena_put(a);
}

// The streams of the calls, kept (making one and destroying it was 0.6 ms of every call), and the stream-ordered allocator
// told to keep what a call frees (1 GB) instead of handing it back to the driver at the next synchronisation.
hipStream_t call_stream_get()
{
    static std::once_flag once;
    std::call_once(once, [] { ss::pool_keep_at_least(1024ull << 20); });
    {
        std::lock_guard<std::mutex> g(g_arena_mu);
        if (!g_stream_free.empty()) { hipStream_t s = g_stream_free.back(); g_stream_free.pop_back(); return s; }
    }
    hipStream_t s = nullptr;
    return hipStreamCreateWithFlags(&s, hipStreamNonBlocking) == hipSuccess ? s : nullptr;
}
void call_stream_put(hipStream_t s)                          // (synchronised by the caller)
{
    if (!s) return;
    {
        std::lock_guard<std::mutex> g(g_arena_mu);
        if (g_stream_free.size() < 4) { g_stream_free.push_back(s); return; }
    }
    hipStreamDestroy(s);
}

}  // namespace ss

// the scratch arenas kept between calls (up to two, ~6 GB each, plus a text buffer) go back to the device
extern "C" int ss_gz_gpu_release(void)
{
    std::vector<ss::Arena *> all;
    std::vector<ss::PinSet *> pins;
    std::vector<hipStream_t> streams;
    {
        std::lock_guard<std::mutex> g(ss::g_arena_mu);
        all.swap(ss::g_arena_free);
        pins.swap(ss::g_pin_free);
        streams.swap(ss::g_stream_free);
    }
    for (ss::Arena *a : all) ss::arena_destroy(a);
    for (ss::PinSet *p : pins) ss::pin_destroy(p);
    for (hipStream_t q : streams) hipStreamDestroy(q);
    ss::reorder_release();
    ss::big_release();
    return SS_OK;
}

// the pinned upload buffers of `n_files` concurrent .gz inputs (at most two sets are kept), made ahead of time
extern "C" int ss_gz_warm_up(int n_files)
{
    std::vector<ss::PinSet *> got;
    for (int i = 0; i < std::min(n_files, 2); i++) {
        ss::PinSet *p = ss::pin_get();
        if (!p) break;
        got.push_back(p);
    }
    const bool ok = (int)got.size() == std::min(n_files, 2);
    for (ss::PinSet *p : got) ss::pin_put(p);
    return ok ? SS_OK : SS_ENOMEM;
}
