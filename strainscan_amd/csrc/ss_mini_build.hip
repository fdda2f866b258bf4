// ss_mini_build.hip -- the page index of ss_mini.hip (its layout: the comment there) built on the host, and the PG_SOLID flags
// that either build's image gets on the device.
#include "ss_common.h"
#include "ss_scan_dev.h"

#include <algorithm>
#include <atomic>
#include <chrono>
#include <functional>
#include <memory>
#include <thread>
#include <vector>

namespace {

struct Ent {
    uint32_t mini;
    uint32_t row;
    uint64_t key;
    uint32_t off;   // offset of the minimizer inside the k-mer (sort key inside the bucket)
    uint32_t part;  // partition of the build sort
};

void parallel_for(unsigned nthreads, uint64_t n, const std::function<void(uint64_t, uint64_t, unsigned)> &fn)
{
    if (nthreads <= 1 || n < 65536) { fn(0, n, 0); return; }
    std::vector<std::thread> pool;
    const uint64_t per = (n + nthreads - 1) / nthreads;
    for (unsigned w = 0; w < nthreads; w++) {
        const uint64_t lo = std::min<uint64_t>(n, per * w), hi = std::min<uint64_t>(n, lo + per);
        if (lo >= hi) break;
        pool.emplace_back(fn, lo, hi, w);
    }
    for (auto &th : pool) th.join();
}

}  // namespace

namespace ss {

// Host build of the minimizer index.  Fills db->d_mkeys / d_dir / d_counts / d_slot_of_row /
// d_row_valid and n_distinct; returns SS_EKEY for an un-owned k-mer when upper_keys == 0.
int build_mini(ss_db *db, const uint64_t *keys, const uint8_t *flags, uint64_t n_rows, int upper_keys)
{
    // the device build first (ss_build_dev.hip: the same image, byte for byte, in a fraction of the time); SS_BUILD=host, or
    // anything it could not do (no memory, an empty table, a HIP error), leaves the work to the host build below
    {
        const char *b = getenv("SS_BUILD");
        if (!(b && !strcmp(b, "host")) && db->k == 31) {
            const int rc = build_mini_dev(db, keys, flags, n_rows, upper_keys);
            if (rc == SS_OK || rc == SS_EKEY) return rc;
            if (getenv("SS_BUILD_TRACE")) fprintf(stderr, "[build] device build declined (%d): host build\n", rc);
        }
    }
    const int k = db->k;
    static const bool trace = getenv("SS_BUILD_TRACE") != nullptr;
    const auto t_begin = std::chrono::steady_clock::now();
    auto lap = [&](const char *what) {
        if (trace) fprintf(stderr, "[build] %-28s at %.3f s\n", what, std::chrono::duration<double>(std::chrono::steady_clock::now() - t_begin).count());
    };
    constexpr int PB = 8, NP = 1 << PB;
    unsigned nthreads = std::min<unsigned>(ss::host_cpus(), 32u);
    if (const char *e = getenv("SS_BUILD_THREADS")) nthreads = (unsigned)std::max(1, std::min(64, atoi(e)));   // tests: the image must not depend on it
    uint32_t inline_max = 2;                        // minimizers with at most this many database k-mers keep them in page slots
                                                    // (decided below, once the minimizers' sizes are known: choose_inline_max)
    double lambda = 2.0;                            // page items per page on average (eight slots: one page in a thousand full)
    if (const char *e = getenv("SS_PAGE_LAMBDA")) lambda = std::max(0.25, std::min(7.8, atof(e)));   // < 8: the pages must hold all items
    // 1. entries of valid rows with their minimizer
    std::vector<uint64_t> pos(n_rows + 1, 0);
    for (uint64_t i = 0; i < n_rows; i++) pos[i + 1] = pos[i] + ((flags[i] & SS_ROW_VALID) ? 1 : 0);
    const uint64_t nv = pos[n_rows];
    // (plain arrays: a std::vector would zero 2 x 0.8 GB on one thread first)
    std::unique_ptr<Ent[]> ents_buf(new (std::nothrow) Ent[std::max<uint64_t>(nv, 1)]), sorted_buf(new (std::nothrow) Ent[std::max<uint64_t>(nv, 1)]);
    if (!ents_buf || !sorted_buf) return SS_ENOMEM;
    Ent *ents = ents_buf.get(), *sorted = sorted_buf.get();
    parallel_for(nthreads, n_rows, [&](uint64_t lo, uint64_t hi, unsigned) {
        for (uint64_t i = lo; i < hi; i++)
            if (flags[i] & SS_ROW_VALID) {
                uint32_t o;
                const uint32_t mx = mini_of_key(keys[i], k, &o);
                ents[pos[i]] = Ent{mx, (uint32_t)i, keys[i], o, mix30(mx) >> (30 - PB)};
            }
    });
    lap("1 minimizers");
    // 2. counting partition on the top 8 bits of h = mix30(minimizer) -- the page order --, then per-partition sort
    //    (threads over index ranges, each with its own counts and cursors: within a partition the entries keep their
    //     index order, whatever the thread count -- a serial pass took 0.15 s of scattered 32-byte writes)
    std::vector<uint64_t> pcount(NP + 1, 0);
    {
        const unsigned T = nv < (1u << 20) ? 1u : nthreads;
        const uint64_t per = (nv + T - 1) / T;
        std::vector<std::vector<uint64_t>> cnt(T, std::vector<uint64_t>(NP, 0));
        auto each_thread = [&](const std::function<void(unsigned)> &fn) {
            std::vector<std::thread> pool;
            for (unsigned w = 1; w < T; w++) pool.emplace_back(fn, w);
            fn(0);
            for (auto &th : pool) th.join();
        };
        each_thread([&](unsigned w) {
            for (uint64_t i = std::min(nv, per * w), e = std::min(nv, per * (w + 1)); i < e; i++) cnt[w][ents[i].part]++;
        });
        uint64_t run = 0;
        for (int p = 0; p < NP; p++) {
            pcount[p] = run;
            for (unsigned w = 0; w < T; w++) { const uint64_t c = cnt[w][p]; cnt[w][p] = run; run += c; }      // -> this thread's cursor
        }
        pcount[NP] = run;
        each_thread([&](unsigned w) {
            for (uint64_t i = std::min(nv, per * w), e = std::min(nv, per * (w + 1)); i < e; i++) sorted[cnt[w][ents[i].part]++] = ents[i];
        });
    }
    ents_buf.reset();
    auto for_partitions = [&](const std::function<void(int)> &fn) {
        std::atomic<int> next(0);
        std::vector<std::thread> pool;
        for (unsigned w = 0; w < nthreads; w++)
            pool.emplace_back([&] { for (int p; (p = next.fetch_add(1)) < NP;) fn(p); });
        for (auto &th : pool) th.join();
    };
    for_partitions([&](int p) {
        std::sort(sorted + pcount[p], sorted + pcount[p + 1], [](const Ent &a, const Ent &b) {
            if (a.mini != b.mini) return a.mini < b.mini;
            if (a.off != b.off) return a.off < b.off;
            if (a.key != b.key) return a.key < b.key;
            return a.row < b.row;
        });
    });
    lap("2 partition + sort");
    // 3. distinct k-mers per minimizer.  Small sets become inline page items (one per k-mer), larger ones a bucket
    //    of d_mkeys (header + k-mers) plus ONE page item, the reference.  Row bookkeeping: dict overwrite, the last
    //    allowed row owns the count.  A minimizer lives in one partition, so the partitions are independent: count,
    //    prefix-sum, fill in parallel (same order as a serial walk: the image does not depend on the thread count).
    struct Item { uint32_t h, lo; uint16_t mid; uint8_t hi8; uint64_t e0, e1; };   // page item; [e0, e1) = its rows in `sorted` (inline items)
    std::vector<uint64_t> p_slots(NP + 1, 0), p_items(NP + 1, 0), p_minis(NP + 1, 0);
    auto walk = [&](int p, const std::function<void(uint64_t, uint64_t, uint32_t)> &bucket) {   // [i, e) = one minimizer, nd distinct k-mers
        for (uint64_t i = pcount[p]; i < pcount[p + 1];) {
            uint64_t e = i;
            uint32_t nd = 0;
            uint64_t last = ~0ull;
            while (e < pcount[p + 1] && sorted[e].mini == sorted[i].mini) {
                if (sorted[e].key != last) { nd++; last = sorted[e].key; }
                e++;
            }
            bucket(i, e, nd);
            i = e;
        }
    };
    {
        std::atomic<uint64_t> small_a(0), all_a(0);
        for_partitions([&](int p) {
            uint64_t sm = 0, al = 0;
            walk(p, [&](uint64_t, uint64_t, uint32_t nd) { al += nd; if (nd <= 2) sm += nd; });
            small_a += sm; all_a += al;
        });
        inline_max = choose_inline_max(small_a.load(), all_a.load());
    }
    for_partitions([&](int p) {
        uint64_t ns_ = 0, ni = 0, nm = 0;
        walk(p, [&](uint64_t, uint64_t, uint32_t nd) {
            nm++;
            if (nd <= inline_max) ni += nd;
            else { ni++; ns_ += 1 + nd; }
        });
        p_slots[p + 1] = ns_; p_items[p + 1] = ni; p_minis[p + 1] = nm;
    });
    for (int p = 0; p < NP; p++) { p_slots[p + 1] += p_slots[p]; p_items[p + 1] += p_items[p]; p_minis[p + 1] += p_minis[p]; }
    const uint64_t n_mslots = std::max<uint64_t>(1, p_slots[NP]), n_items = p_items[NP], n_minis = p_minis[NP];
    if (n_mslots >= (uint64_t)START_MASK) return SS_ERANGE;
    uint64_t n_pages = std::max<uint64_t>(PG_MIN_PAGES, (uint64_t)((double)n_items / lambda) + 1);
    std::vector<uint64_t> mkeys(n_mslots, 0);
    std::vector<Item> items(n_items);
    std::vector<uint32_t> slot_of_row(std::max<uint64_t>(1, n_rows), SS_NO_SLOT);
    std::vector<uint8_t> row_valid(std::max<uint64_t>(1, n_rows), 0);
    std::atomic<uint64_t> orphans_a(0), n_distinct_a(0);
    for_partitions([&](int p) {
        uint64_t ms = p_slots[p], it = p_items[p], orph = 0, ndist = 0;
        walk(p, [&](uint64_t i, uint64_t e, uint32_t nd) {
            const uint32_t h = mix30(sorted[i].mini);
            const bool inl = nd <= inline_max;
            const uint32_t hslot = (uint32_t)ms;
            if (!inl) ms++;
            uint32_t mask = 0, multi = 0;
            for (uint64_t a2 = i; a2 < e;) {
                uint64_t b2 = a2;
                int64_t owner = -1;
                while (b2 < e && sorted[b2].key == sorted[a2].key) {
                    const uint32_t r = sorted[b2].row;
                    if (upper_keys == 1 || !(flags[r] & SS_ROW_LOWER)) owner = r;   // rows ascend within equal k-mers
                    b2++;
                }
                const uint32_t o = sorted[a2].off;
                if (inl) {
                    items[it++] = Item{h, flank_of_key_k(sorted[a2].key, o, k), (uint16_t)(((h >> 8) & 0xFFFu) << 4), (uint8_t)((uint32_t)(k - MINI_M) - o), a2, b2};      // (e = k - 15 - o: 16 - o at k = 31)
                } else {
                    if ((mask >> o) & 1u) multi = 1u;
                    mask |= 1u << o;
                    const uint32_t slot = (uint32_t)ms;
                    mkeys[ms++] = sorted[a2].key;
                    for (uint64_t q = a2; q < b2; q++) slot_of_row[sorted[q].row] = slot;
                }
                if (owner >= 0) row_valid[owner] = 1;
                else orph++;
                ndist++;
                a2 = b2;
            }
            if (!inl) {
                mkeys[hslot] = ((uint64_t)nd << 32) | (multi ? HDR_MULTI : 0u) | mask;
                items[it++] = Item{h, (multi << 31) | hslot, (uint16_t)(mask & 0xFFFFu), (uint8_t)(0x80u | ((mask >> 16) << 6) | ((h >> 8) & 0x3Fu)), 0, 0};
            }
        });
        // page order inside the partition (the partitions themselves are h ranges); stable: a minimizer's items stay together
        std::stable_sort(items.begin() + p_items[p], items.begin() + p_items[p + 1], [](const Item &a, const Item &b) { return a.h < b.h; });
        orphans_a += orph;
        n_distinct_a += ndist;
    });
    const uint64_t orphans = orphans_a.load();
    if (orphans && upper_keys == 0) return SS_EKEY;
    db->n_distinct = n_distinct_a.load();
    lap("3 buckets + items");
    // 4. place the items: home page = page_of(h), or the first page behind it that is not full (a lookup reads on while
    //    the page it sees is full; no wrap-around: a few spare pages follow the last home page).  Serial in h order:
    //    ~20 ns per item.  Exactness of the inline slots: two minimizers whose h agree in the 20 tag bits have home pages
    //    >= D = n_pages / 1024 apart, so neither's lookup can reach the other's slots as long as every run of
    //    consecutive full pages is shorter than D -- checked here; the table grows until it holds (at two items per
    //    page a run of four full pages has probability 1e-12).
    std::vector<uint8_t> pages;
    uint64_t n_alloc = 0;
    for (;; n_pages += n_pages / 4) {
        if (n_mslots + (n_pages + n_pages / 1024) * PG_SLOTS >= 0xFFFFFFF0ull) return SS_ERANGE;
        const uint64_t D = n_pages / 1024;
        n_alloc = n_pages + D;
        pages.resize(n_alloc * 64);
        std::vector<uint8_t> fill(n_alloc, 0);
        parallel_for(nthreads, n_alloc, [&](uint64_t lo, uint64_t hi, unsigned) {
            for (uint64_t pg = lo; pg < hi; pg++) {
                memset(&pages[pg * 64], PG_EMPTY_TAG, 8);
                memset(&pages[pg * 64 + 8], PG_EMPTY_HI, 8);
                memset(&pages[pg * 64 + 16], 0, 48);
            }
        });
        // partition p (the items whose h has top byte p) owns the pages [lo(p), lo(p + 1)); its thread places its items
        // there; items that run past the end of the range (or whose home page straddles into the next range) are
        // placed afterwards, serially, in h order -- the same image for any thread count
        auto place = [&](const Item &it, uint64_t pg, uint64_t end) -> bool {
            while (pg < end && fill[pg] == PG_SLOTS) pg++;
            if (pg >= end) return false;
            const uint32_t sl = fill[pg]++;
            uint8_t *pp = &pages[pg * 64];
            pp[sl] = (uint8_t)(it.h & 0xFFu);
            pp[8 + sl] = it.hi8;
            memcpy(pp + 16 + 4 * sl, &it.lo, 4);
            memcpy(pp + 48 + 2 * sl, &it.mid, 2);
            for (uint64_t q = it.e0; q < it.e1; q++) slot_of_row[sorted[q].row] = (uint32_t)(n_mslots + pg * PG_SLOTS + sl);
            return true;
        };
        auto lo_of = [&](int pt) -> uint64_t { return pt >= NP ? n_pages : page_of((uint32_t)pt << (30 - PB), (uint32_t)n_pages); };
        std::vector<std::vector<uint64_t>> spill(NP);
        for_partitions([&](int pt) {
            const uint64_t end = lo_of(pt + 1);
            for (uint64_t i = p_items[pt]; i < p_items[pt + 1]; i++)
                if (!place(items[i], page_of(items[i].h, (uint32_t)n_pages), end)) spill[pt].push_back(i);
        });
        bool ok = true;
        for (int pt = 0; pt < NP && ok; pt++)
            for (uint64_t i : spill[pt])
                if (!place(items[i], std::max<uint64_t>(page_of(items[i].h, (uint32_t)n_pages), lo_of(pt + 1)), n_alloc)) { ok = false; break; }
        uint64_t run = 0, longest = 0;
        for (uint64_t pg = 0; pg < n_alloc && ok; pg++) {
            run = fill[pg] == PG_SLOTS ? run + 1 : 0;
            longest = std::max(longest, run);
        }
        if (ok && longest < D && fill[n_alloc - 1] < PG_SLOTS) break;
    }
    sorted_buf.reset();
    db->n_mslots = n_mslots;
    db->n_inline = (db->n_distinct + n_items - p_slots[NP]) / 2;   // items = inline k-mers + references; bucket slots = references + their k-mers
    db->n_slots = n_mslots + n_alloc * PG_SLOTS;
    db->n_dir = (uint32_t)n_pages;
    db->n_dir_alloc = (uint32_t)n_alloc;
    db->dirbits = 0;
    db->n_buckets = n_minis;
    db->capacity = db->n_slots;
    lap("4 pages");
    // 5. upload
    const uint64_t nr = std::max<uint64_t>(1, n_rows);
    SS_HIP(hipMalloc((void **)&db->d_mkeys, n_mslots * sizeof(uint64_t)));
    SS_HIP(hipMalloc((void **)&db->d_dir, pages.size()));
    SS_HIP(hipMalloc((void **)&db->d_counts, db->n_slots * sizeof(uint32_t)));
    SS_HIP(hipMalloc((void **)&db->d_slot_of_row, nr * sizeof(uint32_t)));
    SS_HIP(hipMalloc((void **)&db->d_row_valid, nr));
    db->device_bytes = n_mslots * 8 + db->n_slots * 4 + pages.size() + nr * 5;
    SS_HIP(hipMemcpy(db->d_mkeys, mkeys.data(), n_mslots * sizeof(uint64_t), hipMemcpyHostToDevice));
    SS_HIP(hipMemcpy(db->d_dir, pages.data(), pages.size(), hipMemcpyHostToDevice));
    SS_HIP(hipMemset(db->d_counts, 0, db->n_slots * sizeof(uint32_t)));
    {
        // Bloom filter over the minimizers, at most 2^25 bits = 4 MB (the L2 of one XCD; measured on a 25 M-row table of
        // dense node sets -- 2.8 M minimizers -- 2^23: 4.71 ms, 2^25: 4.60 ms, 2^27: 5.29 ms, none: 6.0 ms), and only
        // with >= 4 bits per minimizer: on a table of SAMPLED node sets (17 M minimizers) the filter passes 40 % of the
        // absent minimizers, half of the runs find theirs anyway, and the scan is 7 % faster without it (7.73 -> 7.18 ms).
        // SS_BLOOM_BITS=0 disables, = n forces 2^n bits.
        int bits = 10;
        while (bits < 25 && (1ull << bits) < 8 * n_minis) bits++;
        if ((1ull << bits) < 4 * n_minis) bits = 0;
        const char *bb = getenv("SS_BLOOM_BITS");
        if (bb) bits = atoi(bb);
        if (bits >= 10 && bits <= 30) {
            std::vector<uint32_t> bloom((size_t)1 << (bits - 5), 0);
            uint32_t last = ~0u;
            for (const auto &it : items) {
                if (it.h == last) continue;
                last = it.h;
                const uint32_t hb = it.h >> (30 - bits);
                bloom[hb >> 5] |= 1u << (hb & 31u);
            }
            SS_HIP(hipMalloc((void **)&db->d_bloom, bloom.size() * 4));
            SS_HIP(hipMemcpy(db->d_bloom, bloom.data(), bloom.size() * 4, hipMemcpyHostToDevice));
            db->bloom_bits = (uint32_t)bits;
            db->device_bytes += bloom.size() * 4;
        }
    }
    SS_HIP(hipMemcpy(db->d_slot_of_row, slot_of_row.data(), nr * sizeof(uint32_t), hipMemcpyHostToDevice));
    SS_HIP(hipMemcpy(db->d_row_valid, row_valid.data(), nr, hipMemcpyHostToDevice));
    lap("5 bloom + upload");
    return mark_solid(db);
}

// PG_SOLID for every bucket whose k-mers are one stretch of bases (ss_scan_dev.h): one thread per page slot, after either
// build has put pages and buckets on the device -- the same flags whichever build made the image.
__global__ __launch_bounds__(256) void mark_solid_kernel(uint8_t *__restrict__ pages, uint64_t n_page_slots, const uint64_t *__restrict__ mkeys, int k_of_db)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_page_slots) return;
    uint8_t *pp = pages + (i >> 3) * 64;
    const uint32_t sl = (uint32_t)(i & 7u);
    if (!(pp[8 + sl] & 0x80u)) return;                                   // an inline k-mer, or empty
    uint32_t *lo32 = reinterpret_cast<uint32_t *>(pp + 16) + sl;
    const uint32_t lo = *lo32;
    if (lo >> 31) return;                                                // several k-mers per offset
    const uint32_t b = lo & ss::START_MASK;
    const uint64_t hdr = mkeys[b];
    const uint32_t mask = (uint32_t)hdr & 0x1FFFFu, cnt = (uint32_t)(hdr >> 32);
    if ((hdr & ss::HDR_MULTI) || !mask || cnt != (uint32_t)__popc(mask)) return;
    const uint32_t m = mask >> (__ffs(mask) - 1);
    if (m & (m + 1u)) return;                                            // a gap in the offsets
    // slots ascend with the offset; the k-mer of offset o + 1 begins one base before the k-mer of offset o
    for (uint32_t k = 1; k < cnt; k++)
        if ((mkeys[b + k] & ((1ull << (2 * k_of_db - 2)) - 1ull)) != (mkeys[b + k + 1] >> 2)) return;
    *lo32 = lo | ss::PG_SOLID;
}

int mark_solid(ss_db *db)
{
    const uint64_t n = (uint64_t)db->n_dir_alloc * ss::PG_SLOTS;
    if (!n) return SS_OK;
    hipLaunchKernelGGL(mark_solid_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, (uint8_t *)db->d_dir, n, db->d_mkeys, db->k);
    SS_HIP(hipGetLastError());
    SS_HIP(hipDeviceSynchronize());
    return SS_OK;
}

}  // namespace ss
