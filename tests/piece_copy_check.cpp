// The piece copy of strainscan_amd/csrc/ss_piece_copy.h on the host: a stand-alone program (g++, AddressSanitizer + UBSan) that
// plays the sixteen lanes of a record one after the other over a host buffer and compares with a byte-by-byte model.  The piece_of
// lambdas are those of the kernels: gather_kernel (ss_select.hip), record_gather_kernel (ss_bam_extract.hip), join_kernel
// (ss_pairs.hip: the 'N' alone) and join_kernel (ss_bam_pairs.hip: the 'N' and the '\n').  Every source block is a heap block of
// exactly n bytes, so a load outside it stops the program; every destination span has guard bytes in front and behind, which
// must stay as they were.  Both sweeps are exhaustive over what they list; nothing is sampled.
//     g++ -std=c++17 -fsanitize=address,undefined -I strainscan_amd/csrc tests/piece_copy_check.cpp -o piece_copy_check
#include "ss_piece_copy.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

using namespace ss::dev;

namespace {

constexpr uint8_t GUARD = 0xEE;
unsigned long long g_cases = 0;

[[noreturn]] void die(const char *what, long a = 0, long b = 0, long c = 0, long d = 0, long e = 0, long f = 0)
{
    printf("piece_copy_check FAILED: %s (%ld %ld %ld %ld %ld %ld)\n", what, a, b, c, d, e, f);
    exit(1);
}

// a heap block of exactly n bytes, none of them '\n', 'N' or the guard, no two neighbours equal
struct Block {
    uint8_t *p;
    uint64_t n;
    Block(uint64_t n_, uint32_t salt) : p((uint8_t *)malloc(n_)), n(n_)
    {
        for (uint64_t i = 0; i < n; i++) p[i] = (uint8_t)(0x30 + (i * 7 + salt) % 0x19);      // '0' .. 'H'
    }
    ~Block() { free(p); }
    Block(const Block &) = delete;
};

// a 16-byte aligned destination; a case uses its first n bytes: two pieces of guard, the span, two pieces of guard and more
struct Dest {
    uint8_t *p;
    uint64_t cap, n = 0;
    explicit Dest(uint64_t cap_) : p((uint8_t *)aligned_alloc(16, cap_)), cap(cap_) {}
    ~Dest() { free(p); }
    Dest(const Dest &) = delete;
    void clear(uint64_t span_end)
    {
        n = ((span_end + 15u) & ~15ull) + 32u;
        if (n > cap) die("destination too small", (long)n, (long)cap);
        memset(p, GUARD, n);
    }
};

// the model: want(i) is byte i of the span [D, E), everything else is guard
template <class Want>
void compare(const Dest &dst, uint64_t D, uint64_t E, Want &&want, const char *what, long a, long b, long c, long d, long e)
{
    for (uint64_t i = 0; i < dst.n; i++) {
        const uint8_t w = i >= D && i < E ? want(i - D) : GUARD;
        if (dst.p[i] != w) die(what, a, b, c, d, e, (long)i);
    }
    g_cases++;
}

void check_arithmetic()
{
    piece_t x = 0;
    for (uint32_t j = 0; j < 16; j++) x |= (piece_t)(0xA0u + j) << (8u * j);
    auto byte = [](piece_t v, int j) { return (uint32_t)((v >> (8 * j)) & 0xFFu); };
    for (int64_t sh = -300; sh <= 300; sh++) {                          // 16 bytes and more, either way: all zero, never a 128-bit shift
        const piece_t y = shift_into_piece(x, sh);
        for (int j = 0; j < 16; j++) {
            const int64_t from = j + sh;
            if (byte(y, j) != (from >= 0 && from < 16 ? 0xA0u + (uint32_t)from : 0u)) die("shift_into_piece", (long)sh, j);
        }
    }
    if (shift_into_piece(x, INT64_MIN) != 0 || shift_into_piece(x, INT64_MAX) != 0) die("shift_into_piece at the ends of int64");
    for (uint32_t j0 = 0; j0 < 16; j0++)
        for (uint32_t j1 = j0 + 1; j1 <= 16; j1++) {
            const piece_t m = piece_mask(j0, j1);
            for (uint32_t j = 0; j < 16; j++)
                if (byte(m, (int)j) != (j >= j0 && j < j1 ? 0xFFu : 0u)) die("piece_mask", j0, j1, j);
        }
    for (uint32_t j = 0; j < 16; j++) {
        const piece_t y = with_byte(x, j, '\n');
        for (uint32_t i = 0; i < 16; i++)
            if (byte(y, (int)i) != (i == j ? 0x0Au : 0xA0u + i)) die("with_byte", j, i);
        if (byte(with_byte(x, j, (char)0xF3), (int)j) != 0xF3u) die("with_byte of a byte above 0x7F", j);
    }
    for (uint64_t n : {16ull, 17ull, 64ull})
        for (int64_t base = -40; base <= (int64_t)n + 40; base++) {
            const int64_t q = clamp_base(base, n), want = base < 0 ? 0 : (base > (int64_t)n - 16 ? (int64_t)n - 16 : base);
            if (q != want || q < 0 || q + 16 > (int64_t)n) die("clamp_base", (long)n, (long)base);
        }
    for (uint64_t n : {16ull, 64ull}) {                                 // fetch16: the block's bytes where there are any, else 0
        const Block b(n, 5);
        for (int64_t base = -40; base <= (int64_t)n + 40; base++) {
            const piece_t y = fetch16(b.p, n, base);
            for (int j = 0; j < 16; j++) {
                const int64_t p = base + j;
                if (byte(y, j) != (p >= 0 && p < (int64_t)n ? b.p[p] : 0u)) die("fetch16", (long)n, (long)base, j);
            }
        }
    }
}

// Sweep 1, the single-source copy: a record of len bytes at S of a block of n bytes, w copies of it back to back from D on.
// newline: gather_kernel's piece (a '\n' behind every copy); else record_gather_kernel's (the bytes as they are, len >= 1).
void sweep_single()
{
    Dest dst(768);      // 32 + 15 + 13 * 50 + 47 and some
    for (const uint64_t n : {16ull, 64ull}) {
        const Block src(n, 1);
        for (int newline = 0; newline < 2; newline++)
            for (uint64_t len = newline ? 0 : 1; len <= 49 && len <= n; len++)
                for (uint64_t S = 0; S + len <= n; S++)                 // the start of the block, every place between, ending exactly at n
                    for (uint64_t dmod = 0; dmod < 16; dmod++)
                        for (const uint64_t w : {1ull, 2ull, 13ull}) {
                            const uint64_t D0 = 32 + dmod, ol = len + (uint64_t)newline;
                            dst.clear(D0 + w * ol);
                            for (uint64_t k = 0; k < w; k++) {
                                const uint64_t D = D0 + k * ol;
                                for (uint32_t lane = 0; lane < 16; lane++)
                                    write_span(dst.p, D, D + ol, lane, [&](uint64_t a, uint64_t, uint64_t) {
                                        const piece_t x = fetch16(src.p, n, (int64_t)S + ((int64_t)a - (int64_t)D));
                                        return newline && D + len < a + 16u ? with_byte(x, (uint32_t)(D + len - a), '\n') : x;
                                    });
                            }
                            auto want = [&](uint64_t i) { return i % ol == len ? (uint8_t)'\n' : src.p[S + i % ol]; };
                            compare(dst, D0, D0 + w * ol, want, newline ? "gather" : "record gather", (long)n, (long)len, (long)S, (long)dmod, (long)w);
                        }
    }
}

// Sweep 2, the two-source join: line1 + 'N' + line2 + '\n' from D on.  with_nl == 0: ss_pairs.hip's piece -- either mate brings
// the '\n' behind it along, and the 'N' replaces mate 1's; with_nl == 1: ss_bam_pairs.hip's -- the letters alone are fetched, and
// the 'N' and the '\n' are put in.  A source: a block of 16 bytes (the padded private copy of a short block) or of 64, the line at
// its start, inside it, or ending with it.
void sweep_join()
{
    Dest dst(128);
    struct Source { uint64_t n, s; };
    auto sources = [](uint64_t len, int with_nl) {
        std::vector<Source> v;
        const uint64_t need = len + (with_nl ? 0u : 1u);                // the line, and its '\n' where that is fetched too
        for (const uint64_t n : {16ull, 64ull}) {
            if (need > n) continue;
            v.push_back({n, 0});
            if (n == 64 && 21 + need < n) v.push_back({n, 21});
            if (n - need != 0) v.push_back({n, n - need});
        }
        return v;
    };
    Block b16a(16, 2), b64a(64, 3), b16b(16, 4), b64b(64, 6);
    for (int with_nl = 0; with_nl < 2; with_nl++)
        for (uint64_t len1 = 0; len1 <= 18; len1++)
            for (uint64_t len2 = 0; len2 <= 18; len2++)
                for (const Source &q1 : sources(len1, with_nl))
                    for (const Source &q2 : sources(len2, with_nl)) {
                        Block &B1 = q1.n == 16 ? b16a : b64a, &B2 = q2.n == 16 ? b16b : b64b;
                        const uint64_t s1 = q1.s, s2 = q2.s, n1 = q1.n, n2 = q2.n;
                        uint8_t keep1 = 0, keep2 = 0;
                        if (!with_nl) {                                 // the '\n' that ends either line in its block
                            keep1 = B1.p[s1 + len1], keep2 = B2.p[s2 + len2];
                            B1.p[s1 + len1] = '\n', B2.p[s2 + len2] = '\n';
                        }
                        auto want = [&](uint64_t i) {
                            return i < len1 ? B1.p[s1 + i] : i == len1 ? (uint8_t)'N' : i <= len1 + len2 ? B2.p[s2 + (i - len1 - 1u)] : (uint8_t)'\n';
                        };
                        for (uint64_t dmod = 0; dmod < 16; dmod++) {
                            const uint64_t D = 32 + dmod, J = D + len1, M2 = J + 1u, L = M2 + len2, E = L + 1u;
                            dst.clear(E);
                            for (uint32_t lane = 0; lane < 16; lane++) {
                                if (with_nl)
                                    write_span(dst.p, D, E, lane, [&](uint64_t a, uint64_t lo, uint64_t hi) {
                                        piece_t x = masked_fetch16(B1.p, n1, s1, D, J, a, lo, hi) | masked_fetch16(B2.p, n2, s2, M2, L, a, lo, hi);
                                        if (J >= lo && J < hi) x = with_byte(x, (uint32_t)(J - a), 'N');
                                        if (L >= lo && L < hi) x = with_byte(x, (uint32_t)(L - a), '\n');
                                        return x;
                                    });
                                else
                                    write_span(dst.p, D, E, lane, [&](uint64_t a, uint64_t lo, uint64_t hi) {
                                        const piece_t x = masked_fetch16(B1.p, n1, s1, D, M2, a, lo, hi) | masked_fetch16(B2.p, n2, s2, M2, E, a, lo, hi);
                                        return J >= a && J < a + 16u ? with_byte(x, (uint32_t)(J - a), 'N') : x;
                                    });
                            }
                            compare(dst, D, E, want, with_nl ? "join with 'N' and newline" : "join with 'N'", (long)len1, (long)len2, (long)(n1 * 100 + s1),
                                    (long)(n2 * 100 + s2), (long)dmod);
                        }
                        if (!with_nl) B1.p[s1 + len1] = keep1, B2.p[s2 + len2] = keep2;
                    }
}

}  // namespace

int main()
{
    check_arithmetic();
    sweep_single();
    const unsigned long long single = g_cases;
    sweep_join();
    printf("piece_copy_check ok: %llu single-source copies, %llu joins\n", single, g_cases - single);
    return 0;
}
