// The tagged-record copy of strainscan_amd/csrc/ss_tag_copy.h on the host: a stand-alone program (g++, AddressSanitizer + UBSan)
// that plays the sixteen lanes of tag_copy_kernel (ss_bam_tag.hip) one after the other over a host buffer and compares with a
// memcpy composition: the raised block_size, the record's bytes behind it, the 14 tag bytes.  Every source block is a heap block of
// exactly n bytes, so a load outside it stops the program; every destination span has guard bytes in front and behind, which must
// stay as they were.  The sweep is exhaustive over what it lists: every destination alignment (D mod 16) x record lengths 36..83
// (every length mod 16, three times) x tagged and untagged x the record at the start, inside and at the end of its block.
// aux_walk is checked on heap blocks of the exact field bytes: every type, every B subtype, the malformed forms.
//     g++ -std=c++17 -fsanitize=address,undefined -I strainscan_amd/csrc tests/tag_copy_check.cpp -o tag_copy_check
#include "ss_tag_copy.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

using namespace ss::dev;

namespace {

constexpr uint8_t GUARD = 0xEE;
unsigned long long g_copies = 0, g_walks = 0;

[[noreturn]] void die(const char *what, long a = 0, long b = 0, long c = 0, long d = 0, long e = 0)
{
    printf("tag_copy_check FAILED: %s (%ld %ld %ld %ld %ld)\n", what, a, b, c, d, e);
    exit(1);
}

void put32(uint8_t *p, uint32_t v)
{
    for (int i = 0; i < 4; i++) p[i] = (uint8_t)(v >> (8 * i));
}

// one record of ol bytes at S in a heap block of exactly n bytes, copied to D as the kernel copies it
void one_copy(uint64_t n, uint64_t S, uint64_t ol, uint64_t D, bool tagged, uint32_t tags, int32_t value, uint32_t score)
{
    uint8_t *src = (uint8_t *)malloc(n);
    for (uint64_t i = 0; i < n; i++) src[i] = (uint8_t)(0x30 + (i * 7 + ol) % 0x4F);
    put32(src + S, (uint32_t)(ol - 4));
    const uint64_t E = D + ol + (tagged ? TAG_BYTES : 0u), cap = ((E + 15u) & ~15ull) + 32u;
    uint8_t *dst = (uint8_t *)aligned_alloc(16, cap);
    memset(dst, GUARD, cap);
    const piece_t tag = tag_fields(tags, value, score);
    for (uint32_t lane = 0; lane < 16; lane++) {
        if (tagged)
            write_span(dst, D, E, lane, [&](uint64_t a, uint64_t lo, uint64_t hi) { return tagged_piece(src, n, S, ol, D, tag, a, lo, hi); });
        else
            write_span(dst, D, E, lane, [&](uint64_t a, uint64_t, uint64_t) { return fetch16(src, n, (int64_t)S + ((int64_t)a - (int64_t)D)); });
    }
    std::vector<uint8_t> want(cap, GUARD);
    memcpy(want.data() + D, src + S, ol);
    if (tagged) {
        put32(want.data() + D, (uint32_t)(ol - 4 + 14));
        uint8_t *t = want.data() + D + ol;
        t[0] = (uint8_t)tags; t[1] = (uint8_t)(tags >> 8); t[2] = 'i';
        put32(t + 3, (uint32_t)value);
        t[7] = (uint8_t)(tags >> 16); t[8] = (uint8_t)(tags >> 24); t[9] = 'i';
        put32(t + 10, score);
    }
    for (uint64_t i = 0; i < cap; i++)
        if (dst[i] != want[i]) die("copy", (long)n, (long)S, (long)ol, (long)D, (long)i);
    free(dst);
    free(src);
    g_copies++;
}

void check_copies()
{
    const uint32_t tags = 's' | 'n' << 8 | 's' << 16 | (uint32_t)'c' << 24;
    const int32_t values[3] = {-1, 0x12345678, 7};
    const uint32_t scores[3] = {0, 0x00A1B2C3, 0x7FFFFFFF};
    for (uint64_t ol = 36; ol < 84; ol++)
        for (uint64_t D0 = 0; D0 < 16; D0++)
            for (int tagged = 0; tagged < 2; tagged++)
                for (int v = 0; v < 3; v++) {
                    const uint64_t D = 32 + D0;                         // two pieces of guard in front
                    one_copy(ol, 0, ol, D, tagged, tags, values[v], scores[v]);                  // the block is the record
                    one_copy(ol + 40, 0, ol, D, tagged, tags, values[v], scores[v]);             // at the start
                    one_copy(ol + 40, 21, ol, D, tagged, tags, values[v], scores[v]);            // inside
                    one_copy(ol + 40, 40, ol, D, tagged, tags, values[v], scores[v]);            // at the end
                }
    one_copy(5000, 123, 4321, 32 + 7, true, tags, 65535, 4000);         // the piece loop wraps: 16 lanes x 16 bytes
    one_copy(5000, 123, 4321, 32 + 7, false, tags, 0, 0);
}

// aux_walk over a heap block of exactly the bytes given
uint32_t walk(const std::string &aux, uint32_t tags)
{
    uint8_t *p = (uint8_t *)malloc(aux.size() ? aux.size() : 1);
    memcpy(p, aux.data(), aux.size());
    const uint32_t r = aux_walk(p, 0, aux.size(), tags);
    free(p);
    g_walks++;
    return r;
}

std::string b_array(char sub, uint32_t count, uint32_t size, const char *name = "XB")
{
    std::string s = std::string(name) + "B" + sub;
    for (int i = 0; i < 4; i++) s += (char)(count >> (8 * i));
    s += std::string((size_t)count * size, 's');
    return s;
}

void check_walk()
{
    const uint32_t tags = 's' | 'n' << 8 | 's' << 16 | (uint32_t)'c' << 24;
    const std::string Z0("XZZsnsc\0", 8), fields[] = {std::string("XAAs"), std::string("XccS"), std::string("XCCn"), std::string("XssSN"),
                                                     std::string("XSSsn"), std::string("XiisnSC"), std::string("XIIscsn"), std::string("XffSNSC"),
                                                     Z0, std::string("XHH5A\0", 6), std::string("XzZ\0", 4)};
    std::string all;
    for (const std::string &f : fields) {
        if (walk(f, tags) != AUX_OK) die("a field alone", (long)f.size());
        all += f;
    }
    const char subs[] = "cCsSiIf";
    const uint32_t sizes[] = {1, 1, 2, 2, 4, 4, 4};
    for (int i = 0; i < 7; i++)
        for (uint32_t count : {0u, 1u, 5u}) {
            const std::string f = b_array(subs[i], count, sizes[i]);
            if (walk(f, tags) != AUX_OK) die("a B array alone", i, (long)count);
            all += f;
        }
    if (walk("", tags) != AUX_OK || walk(all, tags) != AUX_OK) die("every field in a row");
    // the tags, as the first, a middle and the last field; inside a value they are no field
    for (const std::string &g : {std::string("snix123"), std::string("scZab\0", 6), std::string("snA!"), std::string("scBc\1\0\0\0x", 9)}) {
        if (walk(g, tags) != AUX_TAGGED || walk(g + all, tags) != AUX_TAGGED || walk(all + g, tags) != AUX_TAGGED ||
            walk(fields[0] + g + all, tags) != AUX_TAGGED)
            die("a tagged record");
    }
    if (walk(std::string("ns") + "Asc", tags) != AUX_DAMAGED) die("a cut field behind a value");      // 'nsA' 's', then "c" alone
    if (walk("nsiabcd", tags) != AUX_OK || walk("SNiabcd", tags) != AUX_OK) die("other names");
    // damaged: every proper prefix of a field that does not end on a field's end, an unknown type, Z without a NUL, B past the end
    for (const std::string &f : fields)
        for (size_t cut = 1; cut < f.size(); cut++)
            if (walk(f.substr(0, cut), tags) != AUX_DAMAGED || walk(all + f.substr(0, cut), tags) != AUX_DAMAGED) die("a cut field", (long)cut);
    for (char c : {'z', 'D', '\0', 'a', 'b', 'h', 'F', 'd'})
        if (walk(std::string("XX") + c + "1234", tags) != AUX_DAMAGED) die("an unknown type", c);
    if (walk("XZZabc", tags) != AUX_DAMAGED || walk("XHHabc", tags) != AUX_DAMAGED) die("no NUL");
    for (int i = 0; i < 7; i++) {
        std::string f = b_array(subs[i], 5, sizes[i]);
        f.pop_back();
        if (walk(f, tags) != AUX_DAMAGED) die("a B array one byte short", i);
        if (walk(f.substr(0, 7), tags) != AUX_DAMAGED) die("a B array cut in its count", i);
    }
    if (walk(b_array('A', 1, 1), tags) != AUX_DAMAGED || walk(b_array('Z', 1, 1), tags) != AUX_DAMAGED) die("a B array of an unknown subtype");
    if (walk(std::string("XBBi\xff\xff\xff\xff", 8) + "abcd", tags) != AUX_DAMAGED) die("a B count of 2^32 - 1");
    // a damaged record stays damaged when it bears a tag as well
    if (walk(std::string("snA!") + "XZZabc", tags) != AUX_DAMAGED) die("damaged wins");
}

}  // namespace

int main()
{
    check_copies();
    check_walk();
    printf("%llu copies, %llu walks\ntag_copy_check ok\n", g_copies, g_walks);
    return 0;
}
