// The packed layout's placement rule on the host (tests/test_host_batch_packed.py builds and runs this with g++, sanitizers on):
// sqy::packed_places against a table written out by hand, then over a grid of cases -- every align from 1 to 65536, lengths that are
// multiples of it and lengths that are not, gaps, a capacity equal to the end and one byte short, a capacity that cuts in mid-table, sums
// past 2^32, ends at and past 2^63 -- one line per case on stdout: the arguments, " => ", the result.  The Python test states the rule
// again and must reproduce every line.  Prints "batch_packed ok" last and returns 0.
#include "../../sqeazy_amd/csrc/sqy_pipeline.hpp"

#include <cinttypes>
#include <cstdio>
#include <vector>

#define CHECK(cond)                                                                   \
    do {                                                                              \
        if (!(cond)) { std::fprintf(stderr, "line %d: %s\n", __LINE__, #cond); return 1; } \
    } while (0)

using sqy::PackedPlaces;
using sqy::packed_places;
typedef std::vector<uint64_t> V;

namespace {

int test_table()
{
    PackedPlaces p = packed_places({10, 6, 16, 1}, {}, 1, 0, 33);
    CHECK(p.ok && p.at == V({0, 10, 16, 32}) && p.end == 33 && p.first_unfit == 4);
    p = packed_places({10, 6, 16, 1}, {}, 1, 0, 32);
    CHECK(p.ok && p.at == V({0, 10, 16, 32}) && p.end == 33 && p.first_unfit == 3);
    p = packed_places({10, 6, 16, 1}, {}, 16, 0, 49);
    CHECK(p.ok && p.at == V({0, 16, 32, 48}) && p.end == 49 && p.first_unfit == 4);
    p = packed_places({10, 6, 16, 1}, {}, 16, 0, 31);                        // the second is the first that does not fit; the rest is placed as if it had
    CHECK(p.ok && p.at == V({0, 16, 32, 48}) && p.end == 49 && p.first_unfit == 2);
    p = packed_places({10, 6, 16, 1}, {}, 16, 0, 0);
    CHECK(p.ok && p.first_unfit == 0 && p.end == 49);
    // a group behind 3 volumes (base 4096), two volumes of 100 and 5000 bytes between its members
    p = packed_places({7, 4096, 9}, {0, 4096, 8192}, 4096, 4096, 1 << 20);
    CHECK(p.ok && p.at == V({4096, 12288, 24576}) && p.end == 24585 && p.first_unfit == 3);
    // no volume: the base
    p = packed_places({}, {}, 16, 48, 0);
    CHECK(p.ok && p.at.empty() && p.end == 48 && p.first_unfit == 0);
    // past 2^32
    p = packed_places({0xffffffffull, 0xffffffffull, 5}, {}, 65536, 0, ~0ull);
    CHECK(p.ok && p.at == V({0, 0x100000000ull, 0x200000000ull}) && p.end == 0x200000005ull && p.first_unfit == 3);
    // the last end may be 2^63 - 1 and not 2^63; nothing wraps
    const uint64_t top = (uint64_t)1 << 63;
    p = packed_places({top - 1}, {}, 1, 0, ~0ull);
    CHECK(p.ok && p.end == top - 1);
    p = packed_places({top}, {}, 1, 0, ~0ull);
    CHECK(!p.ok && p.at.empty() && p.end == 0 && p.first_unfit == 0);
    p = packed_places({top - 16, 16}, {}, 1, 0, ~0ull);
    CHECK(!p.ok);
    p = packed_places({top - 17, 16}, {}, 1, 0, ~0ull);
    CHECK(p.ok && p.end == top - 1);
    p = packed_places({top - 17, 1}, {}, 16, 0, ~0ull);
    CHECK(p.ok && p.at == V({0, top - 16}) && p.end == top - 15);
    p = packed_places({top - 5, 1}, {}, 16, 0, ~0ull);                       // the rounded end passes it
    CHECK(!p.ok);
    p = packed_places({~0ull, 2}, {}, 1, 0, ~0ull);                          // would wrap to 1
    CHECK(!p.ok);
    p = packed_places({1, 1}, {0, ~0ull}, 1, 0, ~0ull);
    CHECK(!p.ok);
    p = packed_places({1}, {}, 1, top, ~0ull);
    CHECK(!p.ok);
    // align
    for (uint64_t bad : V({0, 3, 6, 65537, 131072, ~0ull, top})) CHECK(!packed_places({1, 2}, {}, bad, 0, 100).ok);
    CHECK(!packed_places({1, 2}, {0}, 1, 0, 100).ok);                        // a gap table of another size
    return 0;
}

uint64_t lcg(uint64_t* s) { *s = *s * 6364136223846793005ull + 1442695040888963407ull; return *s >> 24; }

void print_case(const V& lens, const V& gaps, uint64_t align, uint64_t base, uint64_t cap)
{
    const PackedPlaces p = packed_places(lens, gaps, align, base, cap);
    std::printf("%" PRIu64 " %" PRIu64 " %" PRIu64 " |", align, base, cap);
    for (uint64_t x : lens) std::printf(" %" PRIu64, x);
    std::printf(" |");
    for (uint64_t x : gaps) std::printf(" %" PRIu64, x);
    std::printf(" => %d %" PRIu64 " %zu |", p.ok ? 1 : 0, p.end, p.first_unfit);
    for (uint64_t x : p.at) std::printf(" %" PRIu64, x);
    std::printf("\n");
}

int test_grid()
{
    uint64_t seed = 12345;
    for (uint64_t align = 1; align <= 65536; align <<= 1) {
        for (int kind = 0; kind < 4; ++kind) {
            // 0: multiples of align | 1: none a multiple (align > 1) | 2: mixed, with gaps | 3: long ones, the sums pass 2^32
            const size_t n = 3 + (size_t)(lcg(&seed) % 6);
            V lens(n), gaps;
            for (size_t j = 0; j < n; ++j) {
                const uint64_t r = lcg(&seed);
                if (kind == 0) lens[j] = align * (1 + r % 5);
                else if (kind == 1) lens[j] = align * (r % 5) + (align > 1 ? 1 + r % (align - 1) : 1);
                else if (kind == 2) lens[j] = 1 + r % (3 * align + 7);
                else lens[j] = 0x7fff0000ull + r % 0x20000;
            }
            if (kind == 2) { gaps.resize(n); for (size_t j = 0; j < n; ++j) gaps[j] = (lcg(&seed) % 3) * align; }
            const uint64_t base = kind == 2 ? align * (lcg(&seed) % 9) : 0;
            const PackedPlaces all = packed_places(lens, gaps, align, base, ~0ull);
            CHECK(all.ok && all.first_unfit == n);
            print_case(lens, gaps, align, base, ~0ull);
            print_case(lens, gaps, align, base, all.end);                   // exactly enough
            print_case(lens, gaps, align, base, all.end - 1);               // one byte short: the last volume
            print_case(lens, gaps, align, base, all.at[1] + lens[1] + 1);   // cuts in behind the second
            print_case(lens, gaps, align, base, all.at[n / 2]);             // .. at the start of one
            CHECK(packed_places(lens, gaps, align, base, all.end).first_unfit == n && packed_places(lens, gaps, align, base, all.end - 1).first_unfit == n - 1);
            if (align > 1) for (size_t j = 0; j < n; ++j) CHECK((all.at[j] - (gaps.empty() ? 0 : gaps[j])) % align == 0);
        }
        // at the top of the range: refused or placed, never wrapped
        const uint64_t top = (uint64_t)1 << 63;
        print_case({top - 3 * align, align, align}, {}, align, 0, ~0ull);
        print_case({top - 3 * align, align, align + 1}, {}, align, 0, ~0ull);
        print_case({top - 3 * align, align, align - 1}, {}, align, 0, ~0ull);
        print_case({5, top - 2 * align}, {0, align}, align, 0, top);
        print_case({5, top - 2 * align}, {0, align - 1}, align, 0, top);
        print_case({~0ull, align}, {}, align, 0, ~0ull);
    }
    for (uint64_t bad : V({0, 3, 24, 65537, 131072})) print_case({1, 2, 3}, {}, bad, 0, 100);
    return 0;
}

}  // namespace

int main()
{
    if (test_table() || test_grid()) return 1;
    std::printf("batch_packed ok\n");
    return 0;
}
