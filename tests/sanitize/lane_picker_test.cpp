// The parse-lane picker of csrc/sqy_lanes.hpp on the host (tests/test_host_lanes.py builds and runs this with g++, sanitizers on):
// fewest calls leased, round robin among equals, a lease given back on every way out.  Prints "lane_picker ok" and returns 0.
#include "../../sqeazy_amd/csrc/sqy_lanes.hpp"

#include <cstdio>
#include <cstdlib>
#include <stdexcept>
#include <vector>

#define CHECK(cond)                                                                   \
    do {                                                                              \
        if (!(cond)) { std::fprintf(stderr, "line %d: %s\n", __LINE__, #cond); return 1; } \
    } while (0)

namespace {
// what a call does with its lease: taken on the way in, given back by the destructor -- also when the call fails
struct Lease {
    sqy::LanePicker& p;
    int lane;
    Lease(sqy::LanePicker& picker, int lanes) : p(picker), lane(picker.take(lanes)) {}
    ~Lease() { p.give(lane); }
};
int failing_call(sqy::LanePicker& p, int lanes)
{
    Lease l(p, lanes);
    throw std::runtime_error("the call failed");
}
}

int main()
{
    using sqy::LanePicker;
    {   // idle lanes take turns: calls that come and go one at a time spread over all lanes
        LanePicker p;
        for (int i = 0; i < 12; ++i) {
            const int l = p.take(3);
            CHECK(l == i % 3);
            p.give(l);
        }
        for (int l = 0; l < LanePicker::kMaxLanes; ++l) CHECK(p.leased(l) == 0);
    }
    {   // four calls in flight on three lanes: the fourth shares, and the call that follows goes where the oldest call is
        LanePicker p;
        CHECK(p.take(3) == 0 && p.take(3) == 1 && p.take(3) == 2);      // A B C
        CHECK(p.take(3) == 0);                                          // D behind A
        CHECK(p.leased(0) == 2 && p.leased(1) == 1 && p.leased(2) == 1 && p.total() == 4);
        p.give(0);                                                      // A done
        CHECK(p.take(3) == 1);                                          // E: all equal, lane 1's turn (B, the oldest, is there)
        p.give(1);                                                      // B done
        CHECK(p.take(3) == 2);                                          // F behind C
        p.give(2);
        CHECK(p.take(3) == 0);                                          // G behind D
    }
    {   // fewest leased wins over whose turn it is
        LanePicker p;
        const int a = p.take(4), b = p.take(4), c = p.take(4), d = p.take(4);
        CHECK(a == 0 && b == 1 && c == 2 && d == 3);
        p.give(2);
        CHECK(p.take(4) == 2);                                          // (turn: lane 0; fewest: lane 2)
        p.give(1); p.give(3);
        const int e = p.take(4);
        CHECK(e == 3);                                                  // lanes 1 and 3 are equal: the first at or behind lane 3's turn
        CHECK(p.take(4) == 1);
    }
    {   // one lane; counts outside the range are clamped; give() of nothing is harmless
        LanePicker p;
        CHECK(p.take(1) == 0 && p.take(1) == 0 && p.take(0) == 0 && p.take(-5) == 0);
        CHECK(p.leased(0) == 4);
        for (int i = 0; i < 6; ++i) p.give(0);
        CHECK(p.leased(0) == 0);
        p.give(-1); p.give(LanePicker::kMaxLanes); p.give(7);
        std::vector<int> seen(LanePicker::kMaxLanes, 0);
        for (int i = 0; i < LanePicker::kMaxLanes; ++i) seen[p.take(100)] += 1;
        for (int l = 0; l < LanePicker::kMaxLanes; ++l) CHECK(seen[l] == 1 && p.leased(l) == 1);
        CHECK(p.leased(-1) == 0 && p.leased(LanePicker::kMaxLanes) == 0);
    }
    {   // the number of lanes changes between calls (SQYAMD_Set_Option): leases on lanes no longer dealt are still given back
        LanePicker p;
        int held[6];
        for (int i = 0; i < 6; ++i) held[i] = p.take(6);
        CHECK(p.take(2) == 0 || p.leased(1) == 2);
        for (int i = 0; i < 6; ++i) p.give(held[i]);
        CHECK(p.leased(2) == 0 && p.leased(5) == 0 && p.leased(0) + p.leased(1) == 1);
    }
    {   // release on error: a call that throws leaves no lease behind, the next call sees the lanes as they were
        LanePicker p;
        const int a = p.take(3);
        for (int i = 0; i < 5; ++i) {
            try { failing_call(p, 3); CHECK(false); }
            catch (const std::runtime_error&) {}
        }
        CHECK(p.leased(0) + p.leased(1) + p.leased(2) == 1 && p.leased(a) == 1 && p.total() == 1);
        p.give(a);
        CHECK(p.total() == 0);
    }
    std::printf("lane_picker ok\n");
    return 0;
}
