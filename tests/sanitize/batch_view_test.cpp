// Strided views on the host (tests/test_host_batch_views.py builds and runs this with g++, sanitizers on): sqy::admit_view's rules,
// folding and dense flag; the index walk of csrc/sqy_batch_view.hpp -- the one the kernels compile -- against a triple loop, for every
// flat index; sqy::lz4_batch_plan_views, where the packed copies count against the group bound.  Prints "batch_view ok" and returns 0.
#include "../../sqeazy_amd/csrc/sqy_batch_view.hpp"
#include "../../sqeazy_amd/csrc/sqy_pipeline.hpp"

#include <climits>
#include <cstdio>
#include <vector>

#define CHECK(cond)                                                                   \
    do {                                                                              \
        if (!(cond)) { std::fprintf(stderr, "line %d: %s\n", __LINE__, #cond); return 1; } \
    } while (0)

using sqy::BatchView;

namespace {

bool admit(std::vector<long> shape, std::vector<long> strides, BatchView* v)
{
    return sqy::admit_view(shape.data(), strides.empty() ? nullptr : strides.data(), (unsigned)shape.size(), v);
}
bool same(const BatchView& v, uint64_t Z, uint64_t Y, uint64_t X, uint64_t sz, uint64_t sy, bool dense)
{
    return v.Z == Z && v.Y == Y && v.X == X && v.sz == sz && v.sy == sy && v.dense == dense;
}

int test_admit()
{
    BatchView v;
    // dense, every rank: one row
    CHECK(admit({3, 5, 7}, {}, &v) && same(v, 1, 1, 105, 105, 105, true));
    CHECK(admit({3, 5, 7}, {35, 7, 1}, &v) && same(v, 1, 1, 105, 105, 105, true));
    CHECK(admit({5, 7}, {7, 1}, &v) && same(v, 1, 1, 35, 35, 35, true));
    CHECK(admit({7}, {1}, &v) && same(v, 1, 1, 7, 7, 7, true));
    CHECK(admit({7}, {}, &v) && v.dense);
    CHECK(admit({1, 1, 5}, {2880, 72, 1}, &v) && same(v, 1, 1, 5, 5, 5, true));          // a single row is dense whatever its strides
    // a tile of a parent: nothing folds
    CHECK(admit({3, 5, 7}, {2880, 72, 1}, &v) && same(v, 3, 5, 7, 2880, 72, false));
    // whole rows of the parent: y folds into x
    CHECK(admit({3, 5, 72}, {2880, 72, 1}, &v) && same(v, 1, 3, 360, 3 * 2880, 2880, false));
    // whole frames of the parent: dense
    CHECK(admit({3, 40, 72}, {2880, 72, 1}, &v) && same(v, 1, 1, 3 * 2880, 3 * 2880, 3 * 2880, true));
    // frames without a gap, rows with one: z folds into y
    CHECK(admit({3, 5, 7}, {50, 10, 1}, &v) && same(v, 1, 15, 7, 150, 10, false));
    // a padded pitch
    CHECK(admit({6, 10, 24}, {275, 27, 1}, &v) && same(v, 6, 10, 24, 275, 27, false));
    // rank 2 and 1 with a pitch
    CHECK(admit({5, 7}, {9, 1}, &v) && same(v, 1, 5, 7, 45, 9, false));
    CHECK(admit({1, 5, 7}, {1000, 9, 1}, &v) && same(v, 1, 5, 7, 45, 9, false));
    CHECK(admit({4, 1, 8}, {100, 50, 1}, &v) && same(v, 1, 4, 8, 400, 100, false));
    // the rules
    CHECK(!admit({3, 5, 7}, {2880, 72, 2}, &v));                 // innermost stride
    CHECK(!admit({3, 5, 7}, {2880, 0, 1}, &v));                  // a stride of 0
    CHECK(!admit({3, 5, 7}, {0, 72, 1}, &v));
    CHECK(!admit({3, 5, 7}, {-2880, 72, 1}, &v));
    CHECK(!admit({3, 5, 7}, {2880, 6, 1}, &v));                  // rows overlap
    CHECK(!admit({3, 5, 7}, {5 * 72 - 1, 72, 1}, &v));           // frames overlap
    CHECK(admit({3, 5, 7}, {5 * 72, 72, 1}, &v));
    CHECK(!admit({5, 7}, {6, 1}, &v));
    CHECK(!admit({7}, {2}, &v));
    CHECK(!admit({3, 0, 7}, {2880, 72, 1}, &v) && !admit({3, 5, -7}, {}, &v));
    CHECK(!admit({2, 3, 5, 7}, {105, 35, 7, 1}, &v) && !admit({2, 3, 5, 7}, {}, &v));    // rank 4
    CHECK(!sqy::admit_view(nullptr, nullptr, 3, &v));
    long s3[3] = {3, 5, 7};
    CHECK(!sqy::admit_view(s3, nullptr, 0, &v) && !sqy::admit_view(s3, nullptr, 3, nullptr));
    // overflow of shape x stride and of the voxel count
    CHECK(!admit({LONG_MAX, 5, 7}, {LONG_MAX / 2, 72, 1}, &v));
    CHECK(!admit({4, 5, 7}, {LONG_MAX, 72, 1}, &v));
    CHECK(!admit({3, LONG_MAX / 2, 7}, {LONG_MAX, LONG_MAX / 4, 1}, &v));
    CHECK(!admit({LONG_MAX, LONG_MAX, LONG_MAX}, {}, &v));
    CHECK(!admit({1l << 31, 1l << 31, 4}, {}, &v));
    CHECK(!admit({1l << 20, 1l << 20, 4}, {1l << 50, 1l << 20, 1}, &v));
    CHECK(admit({1l << 10, 1l << 10, 4}, {1l << 40, 1l << 20, 1}, &v) && !v.dense);
    return 0;
}

// the walk over a view of shape (Z, Y, X) with strides (sz, sy, 1), as admitted (folded) and as given, against the triple loop
int walk_case(long Z, long Y, long X, long sz, long sy)
{
    BatchView v;
    CHECK(admit({Z, Y, X}, {sz, sy, 1}, &v));
    CHECK(v.Z * v.Y * v.X == (uint64_t)(Z * Y * X));
    const sqy::ViewGeometry folded{v.Y, v.X, v.sz, v.sy}, plain{(uint64_t)Y, (uint64_t)X, (uint64_t)sz, (uint64_t)sy};
    const sqy::ViewGeometry* geo[2] = {&folded, &plain};
    for (int k = 0; k < 2; ++k) {
        const sqy::ViewGeometry& g = *geo[k];
        sqy::ViewWalk step = sqy::view_walk_start(g, 0), run = step, wide = step;
        uint64_t run_at = 0, wide_at = 0;               // where the walks in runs of a row / of up to 8 voxels stand
        uint64_t i = 0;
        for (long z = 0; z < Z; ++z)
            for (long y = 0; y < Y; ++y)
                for (long x = 0; x < X; ++x, ++i) {
                    const uint64_t off = (uint64_t)(z * sz + y * sy + x);
                    const sqy::ViewWalk w = sqy::view_walk_start(g, i);
                    CHECK(w.off == off && w.left >= 1 && w.left <= g.X);
                    if (k == 1) CHECK(w.left == (uint64_t)(X - x) && w.y == (uint64_t)y);
                    // the voxels left are in one run of the view, and the row ends there
                    CHECK(sqy::view_walk_start(g, i + w.left - 1).off == off + w.left - 1);
                    CHECK(step.off == off && step.left == w.left);
                    sqy::view_walk_advance(g, &step, 1);
                    if (run_at == i) { CHECK(run.off == off); run_at += run.left; sqy::view_walk_advance(g, &run, run.left); }
                    if (wide_at == i) {
                        CHECK(wide.off == off);
                        const uint64_t n = wide.left < 8 ? wide.left : 8;
                        wide_at += n;
                        sqy::view_walk_advance(g, &wide, n);
                    }
                }
    }
    return 0;
}

int test_walk()
{
    const long shapes[4][3] = {{3, 5, 7}, {1, 1, 5}, {5, 33, 33}, {2, 3, 130}};
    for (const auto& s : shapes) {
        const long Z = s[0], Y = s[1], X = s[2];
        for (long sy : {X, X + 3})
            for (long sz : {Y * sy, Y * sy + 5})
                if (walk_case(Z, Y, X, sz, sy)) { std::fprintf(stderr, "  in (%ld,%ld,%ld) pitches %ld, %ld\n", Z, Y, X, sz, sy); return 1; }
    }
    CHECK(walk_case(6, 10, 24, 10 * 27 + 5, 27) == 0);
    // the 64-bit divisions: a row longer than 2^32 voxels
    const sqy::ViewGeometry big{3, (uint64_t)5 << 32, (uint64_t)1 << 40, (uint64_t)6 << 32};
    const uint64_t i = 7 * big.X + 12345;                  // z = 2, y = 1
    const sqy::ViewWalk w = sqy::view_walk_start(big, i);
    CHECK(w.off == 2 * big.sz + 1 * big.sy + 12345 && w.left == big.X - 12345 && w.y == 1);
    return 0;
}

int test_plan()
{
    const sqy::Lz4Params p("");
    const uint64_t kNoBound = ~(uint64_t)0;
    const std::vector<uint64_t> totals = {1 << 20, 3 << 18, 1 << 20, 1 << 16, 1 << 20};
    auto equal = [](const sqy::Lz4BatchPlan& a, const sqy::Lz4BatchPlan& b) {
        if (a.group_of != b.group_of || a.groups.size() != b.groups.size()) return false;
        for (size_t g = 0; g < a.groups.size(); ++g) {
            const sqy::Lz4BatchGroup &x = a.groups[g], &y = b.groups[g];
            if (x.vols != y.vols || x.stream_at != y.stream_at || x.first_chunk != y.first_chunk || x.stream_bytes != y.stream_bytes ||
                x.scratch_stride != y.scratch_stride || x.max_chunk != y.max_chunk || x.chunks.size() != y.chunks.size())
                return false;
            for (size_t e = 0; e < x.chunks.size(); ++e)
                if (x.chunks[e].off != y.chunks[e].off || x.chunks[e].n != y.chunks[e].n || x.chunks[e].vol != y.chunks[e].vol || x.chunks[e].slot != y.chunks[e].slot) return false;
        }
        return true;
    };
    // dense input: today's plan, whatever the bound and the tables
    for (uint64_t bound : {kNoBound, (uint64_t)(2 << 20), (uint64_t)1})
        for (uint64_t extra : {(uint64_t)0, (uint64_t)4096}) {
            const sqy::Lz4BatchPlan want = sqy::lz4_batch_plan(p, totals, 8, bound, kNoBound, extra);
            CHECK(equal(want, sqy::lz4_batch_plan_views(p, totals, {}, 8, bound, kNoBound, extra)));
            CHECK(equal(want, sqy::lz4_batch_plan_views(p, totals, std::vector<uint64_t>(totals.size(), 0), 8, bound, kNoBound, extra)));
        }
    // 2 MiB a group: streams alone fit as {0, 1}, {2, 3}, {4} ..
    const sqy::Lz4BatchPlan dense = sqy::lz4_batch_plan(p, totals, 8, 2 << 20, kNoBound);
    CHECK(dense.group_of == (std::vector<int32_t>{0, 0, 1, 1, 2}));
    // .. volume 1's packed copy (its own size again) does not fit behind volume 0 any more, nor volume 2 behind the two of them; volume 3's
    // still fits behind volume 2
    const sqy::Lz4BatchPlan packed = sqy::lz4_batch_plan_views(p, totals, {0, 3 << 18, 0, 1 << 16, 0}, 8, 2 << 20, kNoBound);
    CHECK(packed.group_of == (std::vector<int32_t>{0, 1, 2, 2, 3}));
    for (const sqy::Lz4BatchGroup& g : packed.groups) {
        uint64_t sum = 0;
        const uint64_t pack[5] = {0, 3 << 18, 0, 1 << 16, 0};
        for (uint32_t v : g.vols) sum += totals[v] + pack[v];
        CHECK(sum <= (2 << 20) || g.vols.size() == 1);
    }
    // every volume packed: a group holds at least one volume, its stream is laid out as without the copies
    const sqy::Lz4BatchPlan all = sqy::lz4_batch_plan_views(p, totals, totals, 8, 2 << 20, kNoBound);
    CHECK(all.group_of == (std::vector<int32_t>{0, 1, 2, 3, 4}));
    for (const sqy::Lz4BatchGroup& g : all.groups) CHECK(g.stream_at[0] == 0);
    // the joint bound looks at the stream alone
    CHECK(sqy::lz4_batch_plan_views(p, totals, totals, 8, kNoBound, 1 << 20).group_of == (std::vector<int32_t>{0, 0, 0, 0, 0}));
    return 0;
}

} // namespace

int main()
{
    if (test_admit() || test_walk() || test_plan()) return 1;
    std::printf("batch_view ok\n");
    return 0;
}
