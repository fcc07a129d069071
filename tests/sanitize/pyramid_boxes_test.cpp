// A whole resolution pyramid of boxes of one large blob, on the host (tests/test_host_pyramid_boxes.py builds and runs this with g++,
// sanitizers on): sqy::pyramid_boxes_path against its table, the pyramid jobs' layout, sqy::admit_pyramid at every refusal -- levels 0
// and 9, a non-multiple in each dimension, the sum bound one voxel above on the top level only, a bad output in any level of any box --,
// sqy::pyramid_boxes_plan on grids of 1, prime and budget-straddling sizes with shrunken budgets -- every cell of every fused level lies
// in exactly one block, no block is over either budget, T is what the LDS rule says --, and the whole fused walk of
// SQYAMD_Pyramid_Boxes_*'s bit-plane kernel as bitswap1_decode_range_windows_pyramid_kernel drives it: every block of a box's plan, the
// level-0 cell layers under it one after another (footprint, items, the clip and sqy::bin_run_cells into an array of exactly the
// layer's cells standing in for the LDS accumulators), the stores, the folds (sqy::pyramid_fold_cell into arrays of exactly each level's
// cells: a fold that strays is the sanitizer's) and, for the levels above T, the tail reduce (sqy::pyramid_reduce_cell over the stored
// level-T cells with their pitches).  Afterwards every cell of every level must equal a triple loop's over the voxels, every gap between
// pitched rows its pattern, and every cell must have been stored exactly once.  Blobs 3 x 5 x 7, 2 x 3 x 300, 7 x 33 x 31 and 4 x 8 x 32
// (a frame of whole runs: reduced over z in registers); all three ops; pyramids with ratio 1, ratio 3, z only and a top level beyond T.
// Prints the blocks, the folds, the cells stored by the walk and by the tail, the boxes reduced over z in registers and those with a
// level above T, then "pyramid_boxes ok"; returns 0.
#include "../../sqeazy_amd/csrc/sqy_batch_window.hpp"
#include "../../sqeazy_amd/csrc/sqy_kernels.h"
#include "../../sqeazy_amd/csrc/sqy_pipeline.hpp"

#include <algorithm>
#include <climits>
#include <cstddef>
#include <cstdio>
#include <cstring>
#include <vector>

#define CHECK(cond)                                                                   \
    do {                                                                              \
        if (!(cond)) { std::fprintf(stderr, "line %d: %s\n", __LINE__, #cond); return 1; } \
    } while (0)

using sqy::BoxPath;
using sqy::RangeForm;

namespace {

constexpr uint32_t L = sqy::kPyramidMaxLevels;
unsigned long long g_blocks = 0, g_folds = 0, g_walk_cells = 0, g_tail_cells = 0, g_zreg = 0, g_above = 0;

int test_path()
{
    const struct { RangeForm form; BoxPath on; } table[] = {{RangeForm::plain, BoxPath::subset_copy}, {RangeForm::planes, BoxPath::subset_transposer},
                                                            {RangeForm::planes_lut, BoxPath::subset_transposer}, {RangeForm::shuffle, BoxPath::subset_copy}};
    for (const auto& row : table)
        for (bool fused : {true, false}) {
            CHECK(sqy::pyramid_boxes_path(true, row.form, true, fused).path == row.on && sqy::pyramid_boxes_path(true, row.form, true, fused).fused == fused);
            CHECK(sqy::pyramid_boxes_path(true, row.form, false, fused).path == BoxPath::whole_copy);      // the subset option off
            CHECK(sqy::pyramid_boxes_path(false, row.form, true, fused).path == BoxPath::whole_copy);      // a blob the frame-range plan does not take
            CHECK(sqy::pyramid_boxes_path(false, row.form, false, fused).fused == fused);
        }
    return 0;
}

int test_layout()
{
    static_assert(sizeof(sqy::Bitswap1BoxPyramidJob) == sqy::kBitswap1BoxPyramidJobBytes && sizeof(sqy::Bitswap1BoxPyramidJob) % 16 == 0, "the pyramid box job's layout");
    static_assert(sizeof(sqy::PyramidReduceJob) == sqy::kPyramidReduceJobBytes && sizeof(sqy::PyramidReduceJob) % 16 == 0, "the reduce job's layout");
    static_assert(sqy::kPyramidLdsCells * 4u + 512u <= 64u * 1024u && sqy::kBinBlockCells <= sqy::kPyramidLdsCells, "all accumulators and the look-up: at most 64 KiB");
    static_assert(sqy::kPyramidMaxLevels == 8, "SQYAMD_PYRAMID_MAX_LEVELS");
    for (uint64_t n : {(uint64_t)1, (uint64_t)3, (uint64_t)64, (uint64_t)100001}) {
        const sqy::BatchWindowLayout l = sqy::batch_window_layout(n, sizeof(sqy::Bitswap1BoxPyramidJob));
        CHECK(l.tiles_at == n * sizeof(sqy::Bitswap1BoxPyramidJob) && l.tiles_at % 16 == 0 && l.total == l.tiles_at + (n + 1) * sizeof(uint32_t));
        const sqy::BatchWindowLayout r = sqy::batch_window_layout(n, sizeof(sqy::PyramidReduceJob));
        CHECK(r.tiles_at == n * sizeof(sqy::PyramidReduceJob) && r.tiles_at % 16 == 0);
    }
    return 0;
}

int test_admission()
{
    alignas(16) uint32_t out[64];
    const void* outs[L + 1];
    for (auto& p : outs) p = out;
    sqy::BatchWindow w;
    sqy::Pyramid y;
    const long o[3] = {0, 0, 0};
    const std::vector<uint64_t> shape{3, 5, 7};
    const long o1[3] = {1, 1, 1}, e[3] = {2, 3, 4};
    const long good[3][3] = {{1, 1, 1}, {2, 1, 3}, {2, 2, 3}};
    CHECK(sqy::admit_pyramid(shape, o1, e, 3, 3, &good[0][0], 0, 65535, outs, nullptr, &w, &y));
    CHECK(y.levels == 3 && y.q[0].C[0] == 2 && y.q[0].C[1] == 3 && y.q[0].C[2] == 4 && y.q[1].C[0] == 1 && y.q[1].C[1] == 3 && y.q[1].C[2] == 2);
    CHECK(y.q[2].C[0] == 1 && y.q[2].C[1] == 2 && y.q[2].C[2] == 2 && y.raw[2][1] == 2 && y.raw[1][2] == 3 && w.Z == 2 && w.Y == 3 && w.X == 4);
    // levels 0, 9, negative; 1 and 8 are taken
    long eight[9][3];
    for (int l = 0; l < 9; ++l)
        for (int d = 0; d < 3; ++d) eight[l][d] = 1l << l;
    for (long levels : {0l, 9l, -1l, LONG_MIN, LONG_MAX}) CHECK(!sqy::admit_pyramid(shape, o1, e, 3, levels, &eight[0][0], 0, 65535, outs, nullptr, &w, &y));
    CHECK(sqy::admit_pyramid(shape, o1, e, 3, 1, &eight[0][0], 0, 65535, outs, nullptr, &w, &y) && y.levels == 1);
    CHECK(sqy::admit_pyramid(shape, o1, e, 3, 8, &eight[0][0], 0, 65535, outs, nullptr, &w, &y) && y.levels == 8 && y.q[7].C[2] == 1 && y.raw[7][0] == 128);
    // the nesting: a non-multiple in each dimension, at each level; a level FINER than the one before; a repeated level is taken
    for (int d = 0; d < 3; ++d)
        for (int l = 1; l < 3; ++l) {
            long b[3][3] = {{2, 2, 2}, {4, 4, 4}, {8, 8, 8}};
            b[l][d] += 1;
            CHECK(!sqy::admit_pyramid(shape, o1, e, 3, 3, &b[0][0], 0, 65535, outs, nullptr, &w, &y));
            b[l][d] = b[l - 1][d] / 2;
            CHECK(!sqy::admit_pyramid(shape, o1, e, 3, 3, &b[0][0], 0, 65535, outs, nullptr, &w, &y));
            b[l][d] = b[l - 1][d];
            if (l == 1) b[2][d] = b[1][d] * 3;
            CHECK(sqy::admit_pyramid(shape, o1, e, 3, 3, &b[0][0], 0, 65535, outs, nullptr, &w, &y));
        }
    {
        // taken on the caller's UNCLAMPED values: (5, 5, 5) then (7, 7, 7) both clamp to the extent, and still do not nest
        const long b[2][3] = {{5, 5, 5}, {7, 7, 7}}, c[2][3] = {{5, 5, 5}, {1000, 5, 10}}, same[2][3] = {{2, 2, 2}, {2, 2, 2}};
        CHECK(!sqy::admit_pyramid(shape, o1, e, 3, 2, &b[0][0], 0, 65535, outs, nullptr, &w, &y));
        CHECK(sqy::admit_pyramid(shape, o1, e, 3, 2, &c[0][0], 0, 65535, outs, nullptr, &w, &y) && y.q[1].C[0] == 1 && y.q[1].C[1] == 1 && y.q[1].C[2] == 1);
        CHECK(sqy::admit_pyramid(shape, o1, e, 3, 2, &same[0][0], 0, 65535, outs, nullptr, &w, &y));
    }
    // what admit_binning refuses, at every level: an entry < 1, bins NULL, the op
    for (int l = 0; l < 3; ++l)
        for (int d = 0; d < 3; ++d)
            for (long bad : {0l, -2l, LONG_MIN}) {
                long b[3][3] = {{2, 2, 2}, {4, 4, 4}, {8, 8, 8}};
                b[l][d] = bad;
                CHECK(!sqy::admit_pyramid(shape, o1, e, 3, 3, &b[0][0], 0, 65535, outs, nullptr, &w, &y));
            }
    CHECK(!sqy::admit_pyramid(shape, o1, e, 3, 3, nullptr, 0, 65535, outs, nullptr, &w, &y));
    for (int op : {3, -1, INT_MAX}) CHECK(!sqy::admit_pyramid(shape, o1, e, 3, 3, &good[0][0], op, 65535, outs, nullptr, &w, &y));
    CHECK(!sqy::admit_pyramid(shape, o1, e, 3, 3, &good[0][0], 0, 65535, nullptr, nullptr, &w, &y));
    CHECK(!sqy::admit_pyramid(shape, o1, e, 3, 3, &good[0][0], 0, 65535, outs, nullptr, nullptr, &y) && !sqy::admit_pyramid(shape, o1, e, 3, 3, &good[0][0], 0, 65535, outs, nullptr, &w, nullptr));
    // a bad output in any level: NULL, 2 bytes off; 4 bytes behind the grid is taken
    for (int l = 0; l < 3; ++l) {
        const void* p[3] = {out, out, out};
        p[l] = nullptr;
        CHECK(!sqy::admit_pyramid(shape, o1, e, 3, 3, &good[0][0], 0, 65535, p, nullptr, &w, &y));
        p[l] = reinterpret_cast<const char*>(out) + 2;
        CHECK(!sqy::admit_pyramid(shape, o1, e, 3, 3, &good[0][0], 0, 65535, p, nullptr, &w, &y));
        p[l] = out + 1;
        CHECK(sqy::admit_pyramid(shape, o1, e, 3, 3, &good[0][0], 0, 65535, p, nullptr, &w, &y));
    }
    // the stride rules per output: the grids are 2 x 3 x 4, 1 x 3 x 2, 1 x 2 x 2
    {
        const long ok[3][3] = {{20, 5, 1}, {9, 3, 1}, {4, 2, 1}};
        CHECK(sqy::admit_pyramid(shape, o1, e, 3, 3, &good[0][0], 0, 65535, outs, &ok[0][0], &w, &y));
        CHECK(y.q[0].pz == 20 && y.q[0].py == 5 && y.q[1].py == 3 && y.q[2].py == 2 && y.q[2].pz == 4);
        const long bad[3][4][3] = {{{20, 5, 2}, {20, 3, 1}, {14, 5, 1}, {20, 0, 1}}, {{9, 3, 2}, {9, 1, 1}, {9, 0, 1}, {9, 3, 0}}, {{4, 2, 2}, {4, 1, 1}, {4, 0, 1}, {4, 2, 0}}};
        for (int l = 0; l < 3; ++l)
            for (int k = 0; k < 4; ++k) {
                long s[3][3];
                std::memcpy(s, ok, sizeof s);
                std::memcpy(s[l], bad[l][k], sizeof s[l]);
                CHECK(!sqy::admit_pyramid(shape, o1, e, 3, 3, &good[0][0], 0, 65535, outs, &s[0][0], &w, &y));
            }
    }
    // what Decode_Boxes refuses for a box
    {
        const long neg[3] = {1, -1, 1}, past[3] = {2, 3, 7}, none[3] = {2, 0, 4};
        CHECK(!sqy::admit_pyramid(shape, neg, e, 3, 3, &good[0][0], 0, 65535, outs, nullptr, &w, &y));
        CHECK(!sqy::admit_pyramid(shape, o1, past, 3, 3, &good[0][0], 0, 65535, outs, nullptr, &w, &y));
        CHECK(!sqy::admit_pyramid(shape, o1, none, 3, 3, &good[0][0], 0, 65535, outs, nullptr, &w, &y));
        CHECK(!sqy::admit_pyramid(shape, o1, e, 2, 3, &good[0][0], 0, 65535, outs, nullptr, &w, &y));           // another rank than the header's
        CHECK(!sqy::admit_pyramid(shape, o1, e, 0, 3, &good[0][0], 0, 65535, outs, nullptr, &w, &y) && !sqy::admit_pyramid(shape, o1, e, 4, 3, &good[0][0], 0, 65535, outs, nullptr, &w, &y));
    }
    // the sum bound binds on the TOP level only: V = 65536 there is taken, one voxel (one column) above is not; the levels below are far under it
    {
        const std::vector<uint64_t> big{16, 64, 65};
        const long eb[3] = {16, 64, 65};
        const long fits[2][3] = {{4, 16, 16}, {16, 64, 64}}, over[2][3] = {{16, 64, 1}, {16, 64, 65}};
        CHECK(sqy::admit_pyramid(big, o, eb, 3, 2, &fits[0][0], 2, 65535, outs, nullptr, &w, &y) && y.q[1].C[2] == 2 && y.q[0].C[2] == 5);
        CHECK(!sqy::admit_pyramid(big, o, eb, 3, 2, &over[0][0], 2, 65535, outs, nullptr, &w, &y));
        CHECK(sqy::admit_pyramid(big, o, eb, 3, 1, &over[0][0], 2, 65535, outs, nullptr, &w, &y));                // the level below alone: V = 1024
        CHECK(sqy::admit_pyramid(big, o, eb, 3, 2, &over[0][0], 0, 65535, outs, nullptr, &w, &y) && sqy::admit_pyramid(big, o, eb, 3, 2, &over[0][0], 1, 65535, outs, nullptr, &w, &y));
        const std::vector<uint64_t> line{20000000};
        const long el[1] = {20000000}, f8[2][1] = {{1}, {16843009}}, o8[2][1] = {{1}, {16843010}};
        CHECK(sqy::admit_pyramid(line, o, el, 1, 2, &f8[0][0], 2, 255, outs, nullptr, &w, &y) && y.raw[1][2] == 16843009 && y.raw[1][0] == 1);
        CHECK(!sqy::admit_pyramid(line, o, el, 1, 2, &o8[0][0], 2, 255, outs, nullptr, &w, &y));
    }
    // the launch size: the groups of all boxes summed, the box that passes 2^31 - 1 refused
    {
        sqy::PyramidSizes sizes;
        CHECK(sqy::admit_pyramid(shape, o1, e, 3, 3, &good[0][0], 0, 65535, outs, nullptr, &w, &y, &sizes));
        CHECK(sizes.cell_groups == 1 && sizes.bin_blocks == 2 && sizes.blocks >= 1 && sizes.reduce_groups == 2);
        sizes.reduce_groups = 0x7ffffffeull;
        CHECK(!sqy::admit_pyramid(shape, o1, e, 3, 3, &good[0][0], 0, 65535, outs, nullptr, &w, &y, &sizes));
        sizes = sqy::PyramidSizes{};
        sizes.blocks = 0x7fffffffull;
        CHECK(!sqy::admit_pyramid(shape, o1, e, 3, 3, &good[0][0], 0, 65535, outs, nullptr, &w, &y, &sizes));
    }
    return 0;
}

// a Pyramid for a box of extent E under `levels` rows of bins (dense outputs at `out`)
bool make_pyramid(const uint64_t E[3], uint32_t levels, const uint64_t bins[][3], sqy::Pyramid* y, int op = 0)
{
    alignas(16) static uint32_t out[4];
    const void* outs[L];
    for (auto& p : outs) p = out;
    const std::vector<uint64_t> shape{E[0], E[1], E[2]};
    const long o[3] = {0, 0, 0}, e[3] = {(long)E[0], (long)E[1], (long)E[2]};
    long b[L][3];
    for (uint32_t l = 0; l < levels; ++l)
        for (int d = 0; d < 3; ++d) b[l][d] = (long)bins[l][d];
    sqy::BatchWindow w;
    return sqy::admit_pyramid(shape, o, e, 3, levels, &b[0][0], op, 65535, outs, nullptr, &w, y);
}

// the LDS rule, written out on its own: the highest level of which one cell fits level 0's accumulators in level-0 cells of one layer,
// all fused levels' accumulators for one of its cells fit the budget together, and of which one row of cells over the box's width -- the
// least a block walks -- holds no more voxels than the cap
uint32_t rule_T(const sqy::Pyramid& y, const uint64_t E[3], uint64_t budget0, uint64_t budget, uint64_t cap)
{
    for (uint32_t t = y.levels - 1; t >= 1; --t) {
        uint64_t all = 0, level0 = 0, voxels = 1;
        for (uint32_t l = 0; l <= t; ++l) {
            uint64_t n = 1;
            for (int d = 1; d < 3; ++d) n *= std::min(y.raw[t][d] / y.raw[l][d], y.q[l].C[d]);
            if (l == 0) level0 = n;
            all += n;
        }
        for (int d = 0; d < 3; ++d) voxels *= d == 2 ? E[d] : std::min(y.raw[t][d], E[d]);
        if (level0 <= budget0 && all <= budget && voxels <= cap) return t;
    }
    return 0;
}

// the blocks of a plan cover every cell of every fused level exactly once, none is over a budget, the offsets do not overlap
int check_plan(const uint64_t E[3], uint32_t levels, const uint64_t bins[][3], uint64_t budget0, uint64_t budget, uint64_t cap)
{
    sqy::Pyramid y;
    CHECK(make_pyramid(E, levels, bins, &y));
    const sqy::PyramidPlan p = sqy::pyramid_boxes_plan(y, E, budget0, budget, cap);
    budget = std::max(budget, budget0);
    CHECK(p.levels == levels && p.T < levels && p.T == rule_T(y, E, budget0, budget, cap));
    for (uint32_t l = 0; l < levels; ++l)
        for (int d = 0; d < 3; ++d) {
            CHECK(p.C[l][d] == y.q[l].C[d]);
            if (l) CHECK(p.r[l][d] >= 1 && p.r[l][d] <= p.C[l - 1][d] && p.C[l][d] == (p.C[l - 1][d] + p.r[l][d] - 1) / p.r[l][d]);
            if (l == p.T) CHECK(p.q[l][d] == 1);
            if (l && l <= p.T) CHECK(p.q[l - 1][d] == std::min(p.q[l][d] * p.r[l][d], p.C[l - 1][d]));
        }
    const uint64_t* CT = p.C[p.T];
    CHECK(p.band >= 1 && p.strip >= 1 && p.band <= CT[1] && p.strip <= CT[2]);
    CHECK(p.blocks == CT[0] * p.nbands * p.nstrips && p.nbands == (CT[1] + p.band - 1) / p.band && p.nstrips == (CT[2] + p.strip - 1) / p.strip);
    uint64_t at = 0;
    for (uint32_t l = 0; l <= p.T; ++l) {
        CHECK(p.off[l] == at);
        at += sqy::pyramid_level_cells(p, l, p.band, p.strip);
    }
    CHECK(at <= budget && sqy::pyramid_level_cells(p, 0, p.band, p.strip) <= budget0);
    std::vector<std::vector<unsigned char>> seen(p.T + 1);
    for (uint32_t l = 0; l <= p.T; ++l) seen[l].assign(p.C[l][0] * p.C[l][1] * p.C[l][2], 0);
    const sqy::BinPlan top = sqy::pyramid_top_plan(p);
    for (uint64_t own = 0; own < p.blocks; ++own) {
        const sqy::BinBlock b = sqy::bin_block_of(top, own);
        CHECK(b.cz < CT[0] && b.ncy >= 1 && b.ncx >= 1 && b.cy0 + b.ncy <= CT[1] && b.cx0 + b.ncx <= CT[2]);
        uint64_t cells = 0;
        for (uint32_t l = 0; l <= p.T; ++l) {
            uint64_t f[3], n[3];
            sqy::pyramid_level_span(p, l, 0, b.cz, 1, &f[0], &n[0]);
            sqy::pyramid_level_span(p, l, 1, b.cy0, b.ncy, &f[1], &n[1]);
            sqy::pyramid_level_span(p, l, 2, b.cx0, b.ncx, &f[2], &n[2]);
            CHECK(n[0] >= 1 && n[1] >= 1 && n[2] >= 1 && n[1] * n[2] <= sqy::pyramid_level_cells(p, l, p.band, p.strip));
            if (l == 0) CHECK(n[1] * n[2] <= budget0);
            cells += n[1] * n[2];
            for (uint64_t z = f[0]; z < f[0] + n[0]; ++z)
                for (uint64_t yy = f[1]; yy < f[1] + n[1]; ++yy)
                    for (uint64_t x = f[2]; x < f[2] + n[2]; ++x) {
                        unsigned char& s = seen[l].at((z * p.C[l][1] + yy) * p.C[l][2] + x);
                        CHECK(s == 0);
                        s = 1;
                    }
        }
        CHECK(cells <= budget);
    }
    for (uint32_t l = 0; l <= p.T; ++l) CHECK(std::count(seen[l].begin(), seen[l].end(), 1) == (long)seen[l].size());
    return 0;
}

int test_plan()
{
    const uint64_t sizes[] = {1, 2, 7, 13, 31, 64, 65, 127, 129};                         // 1, primes, and the budgets below straddled
    const uint64_t pyramids[][4][3] = {{{1, 1, 1}, {2, 2, 2}, {4, 4, 4}, {8, 8, 8}}, {{1, 2, 2}, {1, 4, 4}, {1, 8, 8}, {1, 8, 8}}, {{3, 5, 7}, {6, 5, 21}, {12, 10, 42}, {12, 10, 42}},
                                       {{2, 1, 1}, {1000, 1, 1}, {1000, 1, 1}, {2000, 1, 1}}, {{1, 1, 1}, {1, 1, 1}, {1, 128, 128}, {1, 128, 256}}};
    for (const auto& py : pyramids)
        for (uint32_t levels : {1u, 3u, 4u})
            for (uint64_t ez : {(uint64_t)1, (uint64_t)5})
                for (uint64_t ey : sizes)
                    for (uint64_t ex : sizes) {
                        const uint64_t E[3] = {ez, ey, ex};
                        const uint64_t budgets[][3] = {{1, 1, 1}, {1, 3, 1u << 20}, {8, 12, 1u << 20}, {64, 100, 200}, {64, 64, 1u << 20}, {128, 300, 1u << 16}};
                        for (const auto& b : budgets)
                            if (check_plan(E, levels, py, b[0], b[1], b[2])) {
                                std::fprintf(stderr, "extent %llu %llu %llu levels %u first bins %llu %llu %llu budgets %llu %llu %llu\n", (unsigned long long)ez,
                                             (unsigned long long)ey, (unsigned long long)ex, levels, (unsigned long long)py[0][0], (unsigned long long)py[0][1],
                                             (unsigned long long)py[0][2], (unsigned long long)b[0], (unsigned long long)b[1], (unsigned long long)b[2]);
                                return 1;
                            }
                    }
    // the library's own budgets
    {
        const uint64_t E[3] = {64, 1024, 1024};
        const uint64_t b[4][3] = {{1, 2, 2}, {1, 4, 4}, {1, 8, 8}, {1, 16, 16}};
        if (check_plan(E, 4, b, sqy::kBinBlockCells, sqy::kPyramidLdsCells, sqy::kPyramidBlockVoxels)) return 1;
        sqy::Pyramid y;
        CHECK(make_pyramid(E, 4, b, &y));
        const sqy::PyramidPlan p = sqy::pyramid_boxes_plan(y, E);
        CHECK(p.T == 3 && p.strip == 64 && p.q[0][1] == 8 && p.q[0][2] == 8);
        // a top level of 128 x 128 level-0 cells per layer does not fit level 0's accumulators: it is the tail's, whatever the cap
        const uint64_t E2[3] = {16, 128, 128}, t[2][3] = {{1, 1, 1}, {1, 128, 128}}, t3[3][3] = {{1, 1, 1}, {1, 64, 128}, {1, 128, 128}};
        CHECK(make_pyramid(E2, 2, t, &y));
        CHECK(sqy::pyramid_boxes_plan(y, E2).T == 0 && sqy::pyramid_boxes_plan(y, E2, sqy::kBinBlockCells, sqy::kPyramidLdsCells, ~(uint64_t)0).T == 0);
        CHECK(make_pyramid(E2, 3, t3, &y));
        CHECK(sqy::pyramid_boxes_plan(y, E2).T == 1);                                      // 8192 level-0 cells: just fits, with its own one cell beside them
        if (check_plan(E2, 3, t3, sqy::kBinBlockCells, sqy::kPyramidLdsCells, sqy::kPyramidBlockVoxels)) return 1;
        // bins that would overflow a product
        const uint64_t E3[3] = {2, 3, 4}, h[2][3] = {{1, 1, 1}, {(uint64_t)1 << 62, (uint64_t)1 << 62, (uint64_t)1 << 62}};
        if (check_plan(E3, 2, h, sqy::kBinBlockCells, sqy::kPyramidLdsCells, sqy::kPyramidBlockVoxels)) return 1;
    }
    return 0;
}

uint32_t voxel(uint64_t i) { return (uint32_t)((i * 2654435761ull >> 7) % 65521ull); }

struct ArraySink {
    std::vector<uint32_t>* acc;
    uint32_t op;
    void combine(uint64_t cell, uint32_t v) { uint32_t& a = acc->at(cell); a = sqy::project_combine(op, a, v); }
};

// an output of a level: its cells with pitches, a pattern in the gaps, a count of the stores per element
struct Out {
    uint64_t C[3], pz, py;
    std::vector<uint32_t> v;
    std::vector<unsigned char> stored;
    int store(uint64_t at, uint32_t x)
    {
        CHECK(at < v.size() && stored[at] == 0);
        stored[at] = 1;
        v[at] = x;
        return 0;
    }
};

// one box of a blob through the kernel's walk and the tail into its outputs, under a plan with the given budgets
int walk_box(const uint64_t shape[3], const uint64_t o[3], const uint64_t e[3], uint32_t levels, const uint64_t rawbins[][3], uint32_t op, uint64_t budget0, uint64_t budget,
             uint64_t cap, bool pitched)
{
    const uint64_t n = shape[0] * shape[1] * shape[2], frame = shape[1] * shape[2];
    std::vector<Out> outs(levels);
    long strides[L][3], b[L][3];
    const void* ptrs[L];
    for (uint32_t l = 0; l < levels; ++l) {
        Out& t = outs[l];
        for (int d = 0; d < 3; ++d) {
            const uint64_t bin = std::min(rawbins[l][d], e[d]);
            t.C[d] = (e[d] + bin - 1) / bin;
            b[l][d] = (long)rawbins[l][d];
        }
        t.py = t.C[2] + (pitched ? 3 + l : 0);
        t.pz = t.C[1] * t.py + (pitched ? 5 : 0);
        t.v.assign((t.C[0] - 1) * t.pz + (t.C[1] - 1) * t.py + t.C[2], 0xA5A5A5A5u);
        t.stored.assign(t.v.size(), 0);
        strides[l][0] = (long)t.pz; strides[l][1] = (long)t.py; strides[l][2] = 1;
        ptrs[l] = t.v.data();
    }
    const std::vector<uint64_t> hshape{shape[0], shape[1], shape[2]};
    const long lo_[3] = {(long)o[0], (long)o[1], (long)o[2]}, le[3] = {(long)e[0], (long)e[1], (long)e[2]};
    sqy::BatchWindow w;
    sqy::Pyramid y;
    CHECK(sqy::admit_pyramid(hshape, lo_, le, 3, levels, &b[0][0], (int)op, 65535, ptrs, &strides[0][0], &w, &y));
    for (uint32_t l = 0; l < levels; ++l) CHECK(y.q[l].pz == outs[l].pz && y.q[l].py == outs[l].py && y.q[l].C[0] == outs[l].C[0] && y.q[l].C[2] == outs[l].C[2]);
    const sqy::WindowGeometry box{shape[1], shape[2], o[0], o[1], o[2], e[0], e[1], e[2], outs[0].pz, outs[0].py};
    const sqy::PyramidPlan P = sqy::pyramid_boxes_plan(y, e, budget0, budget, cap);
    const uint32_t T = P.T;
    CHECK(T < levels && T == rule_T(y, e, budget0, std::max(budget, budget0), cap));
    const uint64_t* bins = y.q[0].bins;
    const bool zreg = frame % 32 == 0;
    g_zreg += zreg;
    g_above += T + 1 < levels;
    const sqy::BinPlan top_plan = sqy::pyramid_top_plan(P);
    for (uint64_t own = 0; own < P.blocks; ++own) {
        ++g_blocks;
        const sqy::BinBlock top = sqy::bin_block_of(top_plan, own);
        uint64_t z0, nz0, cy0, ncy, cx0, ncx;
        sqy::pyramid_level_span(P, 0, 0, top.cz, 1, &z0, &nz0);
        sqy::pyramid_level_span(P, 0, 1, top.cy0, top.ncy, &cy0, &ncy);
        sqy::pyramid_level_span(P, 0, 2, top.cx0, top.ncx, &cx0, &ncx);
        CHECK(ncy * ncx <= budget0);
        // the stand-ins for LDS: every level's array holds exactly the block's cells of one layer
        std::vector<std::vector<uint32_t>> acc(T + 1);
        for (uint32_t l = 0; l <= T; ++l) {
            uint64_t f, ny, nx;
            sqy::pyramid_level_span(P, l, 1, top.cy0, top.ncy, &f, &ny);
            sqy::pyramid_level_span(P, l, 2, top.cx0, top.ncx, &f, &nx);
            acc[l].assign(ny * nx, 0xDEADBEEFu);
            CHECK(P.off[l] + ny * nx <= (l < T ? P.off[l + 1] : std::max(budget, budget0)));
        }
        for (uint64_t k = 0; k < nz0; ++k) {
            const sqy::BinBlock blk{z0 + k, cy0, ncy, cx0, ncx};
            std::fill(acc[0].begin(), acc[0].end(), sqy::project_neutral(op));
            ArraySink sink{&acc[0], op};
            const sqy::BinFootprint f = sqy::bin_block_footprint(box, bins, blk);
            CHECK(f.nz >= 1 && f.z0 >= o[0] && f.z0 + f.nz <= o[0] + e[0] && f.g.oy >= o[1] && f.g.oy + f.g.Y <= o[1] + e[1] && f.g.ox >= o[2] && f.g.ox + f.g.X <= o[2] + e[2]);
            const uint64_t items = sqy::bin_block_items(f, zreg);
            for (uint64_t t = 0; t < items; ++t) {
                uint64_t z, run;
                if (!sqy::bin_block_item(f, zreg, t, &z, &run)) continue;
                sqy::WindowGeometry g = f.g;
                g.oz = z;
                sqy::WindowClip c = sqy::window_clip_start(g, run * 32, 32);
                sqy::WindowPiece cur;
                bool have = sqy::window_clip_next(g, &c, &cur);
                if (!have) continue;
                uint32_t red[32];
                for (uint32_t i = 0; i < 32; ++i) red[i] = run * 32 + i < n ? voxel(run * 32 + i) : 0xdeadu;       // (behind the blob: never inside a footprint)
                if (zreg)
                    for (uint64_t zz = 1; zz < f.nz; ++zz)
                        for (uint32_t i = 0; i < 32; ++i) red[i] = sqy::project_combine(op, red[i], voxel(run * 32 + zz * frame + i));
                sqy::bin_run_cells(sink, g, c, cur, have, red, bins[1], bins[2], ncx, op);
                CHECK(!have);
            }
            // the kernel's stores of the layer
            {
                const uint64_t base = blk.cz * outs[0].pz + cy0 * outs[0].py + cx0;
                for (uint64_t cl = 0; cl < acc[0].size(); ++cl) {
                    const uint64_t cy = cl / ncx;
                    if (outs[0].store(base + cy * outs[0].py + (cl - cy * ncx), acc[0][cl])) return 1;
                    ++g_walk_cells;
                }
            }
            // the folds
            uint64_t done = blk.cz, mcy = ncy, mcx = ncx;
            for (uint32_t l = 1; l <= T; ++l) {
                const uint64_t rz = P.r[l][0], cz = done / rz, last = std::min((cz + 1) * rz, P.C[l - 1][0]);
                const bool first = done == cz * rz, complete = done + 1 == last;
                uint64_t ly0, lcy, lx0, lcx;
                sqy::pyramid_level_span(P, l, 1, top.cy0, top.ncy, &ly0, &lcy);
                sqy::pyramid_level_span(P, l, 2, top.cx0, top.ncx, &lx0, &lcx);
                CHECK(acc[l].size() == lcy * lcx && acc[l - 1].size() == mcy * mcx && lcy == (mcy + P.r[l][1] - 1) / P.r[l][1] && lcx == (mcx + P.r[l][2] - 1) / P.r[l][2]);
                const uint64_t base = cz * outs[l].pz + ly0 * outs[l].py + lx0;
                ++g_folds;
                for (uint64_t c = 0; c < lcy * lcx; ++c) {
                    const uint64_t yy = c / lcx, x = c - yy * lcx;
                    uint32_t v = sqy::pyramid_fold_cell(acc[l - 1].data(), mcy, mcx, P.r[l][1], P.r[l][2], yy, x, op);
                    if (!first) v = sqy::project_combine(op, acc[l][c], v);
                    acc[l][c] = v;
                    if (complete) {
                        if (outs[l].store(base + yy * outs[l].py + x, v)) return 1;
                        ++g_walk_cells;
                    }
                }
                if (!complete) break;
                done = cz; mcy = lcy; mcx = lcx;
            }
        }
    }
    // the tail: every level above T from the stored level-T cells, a thread per cell
    for (uint32_t l = T + 1; l < levels; ++l) {
        uint64_t r[3];
        for (int d = 0; d < 3; ++d) {
            r[d] = std::min(y.raw[l][d] / y.raw[T][d], outs[T].C[d]);
            CHECK(r[d] == P.q[l][d]);
        }
        for (uint64_t cz = 0; cz < outs[l].C[0]; ++cz)
            for (uint64_t cy = 0; cy < outs[l].C[1]; ++cy)
                for (uint64_t cx = 0; cx < outs[l].C[2]; ++cx) {
                    const uint32_t v = sqy::pyramid_reduce_cell(outs[T].v.data(), outs[T].C, outs[T].pz, outs[T].py, r, cz, cy, cx, op);
                    if (outs[l].store(cz * outs[l].pz + cy * outs[l].py + cx, v)) return 1;
                    ++g_tail_cells;
                }
    }
    // the triple loop, per level
    for (uint32_t l = 0; l < levels; ++l) {
        Out& t = outs[l];
        const uint64_t* rb = rawbins[l];
        for (uint64_t cz = 0; cz < t.C[0]; ++cz)
            for (uint64_t cy = 0; cy < t.C[1]; ++cy)
                for (uint64_t cx = 0; cx < t.C[2]; ++cx) {
                    uint32_t want = sqy::project_neutral(op);
                    for (uint64_t z = cz * rb[0]; z < std::min((cz + 1) * rb[0], e[0]); ++z)
                        for (uint64_t yy = cy * rb[1]; yy < std::min((cy + 1) * rb[1], e[1]); ++yy)
                            for (uint64_t x = cx * rb[2]; x < std::min((cx + 1) * rb[2], e[2]); ++x)
                                want = sqy::project_combine(op, want, voxel(((o[0] + z) * shape[1] + o[1] + yy) * shape[2] + o[2] + x));
                    const uint64_t at = cz * t.pz + cy * t.py + cx;
                    CHECK(t.stored[at] == 1 && t.v[at] == want);
                    t.stored[at] = 2;
                }
        for (uint64_t at = 0; at < t.v.size(); ++at) CHECK(t.stored[at] == 2 || (t.stored[at] == 0 && t.v[at] == 0xA5A5A5A5u));
    }
    return 0;
}

int test_walk()
{
    const uint64_t shapes[][3] = {{3, 5, 7}, {2, 3, 300}, {7, 33, 31}, {4, 8, 32}};
    // four levels; ratio 2; ratio 1 and x, y only; ratio 3 (and 1, 2 beside it); z only with a bin beyond the extent; a top level beyond T
    // under every budget below (its cell is the whole box); a repeated level
    const struct { uint32_t levels; uint64_t bins[4][3]; } pyramids[] = {
        {4, {{1, 1, 1}, {2, 2, 2}, {4, 4, 4}, {8, 8, 8}}}, {3, {{1, 2, 2}, {1, 4, 4}, {1, 8, 8}}}, {3, {{3, 5, 7}, {6, 5, 21}, {12, 10, 42}}},
        {2, {{2, 1, 1}, {1000, 1, 1}}}, {3, {{1, 1, 1}, {1, 3, 3}, {1000, 999, 999}}}, {2, {{2, 2, 2}, {2, 2, 2}}}, {1, {{2, 2, 2}}}, {2, {{1, 1, 32}, {2, 1, 128}}}};
    for (const auto& shape : shapes) {
        const uint64_t Z = shape[0], Y = shape[1], X = shape[2];
        const uint64_t boxes[][2][3] = {{{0, 0, 0}, {Z, Y, X}}, {{1, 1, 2}, {Z - 1, Y - 2, X - 3}}, {{Z - 1, 0, 0}, {1, Y, X}}, {{0, Y - 1, X - 1}, {Z, 1, 1}},
                                        {{0, 2, 0}, {2, 1, X}}, {{1, 0, 3}, {1, Y, 1}}};
        unsigned k = 0;
        for (const auto& box : boxes)
            for (const auto& py : pyramids)
                for (uint32_t op = 0; op < 3; ++op, ++k) {
                    // the library's budgets; ones that cut level-T rows into strips; ones that make bands of a few rows; a level-0 budget that
                    // pushes levels into the tail
                    const uint64_t budgets[][3] = {{sqy::kBinBlockCells, sqy::kPyramidLdsCells, sqy::kPyramidBlockVoxels}, {16, 24, 64}, {40, 100, 1u << 16}, {4, 4, 1u << 16}};
                    const auto& bc = budgets[k % 4];
                    if (walk_box(shape, box[0], box[1], py.levels, py.bins, op, bc[0], bc[1], bc[2], (k / 4) % 2 == 1)) {
                        std::fprintf(stderr, "shape %llu %llu %llu box %llu %llu %llu + %llu %llu %llu levels %u first bins %llu %llu %llu op %u budget %llu\n",
                                     (unsigned long long)Z, (unsigned long long)Y, (unsigned long long)X, (unsigned long long)box[0][0], (unsigned long long)box[0][1],
                                     (unsigned long long)box[0][2], (unsigned long long)box[1][0], (unsigned long long)box[1][1], (unsigned long long)box[1][2], py.levels,
                                     (unsigned long long)py.bins[0][0], (unsigned long long)py.bins[0][1], (unsigned long long)py.bins[0][2], op, (unsigned long long)bc[0]);
                        return 1;
                    }
                }
    }
    return 0;
}

} // namespace

int main()
{
    if (test_path() || test_layout() || test_admission() || test_plan() || test_walk()) return 1;
    std::printf("walk blocks %llu folds %llu stored %llu tail %llu zreg %llu above %llu\n", g_blocks, g_folds, g_walk_cells, g_tail_cells, g_zreg, g_above);
    std::printf("pyramid_boxes ok\n");
    return 0;
}
