// Boxes of one large blob read at a coarser resolution, on the host (tests/test_host_bin_boxes.py builds and runs this with g++,
// sanitizers on): sqy::bin_boxes_path against its table, the binning jobs' layout, sqy::admit_binning at every refusal and at the sum
// bound, sqy::bin_boxes_plan -- its blocks cover every cell of a grid exactly once and stay inside the accumulators' budget, on grids of
// 1, prime and budget-straddling sizes --, and the cell walk of SQYAMD_Bin_Boxes_*'s bit-plane kernel item by item as
// bitswap1_decode_range_windows_bin_kernel drives it: every block of a box's plan, its footprint, its items (a 32-voxel run of a
// footprint frame each; where a frame is a whole number of runs the run's positions reduced over the cell layer's frames first), the
// clip of csrc/sqy_batch_window.hpp on the run and sqy::bin_run_cells into an array of exactly the block's cells standing in for the LDS
// accumulators (a combine that strays is the sanitizer's); the block's cells then go to the output as the kernel stores them.  Afterwards
// every cell must equal a triple loop's, every gap between pitched rows its pattern, and every cell must have been stored once.  Blobs
// 3 x 5 x 7, 2 x 3 x 300, 7 x 33 x 31 and 4 x 8 x 32 (a frame of whole runs); all three ops; budgets that force bands and strips.
// Prints the items outside, inside and partly inside a footprint, the blocks, and the boxes reduced over z in registers, then
// "bin_boxes ok"; returns 0.
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

unsigned long long g_outside = 0, g_inside = 0, g_partly = 0, g_blocks = 0, g_zreg = 0;

int test_path()
{
    const struct { RangeForm form; BoxPath on; } table[] = {{RangeForm::plain, BoxPath::subset_copy}, {RangeForm::planes, BoxPath::subset_transposer},
                                                            {RangeForm::planes_lut, BoxPath::subset_transposer}, {RangeForm::shuffle, BoxPath::subset_copy}};
    for (const auto& row : table) {
        CHECK(sqy::bin_boxes_path(true, row.form, true) == row.on);
        CHECK(sqy::bin_boxes_path(true, row.form, false) == BoxPath::whole_copy);           // the option off
        CHECK(sqy::bin_boxes_path(false, row.form, true) == BoxPath::whole_copy);           // a blob the frame-range plan does not take
        CHECK(sqy::bin_boxes_path(false, row.form, false) == BoxPath::whole_copy);
    }
    return 0;
}

int test_layout()
{
    static_assert(sizeof(sqy::Bitswap1BoxBinJob) == sqy::kBitswap1BoxBinJobBytes && sizeof(sqy::Bitswap1BoxBinJob) % 16 == 0, "the binning box job's layout");
    static_assert(offsetof(sqy::Bitswap1BoxBinJob, g) == offsetof(sqy::Bitswap1BoxJob, g) && offsetof(sqy::Bitswap1BoxBinJob, r) == offsetof(sqy::Bitswap1BoxJob, r) &&
                      offsetof(sqy::Bitswap1BoxBinJob, t0) == offsetof(sqy::Bitswap1BoxJob, t0) && offsetof(sqy::Bitswap1BoxBinJob, bins) == sizeof(sqy::Bitswap1BoxJob),
                  "Bitswap1BoxJob's fields, the bins and the tiling behind them");
    static_assert(sizeof(sqy::BoxBinJob) == sqy::kBoxBinJobBytes && sizeof(sqy::BoxBinJob) % 16 == 0, "the per-cell job's layout");
    static_assert(sqy::kBinBlockCells * 4u <= 40u * 1024u, "the accumulators: well under the CU's 160 KiB of LDS");
    for (uint64_t n : {(uint64_t)1, (uint64_t)3, (uint64_t)64, (uint64_t)100001}) {
        const sqy::BatchWindowLayout l = sqy::batch_window_layout(n, sizeof(sqy::Bitswap1BoxBinJob));
        CHECK(l.tiles_at == n * sizeof(sqy::Bitswap1BoxBinJob) && l.tiles_at % 16 == 0 && l.total == l.tiles_at + (n + 1) * sizeof(uint32_t));
    }
    return 0;
}

int test_admission()
{
    alignas(16) uint32_t out[64];
    sqy::BatchWindow w;
    sqy::Binning q;
    const long o[3] = {0, 0, 0};
    // the sum bound, 16-bit voxels: a cell of V = 65536 voxels is taken, the first V above it is not; max and min have no bound
    {
        const std::vector<uint64_t> shape{16, 64, 65};
        const long e[3] = {16, 64, 65}, fits[3] = {16, 64, 64}, over[3] = {16, 64, 65}, over1[3] = {16, 4097, 1};
        CHECK(sqy::admit_binning(shape, o, e, 3, fits, 2, 65535, out, nullptr, &w, &q));
        CHECK(q.C[0] == 1 && q.C[1] == 1 && q.C[2] == 2 && q.bins[0] == 16 && q.bins[1] == 64 && q.bins[2] == 64 && q.py == 2 && q.pz == 2);
        CHECK(!sqy::admit_binning(shape, o, e, 3, over, 2, 65535, out, nullptr, &w, &q));
        CHECK(sqy::admit_binning(shape, o, e, 3, over, 0, 65535, out, nullptr, &w, &q) && sqy::admit_binning(shape, o, e, 3, over, 1, 65535, out, nullptr, &w, &q));
        const std::vector<uint64_t> tall{16, 5000, 1};
        const long et[3] = {16, 5000, 1}, fits1[3] = {16, 4096, 1};
        CHECK(sqy::admit_binning(tall, o, et, 3, fits1, 2, 65535, out, nullptr, &w, &q));                  // V = 65536
        CHECK(!sqy::admit_binning(tall, o, et, 3, over1, 2, 65535, out, nullptr, &w, &q));                 // V = 65552: the first above it with bz = 16
        // rank 1: V = the bin itself, 65536 | 65537
        const std::vector<uint64_t> line{70000};
        const long el[1] = {70000}, b0[1] = {65536}, b1[1] = {65537};
        CHECK(sqy::admit_binning(line, o, el, 1, b0, 2, 65535, out, nullptr, &w, &q) && q.C[2] == 2 && q.C[1] == 1 && q.C[0] == 1);
        CHECK(!sqy::admit_binning(line, o, el, 1, b1, 2, 65535, out, nullptr, &w, &q));
    }
    // the clamp: bins far beyond the extents count as the extents -- V = 2 x 3 x 4, no overflow whatever the bins
    {
        const std::vector<uint64_t> shape{2, 3, 4};
        const long e[3] = {2, 3, 4}, huge[3] = {LONG_MAX, LONG_MAX, LONG_MAX}, big[3] = {1000, 1000, 1000};
        CHECK(sqy::admit_binning(shape, o, e, 3, huge, 2, 65535, out, nullptr, &w, &q));
        CHECK(q.bins[0] == 2 && q.bins[1] == 3 && q.bins[2] == 4 && q.C[0] == 1 && q.C[1] == 1 && q.C[2] == 1);
        CHECK(sqy::admit_binning(shape, o, e, 3, big, 2, 255, out, nullptr, &w, &q));
        // extents whose clamped product passes 2^64: refused, not wrapped to a small V
        const std::vector<uint64_t> vast{(uint64_t)1 << 22, (uint64_t)1 << 22, (uint64_t)1 << 22};
        const long ev[3] = {1l << 22, 1l << 22, 1l << 22};
        CHECK(!sqy::admit_binning(vast, o, ev, 3, huge, 2, 65535, out, nullptr, &w, &q));
        CHECK(!sqy::admit_binning(vast, o, ev, 3, huge, 2, 255, out, nullptr, &w, &q));
        CHECK(sqy::admit_binning(vast, o, ev, 3, huge, 0, 255, out, nullptr, &w, &q) && q.C[0] == 1);
    }
    // 8-bit voxels: 255 V < 2^32 is taken (V = 16843009), 255 V >= 2^32 is not
    {
        const std::vector<uint64_t> line{20000000};
        const long el[1] = {20000000}, fits[1] = {16843009}, over[1] = {16843010};
        CHECK(sqy::admit_binning(line, o, el, 1, fits, 2, 255, out, nullptr, &w, &q));
        CHECK(!sqy::admit_binning(line, o, el, 1, over, 2, 255, out, nullptr, &w, &q));
    }
    // every other refusal; the good call between them
    {
        const std::vector<uint64_t> shape{3, 5, 7};
        const long o1[3] = {1, 1, 1}, e[3] = {2, 3, 4}, b[3] = {2, 2, 3};                                  // cells 1 x 2 x 2
        CHECK(sqy::admit_binning(shape, o1, e, 3, b, 0, 65535, out, nullptr, &w, &q) && q.C[0] == 1 && q.C[1] == 2 && q.C[2] == 2 && q.py == 2 && q.pz == 4);
        CHECK(!sqy::admit_binning(shape, o1, e, 3, nullptr, 0, 65535, out, nullptr, &w, &q));              // bins NULL
        for (int d = 0; d < 3; ++d)
            for (long bad : {0l, -1l, LONG_MIN}) {
                long bb[3] = {2, 2, 3};
                bb[d] = bad;
                CHECK(!sqy::admit_binning(shape, o1, e, 3, bb, 0, 65535, out, nullptr, &w, &q));            // an entry < 1
            }
        for (int op : {3, -1, INT_MAX}) CHECK(!sqy::admit_binning(shape, o1, e, 3, b, op, 65535, out, nullptr, &w, &q));
        CHECK(!sqy::admit_binning(shape, o1, e, 3, b, 0, 65535, nullptr, nullptr, &w, &q));                // a NULL output
        CHECK(!sqy::admit_binning(shape, o1, e, 3, b, 0, 65535, reinterpret_cast<const char*>(out) + 2, nullptr, &w, &q));      // 2 bytes off
        CHECK(sqy::admit_binning(shape, o1, e, 3, b, 0, 65535, out + 1, nullptr, &w, &q));                 // 4 bytes behind the grid: taken
        const long pitched[3] = {9, 4, 1}, inner2[3] = {8, 4, 2}, overlap[3] = {4, 1, 1}, reach[3] = {7, 4, 1}, zero[3] = {0, 4, 1};
        CHECK(sqy::admit_binning(shape, o1, e, 3, b, 0, 65535, out, pitched, &w, &q) && q.py == 4 && q.pz == 9);
        for (const long* s : {inner2, overlap, reach, zero}) CHECK(!sqy::admit_binning(shape, o1, e, 3, b, 0, 65535, out, s, &w, &q));
        // what Decode_Boxes refuses for a box
        const long neg[3] = {1, -1, 1}, past[3] = {2, 3, 7}, none[3] = {2, 0, 4}, far[3] = {LONG_MAX, 0, 0}, one[3] = {1, 1, 1};
        CHECK(!sqy::admit_binning(shape, neg, e, 3, b, 0, 65535, out, nullptr, &w, &q));
        CHECK(!sqy::admit_binning(shape, o1, past, 3, b, 0, 65535, out, nullptr, &w, &q));
        CHECK(!sqy::admit_binning(shape, o1, none, 3, b, 0, 65535, out, nullptr, &w, &q));
        CHECK(!sqy::admit_binning(shape, far, one, 3, b, 0, 65535, out, nullptr, &w, &q));
        CHECK(!sqy::admit_binning(shape, o1, e, 2, b, 0, 65535, out, nullptr, &w, &q));                    // another rank than the header's
        CHECK(!sqy::admit_binning(shape, o1, e, 3, b, 0, 65535, out, nullptr, nullptr, &q) && !sqy::admit_binning(shape, o1, e, 3, b, 0, 65535, out, nullptr, &w, nullptr));
        // rank 2: frames are the first dimension; the pitches are the two the caller gave
        const std::vector<uint64_t> flat{40, 300};
        const long o2[2] = {3, 17}, e2[2] = {30, 200}, b2[2] = {4, 7}, s2[2] = {40, 1};
        CHECK(sqy::admit_binning(flat, o2, e2, 2, b2, 2, 65535, out, s2, &w, &q));
        CHECK(q.C[0] == 1 && q.C[1] == 8 && q.C[2] == 29 && q.bins[0] == 1 && q.bins[1] == 4 && q.bins[2] == 7 && q.py == 40);
    }
    return 0;
}

// the blocks of a plan cover every cell exactly once and none holds more cells than the budget
int check_plan(const uint64_t C[3], const uint64_t bins[3], uint64_t X, uint64_t budget, uint64_t cap)
{
    const sqy::BinPlan p = sqy::bin_boxes_plan(C, bins, X, budget, cap);
    CHECK(p.C[0] == C[0] && p.C[1] == C[1] && p.C[2] == C[2] && p.band >= 1 && p.strip >= 1 && p.band * p.strip <= budget);
    CHECK(p.blocks == C[0] * p.nbands * p.nstrips && p.nbands == (C[1] + p.band - 1) / p.band && p.nstrips == (C[2] + p.strip - 1) / p.strip);
    std::vector<unsigned char> seen(C[0] * C[1] * C[2], 0);
    for (uint64_t own = 0; own < p.blocks; ++own) {
        const sqy::BinBlock b = sqy::bin_block_of(p, own);
        CHECK(b.cz < C[0] && b.ncy >= 1 && b.ncx >= 1 && b.cy0 + b.ncy <= C[1] && b.cx0 + b.ncx <= C[2] && b.ncy * b.ncx <= budget);
        for (uint64_t y = b.cy0; y < b.cy0 + b.ncy; ++y)
            for (uint64_t x = b.cx0; x < b.cx0 + b.ncx; ++x) {
                unsigned char& s = seen.at((b.cz * C[1] + y) * C[2] + x);
                CHECK(s == 0);
                s = 1;
            }
    }
    CHECK(std::count(seen.begin(), seen.end(), 1) == (long)seen.size());
    return 0;
}

int test_plan()
{
    const uint64_t sizes[] = {1, 2, 7, 13, 31, 63, 64, 65, 127, 128, 129, 257};            // 1, primes, and the budgets below straddled
    const uint64_t ones[3] = {1, 1, 1}, coarse[3] = {3, 5, 7};
    for (uint64_t budget : {(uint64_t)1, (uint64_t)64, (uint64_t)128})
        for (uint64_t cz : {(uint64_t)1, (uint64_t)3})
            for (uint64_t cy : sizes)
                for (uint64_t cx : sizes) {
                    const uint64_t C[3] = {cz, cy, cx};
                    for (uint64_t cap : {(uint64_t)1, (uint64_t)200, (uint64_t)1 << 16}) {
                        if (check_plan(C, ones, cx, budget, cap)) return 1;
                        if (check_plan(C, coarse, cx * 7 - 3, budget, cap)) return 1;
                    }
                }
    // the library's own budget, straddled by one cell row and by the rows of a band
    for (uint64_t cx : {(uint64_t)sqy::kBinBlockCells - 1, (uint64_t)sqy::kBinBlockCells, (uint64_t)sqy::kBinBlockCells + 1, (uint64_t)2 * sqy::kBinBlockCells + 3}) {
        const uint64_t C[3] = {2, 3, cx};
        if (check_plan(C, ones, cx, sqy::kBinBlockCells, sqy::kBinBlockVoxels)) return 1;
    }
    {
        const uint64_t C[3] = {64, 512, 512}, b[3] = {1, 2, 2};
        const sqy::BinPlan p = sqy::bin_boxes_plan(C, b, 1024);
        CHECK(p.strip == 512 && p.band == 16 && p.blocks == 64 * 32);                    // 16 cell rows x 512: the budget; 32 rows x 1024 voxels: half the cap
        const uint64_t huge[3] = {(uint64_t)1 << 62, (uint64_t)1 << 62, 4};
        const uint64_t one[3] = {1, 1, 3};
        const sqy::BinPlan h = sqy::bin_boxes_plan(one, huge, (uint64_t)1 << 40);         // bins that would overflow a product: one cell row to a block
        CHECK(h.band == 1 && h.strip == 3 && h.blocks == 1);
    }
    return 0;
}

uint32_t voxel(uint64_t i) { return (uint32_t)((i * 2654435761ull >> 7) % 65521ull); }

struct ArraySink {
    std::vector<uint32_t>* acc;
    uint32_t op;
    void combine(uint64_t cell, uint32_t v) { uint32_t& a = acc->at(cell); a = sqy::project_combine(op, a, v); }
};

// one box of a blob through the kernel's walk into `out` (pitches pz, py), under a plan with the given budget and cap
int walk_box(const uint64_t shape[3], const uint64_t o[3], const uint64_t e[3], const uint64_t rawbins[3], uint32_t op, uint64_t budget, uint64_t cap, bool pitched)
{
    const uint64_t n = shape[0] * shape[1] * shape[2], frame = shape[1] * shape[2];
    uint64_t bins[3], C[3];
    for (int d = 0; d < 3; ++d) { bins[d] = std::min(rawbins[d], e[d]); C[d] = (e[d] + bins[d] - 1) / bins[d]; }
    const uint64_t py = C[2] + (pitched ? 3 : 0), pz = C[1] * py + (pitched ? 5 : 0);
    const sqy::WindowGeometry box{shape[1], shape[2], o[0], o[1], o[2], e[0], e[1], e[2], pz, py};
    const sqy::BinPlan plan = sqy::bin_boxes_plan(C, bins, e[2], budget, cap);
    const bool zreg = frame % 32 == 0;
    g_zreg += zreg;
    std::vector<uint32_t> out((C[0] - 1) * pz + (C[1] - 1) * py + C[2], 0xA5A5A5A5u);
    std::vector<unsigned char> stored(out.size(), 0);
    for (uint64_t own = 0; own < plan.blocks; ++own) {
        ++g_blocks;
        const sqy::BinBlock blk = sqy::bin_block_of(plan, own);
        CHECK(blk.ncy * blk.ncx <= budget);
        std::vector<uint32_t> acc(blk.ncy * blk.ncx, sqy::project_neutral(op));
        ArraySink sink{&acc, op};
        const sqy::BinFootprint f = sqy::bin_block_footprint(box, bins, blk);
        CHECK(f.nz >= 1 && f.z0 >= o[0] && f.z0 + f.nz <= o[0] + e[0] && f.g.oy >= o[1] && f.g.oy + f.g.Y <= o[1] + e[1] && f.g.ox >= o[2] && f.g.ox + f.g.X <= o[2] + e[2]);
        CHECK(f.g.sy >= f.g.X && (f.g.sy & (f.g.sy - 1)) == 0 && f.g.sz == 0);
        const uint64_t items = sqy::bin_block_items(f, zreg);
        for (uint64_t t = 0; t < items; ++t) {
            uint64_t z, run;
            if (!sqy::bin_block_item(f, zreg, t, &z, &run)) continue;
            sqy::WindowGeometry g = f.g;
            g.oz = z;
            sqy::WindowClip c = sqy::window_clip_start(g, run * 32, 32);
            sqy::WindowPiece cur;
            bool have = sqy::window_clip_next(g, &c, &cur);
            if (!have) { ++g_outside; continue; }
            uint64_t inside = 0;
            for (uint64_t i = run * 32; i < run * 32 + 32 && i < n; ++i) {
                const uint64_t zz = i / frame, yy = i % frame / shape[2], xx = i % shape[2];
                inside += zz == z && yy >= f.g.oy && yy < f.g.oy + f.g.Y && xx >= f.g.ox && xx < f.g.ox + f.g.X;
            }
            CHECK(inside > 0);
            ++(inside == 32 ? g_inside : g_partly);
            uint32_t red[32];
            for (uint32_t i = 0; i < 32; ++i) red[i] = run * 32 + i < n ? voxel(run * 32 + i) : 0xdeadu;       // (behind the blob: never inside a footprint)
            if (zreg)
                for (uint64_t zz = 1; zz < f.nz; ++zz)
                    for (uint32_t i = 0; i < 32; ++i) red[i] = sqy::project_combine(op, red[i], voxel(run * 32 + zz * frame + i));
            sqy::bin_run_cells(sink, g, c, cur, have, red, bins[1], bins[2], blk.ncx, op);
            CHECK(!have);
        }
        // the kernel's stores
        const uint64_t base = blk.cz * pz + blk.cy0 * py + blk.cx0;
        for (uint64_t cl = 0; cl < acc.size(); ++cl) {
            const uint64_t cy = cl / blk.ncx, at = base + cy * py + (cl - cy * blk.ncx);
            CHECK(stored.at(at) == 0);
            stored[at] = 1;
            out.at(at) = acc[cl];
        }
    }
    // the triple loop
    for (uint64_t cz = 0; cz < C[0]; ++cz)
        for (uint64_t cy = 0; cy < C[1]; ++cy)
            for (uint64_t cx = 0; cx < C[2]; ++cx) {
                uint32_t want = sqy::project_neutral(op);
                for (uint64_t z = cz * rawbins[0]; z < std::min((cz + 1) * rawbins[0], e[0]); ++z)
                    for (uint64_t y = cy * rawbins[1]; y < std::min((cy + 1) * rawbins[1], e[1]); ++y)
                        for (uint64_t x = cx * rawbins[2]; x < std::min((cx + 1) * rawbins[2], e[2]); ++x)
                            want = sqy::project_combine(op, want, voxel(((o[0] + z) * shape[1] + o[1] + y) * shape[2] + o[2] + x));
                const uint64_t at = cz * pz + cy * py + cx;
                CHECK(stored[at] == 1 && out[at] == want);
                stored[at] = 2;
            }
    for (uint64_t at = 0; at < out.size(); ++at) CHECK(stored[at] == 2 || (stored[at] == 0 && out[at] == 0xA5A5A5A5u));
    return 0;
}

int test_walk()
{
    const uint64_t shapes[][3] = {{3, 5, 7}, {2, 3, 300}, {7, 33, 31}, {4, 8, 32}};
    const uint64_t binsets[][3] = {{1, 1, 1}, {2, 2, 2}, {3, 5, 7}, {1, 1, 32}, {1, 1, 128}, {2, 1, 1}, {1000, 1, 1}, {1, 1000, 1}, {1, 1, 1000}, {4, 3, 33}};
    for (const auto& shape : shapes) {
        const uint64_t Z = shape[0], Y = shape[1], X = shape[2];
        const uint64_t boxes[][2][3] = {{{0, 0, 0}, {Z, Y, X}}, {{1, 1, 2}, {Z - 1, Y - 2, X - 3}}, {{Z - 1, 0, 0}, {1, Y, X}}, {{0, Y - 1, X - 1}, {Z, 1, 1}},
                                        {{0, 2, 0}, {2, 1, X}}, {{1, 0, 3}, {1, Y, 1}}};
        unsigned k = 0;
        for (const auto& box : boxes)
            for (const auto& bins : binsets)
                for (uint32_t op = 0; op < 3; ++op, ++k) {
                    // the library's budget; one that cuts cell rows into strips; one that makes bands of a few rows
                    const uint64_t budgets[][2] = {{sqy::kBinBlockCells, sqy::kBinBlockVoxels}, {5, 64}, {40, 1u << 16}};
                    const auto& bc = budgets[k % 3];
                    if (walk_box(shape, box[0], box[1], bins, op, bc[0], bc[1], (k / 3) % 2 == 1)) {
                        std::fprintf(stderr, "shape %llu %llu %llu box %llu %llu %llu + %llu %llu %llu bins %llu %llu %llu op %u budget %llu\n", (unsigned long long)Z,
                                     (unsigned long long)Y, (unsigned long long)X, (unsigned long long)box[0][0], (unsigned long long)box[0][1], (unsigned long long)box[0][2],
                                     (unsigned long long)box[1][0], (unsigned long long)box[1][1], (unsigned long long)box[1][2], (unsigned long long)bins[0],
                                     (unsigned long long)bins[1], (unsigned long long)bins[2], op, (unsigned long long)bc[0]);
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
    std::printf("items outside %llu inside %llu partly %llu blocks %llu zreg %llu\n", g_outside, g_inside, g_partly, g_blocks, g_zreg);
    std::printf("bin_boxes ok\n");
    return 0;
}
