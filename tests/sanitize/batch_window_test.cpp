// Windows on the host (tests/test_host_batch_windows.py builds and runs this with g++, sanitizers on): sqy::admit_window's rules for ranks
// 1 to 3 and an origin + extent that overflows `long`; the clip of csrc/sqy_batch_window.hpp -- the one the kernels compile -- against a
// triple loop for EVERY window of small blobs, in runs of 128 voxels as the windowed transposer cuts them, with a short last run and the
// tail of up to 16 voxels one by one; the tiles a window's frames reach; the window table's layout against the kernels' job struct.
// Prints "batch_window ok" and returns 0.
#include "../../sqeazy_amd/csrc/sqy_batch_window.hpp"
#include "../../sqeazy_amd/csrc/sqy_kernels.h"
#include "../../sqeazy_amd/csrc/sqy_pipeline.hpp"

#include <climits>
#include <cstdio>
#include <vector>

#define CHECK(cond)                                                                   \
    do {                                                                              \
        if (!(cond)) { std::fprintf(stderr, "line %d: %s\n", __LINE__, #cond); return 1; } \
    } while (0)

using sqy::BatchWindow;

namespace {

bool admit(std::vector<uint64_t> header, std::vector<long> origin, std::vector<long> extent, BatchWindow* w)
{
    return sqy::admit_window(header, origin.empty() ? nullptr : origin.data(), extent.data(), (unsigned)extent.size(), w);
}
bool same(const BatchWindow& w, uint64_t bZ, uint64_t bY, uint64_t bX, uint64_t oz, uint64_t oy, uint64_t ox, uint64_t Z, uint64_t Y, uint64_t X, bool whole)
{
    return w.bZ == bZ && w.bY == bY && w.bX == bX && w.oz == oz && w.oy == oy && w.ox == ox && w.Z == Z && w.Y == Y && w.X == X && w.whole == whole;
}

int test_admit()
{
    BatchWindow w;
    // every rank, padded in front; the whole blob with and without an origin
    CHECK(admit({3, 5, 7}, {}, {3, 5, 7}, &w) && same(w, 3, 5, 7, 0, 0, 0, 3, 5, 7, true));
    CHECK(admit({3, 5, 7}, {0, 0, 0}, {3, 5, 7}, &w) && w.whole);
    CHECK(admit({3, 5, 7}, {1, 2, 3}, {2, 3, 4}, &w) && same(w, 3, 5, 7, 1, 2, 3, 2, 3, 4, false));
    CHECK(admit({3, 5, 7}, {}, {3, 5, 6}, &w) && same(w, 3, 5, 7, 0, 0, 0, 3, 5, 6, false));
    CHECK(admit({5, 7}, {4, 6}, {1, 1}, &w) && same(w, 1, 5, 7, 0, 4, 6, 1, 1, 1, false));
    CHECK(admit({5, 7}, {}, {5, 7}, &w) && same(w, 1, 5, 7, 0, 0, 0, 1, 5, 7, true));
    CHECK(admit({7}, {2}, {5}, &w) && same(w, 1, 1, 7, 0, 0, 2, 1, 1, 5, false));
    CHECK(admit({7}, {0}, {7}, &w) && w.whole);
    // the last voxel, in every dimension in turn one beyond
    CHECK(admit({3, 5, 7}, {2, 4, 6}, {1, 1, 1}, &w));
    CHECK(!admit({3, 5, 7}, {3, 4, 6}, {1, 1, 1}, &w) && !admit({3, 5, 7}, {2, 5, 6}, {1, 1, 1}, &w) && !admit({3, 5, 7}, {2, 4, 7}, {1, 1, 1}, &w));
    CHECK(!admit({3, 5, 7}, {1, 0, 0}, {3, 5, 7}, &w) && !admit({3, 5, 7}, {0, 1, 0}, {3, 5, 7}, &w) && !admit({3, 5, 7}, {0, 0, 1}, {3, 5, 7}, &w));
    CHECK(!admit({3, 5, 7}, {}, {4, 5, 7}, &w) && !admit({5, 7}, {}, {5, 8}, &w) && !admit({7}, {}, {8}, &w) && !admit({7}, {7}, {1}, &w));
    // a negative origin, an extent below 1
    CHECK(!admit({3, 5, 7}, {-1, 0, 0}, {1, 1, 1}, &w) && !admit({3, 5, 7}, {0, 0, -1}, {1, 1, 1}, &w) && !admit({7}, {-1}, {1}, &w));
    CHECK(!admit({3, 5, 7}, {}, {0, 5, 7}, &w) && !admit({3, 5, 7}, {}, {3, 5, 0}, &w) && !admit({3, 5, 7}, {}, {3, -5, 7}, &w) && !admit({5, 7}, {}, {0, 7}, &w));
    // the rank: the header's, 1 to 3
    CHECK(!admit({3, 5, 7}, {}, {5, 7}, &w) && !admit({5, 7}, {}, {1, 5, 7}, &w) && !admit({35}, {}, {5, 7}, &w));
    CHECK(!admit({2, 3, 5, 7}, {}, {2, 3, 5, 7}, &w) && !admit({}, {}, {}, &w));
    long e3[3] = {3, 5, 7};
    const std::vector<uint64_t> h3 = {3, 5, 7};
    CHECK(!sqy::admit_window(h3, nullptr, nullptr, 3, &w) && !sqy::admit_window(h3, nullptr, e3, 3, nullptr) && !sqy::admit_window(h3, nullptr, e3, 0, &w));
    // origin + extent past LONG_MAX: beyond every shape, no wrap to a small sum
    CHECK(!admit({3, 5, 7}, {LONG_MAX, 0, 0}, {1, 1, 1}, &w) && !admit({3, 5, 7}, {0, 0, LONG_MAX}, {1, 1, LONG_MAX}, &w));
    CHECK(!admit({3, 5, 7}, {0, 1, 0}, {1, LONG_MAX, 1}, &w) && !admit({7}, {LONG_MAX}, {LONG_MAX}, &w));
    CHECK(admit({~(uint64_t)0}, {LONG_MAX}, {LONG_MAX}, &w) && w.ox == (uint64_t)LONG_MAX && w.X == (uint64_t)LONG_MAX && !w.whole);
    CHECK(admit({(uint64_t)LONG_MAX + 5}, {LONG_MAX}, {5}, &w) && !admit({(uint64_t)LONG_MAX + 5}, {LONG_MAX}, {6}, &w));
    return 0;
}

// Every window of a blob of (bZ, bY, bX) voxels into a pitched view: the runs [i0, i0 + n) of the dense order -- of `run` voxels, the last
// one of the planes short, then the tail voxel by voxel, as the windowed transposer cuts a blob of voxels of `elem` bytes -- must write
// each voxel of the window exactly once, from its place in the run to its place in the view, in ascending order, and nothing else
int clip_blob(uint64_t bZ, uint64_t bY, uint64_t bX, uint64_t run, int elem)
{
    const uint64_t len = bZ * bY * bX, W = 8 * (uint64_t)elem, L = len / W * W;
    std::vector<uint32_t> written;
    for (uint64_t oz = 0; oz < bZ; ++oz) for (uint64_t Z = 1; oz + Z <= bZ; ++Z)
    for (uint64_t oy = 0; oy < bY; ++oy) for (uint64_t Y = 1; oy + Y <= bY; ++Y)
    for (uint64_t ox = 0; ox < bX; ++ox) for (uint64_t X = 1; ox + X <= bX; ++X) {
        const sqy::WindowGeometry g{bY, bX, oz, oy, ox, Z, Y, X, Y * (X + 3) + 5, X + 3};
        written.assign((size_t)(Z * g.sz), 0);
        uint64_t count = 0;
        for (uint64_t i0 = 0; i0 < len;) {
            const uint64_t n = i0 < L ? (L - i0 < run ? L - i0 : run) : 1;
            sqy::WindowClip c = sqy::window_clip_start(g, i0, n);
            sqy::WindowPiece p;
            uint64_t behind = 0;                 // pieces ascend and do not overlap
            while (sqy::window_clip_next(g, &c, &p)) {
                CHECK(p.len >= 1 && p.run_off >= behind && p.run_off + p.len <= n);
                behind = p.run_off + p.len;
                for (uint64_t k = 0; k < p.len; ++k) {
                    const uint64_t i = i0 + p.run_off + k, z = i / (bY * bX), y = i / bX % bY, x = i % bX;
                    CHECK(z >= oz && z < oz + Z && y >= oy && y < oy + Y && x >= ox && x < ox + X);
                    CHECK(p.dst_off + k == (z - oz) * g.sz + (y - oy) * g.sy + (x - ox));
                    CHECK(written[(size_t)(p.dst_off + k)]++ == 0);
                    ++count;
                }
            }
            CHECK(!sqy::window_clip_next(g, &c, &p));       // (exhausted stays exhausted)
            i0 += n;
        }
        CHECK(count == Z * Y * X);
        // the tiles of the transposer's grid: every tile that holds a voxel of the window's frames, no tile in front of them
        for (uint64_t tile : {(uint64_t)16, (uint64_t)128, (uint64_t)32768}) {
            const uint64_t t0 = sqy::window_first_tile(g, tile), nt = sqy::window_tile_count(g, tile);
            CHECK(nt >= 1 && t0 == oz * bY * bX / tile && t0 + nt - 1 == ((oz + Z) * bY * bX - 1) / tile);
        }
    }
    return 0;
}

int test_clip()
{
    // every origin and every extent; runs of 128 (one run here) and of 16 voxels, so that runs begin and end inside rows
    for (uint64_t run : {(uint64_t)128, (uint64_t)16})
        for (int elem : {2, 1}) {
            CHECK(clip_blob(3, 5, 7, run, elem) == 0);
            CHECK(clip_blob(2, 3, 9, run, elem) == 0);
        }
    return 0;
}

// shapes whose rows cross the boundary of a 128-voxel run: all runs i0 = 128 k, the short last run, the tail -- and every window of them
// along x, with a sample of the others (every window of (2,3,130) would be 10^8 voxel checks)
int clip_long_rows(uint64_t bZ, uint64_t bY, uint64_t bX, int elem)
{
    const uint64_t len = bZ * bY * bX, W = 8 * (uint64_t)elem, L = len / W * W;
    std::vector<uint32_t> written;
    for (uint64_t oz = 0; oz < bZ; ++oz) for (uint64_t Z = 1; oz + Z <= bZ; ++Z)
    for (uint64_t oy = 0; oy < bY; ++oy) for (uint64_t Y = 1; oy + Y <= bY; ++Y)
    for (uint64_t ox : {(uint64_t)0, (uint64_t)1, (uint64_t)15, (uint64_t)16, (uint64_t)127, (uint64_t)128, bX - 2, bX - 1})
    for (uint64_t X : {(uint64_t)1, (uint64_t)2, (uint64_t)16, (uint64_t)113, (uint64_t)128, (uint64_t)129, bX - ox}) {
        if (ox + X > bX) continue;
        const sqy::WindowGeometry g{bY, bX, oz, oy, ox, Z, Y, X, Y * (X + 3), X + 3};
        written.assign((size_t)(Z * g.sz), 0);
        uint64_t count = 0;
        for (uint64_t i0 = 0; i0 < len;) {
            const uint64_t n = i0 < L ? (L - i0 < 128 ? L - i0 : 128) : 1;
            if (i0 < L) CHECK(i0 % 128 == 0);
            sqy::WindowClip c = sqy::window_clip_start(g, i0, n);
            sqy::WindowPiece p;
            while (sqy::window_clip_next(g, &c, &p)) {
                CHECK(p.len >= 1 && p.run_off + p.len <= n);
                for (uint64_t k = 0; k < p.len; ++k) {
                    const uint64_t i = i0 + p.run_off + k, z = i / (bY * bX), y = i / bX % bY, x = i % bX;
                    CHECK(z >= oz && z < oz + Z && y >= oy && y < oy + Y && x >= ox && x < ox + X);
                    CHECK(p.dst_off + k == (z - oz) * g.sz + (y - oy) * g.sy + (x - ox));
                    CHECK(written[(size_t)(p.dst_off + k)]++ == 0);
                    ++count;
                }
            }
            i0 += n;
        }
        CHECK(count == Z * Y * X);
    }
    return 0;
}

int test_long_rows()
{
    for (int elem : {2, 1}) {
        CHECK(clip_long_rows(2, 3, 130, elem) == 0);         // 780 voxels: six runs and a short one of 12 (16 bit: tail of 12 / 8 bit: of 4)
        CHECK(clip_long_rows(1, 2, 300, elem) == 0);         // 600 voxels: four runs and a short one of 80 (88), a tail of 8 (0)
    }
    // the 64-bit divisions: a row longer than 2^32 voxels
    const sqy::WindowGeometry big{3, (uint64_t)5 << 32, 1, 1, 7, 1, 1, (uint64_t)1 << 33, (uint64_t)1 << 40, (uint64_t)1 << 34};
    sqy::WindowClip c = sqy::window_clip_start(big, 4 * big.bX + 3, 128);          // z = 1, y = 1, x = 3
    CHECK(c.z == 1 && c.y == 1 && c.x == 3);
    sqy::WindowPiece p;
    CHECK(sqy::window_clip_next(big, &c, &p) && p.run_off == 4 && p.dst_off == 0 && p.len == 124 && !sqy::window_clip_next(big, &c, &p));
    return 0;
}

int test_layout()
{
    static_assert(sizeof(sqy::BatchWindowJob) == sqy::kBatchWindowJobBytes, "the window job's layout");
    for (uint64_t n : {(uint64_t)1, (uint64_t)2, (uint64_t)3, (uint64_t)7, (uint64_t)256, (uint64_t)100001}) {
        const sqy::BatchWindowLayout l = sqy::batch_window_layout(n);
        CHECK(l.tiles_at >= n * sizeof(sqy::BatchWindowJob) && l.tiles_at < n * sizeof(sqy::BatchWindowJob) + 16 && l.tiles_at % 16 == 0);
        CHECK(l.total == l.tiles_at + (n + 1) * sizeof(uint32_t));
    }
    return 0;
}

} // namespace

int main()
{
    if (test_admit() || test_clip() || test_long_rows() || test_layout()) return 1;
    std::printf("batch_window ok\n");
    return 0;
}
