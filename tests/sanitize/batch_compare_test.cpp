// The window compare on the host (tests/test_host_batch_compare.py builds and runs this with g++, sanitizers on): the accumulate routine
// of csrc/sqy_batch_window.hpp -- window_compare16, compare_piece, compare_voxel, the text the comparing transposer compiles -- driven
// run by run as that kernel drives it: runs of 128 voxels of the blob's dense order, the short last run of the planes, pieces of
// sixteen bytes in ascending order, the tail voxel by voxel.  The per-run sums, added up as a workgroup adds them, must equal a triple
// loop over the window for EVERY window of small blobs and for windows of (2,3,300), whose rows cross the runs; both voxel sizes, dense
// and pitched views, view bases on and one voxel behind the 16-byte grid.  The view buffer is exactly as long as the view reaches, so a
// load that strays is the sanitizer's.  Prints the runs outside, inside and partly inside, then "batch_compare ok", and returns 0.
#include "../../sqeazy_amd/csrc/sqy_batch_window.hpp"
#include "../../sqeazy_amd/csrc/sqy_kernels.h"
#include "../../sqeazy_amd/csrc/sqy_pipeline.hpp"

#include <cstdio>
#include <cstring>
#include <vector>

#define CHECK(cond)                                                                   \
    do {                                                                              \
        if (!(cond)) { std::fprintf(stderr, "line %d: %s\n", __LINE__, #cond); return 1; } \
    } while (0)

namespace {

unsigned long long g_outside = 0, g_inside = 0, g_partly = 0;

// the eight fields of a record, in the header's order
struct Totals {
    unsigned long long f[8] = {0, 0, 0, 0, 0, 0, ~0ull, 0};
    void add(const sqy::CompareSums& s)                                // (what a workgroup's reduction and its atomics do)
    {
        if (!s.n) return;
        f[0] += s.n; f[1] += s.ndiff; f[2] += s.sum_abs; f[3] += s.sum_sq; f[5] += s.view_sum;
        if (s.max_abs > f[4]) f[4] = s.max_abs;
        if (s.view_min < f[6]) f[6] = s.view_min;
        if (s.view_max > f[7]) f[7] = s.view_max;
    }
    void voxel(unsigned long long a, unsigned long long b)             // the triple loop's side: plain 64-bit arithmetic
    {
        const unsigned long long d = a > b ? a - b : b - a;
        ++f[0]; f[1] += d != 0; f[2] += d; f[3] += d * d; f[5] += b;
        if (d > f[4]) f[4] = d;
        if (b < f[6]) f[6] = b;
        if (b > f[7]) f[7] = b;
    }
};

uint32_t mix(uint64_t x) { x *= 0x9E3779B97F4A7C15ull; x ^= x >> 29; x *= 0xBF58476D1CE4E5B9ull; return (uint32_t)(x >> 32); }

// mode 0: the view is the window with every third voxel changed; 1: blob all zeros, view all ones (the largest difference everywhere)
template <class T>
int compare_window(const std::vector<T>& blob, uint64_t bY, uint64_t bX, const sqy::WindowGeometry& g, unsigned shift, int mode)
{
    constexpr int ELEM = (int)sizeof(T);
    constexpr uint32_t W = 8 * ELEM, G = 16 / ELEM;
    const uint64_t len = blob.size(), L = len / W * W;
    // the view: exactly as long as its last voxel reaches, pattern bytes in the gaps
    const uint64_t reach = (g.Z - 1) * g.sz + (g.Y - 1) * g.sy + g.X;
    std::vector<uint8_t> buf((size_t)(shift * ELEM + reach * ELEM));
    for (size_t i = 0; i < buf.size(); ++i) buf[i] = (uint8_t)(0xA5u ^ mix(i));
    uint8_t* view = buf.data() + shift * ELEM;
    Totals want;
    for (uint64_t z = 0; z < g.Z; ++z) for (uint64_t y = 0; y < g.Y; ++y) for (uint64_t x = 0; x < g.X; ++x) {
        const uint64_t i = ((g.oz + z) * bY + g.oy + y) * bX + g.ox + x, off = z * g.sz + y * g.sy + x;
        const T a = blob[(size_t)i];
        T b = a;
        if (mode == 1) b = (T)~(T)0;
        else if (mix(i + 77) % 3 == 0) b = (T)mix(i * 31 + off);
        std::memcpy(view + off * ELEM, &b, ELEM);
        want.voxel(a, b);
    }
    const uint8_t* dense = reinterpret_cast<const uint8_t*>(blob.data());
    Totals got;
    for (uint64_t i0 = 0; i0 < L; i0 += 128) {                         // a thread's run: its plane words' voxels
        const uint32_t n = (uint32_t)(L - i0 < 128 ? L - i0 : 128);
        sqy::CompareSums s = sqy::compare_sums_neutral();
        sqy::WindowClip c = sqy::window_clip_start(g, i0, n);
        sqy::WindowPiece cur;
        bool have = sqy::window_clip_next(g, &c, &cur);
        if (!have) { ++g_outside; continue; }
        for (uint32_t p = 0; p < n && have; p += G) {                  // pieces of sixteen decoded bytes (8 bit: a last odd word is eight)
            const uint32_t pn = n - p < G ? n - p : G;
            uint32_t a[4] = {0, 0, 0, 0};
            std::memcpy(a, dense + (i0 + p) * ELEM, (size_t)pn * ELEM);
            sqy::window_compare16<ELEM>(view, g, c, cur, have, a, p, pn, &s);
        }
        CHECK(s.n >= 1 && s.n <= n);
        ++(s.n == n ? g_inside : g_partly);
        got.add(s);
    }
    for (uint64_t i = L; i < len; ++i) {                               // the tail, voxel by voxel
        sqy::CompareSums s = sqy::compare_sums_neutral();
        sqy::WindowClip c = sqy::window_clip_start(g, i, 1);
        sqy::WindowPiece cur;
        if (sqy::window_clip_next(g, &c, &cur)) sqy::compare_voxel(&s, sqy::window_voxel_load<ELEM>(dense, i), sqy::window_voxel_load<ELEM>(view, cur.dst_off));
        got.add(s);
    }
    for (int k = 0; k < 8; ++k)
        if (got.f[k] != want.f[k]) {
            std::fprintf(stderr, "field %d: %llu, expected %llu (window %llu %llu %llu + %llu %llu %llu, elem %d, shift %u, mode %d)\n", k, got.f[k], want.f[k],
                         (unsigned long long)g.oz, (unsigned long long)g.oy, (unsigned long long)g.ox, (unsigned long long)g.Z, (unsigned long long)g.Y, (unsigned long long)g.X,
                         ELEM, shift, mode);
            return 1;
        }
    CHECK(want.f[0] == g.Z * g.Y * g.X);
    return 0;
}

template <class T>
std::vector<T> make_blob(uint64_t len, int mode)
{
    std::vector<T> blob((size_t)len);
    for (uint64_t i = 0; i < len; ++i) blob[(size_t)i] = mode == 1 ? (T)0 : (T)mix(i + 5 * len);
    return blob;
}

sqy::WindowGeometry geometry(uint64_t bY, uint64_t bX, uint64_t oz, uint64_t oy, uint64_t ox, uint64_t Z, uint64_t Y, uint64_t X, bool pitch)
{
    return pitch ? sqy::WindowGeometry{bY, bX, oz, oy, ox, Z, Y, X, Y * (X + 3) + 5, X + 3} : sqy::WindowGeometry{bY, bX, oz, oy, ox, Z, Y, X, Y * X, X};
}

// every window of a small blob
template <class T>
int every_window(uint64_t bZ, uint64_t bY, uint64_t bX)
{
    const std::vector<T> blob = make_blob<T>(bZ * bY * bX, 0);
    for (uint64_t oz = 0; oz < bZ; ++oz) for (uint64_t Z = 1; oz + Z <= bZ; ++Z)
    for (uint64_t oy = 0; oy < bY; ++oy) for (uint64_t Y = 1; oy + Y <= bY; ++Y)
    for (uint64_t ox = 0; ox < bX; ++ox) for (uint64_t X = 1; ox + X <= bX; ++X)
        for (int pitch = 0; pitch < 2; ++pitch)
            for (unsigned shift = 0; shift < 2; ++shift)
                if (compare_window(blob, bY, bX, geometry(bY, bX, oz, oy, ox, Z, Y, X, pitch != 0), shift, 0)) return 1;
    return 0;
}

// (2,3,300): rows that cross the 128-voxel runs; every window along z and y, a sample along x
template <class T>
int long_rows()
{
    const uint64_t bZ = 2, bY = 3, bX = 300;
    for (int mode = 0; mode < 2; ++mode) {
        const std::vector<T> blob = make_blob<T>(bZ * bY * bX, mode);
        for (uint64_t oz = 0; oz < bZ; ++oz) for (uint64_t Z = 1; oz + Z <= bZ; ++Z)
        for (uint64_t oy = 0; oy < bY; ++oy) for (uint64_t Y = 1; oy + Y <= bY; ++Y)
        for (uint64_t ox : {(uint64_t)0, (uint64_t)1, (uint64_t)7, (uint64_t)8, (uint64_t)15, (uint64_t)16, (uint64_t)127, (uint64_t)128, bX - 2, bX - 1})
        for (uint64_t X : {(uint64_t)1, (uint64_t)2, (uint64_t)16, (uint64_t)113, (uint64_t)128, (uint64_t)129, bX - ox}) {
            if (ox + X > bX) continue;
            for (int pitch = 0; pitch < 2; ++pitch)
                for (unsigned shift = 0; shift < 2; ++shift)
                    if (compare_window(blob, bY, bX, geometry(bY, bX, oz, oy, ox, Z, Y, X, pitch != 0), shift, mode)) return 1;
        }
    }
    return 0;
}

// zeros against the largest value everywhere: 128 voxels x 65535^2 is above 2^32 in ONE run, the whole blob far above it
int all_maximal()
{
    const uint64_t bZ = 2, bY = 128, bX = 128;
    const std::vector<uint16_t> blob = make_blob<uint16_t>(bZ * bY * bX, 1);
    const sqy::WindowGeometry g = geometry(bY, bX, 0, 0, 0, bZ, bY, bX, false);
    if (compare_window(blob, bY, bX, g, 0, 1)) return 1;
    sqy::CompareSums s = sqy::compare_sums_neutral();
    for (int k = 0; k < 128; ++k) sqy::compare_voxel(&s, 0, 65535);
    CHECK(s.sum_sq == 128ull * 65535ull * 65535ull && s.sum_sq > 0xffffffffull && s.sum_abs == 128u * 65535u && s.max_abs == 65535u && s.ndiff == 128u);
    CHECK(s.view_sum == 128u * 65535u && s.view_min == 65535u && s.view_max == 65535u);
    return 0;
}

int test_layout()
{
    static_assert(sizeof(sqy::BatchCompareJob) == sqy::kBatchCompareJobBytes, "the compare job's layout");
    static_assert(sizeof(sqy::WindowBytes16) == 16 && alignof(sqy::WindowBytes16) == 16, "sixteen bytes on the grid");
    for (uint64_t n : {(uint64_t)1, (uint64_t)3, (uint64_t)256, (uint64_t)100001}) {
        const sqy::BatchWindowLayout l = sqy::batch_window_layout(n, sizeof(sqy::BatchCompareJob));
        CHECK(l.tiles_at == n * sizeof(sqy::BatchCompareJob) && l.total == l.tiles_at + (n + 1) * sizeof(uint32_t));
        const sqy::BatchWindowLayout w = sqy::batch_window_layout(n);
        CHECK(w.tiles_at >= n * sizeof(sqy::BatchWindowJob) && w.tiles_at < n * sizeof(sqy::BatchWindowJob) + 16);
    }
    return 0;
}

} // namespace

int main()
{
    if (every_window<uint16_t>(3, 5, 7) || every_window<uint8_t>(3, 5, 7) || every_window<uint16_t>(2, 3, 9) || every_window<uint8_t>(2, 3, 9)) return 1;
    if (long_rows<uint16_t>() || long_rows<uint8_t>() || all_maximal() || test_layout()) return 1;
    std::printf("runs outside %llu inside %llu partly %llu\n", g_outside, g_inside, g_partly);
    std::printf("batch_compare ok\n");
    return 0;
}
