// The compare of boxes of one large blob on the host (tests/test_host_compare_boxes.py builds and runs this with g++, sanitizers on):
// sqy::compare_boxes_path against its table, the comparing job's layout, and the comparing range transposer of SQYAMD_Compare_Boxes_* run by
// run as bitswap1_decode_range_windows_compare_kernel drives it -- sqy::range_run's threads over the ABSOLUTE plane words of a range, the
// clip of csrc/sqy_batch_window.hpp on each thread's run, every plane word read at Bitswap1Range's address in a buffer of exactly the bytes
// sqy::frame_range_plan says the pruned LZ4 decode leaves, the voxels handed to window_compare16 in the kernel's pieces (two of eight
// voxels a 16-bit word, one of sixteen for two 8-bit words, one of eight looked-up voxels behind the quantiser's table), the tail through
// compare_voxel.  The per-thread sums, added up as a workgroup adds them, must equal a triple loop over the box for every z-range of
// 7 x 33 x 31 and 2 x 3 x 300 and a table of boxes in each; both element sizes and the LUT form, dense and pitched views, view bases on and
// one voxel behind the 16-byte grid.  The view buffer is exactly as long as the view reaches, so a load that strays is the sanitizer's.
// Prints the runs outside, inside and partly inside a box and the first and last threads of a range, then "compare_boxes ok"; returns 0.
#include "../../sqeazy_amd/csrc/sqy_batch_window.hpp"
#include "../../sqeazy_amd/csrc/sqy_kernels.h"
#include "../../sqeazy_amd/csrc/sqy_pipeline.hpp"

#include <algorithm>
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

unsigned long long g_outside = 0, g_inside = 0, g_partly = 0, g_first = 0, g_last = 0;

int test_path()
{
    const struct { RangeForm form; BoxPath on; } table[] = {{RangeForm::plain, BoxPath::subset_copy}, {RangeForm::planes, BoxPath::subset_transposer},
                                                            {RangeForm::planes_lut, BoxPath::subset_transposer}, {RangeForm::shuffle, BoxPath::subset_copy}};
    for (const auto& row : table) {
        CHECK(sqy::compare_boxes_path(true, row.form, true) == row.on);
        CHECK(sqy::compare_boxes_path(true, row.form, false) == BoxPath::whole_copy);       // the option off
        CHECK(sqy::compare_boxes_path(false, row.form, true) == BoxPath::whole_copy);       // a blob the frame-range plan does not take
        CHECK(sqy::compare_boxes_path(false, row.form, false) == BoxPath::whole_copy);
    }
    return 0;
}

int test_layout()
{
    static_assert(sizeof(sqy::Bitswap1BoxCompareJob) == sqy::kBitswap1BoxCompareJobBytes && sizeof(sqy::Bitswap1BoxCompareJob) % 16 == 0, "the comparing box job's layout");
    static_assert(offsetof(sqy::Bitswap1BoxCompareJob, g) == offsetof(sqy::Bitswap1BoxJob, g) && offsetof(sqy::Bitswap1BoxCompareJob, r) == offsetof(sqy::Bitswap1BoxJob, r) &&
                      offsetof(sqy::Bitswap1BoxCompareJob, t0) == offsetof(sqy::Bitswap1BoxJob, t0) && offsetof(sqy::Bitswap1BoxCompareJob, record) == sizeof(sqy::Bitswap1BoxJob),
                  "Bitswap1BoxJob's fields, the record behind them");
    for (uint64_t n : {(uint64_t)1, (uint64_t)3, (uint64_t)64, (uint64_t)100001}) {
        const sqy::BatchWindowLayout l = sqy::batch_window_layout(n, sizeof(sqy::Bitswap1BoxCompareJob));
        CHECK(l.tiles_at == n * sizeof(sqy::Bitswap1BoxCompareJob) && l.tiles_at % 16 == 0 && l.total == l.tiles_at + (n + 1) * sizeof(uint32_t));
    }
    return 0;
}

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

// bitswap1's stream of n voxels of `we` bytes: W = 8 we plane segments of n / W words (plane W - 1 - b, word w, bit W - 1 - k = bit b of
// voxel W w + k), then the n % W voxels behind them verbatim
std::vector<uint8_t> plane_stream(const std::vector<uint32_t>& vox, uint32_t we)
{
    const uint64_t n = vox.size(), W = 8 * we, seg = n / W;
    std::vector<uint8_t> s(n * we, 0);
    for (uint64_t w = 0; w < seg; ++w)
        for (uint64_t b = 0; b < W; ++b) {
            uint32_t word = 0;
            for (uint64_t k = 0; k < W; ++k) word |= ((vox[W * w + k] >> b) & 1u) << (W - 1 - k);
            for (uint32_t i = 0; i < we; ++i) s[((W - 1 - b) * seg + w) * we + i] = (uint8_t)(word >> (8 * i));
        }
    for (uint64_t v = seg * W; v < n; ++v)
        for (uint32_t i = 0; i < we; ++i) s[v * we + i] = (uint8_t)(vox[v] >> (8 * i));
    return s;
}

// One box of the range p (whose decoded LZ4 frames are `in`): the sums the comparing transposer's threads gather against a view of the
// decoded box with every third voxel changed, held to the triple loop's.  WE: bytes of a stored voxel; LUT: 16-bit voxels out of `lut`
template <int WE, bool LUT>
int compare_box(const sqy::FrameRangePlan& p, const std::vector<uint8_t>& in, const std::vector<uint32_t>& volume, const uint16_t* lut, const sqy::WindowGeometry& g,
                unsigned shift)
{
    constexpr int OUT = LUT ? 2 : WE;                                  // bytes of a voxel in the view
    constexpr uint32_t W = 8 * WE, wpt = 128 / W;
    const uint64_t reach = (g.Z - 1) * g.sz + (g.Y - 1) * g.sy + g.X;
    std::vector<uint8_t> buf((size_t)((shift + reach) * OUT));       // the view: exactly as long as its last voxel reaches, pattern bytes in the gaps
    for (size_t i = 0; i < buf.size(); ++i) buf[i] = (uint8_t)(0xA5u ^ mix(i));
    uint8_t* view = buf.data() + shift * OUT;
    Totals want;
    for (uint64_t z = 0; z < g.Z; ++z) for (uint64_t y = 0; y < g.Y; ++y) for (uint64_t x = 0; x < g.X; ++x) {
        const uint64_t i = ((g.oz + z) * g.bY + g.oy + y) * g.bX + g.ox + x, off = z * g.sz + y * g.sy + x;
        const uint32_t a = volume[(size_t)i];
        uint32_t b = a;
        if (mix(i + 77) % 3 == 0) b = mix(i * 31 + off) & (OUT == 2 ? 0xffffu : 0xffu);
        std::memcpy(view + off * OUT, &b, OUT);                         // (little endian)
        want.voxel(a, b);
    }
    // voxel k of plane word w of the range, out of the planes at Bitswap1Range's addresses
    auto stored = [&](uint64_t w, uint32_t k) {
        uint32_t v = 0;
        for (uint32_t b = 0; b < W; ++b) {
            uint32_t word = 0;
            for (int j = 0; j < WE; ++j) word |= (uint32_t)in.at((size_t)(p.plane[W - 1 - b] + (w - p.w0) * WE + j)) << (8 * j);
            v |= ((word >> (W - 1 - k)) & 1u) << b;
        }
        return v;
    };
    Totals got;
    sqy::WindowPiece cur;
    // workgroup 0's tail voxels
    const uint64_t tail0 = p.v0 > p.L ? p.v0 : p.L;
    for (uint64_t t = 0; tail0 + t < p.v1; ++t) {
        CHECK(t < 256);
        sqy::CompareSums s = sqy::compare_sums_neutral();
        sqy::WindowClip ct = sqy::window_clip_start(g, tail0 + t, 1);
        if (sqy::window_clip_next(g, &ct, &cur)) {
            const uint32_t x = sqy::window_voxel_load<WE>(in.data() + p.tail, t);
            CHECK(p.tail + (t + 1) * WE <= in.size());
            sqy::compare_voxel(&s, LUT ? (uint32_t)lut[x & 0xffu] : x, sqy::window_voxel_load<OUT>(view, cur.dst_off));
        }
        got.add(s);
    }
    // the grid's threads; the ones in front of and behind the range own no word and bring the neutral element
    const uint64_t t0 = sqy::range_first_thread(p.w0, wpt), nt = sqy::range_thread_count(p.w0, p.w1, wpt);
    for (uint64_t t = t0 ? t0 - 1 : 0; t < t0 + nt + 1; ++t) {
        const sqy::RangeRun run = sqy::range_run(t, wpt, p.w0, p.w1);
        const bool owns = run.lo != run.hi;
        CHECK(owns == (t >= t0 && t < t0 + nt));
        sqy::CompareSums s = sqy::compare_sums_neutral();
        sqy::WindowClip c = sqy::window_clip_start(g, owns ? run.first * W : 0, owns ? (uint64_t)run.hi * W : 0);
        bool have = owns && sqy::window_clip_next(g, &c, &cur);
        if (owns) {
            if (run.lo > 0) ++g_first;
            if (run.hi < wpt) ++g_last;
        }
        if (!have) { if (owns) ++g_outside; got.add(s); continue; }
        // the words the thread owns, transposed: voxel k of word i of its run (the words in front of run.lo are never read: zeros)
        uint32_t vox[128] = {};
        for (uint32_t i = run.lo; i < run.hi; ++i)
            for (uint32_t k = 0; k < W; ++k) vox[i * W + k] = stored(run.first + i, k);
        auto piece = [&](uint32_t first, uint32_t n, uint32_t a[4]) {  // n voxels from `first` of the run, packed as in a dense copy
            a[0] = a[1] = a[2] = a[3] = 0;
            for (uint32_t k = 0; k < n; ++k) {
                const uint32_t v = LUT ? (uint32_t)lut[vox[first + k] & 0xffu] : vox[first + k];
                a[k * OUT / 4] |= v << (8u * ((k * OUT) & 3u));
            }
        };
        uint32_t a[4];
        if (WE == 2) {
            for (uint32_t q = 0; q < 4 && 2 * q < run.hi && have; ++q) {   // word first + 2 q, then first + 2 q + 1: two pieces of eight each
                piece(32 * q, 8, a); sqy::window_compare16<2>(view, g, c, cur, have, a, 32u * q, 8, &s);
                piece(32 * q + 8, 8, a); sqy::window_compare16<2>(view, g, c, cur, have, a, 32u * q + 8u, 8, &s);
                if (2 * q + 1 >= run.hi) break;
                piece(32 * q + 16, 8, a); sqy::window_compare16<2>(view, g, c, cur, have, a, 32u * q + 16u, 8, &s);
                piece(32 * q + 24, 8, a); sqy::window_compare16<2>(view, g, c, cur, have, a, 32u * q + 24u, 8, &s);
            }
        } else {
            for (uint32_t gq = 0; gq < 16 && gq < run.hi && have; gq += 2) {
                if (LUT) {
                    for (uint32_t u = 0; u < 2 && gq + u < run.hi; ++u) {  // a word's eight looked-up voxels: one piece
                        piece(8 * (gq + u), 8, a);
                        sqy::window_compare16<2>(view, g, c, cur, have, a, 8u * (gq + u), 8, &s);
                    }
                } else {
                    const uint32_t n = run.hi - gq >= 2u ? 16u : 8u;
                    piece(8 * gq, n, a);
                    sqy::window_compare16<1>(view, g, c, cur, have, a, 8u * gq, n, &s);
                }
            }
        }
        CHECK(s.n >= 1 && s.n <= (run.hi - run.lo) * W);
        ++(s.n == (run.hi - run.lo) * W ? g_inside : g_partly);
        got.add(s);
    }
    for (int k = 0; k < 8; ++k)
        if (got.f[k] != want.f[k]) {
            std::fprintf(stderr, "field %d: %llu, expected %llu (box %llu %llu %llu + %llu %llu %llu, stored %d bytes, lut %d, shift %u)\n", k, got.f[k], want.f[k],
                         (unsigned long long)g.oz, (unsigned long long)g.oy, (unsigned long long)g.ox, (unsigned long long)g.Z, (unsigned long long)g.Y, (unsigned long long)g.X,
                         WE, (int)LUT, shift);
            return 1;
        }
    CHECK(want.f[0] == g.Z * g.Y * g.X);
    return 0;
}

// every z-range of a blob of (bZ, bY, bX) voxels with a table of boxes in it, the stream cut into chunks of `chunk` bytes
template <int WE, bool LUT>
int box_blob(uint64_t bZ, uint64_t bY, uint64_t bX, uint64_t chunk)
{
    const RangeForm form = LUT ? RangeForm::planes_lut : RangeForm::planes;
    const int elem = LUT ? 2 : WE;
    const uint64_t n = bZ * bY * bX;
    uint16_t lut[256];
    for (uint32_t i = 0; i < 256; ++i) lut[i] = (uint16_t)mix(1000 + i);
    std::vector<uint32_t> stored(n), volume(n);                        // what the planes hold; what the decode gives
    for (uint64_t i = 0; i < n; ++i) {
        stored[i] = mix(i + 5 * n) & (WE == 2 ? 0xffffu : 0xffu);
        volume[i] = LUT ? (uint32_t)lut[stored[i]] : stored[i];
    }
    const std::vector<uint8_t> stream = plane_stream(stored, WE);
    const uint64_t total = stream.size();
    const uint32_t nframes = (uint32_t)((total + chunk - 1) / chunk);
    for (uint64_t oz = 0; oz < bZ; ++oz) for (uint64_t Z = 1; oz + Z <= bZ; ++Z) {
        const sqy::FrameRangePlan p = sqy::frame_range_plan(form, n, elem, bZ, oz, Z, chunk, total, nframes);
        CHECK(p.ok && p.we == WE && p.v0 == oz * bY * bX && p.v1 == (oz + Z) * bY * bX);
        std::vector<uint8_t> in;                                       // what the pruned LZ4 decode leaves: the chunks of p.ids back to back
        for (uint32_t f : p.ids) in.insert(in.end(), stream.begin() + (size_t)(f * chunk), stream.begin() + (size_t)std::min<uint64_t>((f + 1) * chunk, total));
        CHECK(in.size() == p.out_bytes);
        for (uint64_t oy : {(uint64_t)0, (uint64_t)1}) for (uint64_t Y : {(uint64_t)1, bY - oy})
        for (uint64_t ox : {(uint64_t)0, (uint64_t)3, bX - 1}) for (uint64_t X : {(uint64_t)1, (uint64_t)5, (uint64_t)129, bX - ox}) {
            if (oy >= bY || ox + X > bX) continue;
            for (int v = 0; v < 2; ++v) {                               // dense on the grid; pitched, one voxel behind it
                const sqy::WindowGeometry g = v ? sqy::WindowGeometry{bY, bX, oz, oy, ox, Z, Y, X, Y * (X + 3) + 5, X + 3} : sqy::WindowGeometry{bY, bX, oz, oy, ox, Z, Y, X, Y * X, X};
                if (compare_box<WE, LUT>(p, in, volume, lut, g, (unsigned)v)) return 1;
            }
        }
    }
    return 0;
}

} // namespace

int main()
{
    if (test_path() || test_layout()) return 1;
    if (box_blob<2, false>(7, 33, 31, 1024) || box_blob<1, false>(7, 33, 31, 1024) || box_blob<1, true>(7, 33, 31, 1024)) return 1;
    if (box_blob<2, false>(2, 3, 300, 256) || box_blob<1, false>(2, 3, 300, 256) || box_blob<1, true>(2, 3, 300, 256)) return 1;
    std::printf("runs outside %llu inside %llu partly %llu first %llu last %llu\n", g_outside, g_inside, g_partly, g_first, g_last);
    std::printf("compare_boxes ok\n");
    return 0;
}
