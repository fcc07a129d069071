// The intensity histograms of boxes of one large blob, on the host (tests/test_host_histogram_boxes.py builds and runs this with g++,
// sanitizers on): sqy::histogram_boxes_path against its table, sqy::admit_histogram at every refusal -- the shift at 0, 15 | 16 and
// 7 | 8, origins near 2^63 --, and the counting walk of SQYAMD_Histogram_Boxes_*'s range transposer workgroup by workgroup as
// bitswap1_decode_range_windows_histogram_kernel drives it: the job's threads in groups of 256, each group with an array of exactly
// sqy::hist_window_bins(nbins) counters standing in for its LDS (a count that strays is the sanitizer's), the vote of the threads' first
// voxels inside the box, the clip of csrc/sqy_batch_window.hpp on each thread's run, sqy::window_histogram16 with each of the three merges
// of equal neighbours, the flush of the non-zero counters; bins outside the window and the tail voxels go straight to the output.
// Afterwards the output must equal a triple loop's counts.  Blobs 7 x 33 x 31 and 2 x 3 x 300 with every z-range and a table of boxes,
// and 3 x 128 x 130 (two workgroups to a frame range) with a few; 16-bit, 8-bit and looked-up voxels; values crowded into each quarter
// of the range in turn, so that each of the four windows wins, with 0, 16383 | 16384, 32767 | 32768, 49151 | 49152 and 65535 planted.
// Prints the runs outside, inside and partly inside a box, the workgroups each window won, the adds that missed the window and the adds
// of more than one voxel and of eight or more, then "histogram_boxes ok"; returns 0.
#include "../../sqeazy_amd/csrc/sqy_batch_window.hpp"
#include "../../sqeazy_amd/csrc/sqy_kernels.h"
#include "../../sqeazy_amd/csrc/sqy_pipeline.hpp"

#include <algorithm>
#include <climits>
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

unsigned long long g_outside = 0, g_inside = 0, g_partly = 0, g_window[4] = {0, 0, 0, 0}, g_offwindow = 0, g_merged = 0, g_pieces = 0, g_groups2 = 0;

int test_path()
{
    const struct { RangeForm form; BoxPath on; } table[] = {{RangeForm::plain, BoxPath::subset_copy}, {RangeForm::planes, BoxPath::subset_transposer},
                                                            {RangeForm::planes_lut, BoxPath::subset_transposer}, {RangeForm::shuffle, BoxPath::subset_copy}};
    for (const auto& row : table) {
        CHECK(sqy::histogram_boxes_path(true, row.form, true) == row.on);
        CHECK(sqy::histogram_boxes_path(true, row.form, false) == BoxPath::whole_copy);     // the option off
        CHECK(sqy::histogram_boxes_path(false, row.form, true) == BoxPath::whole_copy);     // a blob the frame-range plan does not take
        CHECK(sqy::histogram_boxes_path(false, row.form, false) == BoxPath::whole_copy);
    }
    return 0;
}

int test_bins()
{
    CHECK(sqy::histogram_bins(2, 0) == 65536 && sqy::histogram_bins(2, 1) == 32768 && sqy::histogram_bins(2, 15) == 2 && sqy::histogram_bins(2, 16) == 0);
    CHECK(sqy::histogram_bins(1, 0) == 256 && sqy::histogram_bins(1, 7) == 2 && sqy::histogram_bins(1, 8) == 0 && sqy::histogram_bins(2, -1) == 0);
    CHECK(sqy::histogram_bins(0, 0) == 0 && sqy::histogram_bins(3, 0) == 0 && sqy::histogram_bins(4, 0) == 0);
    CHECK(sqy::hist_window_bins(65536) == 16384 && sqy::hist_windows(65536) == 4 && sqy::hist_window_bins(32768) == 16384 && sqy::hist_windows(32768) == 2);
    CHECK(sqy::hist_window_bins(16384) == 16384 && sqy::hist_windows(16384) == 1 && sqy::hist_window_bins(2) == 2 && sqy::hist_windows(2) == 1);
    static_assert(sqy::kHistWindowBins * 4u == 64u * 1024u, "the window: 64 KiB, two workgroups to a CU's 160 KiB of LDS");
    // the vote: the first of the windows with the most votes, among the windows there are
    const uint32_t a[4] = {1, 5, 5, 2}, b[4] = {0, 0, 0, 9}, c[4] = {0, 0, 0, 0};
    CHECK(sqy::hist_best_window(a, 4) == 1 && sqy::hist_best_window(a, 2) == 1 && sqy::hist_best_window(b, 4) == 3 && sqy::hist_best_window(b, 2) == 0);
    CHECK(sqy::hist_best_window(c, 4) == 0 && sqy::hist_best_window(a, 1) == 0);
    for (uint32_t v : {0u, 16383u, 16384u, 32767u, 32768u, 49151u, 49152u, 65535u}) {
        CHECK(sqy::hist_vote_window(sqy::hist_bin(v, 0)) == v / 16384u && sqy::hist_vote_window(sqy::hist_bin(v, 1)) == v / 32768u);
        uint32_t slot = 0;
        for (uint32_t k = 0; k < 4; ++k) {
            CHECK(sqy::hist_window_slot(v, k * 16384u, 16384u, &slot) == (v / 16384u == k));
            if (v / 16384u == k) CHECK(slot == v % 16384u);
        }
    }
    return 0;
}

int test_admission()
{
    alignas(16) uint32_t out[8];
    sqy::BatchWindow w;
    const std::vector<uint64_t> shape{3, 5, 7};
    const long o[3] = {1, 2, 3}, e[3] = {2, 3, 4};
    CHECK(sqy::admit_histogram(shape, o, e, 3, 0, 2, out, &w) && w.oz == 1 && w.oy == 2 && w.ox == 3 && w.Z == 2 && w.Y == 3 && w.X == 4 && w.bY == 5 && w.bX == 7);
    // the shift: [0, 16) for 16-bit voxels, [0, 8) for 8-bit ones
    CHECK(sqy::admit_histogram(shape, o, e, 3, 15, 2, out, &w) && !sqy::admit_histogram(shape, o, e, 3, 16, 2, out, &w));
    CHECK(sqy::admit_histogram(shape, o, e, 3, 7, 1, out, &w) && !sqy::admit_histogram(shape, o, e, 3, 8, 1, out, &w) && sqy::admit_histogram(shape, o, e, 3, 8, 2, out, &w));
    CHECK(sqy::admit_histogram(shape, o, e, 3, 0, 1, out, &w) && !sqy::admit_histogram(shape, o, e, 3, -1, 2, out, &w) && !sqy::admit_histogram(shape, o, e, 3, -1, 1, out, &w));
    CHECK(!sqy::admit_histogram(shape, o, e, 3, INT_MAX, 2, out, &w) && !sqy::admit_histogram(shape, o, e, 3, INT_MIN, 2, out, &w));
    CHECK(!sqy::admit_histogram(shape, o, e, 3, 0, 0, out, &w) && !sqy::admit_histogram(shape, o, e, 3, 0, 3, out, &w) && !sqy::admit_histogram(shape, o, e, 3, 0, 4, out, &w));
    // the histogram: not NULL, on the 4-byte grid
    CHECK(!sqy::admit_histogram(shape, o, e, 3, 0, 2, nullptr, &w));
    for (int k = 1; k < 4; ++k) CHECK(!sqy::admit_histogram(shape, o, e, 3, 0, 2, reinterpret_cast<const uint8_t*>(out) + k, &w));
    CHECK(sqy::admit_histogram(shape, o, e, 3, 0, 2, out + 1, &w) && !sqy::admit_histogram(shape, o, e, 3, 0, 2, out, nullptr));
    // the box: what admit_window refuses
    CHECK(!sqy::admit_histogram(shape, o, e, 0, 0, 2, out, &w) && !sqy::admit_histogram(shape, o, e, 4, 0, 2, out, &w) && !sqy::admit_histogram(shape, o, e, 2, 0, 2, out, &w));
    CHECK(!sqy::admit_histogram(shape, o, nullptr, 3, 0, 2, out, &w));
    for (int k = 0; k < 3; ++k) {
        long oo[3] = {1, 2, 3}, ee[3] = {2, 3, 4};
        oo[k] = -1;
        CHECK(!sqy::admit_histogram(shape, oo, e, 3, 0, 2, out, &w));
        oo[k] = o[k]; ee[k] = 0;
        CHECK(!sqy::admit_histogram(shape, o, ee, 3, 0, 2, out, &w));
        ee[k] = -1;
        CHECK(!sqy::admit_histogram(shape, o, ee, 3, 0, 2, out, &w));
        ee[k] = e[k] + 1;                                               // one past the shape
        CHECK(!sqy::admit_histogram(shape, o, ee, 3, 0, 2, out, &w));
        ee[k] = e[k];
        CHECK(sqy::admit_histogram(shape, oo, ee, 3, 0, 2, out, &w));  // the good call between them
        // origins near 2^63: origin + extent wraps `long` -- past the shape, not a small sum
        oo[k] = LONG_MAX; ee[k] = 1;
        CHECK(!sqy::admit_histogram(shape, oo, ee, 3, 0, 2, out, &w));
        oo[k] = LONG_MAX - 1; ee[k] = 2;
        CHECK(!sqy::admit_histogram(shape, oo, ee, 3, 0, 2, out, &w));
        oo[k] = LONG_MAX; ee[k] = LONG_MAX;
        CHECK(!sqy::admit_histogram(shape, oo, ee, 3, 0, 2, out, &w));
        oo[k] = LONG_MIN; ee[k] = 1;
        CHECK(!sqy::admit_histogram(shape, oo, ee, 3, 0, 2, out, &w));
        oo[k] = 1; ee[k] = LONG_MAX;
        CHECK(!sqy::admit_histogram(shape, oo, ee, 3, 0, 2, out, &w));
    }
    // origin nullptr: all zeros; ranks 1 and 2
    CHECK(sqy::admit_histogram(shape, nullptr, e, 3, 0, 2, out, &w) && w.oz == 0 && w.oy == 0 && w.ox == 0);
    const std::vector<uint64_t> line{9000}, sheet{40, 300};
    const long ol[1] = {8999}, el[1] = {1}, el2[1] = {2}, os[2] = {39, 0}, es[2] = {1, 300};
    CHECK(sqy::admit_histogram(line, ol, el, 1, 6, 2, out, &w) && w.X == 1 && w.Y == 1 && w.Z == 1 && !sqy::admit_histogram(line, ol, el2, 1, 6, 2, out, &w));
    CHECK(sqy::admit_histogram(sheet, os, es, 2, 3, 1, out, &w) && w.Z == 1 && w.Y == 1 && w.X == 300 && !sqy::admit_histogram(sheet, os, es, 3, 3, 1, out, &w));
    return 0;
}

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

// the kernels' sink: counters standing in for the workgroup's LDS, the output for what misses the window
struct HostSink {
    std::vector<uint32_t>& lds;
    std::vector<uint32_t>& out;
    uint32_t wbase, wbins;
    unsigned long long total = 0;                                       // voxels counted so far
    void add(uint32_t bin, uint32_t n)
    {
        uint32_t slot;
        total += n;
        if (n > 1) ++g_merged;
        if (n >= 8) ++g_pieces;
        if (sqy::hist_window_slot(bin, wbase, wbins, &slot)) lds.at(slot) += n;
        else { out.at(bin) += n; ++g_offwindow; }
    }
};

// One box of the range p (whose decoded LZ4 frames are `in`): the histogram the counting transposer's workgroups gather, held to the
// triple loop's.  WE: bytes of a stored voxel; LUT: 16-bit voxels out of `lut`
template <int WE, bool LUT, int MERGE>
int histogram_box(const sqy::FrameRangePlan& p, const std::vector<uint8_t>& in, const std::vector<uint32_t>& volume, const uint16_t* lut, const sqy::WindowGeometry& g,
                  uint32_t shift)
{
    constexpr int OUT = LUT ? 2 : WE;                                  // bytes of a counted voxel
    constexpr uint32_t W = 8 * WE, wpt = 128 / W;
    const uint32_t nbins = sqy::histogram_bins(OUT, (int)shift), wbins = sqy::hist_window_bins(nbins), nwin = sqy::hist_windows(nbins);
    CHECK(nbins != 0 && wbins * nwin == nbins);
    std::vector<uint32_t> want(nbins, 0), got(nbins, 0);
    for (uint64_t z = 0; z < g.Z; ++z) for (uint64_t y = 0; y < g.Y; ++y) for (uint64_t x = 0; x < g.X; ++x)
        ++want.at(volume[(size_t)(((g.oz + z) * g.bY + g.oy + y) * g.bX + g.ox + x)] >> shift);
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
    sqy::WindowPiece cur;
    // workgroup 0's tail voxels: straight to the output
    const uint64_t tail0 = p.v0 > p.L ? p.v0 : p.L;
    for (uint64_t t = 0; tail0 + t < p.v1; ++t) {
        CHECK(t < 256);
        sqy::WindowClip ct = sqy::window_clip_start(g, tail0 + t, 1);
        if (sqy::window_clip_next(g, &ct, &cur)) {
            const uint32_t x = sqy::window_voxel_load<WE>(in.data() + p.tail, t);
            CHECK(p.tail + (t + 1) * WE <= in.size());
            ++got.at(sqy::hist_bin(LUT ? (uint32_t)lut[x & 0xffu] : x, shift));
        }
    }
    const uint64_t t0 = sqy::range_first_thread(p.w0, wpt), groups = sqy::range_job_groups(p.w0, p.w1, wpt);
    if (groups > 1) ++g_groups2;
    for (uint64_t own = 0; own < groups; ++own) {
        std::vector<uint32_t> lds(wbins, 0);                            // exactly the window: a stray count is the sanitizer's
        uint32_t votes[4] = {0, 0, 0, 0};
        struct Thread { sqy::RangeRun run; sqy::WindowClip c; sqy::WindowPiece cur; bool have; uint32_t vox[128]; };
        std::vector<Thread> threads(256);
        // in front of the vote's barrier: every thread's clip, its plane words and its first voxel inside the box
        for (uint32_t tid = 0; tid < 256; ++tid) {
            Thread& th = threads[tid];
            th.run = sqy::range_run(t0 + own * 256u + tid, wpt, p.w0, p.w1);
            const bool owns = th.run.lo != th.run.hi;
            th.c = sqy::window_clip_start(g, owns ? th.run.first * W : 0, owns ? (uint64_t)th.run.hi * W : 0);
            th.have = owns && sqy::window_clip_next(g, &th.c, &th.cur);
            std::memset(th.vox, 0, sizeof th.vox);
            if (!th.have) { if (owns) ++g_outside; continue; }     // (no plane word is loaded)
            for (uint32_t i = th.run.lo; i < th.run.hi; ++i)
                for (uint32_t k = 0; k < W; ++k) th.vox[i * W + k] = stored(th.run.first + i, k);
            if (nwin > 1) {
                CHECK(th.cur.run_off < 128 && th.cur.run_off / W >= th.run.lo);
                const uint32_t v = th.vox[th.cur.run_off];
                ++votes[sqy::hist_vote_window(sqy::hist_bin(LUT ? (uint32_t)lut[v & 0xffu] : v, shift))];
            }
        }
        const uint32_t best = nwin > 1 ? sqy::hist_best_window(votes, nwin) : 0u, wbase = best * sqy::kHistWindowBins;
        CHECK(best < nwin);
        bool any = false;
        HostSink sink{lds, got, wbase, wbins};
        for (uint32_t tid = 0; tid < 256; ++tid) {
            Thread& th = threads[tid];
            if (!th.have) continue;
            any = true;
            const sqy::RangeRun& run = th.run;
            sqy::WindowClip& c = th.c;
            sqy::WindowPiece& pc = th.cur;
            bool& have = th.have;
            const unsigned long long before = sink.total;
            auto piece = [&](uint32_t first, uint32_t n, uint32_t a[4]) {  // n voxels from `first` of the run, packed as in a dense copy
                a[0] = a[1] = a[2] = a[3] = 0;
                for (uint32_t k = 0; k < n; ++k) {
                    const uint32_t v = LUT ? (uint32_t)lut[th.vox[first + k] & 0xffu] : th.vox[first + k];
                    a[k * OUT / 4] |= v << (8u * ((k * OUT) & 3u));
                }
            };
            sqy::HistRun hr{0, 0};
            uint32_t a[4];
            if (WE == 2) {
                for (uint32_t q = 0; q < 4 && 2 * q < run.hi && have; ++q) {   // word first + 2 q, then first + 2 q + 1: two pieces of eight each
                    piece(32 * q, 8, a); sqy::window_histogram16<2, MERGE>(sink, g, c, pc, have, a, 32u * q, 8, shift, &hr);
                    piece(32 * q + 8, 8, a); sqy::window_histogram16<2, MERGE>(sink, g, c, pc, have, a, 32u * q + 8u, 8, shift, &hr);
                    if (2 * q + 1 >= run.hi) break;
                    piece(32 * q + 16, 8, a); sqy::window_histogram16<2, MERGE>(sink, g, c, pc, have, a, 32u * q + 16u, 8, shift, &hr);
                    piece(32 * q + 24, 8, a); sqy::window_histogram16<2, MERGE>(sink, g, c, pc, have, a, 32u * q + 24u, 8, shift, &hr);
                }
            } else {
                for (uint32_t gq = 0; gq < 16 && gq < run.hi && have; gq += 2) {
                    if (LUT) {
                        for (uint32_t u = 0; u < 2 && gq + u < run.hi; ++u) {  // a word's eight looked-up voxels: one piece
                            piece(8 * (gq + u), 8, a);
                            sqy::window_histogram16<2, MERGE>(sink, g, c, pc, have, a, 8u * (gq + u), 8, shift, &hr);
                        }
                    } else {
                        const uint32_t n = run.hi - gq >= 2u ? 16u : 8u;
                        piece(8 * gq, n, a);
                        sqy::window_histogram16<1, MERGE>(sink, g, c, pc, have, a, 8u * gq, n, shift, &hr);
                    }
                }
            }
            sqy::hist_flush(sink, &hr);
            CHECK(hr.n == 0);
            const unsigned long long n = sink.total - before;
            CHECK(n >= 1 && n <= (unsigned long long)(run.hi - run.lo) * W);
            ++(n == (unsigned long long)(run.hi - run.lo) * W ? g_inside : g_partly);
        }
        if (any && nwin == 4) ++g_window[best];
        for (uint32_t i = 0; i < wbins; ++i)                            // the flush: the non-zero counters
            if (lds[i]) got.at(wbase + i) += lds[i];
    }
    for (uint32_t b = 0; b < nbins; ++b)
        if (got[b] != want[b]) {
            std::fprintf(stderr, "bin %u: %u, expected %u (box %llu %llu %llu + %llu %llu %llu, stored %d bytes, lut %d, shift %u, merge %d)\n", b, got[b], want[b],
                         (unsigned long long)g.oz, (unsigned long long)g.oy, (unsigned long long)g.ox, (unsigned long long)g.Z, (unsigned long long)g.Y, (unsigned long long)g.X,
                         WE, (int)LUT, shift, (int)MERGE);
            return 1;
        }
    return 0;
}

// the planted values: both sides of every window's border, and the range's ends
const uint32_t kPlanted[8] = {0, 16383, 16384, 32767, 32768, 49151, 49152, 65535};

// z-ranges of a blob of (bZ, bY, bX) voxels with a table of boxes in it, the stream cut into chunks of `chunk` bytes.  Box after box the
// values' quarter, the shift and the merge (none, runs, pieces) change in turn; few: only the whole z-range and two others
template <int WE, bool LUT>
int box_blob(uint64_t bZ, uint64_t bY, uint64_t bX, uint64_t chunk, bool few)
{
    const RangeForm form = LUT ? RangeForm::planes_lut : RangeForm::planes;
    const int elem = LUT ? 2 : WE;
    const uint64_t n = bZ * bY * bX;
    const std::vector<uint32_t> shifts = elem == 2 ? std::vector<uint32_t>{0, 1, 2, 6, 15} : std::vector<uint32_t>{0, 3, 7};
    const uint32_t M = WE == 2 ? 0xffffu : 0xffu;
    // four volumes: values crowded into quarter `mode` of the COUNTED range, one voxel in eight anywhere, runs of equal voxels, the planted ones
    std::vector<std::vector<uint32_t>> volumes(4, std::vector<uint32_t>(n)), stored(4, std::vector<uint32_t>(n));
    std::vector<std::vector<uint16_t>> luts(4, std::vector<uint16_t>(256));
    std::vector<std::vector<uint8_t>> streams(4);
    for (uint32_t mode = 0; mode < 4; ++mode) {
        for (uint32_t i = 0; i < 256; ++i)
            luts[mode][i] = i < 8 ? (uint16_t)kPlanted[i] : (uint16_t)(i % 8 == 7 ? mix(1000 + i) : mode * 16384u + mix(2000 + i) % 16384u);
        for (uint64_t i = 0; i < n; ++i) {
            const uint64_t r = i - i % (mix(i / 64 + mode) % 5 == 4 ? 40 : 1 + mix(i / 64 + mode) % 5);   // (runs of up to four equal voxels, or of 40 and 24)
            uint32_t v;
            if (WE == 2) v = mix(r) % 8 == 0 ? mix(r + 3 * n) & M : mode * 16384u + mix(r + 5 * n) % 16384u;
            else v = mix(r + 5 * n + mode) & M;
            if (i % 97 == 0) v = WE == 2 ? kPlanted[(i / 97) % 8] : (uint32_t)((i / 97) % 8);      // (8-bit: the look-up's first eight codes)
            stored[mode][i] = v;
            volumes[mode][i] = LUT ? (uint32_t)luts[mode][v] : v;
        }
        streams[mode] = plane_stream(stored[mode], WE);
    }
    const uint64_t total = streams[0].size();
    const uint32_t nframes = (uint32_t)((total + chunk - 1) / chunk);
    uint64_t counter = 0;
    for (uint64_t oz = 0; oz < bZ; ++oz) for (uint64_t Z = 1; oz + Z <= bZ; ++Z) {
        if (few && !((oz == 0 && Z == bZ) || (oz == 1 && Z == 1) || (oz == bZ - 1))) continue;
        const sqy::FrameRangePlan p = sqy::frame_range_plan(form, n, elem, bZ, oz, Z, chunk, total, nframes);
        CHECK(p.ok && p.we == WE && p.v0 == oz * bY * bX && p.v1 == (oz + Z) * bY * bX);
        std::vector<std::vector<uint8_t>> ins(4);                       // what the pruned LZ4 decode leaves: the chunks of p.ids back to back
        for (uint32_t mode = 0; mode < 4; ++mode) {
            for (uint32_t f : p.ids)
                ins[mode].insert(ins[mode].end(), streams[mode].begin() + (size_t)(f * chunk), streams[mode].begin() + (size_t)std::min<uint64_t>((f + 1) * chunk, total));
            CHECK(ins[mode].size() == p.out_bytes);
        }
        for (uint64_t oy : {(uint64_t)0, (uint64_t)1}) for (uint64_t Y : {(uint64_t)1, bY - oy})
        for (uint64_t ox : {(uint64_t)0, (uint64_t)3, bX - 1}) for (uint64_t X : {(uint64_t)1, (uint64_t)5, (uint64_t)129, bX - ox}) {
            if (oy >= bY || ox + X > bX) continue;
            if (few && !(Y == bY - oy && (X == bX - ox || X == 5))) continue;
            const sqy::WindowGeometry g{bY, bX, oz, oy, ox, Z, Y, X, Y * X, X};
            const uint32_t mode = (uint32_t)(counter % 4), shift = shifts[(counter / 4) % shifts.size()];
            const int merge = (int)((counter / (4 * shifts.size())) % 3);
            ++counter;
            const int rc = merge == sqy::kHistMergeRuns     ? histogram_box<WE, LUT, sqy::kHistMergeRuns>(p, ins[mode], volumes[mode], luts[mode].data(), g, shift)
                           : merge == sqy::kHistMergePieces ? histogram_box<WE, LUT, sqy::kHistMergePieces>(p, ins[mode], volumes[mode], luts[mode].data(), g, shift)
                                                            : histogram_box<WE, LUT, sqy::kHistMergeNone>(p, ins[mode], volumes[mode], luts[mode].data(), g, shift);
            if (rc) return 1;
        }
    }
    CHECK(counter >= (few ? 4 : 12) * shifts.size());                   // every quarter and shift met, and all three merges but for the few
    return 0;
}

} // namespace

int main()
{
    if (test_path() || test_bins() || test_admission()) return 1;
    if (box_blob<2, false>(7, 33, 31, 1024, false) || box_blob<1, false>(7, 33, 31, 1024, false) || box_blob<1, true>(7, 33, 31, 1024, false)) return 1;
    if (box_blob<2, false>(2, 3, 300, 256, false) || box_blob<1, false>(2, 3, 300, 256, false) || box_blob<1, true>(2, 3, 300, 256, false)) return 1;
    if (box_blob<2, false>(3, 128, 130, 4096, true) || box_blob<1, true>(3, 128, 130, 4096, true)) return 1;
    std::printf("runs outside %llu inside %llu partly %llu window0 %llu window1 %llu window2 %llu window3 %llu offwindow %llu merged %llu pieces %llu groups2 %llu\n", g_outside,
                g_inside, g_partly, g_window[0], g_window[1], g_window[2], g_window[3], g_offwindow, g_merged, g_pieces, g_groups2);
    std::printf("histogram_boxes ok\n");
    return 0;
}
