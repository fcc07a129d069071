// The projection of boxes of one large blob on the host (tests/test_host_project_boxes.py builds and runs this with g++, sanitizers on):
// sqy::project_boxes_path against its table, sqy::admit_projection at its bounds, the projecting jobs' layout, and the projecting range
// transposer of SQYAMD_Project_Boxes_* run by run as bitswap1_decode_range_windows_project_kernel drives it -- sqy::range_run's threads
// over the ABSOLUTE plane words of a range, the clip of csrc/sqy_batch_window.hpp on each thread's run under the geometry admit_projection
// fills, every plane word read at Bitswap1Range's address in a buffer of exactly the bytes sqy::frame_range_plan says the pruned LZ4
// decode leaves, the voxels handed to window_project16 in the kernel's pieces, the tail voxels combined one by one.  The sink is an
// array of exactly the image's reach standing in for the atomics (a combine that strays is the sanitizer's), made ready with the op's
// neutral element as boxes_project_init_kernel walks it; afterwards every element must equal a triple loop's and every gap its pattern.
// All three axes and ops; blobs 3 x 5 x 7, 2 x 3 x 300, 7 x 33 x 31 and 3 x 8 x 32 (Y X % 128 == 0); both element sizes and the LUT
// form; dense and pitched images.  Prints the runs outside, inside and partly inside a box, the first and last threads of a range and
// the axis-2 rows that took more than one combine and the boxes that took the z-walking form as well, then "project_boxes ok"; returns 0.
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

unsigned long long g_outside = 0, g_inside = 0, g_partly = 0, g_first = 0, g_last = 0, g_joined = 0, g_walked = 0;

int test_path()
{
    const struct { RangeForm form; BoxPath on; } table[] = {{RangeForm::plain, BoxPath::subset_copy}, {RangeForm::planes, BoxPath::subset_transposer},
                                                            {RangeForm::planes_lut, BoxPath::subset_transposer}, {RangeForm::shuffle, BoxPath::subset_copy}};
    for (const auto& row : table) {
        CHECK(sqy::project_boxes_path(true, row.form, true) == row.on);
        CHECK(sqy::project_boxes_path(true, row.form, false) == BoxPath::whole_copy);       // the option off
        CHECK(sqy::project_boxes_path(false, row.form, true) == BoxPath::whole_copy);       // a blob the frame-range plan does not take
        CHECK(sqy::project_boxes_path(false, row.form, false) == BoxPath::whole_copy);
    }
    return 0;
}

int test_layout()
{
    static_assert(sizeof(sqy::Bitswap1BoxProjectJob) == sqy::kBitswap1BoxProjectJobBytes && sizeof(sqy::Bitswap1BoxProjectJob) % 16 == 0, "the projecting box job's layout");
    static_assert(offsetof(sqy::Bitswap1BoxProjectJob, g) == offsetof(sqy::Bitswap1BoxJob, g) && offsetof(sqy::Bitswap1BoxProjectJob, r) == offsetof(sqy::Bitswap1BoxJob, r) &&
                      offsetof(sqy::Bitswap1BoxProjectJob, t0) == offsetof(sqy::Bitswap1BoxJob, t0) && offsetof(sqy::Bitswap1BoxProjectJob, op) == sizeof(sqy::Bitswap1BoxJob),
                  "Bitswap1BoxJob's fields, the image's behind them");
    static_assert(sizeof(sqy::BoxProjectJob) == sqy::kBoxProjectJobBytes && sizeof(sqy::BoxProjectJob) % 16 == 0, "the per-element job's layout");
    for (uint64_t n : {(uint64_t)1, (uint64_t)3, (uint64_t)64, (uint64_t)100001}) {
        const sqy::BatchWindowLayout l = sqy::batch_window_layout(n, sizeof(sqy::Bitswap1BoxProjectJob));
        CHECK(l.tiles_at == n * sizeof(sqy::Bitswap1BoxProjectJob) && l.tiles_at % 16 == 0 && l.total == l.tiles_at + (n + 1) * sizeof(uint32_t));
    }
    return 0;
}

int test_admission()
{
    alignas(16) uint32_t image[4];
    sqy::BatchWindow w;
    sqy::Projection q;
    // the sum bound, 16-bit voxels: an extent of 65536 along the axis is taken, 65537 is not; max and min have no bound
    {
        const std::vector<uint64_t> shape{70000, 1, 2};
        const long o[3] = {0, 0, 0}, fits[3] = {65536, 1, 2}, over[3] = {65537, 1, 2};
        CHECK(sqy::admit_projection(shape, o, fits, 3, 0, 2, 65535, image, nullptr, &w, &q) && q.n == 65536 && q.E0 == 1 && q.E1 == 2);
        CHECK(!sqy::admit_projection(shape, o, over, 3, 0, 2, 65535, image, nullptr, &w, &q));
        CHECK(sqy::admit_projection(shape, o, over, 3, 0, 0, 65535, image, nullptr, &w, &q));
        CHECK(sqy::admit_projection(shape, o, over, 3, 0, 1, 65535, image, nullptr, &w, &q));
        CHECK(sqy::admit_projection(shape, o, over, 3, 2, 2, 65535, image, nullptr, &w, &q));         // (the bound is the axis' extent alone)
    }
    // .. 8-bit voxels: 16843009 | 16843010 (255 x 16843009 = 2^32 - 1)
    {
        const std::vector<uint64_t> shape{1, 16843010};
        const long o[2] = {0, 0}, fits[2] = {1, 16843009}, over[2] = {1, 16843010};
        CHECK(sqy::admit_projection(shape, o, fits, 2, 1, 2, 255, image, nullptr, &w, &q) && q.n == 16843009 && q.axis3 == 2);
        CHECK(!sqy::admit_projection(shape, o, over, 2, 1, 2, 255, image, nullptr, &w, &q));
        CHECK(sqy::admit_projection(shape, o, over, 2, 1, 0, 255, image, nullptr, &w, &q));
    }
    const std::vector<uint64_t> shape{4, 5, 6};
    const long o[3] = {1, 1, 1}, e[3] = {2, 3, 4};
    for (int axis = 0; axis < 3; ++axis)
        for (int op = 0; op < 3; ++op) CHECK(sqy::admit_projection(shape, o, e, 3, axis, op, 65535, image, nullptr, &w, &q) && q.axis3 == (uint32_t)axis && q.n == (uint64_t)e[axis]);
    // axis == rank, a negative axis, ops outside 0 .. 2
    CHECK(!sqy::admit_projection(shape, o, e, 3, 3, 0, 65535, image, nullptr, &w, &q));
    CHECK(!sqy::admit_projection(shape, o, e, 3, -1, 0, 65535, image, nullptr, &w, &q));
    CHECK(!sqy::admit_projection(shape, o, e, 3, 0, 3, 65535, image, nullptr, &w, &q));
    CHECK(!sqy::admit_projection(shape, o, e, 3, 0, -1, 65535, image, nullptr, &w, &q));
    {
        const std::vector<uint64_t> s2{5, 6};
        CHECK(sqy::admit_projection(s2, o, e, 2, 1, 0, 65535, image, nullptr, &w, &q) && q.axis3 == 2 && q.E0 == 1 && q.E1 == 2);
        CHECK(!sqy::admit_projection(s2, o, e, 2, 2, 0, 65535, image, nullptr, &w, &q));
        const std::vector<uint64_t> s1{6};
        CHECK(sqy::admit_projection(s1, o, e, 1, 0, 2, 65535, image, nullptr, &w, &q) && q.axis3 == 2 && q.E0 == 1 && q.E1 == 1 && q.n == 2);
        CHECK(!sqy::admit_projection(s1, o, e, 1, 1, 2, 65535, image, nullptr, &w, &q));
    }
    // a NULL image, an image 2 bytes off
    CHECK(!sqy::admit_projection(shape, o, e, 3, 0, 0, 65535, nullptr, nullptr, &w, &q));
    CHECK(!sqy::admit_projection(shape, o, e, 3, 0, 0, 65535, reinterpret_cast<const uint8_t*>(image) + 2, nullptr, &w, &q));
    CHECK(sqy::admit_projection(shape, o, e, 3, 0, 0, 65535, image + 1, nullptr, &w, &q));
    // the stride rules: the image of axis 0 is 3 x 4
    {
        const long good[2] = {7, 1}, tight[2] = {4, 1}, overlap[2] = {3, 1}, inner[2] = {7, 2}, zero[2] = {0, 1};
        CHECK(sqy::admit_projection(shape, o, e, 3, 0, 0, 65535, image, good, &w, &q) && q.p0 == 7 && q.sy == 7 && q.sz == 0);
        CHECK(sqy::admit_projection(shape, o, e, 3, 0, 0, 65535, image, tight, &w, &q) && q.p0 == 4);
        CHECK(!sqy::admit_projection(shape, o, e, 3, 0, 0, 65535, image, overlap, &w, &q));
        CHECK(!sqy::admit_projection(shape, o, e, 3, 0, 0, 65535, image, inner, &w, &q));
        CHECK(!sqy::admit_projection(shape, o, e, 3, 0, 0, 65535, image, zero, &w, &q));
        CHECK(sqy::admit_projection(shape, o, e, 3, 1, 0, 65535, image, good, &w, &q) && q.sz == 7 && q.sy == 0 && q.E0 == 2 && q.E1 == 4);
        CHECK(sqy::admit_projection(shape, o, e, 3, 2, 0, 65535, image, good, &w, &q) && q.sy == 4 && q.sz == 28 && q.E0 == 2 && q.E1 == 3);
    }
    // a box past the shape; origin + extent that overflows `long`
    {
        const long past[3] = {2, 3, 6};
        CHECK(!sqy::admit_projection(shape, o, past, 3, 0, 0, 65535, image, nullptr, &w, &q));
        const long big_o[3] = {LONG_MAX, 1, 1}, big_e[3] = {LONG_MAX, 3, 4};
        CHECK(!sqy::admit_projection(shape, big_o, e, 3, 0, 0, 65535, image, nullptr, &w, &q));
        CHECK(!sqy::admit_projection(shape, o, big_e, 3, 0, 0, 65535, image, nullptr, &w, &q));
        CHECK(!sqy::admit_projection(shape, big_o, big_e, 3, 0, 0, 65535, image, nullptr, &w, &q));
    }
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

// the array that stands in for the atomics: plain combines, counted per element
struct ArraySink {
    uint32_t* out;
    uint32_t* hits;
    uint32_t op;
    void combine(uint64_t off, uint32_t v)
    {
        out[off] = sqy::project_combine(op, out[off], v);
        ++hits[off];
    }
};

constexpr uint32_t kGap = 0xC3C3C3C3u;

// One box of the range p (whose decoded LZ4 frames are `in`) projected along `axis` with `op` into an image of pitch E1 + pad, held to
// the triple loop's.  WE: bytes of a stored voxel; LUT: 16-bit voxels out of `lut`
template <int WE, bool LUT>
int project_box(const sqy::FrameRangePlan& p, const std::vector<uint8_t>& in, const std::vector<uint32_t>& volume, const uint16_t* lut, const std::vector<uint64_t>& shape,
                const long* o, const long* e, int axis, int op, uint64_t pad)
{
    constexpr int OUT = LUT ? 2 : WE;                                  // bytes of a decoded voxel
    constexpr uint32_t W = 8 * WE, wpt = 128 / W;
    long dims[2];
    for (int k = 0, k2 = 0; k < 3; ++k) if (k != axis) dims[k2++] = e[k];
    const long strides[2] = {(long)(dims[1] + pad), 1};
    const uint64_t reach = (uint64_t)(dims[0] - 1) * strides[0] + dims[1];
    std::vector<uint32_t> image((size_t)reach, kGap), hits((size_t)reach, 0);     // exactly as long as its last element reaches
    sqy::BatchWindow w;
    sqy::Projection q;
    CHECK(sqy::admit_projection(shape, o, e, 3, axis, op, OUT == 2 ? 65535 : 255, image.data(), pad ? strides : nullptr, &w, &q));
    CHECK(q.E0 == (uint64_t)dims[0] && q.E1 == (uint64_t)dims[1] && q.p0 == (uint64_t)strides[0] && q.n == (uint64_t)e[axis]);
    const sqy::WindowGeometry g{w.bY, w.bX, w.oz, w.oy, w.ox, w.Z, w.Y, w.X, q.sz, q.sy};
    sqy::Bitswap1BoxProjectJob job{};
    job.out = image.data();
    job.g = g;
    std::copy(p.plane, p.plane + 16, job.r.plane);
    job.r.tail = p.tail; job.r.w0 = p.w0; job.r.w1 = p.w1; job.r.v0 = p.v0; job.r.v1 = p.v1; job.r.L = p.L;
    job.op = (uint32_t)op; job.axis = q.axis3; job.E0 = q.E0; job.E1 = q.E1; job.p0 = q.p0;
    // (bitswap1_box_project_job_ok lives with the kernels; its rule, the clip's last element = the image's last, is held here)
    {
        const uint64_t last = (g.Z - 1) * g.sz + (g.Y - 1) * g.sy + (g.X - 1);
        CHECK((axis == 2 ? last >> sqy::project_row_shift(g) : last) == (q.E0 - 1) * q.p0 + (q.E1 - 1));
    }
    // the triple loop
    std::vector<uint64_t> want((size_t)(q.E0 * q.E1), op == 1 ? ~0ull : 0ull);
    for (uint64_t z = 0; z < g.Z; ++z) for (uint64_t y = 0; y < g.Y; ++y) for (uint64_t x = 0; x < g.X; ++x) {
        const uint64_t v = volume[(size_t)(((g.oz + z) * g.bY + g.oy + y) * g.bX + g.ox + x)];
        const uint64_t u0 = axis == 0 ? y : z, u1 = axis == 2 ? y : x;
        uint64_t& t = want[(size_t)(u0 * q.E1 + u1)];
        t = op == 0 ? std::max(t, v) : op == 1 ? std::min(t, v) : t + v;
    }
    // the neutral elements, as the init launch's groups walk the image
    const uint64_t groups = sqy::range_job_groups(p.w0, p.w1, wpt);
    for (uint64_t own = 0; own < groups; ++own)
        for (uint64_t tid = 0; tid < 256; ++tid)
            for (uint64_t el = own * 256 + tid; el < q.E0 * q.E1; el += groups * 256) {
                const uint64_t u = el / q.E1;
                CHECK(image[(size_t)(u * q.p0 + (el - u * q.E1))] == kGap);      // (every element once)
                image[(size_t)(u * q.p0 + (el - u * q.E1))] = sqy::project_neutral((uint32_t)op);
            }
    // voxel k of plane word w of the range, out of the planes at Bitswap1Range's addresses
    auto stored = [&](uint64_t wd, uint32_t k) {
        uint32_t v = 0;
        for (uint32_t b = 0; b < W; ++b) {
            uint32_t word = 0;
            for (int j = 0; j < WE; ++j) word |= (uint32_t)in.at((size_t)(p.plane[W - 1 - b] + (wd - p.w0) * WE + j)) << (8 * j);
            v |= ((word >> (W - 1 - k)) & 1u) << b;
        }
        return v;
    };
    ArraySink sink{image.data(), hits.data(), (uint32_t)op};
    const uint32_t uop = (uint32_t)op, uaxis = q.axis3;
    sqy::WindowPiece cur;
    // workgroup 0's tail voxels
    const uint64_t tail0 = p.v0 > p.L ? p.v0 : p.L;
    for (uint64_t t = 0; tail0 + t < p.v1; ++t) {
        CHECK(t < 256);
        sqy::WindowClip ct = sqy::window_clip_start(g, tail0 + t, 1);
        if (sqy::window_clip_next(g, &ct, &cur)) {
            const uint32_t x = sqy::window_voxel_load<WE>(in.data() + p.tail, t);
            CHECK(p.tail + (t + 1) * WE <= in.size());
            sink.combine(uaxis == 2 ? cur.dst_off >> sqy::project_row_shift(g) : cur.dst_off, LUT ? (uint32_t)lut[x & 0xffu] : x);
        }
    }
    // the grid's threads; the ones in front of and behind the range own no word and send nothing
    const uint64_t t0 = sqy::range_first_thread(p.w0, wpt), nt = sqy::range_thread_count(p.w0, p.w1, wpt);
    for (uint64_t t = t0 ? t0 - 1 : 0; t < t0 + nt + 1; ++t) {
        const sqy::RangeRun run = sqy::range_run(t, wpt, p.w0, p.w1);
        const bool owns = run.lo != run.hi;
        CHECK(owns == (t >= t0 && t < t0 + nt));
        sqy::WindowClip c = sqy::window_clip_start(g, owns ? run.first * W : 0, owns ? (uint64_t)run.hi * W : 0);
        bool have = owns && sqy::window_clip_next(g, &c, &cur);
        if (owns) {
            if (run.lo > 0) ++g_first;
            if (run.hi < wpt) ++g_last;
        }
        if (!have) { if (owns) ++g_outside; continue; }
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
        unsigned long long sent = 0;
        for (uint32_t h : hits) sent += h;
        sqy::ProjectPending pend{0, 0, false};
        uint32_t a[4];
        if (WE == 2) {
            for (uint32_t qd = 0; qd < 4 && 2 * qd < run.hi && have; ++qd) {   // word first + 2 q, then first + 2 q + 1: two pieces of eight each
                piece(32 * qd, 8, a); sqy::window_project16<2>(sink, g, c, cur, have, a, 32u * qd, 8, uop, uaxis, &pend);
                piece(32 * qd + 8, 8, a); sqy::window_project16<2>(sink, g, c, cur, have, a, 32u * qd + 8u, 8, uop, uaxis, &pend);
                if (2 * qd + 1 >= run.hi) break;
                piece(32 * qd + 16, 8, a); sqy::window_project16<2>(sink, g, c, cur, have, a, 32u * qd + 16u, 8, uop, uaxis, &pend);
                piece(32 * qd + 24, 8, a); sqy::window_project16<2>(sink, g, c, cur, have, a, 32u * qd + 24u, 8, uop, uaxis, &pend);
            }
        } else {
            for (uint32_t gq = 0; gq < 16 && gq < run.hi && have; gq += 2) {
                if (LUT) {
                    for (uint32_t u = 0; u < 2 && gq + u < run.hi; ++u) {  // a word's eight looked-up voxels: one piece
                        piece(8 * (gq + u), 8, a);
                        sqy::window_project16<2>(sink, g, c, cur, have, a, 8u * (gq + u), 8, uop, uaxis, &pend);
                    }
                } else {
                    const uint32_t n = run.hi - gq >= 2u ? 16u : 8u;
                    piece(8 * gq, n, a);
                    sqy::window_project16<1>(sink, g, c, cur, have, a, 8u * gq, n, uop, uaxis, &pend);
                }
            }
        }
        CHECK(!pend.any);                                               // (a sub-run ends with the run at the latest: the kernel's last send finds nothing)
        unsigned long long now = 0;
        for (uint32_t h : hits) now += h;
        CHECK(now > sent && now - sent <= (unsigned long long)(run.hi - run.lo) * W);
        ++(uaxis != 2 && now - sent == (unsigned long long)(run.hi - run.lo) * W ? g_inside : g_partly);
    }
    for (uint64_t u = 0; u < q.E0; ++u)
        for (uint64_t col = 0; col < q.p0 && u * q.p0 + col < reach; ++col) {
            const uint32_t got = image[(size_t)(u * q.p0 + col)];
            if (col >= q.E1) { CHECK(got == kGap && hits[(size_t)(u * q.p0 + col)] == 0); continue; }
            const uint64_t t = want[(size_t)(u * q.E1 + col)];
            CHECK(t < (1ull << 32));
            if (got != (uint32_t)t) {
                std::fprintf(stderr, "element (%llu, %llu): %u, expected %llu (box %ld %ld %ld + %ld %ld %ld, axis %d, op %d, stored %d bytes, lut %d, pad %llu)\n",
                             (unsigned long long)u, (unsigned long long)col, got, (unsigned long long)t, o[0], o[1], o[2], e[0], e[1], e[2], axis, op, WE, (int)LUT,
                             (unsigned long long)pad);
                return 1;
            }
            // axes 0 and 1: one combine per voxel; axis 2: one per (row, sub-run), more than one where the row meets a run's end -- and one
            // per tail voxel (at most W - 1 of them, combined one by one)
            const uint32_t h = hits[(size_t)(u * q.p0 + col)];
            if (axis != 2) CHECK(h == (uint32_t)e[axis]);
            else { CHECK(h >= 1 && h <= (uint32_t)e[2] / 128u + 2u + (W - 1u)); if (h > 1) ++g_joined; }
        }
    // the z-walking form where the job is admitted to it: a thread per frame-local run of 32 voxels, four bytes of every plane per frame
    // on the 4-byte grid, the reduction by position, the clip in the box's first frame, every element stored exactly once -- no neutral
    // elements first
    if (axis != 0 || (g.bY * g.bX) % 32 != 0) CHECK(!sqy::bitswap1_box_project_walk_ok(job, WE));
    if (sqy::bitswap1_box_project_walk_ok(job, WE)) {
        ++g_walked;
        std::vector<uint32_t> image2((size_t)reach, kGap), stores((size_t)reach, 0);
        const uint64_t frame = g.bY * g.bX, groups2 = sqy::project_walk_groups(g);
        for (uint64_t t = 0; t < groups2 * 256; ++t) {
            const uint64_t run = sqy::project_walk_first_run(g) + t;
            if ((run + 1) * 32 > frame) continue;
            sqy::WindowClip c = sqy::window_clip_start(g, g.oz * frame + run * 32, 32);
            bool have = sqy::window_clip_next(g, &c, &cur);
            if (!have) continue;
            uint32_t acc[32];
            for (int i = 0; i < 32; ++i) acc[i] = sqy::project_neutral(uop);
            for (uint64_t z = 0; z < g.Z; ++z) {
                const uint64_t first = ((g.oz + z) * frame + run * 32) / W, at = (first - p.w0) * WE;
                CHECK(first >= p.w0 && first + 32 / W <= p.w1);
                for (uint32_t b = 0; b < W; ++b) CHECK((p.plane[b] + at) % 4 == 0 && p.plane[b] + at + 4 <= in.size());
                for (uint32_t i = 0; i < 32; ++i) {
                    const uint32_t x = stored(first + i / W, i % W);
                    acc[i] = sqy::project_combine(uop, acc[i], LUT ? (uint32_t)lut[x & 0xffu] : x);
                }
            }
            for (uint32_t i = 0; i < 32; ++i)
                if (have && i >= cur.run_off) {
                    image2[(size_t)(cur.dst_off + (i - cur.run_off))] = acc[i];
                    ++stores[(size_t)(cur.dst_off + (i - cur.run_off))];
                    if (i + 1 == cur.run_off + cur.len) have = sqy::window_clip_next(g, &c, &cur);
                }
        }
        for (uint64_t u = 0; u < q.E0; ++u)
            for (uint64_t col = 0; col < q.p0 && u * q.p0 + col < reach; ++col) {
                const size_t at = (size_t)(u * q.p0 + col);
                if (col >= q.E1) CHECK(image2[at] == kGap && stores[at] == 0);
                else CHECK(image2[at] == (uint32_t)want[(size_t)(u * q.E1 + col)] && stores[at] == 1);
            }
    }
    return 0;
}

// z-ranges of a blob of (bZ, bY, bX) voxels with a table of boxes in each, the stream cut into chunks of `chunk` bytes
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
    const std::vector<uint64_t> shape{bZ, bY, bX};
    uint64_t turn = 0;
    for (uint64_t oz : {(uint64_t)0, (uint64_t)1, bZ - 1}) for (uint64_t Z : {(uint64_t)1, (uint64_t)2, bZ - oz}) {
        if (oz >= bZ || oz + Z > bZ) continue;
        const sqy::FrameRangePlan p = sqy::frame_range_plan(form, n, elem, bZ, oz, Z, chunk, total, nframes);
        CHECK(p.ok && p.we == WE && p.v0 == oz * bY * bX && p.v1 == (oz + Z) * bY * bX);
        std::vector<uint8_t> in;                                       // what the pruned LZ4 decode leaves: the chunks of p.ids back to back
        for (uint32_t f : p.ids) in.insert(in.end(), stream.begin() + (size_t)(f * chunk), stream.begin() + (size_t)std::min<uint64_t>((f + 1) * chunk, total));
        CHECK(in.size() == p.out_bytes);
        for (uint64_t oy : {(uint64_t)0, (uint64_t)1}) for (uint64_t Y : {(uint64_t)1, bY - oy})
        for (uint64_t ox : {(uint64_t)0, (uint64_t)3, bX - 1}) for (uint64_t X : {(uint64_t)1, (uint64_t)5, (uint64_t)129, bX - ox}) {
            if (oy >= bY || ox + X > bX) continue;
            const long o[3] = {(long)oz, (long)oy, (long)ox}, e[3] = {(long)Z, (long)Y, (long)X};
            for (int axis = 0; axis < 3; ++axis)
                for (int op = 0; op < 3; ++op, ++turn)                  // dense and pitched in turn, every (axis, op) both ways over the table
                    if (project_box<WE, LUT>(p, in, volume, lut, shape, o, e, axis, op, (turn % 2) * 3)) return 1;
        }
    }
    return 0;
}

template <int WE, bool LUT>
int blobs()
{
    return box_blob<WE, LUT>(3, 5, 7, 64) || box_blob<WE, LUT>(2, 3, 300, 256) || box_blob<WE, LUT>(7, 33, 31, 1024) || box_blob<WE, LUT>(3, 8, 32, 256);
}

} // namespace

int main()
{
    if (test_path() || test_layout() || test_admission()) return 1;
    if (blobs<2, false>() || blobs<1, false>() || blobs<1, true>()) return 1;
    std::printf("runs outside %llu inside %llu partly %llu first %llu last %llu joined %llu walked %llu\n", g_outside, g_inside, g_partly, g_first, g_last, g_joined, g_walked);
    std::printf("project_boxes ok\n");
    return 0;
}
