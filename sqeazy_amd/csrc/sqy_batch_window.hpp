// sqy_batch_window.hpp -- the clip of a window (SQYAMD_Decode_BatchWindow_*), written once for two callers under sqy_batch_view.hpp's
// rule: the kernels that store only a window's voxels (sqy_kernels.hip) and plain host C++ (no HIP header needed:
// tests/sanitize/batch_window_test.cpp holds it against a triple loop for every window of small blobs).
//
// A blob is bZ x bY x bX voxels in dense order i = (z bY + y) bX + x.  A window is the box [oz, oz + Z) x [oy, oy + Y) x [ox, ox + X) of
// it; its voxel (z, y, x) goes to offset (z - oz) sz + (y - oy) sy + (x - ox) of the destination view.  The clip takes a run [i0, i0 + n)
// of the blob's dense order and yields the sub-runs that lie inside the window -- each one within a row, so consecutive on both sides --
// with two divisions at its start and none afterwards: what lies outside is stepped over with multiplications.
// Behind the clip: the mask and the merge of a window's update in the bit-plane layout (SQYAMD_Update_BatchWindow_*), and the sums of a
// window's compare with a view (SQYAMD_Compare_BatchWindow_*; tests/sanitize/batch_compare_test.cpp holds them against a triple loop;
// SQYAMD_Compare_Boxes_* gathers the same sums over the range transposer's runs: tests/sanitize/compare_boxes_test.cpp).
// And the projection of a box along an axis (SQYAMD_Project_Boxes_*): a combine into an image where the scatter stores
// (tests/sanitize/project_boxes_test.cpp).  And the intensity histogram of a box (SQYAMD_Histogram_Boxes_*): a count into a window of
// bins where the scatter stores (tests/sanitize/histogram_boxes_test.cpp).
#ifndef SQY_BATCH_WINDOW_HPP_
#define SQY_BATCH_WINDOW_HPP_

#include "sqy_batch_view.hpp"

namespace sqy {

// the blob's rows and the window in it (the blob's bZ is not needed: the run ends where the caller says), the destination view's pitches
struct WindowGeometry { uint64_t bY, bX, oz, oy, ox, Z, Y, X, sz, sy; };

struct WindowClip {
    uint64_t z, y, x;        // the blob coordinates of the voxel at `pos`
    uint64_t pos, n;         // where the clip stands in the run, the run's length
};

// a sub-run: `len` voxels from offset `run_off` of the run go to offset `dst_off` of the destination view
struct WindowPiece { uint64_t run_off, dst_off, len; };

// the clip of the run [i0, i0 + n) (i0 + n <= bZ bY bX)
SQY_VIEW_HD inline WindowClip window_clip_start(const WindowGeometry& g, uint64_t i0, uint64_t n)
{
    uint64_t row, z;
    if (((i0 | g.bX | g.bY) >> 32) == 0) {
        row = (uint32_t)i0 / (uint32_t)g.bX;
        z = (uint32_t)row / (uint32_t)g.bY;
    } else {
        row = i0 / g.bX;
        z = row / g.bY;
    }
    return WindowClip{z, row - z * g.bY, i0 - row * g.bX, 0, n};
}

// The next sub-run inside the window, false when the run has none left.  Every turn of the loop either yields or steps over at least one
// voxel that lies outside, whole rows and frames at a time.
SQY_VIEW_HD inline bool window_clip_next(const WindowGeometry& g, WindowClip* c, WindowPiece* out)
{
    while (c->pos < c->n) {
        if (c->z >= g.oz + g.Z) break;                                  // behind the window's last frame: nothing more
        if (c->z < g.oz) {                                              // to the window's first frame
            c->pos += (g.oz - c->z) * g.bY * g.bX - (c->y * g.bX + c->x);
            c->z = g.oz; c->y = 0; c->x = 0;
        } else if (c->y < g.oy) {                                       // to its first row in this frame
            c->pos += (g.oy - c->y) * g.bX - c->x;
            c->y = g.oy; c->x = 0;
        } else if (c->y >= g.oy + g.Y) {                                // to the next frame
            c->pos += (g.bY - c->y) * g.bX - c->x;
            ++c->z; c->y = 0; c->x = 0;
        } else if (c->x < g.ox) {                                       // to its first column in this row
            c->pos += g.ox - c->x;
            c->x = g.ox;
        } else if (c->x >= g.ox + g.X) {                                // to the next row
            c->pos += g.bX - c->x;
            c->x = 0;
            if (++c->y == g.bY) { c->y = 0; ++c->z; }
        } else {
            const uint64_t in_row = g.ox + g.X - c->x, in_run = c->n - c->pos, len = in_row < in_run ? in_row : in_run;
            out->run_off = c->pos;
            out->dst_off = (c->z - g.oz) * g.sz + (c->y - g.oy) * g.sy + (c->x - g.ox);
            out->len = len;
            c->pos += len;
            c->x += len;
            if (c->x == g.bX) {
                c->x = 0;
                if (++c->y == g.bY) { c->y = 0; ++c->z; }
            }
            return true;
        }
    }
    c->pos = c->n;
    return false;
}

// The tiles of `tile` voxels of the blob's dense order that hold a voxel of the window's frames [oz, oz + Z): the first one and their
// count (the transposer's grid holds no others)
SQY_VIEW_HD inline uint64_t window_first_tile(const WindowGeometry& g, uint64_t tile) { return g.oz * g.bY * g.bX / tile; }
SQY_VIEW_HD inline uint64_t window_tile_count(const WindowGeometry& g, uint64_t tile)
{
    return ((g.oz + g.Z) * g.bY * g.bX - 1) / tile - window_first_tile(g, tile) + 1;
}

// ---- the box of one large blob (SQYAMD_Decode_Box_*): the windowed transposer over a RANGE [w0, w1) of the plane words ----
// Its grid runs over ABSOLUTE words: thread t owns the words [t wpt, (t + 1) wpt) n [w0, w1), so the 16 bytes it reads of a plane lie on
// the 16-byte grid of the original stream wherever the range begins.  The run it clips begins at its own first voxel, t wpt W, and ends
// behind its last owned word: the words in front of w0 hold voxels in front of the box's first frame (w0 W <= the box's first voxel),
// which the clip steps over like any others outside -- they are never loaded and never stored.
struct RangeRun {
    uint64_t first;          // the thread's first word, t wpt
    uint32_t lo, hi;         // it owns the words first + [lo, hi) (lo == hi: none)
};
SQY_VIEW_HD inline uint64_t range_first_thread(uint64_t w0, uint32_t wpt) { return w0 / wpt; }
SQY_VIEW_HD inline uint64_t range_thread_count(uint64_t w0, uint64_t w1, uint32_t wpt) { return w1 > w0 ? (w1 - 1) / wpt - w0 / wpt + 1 : 0; }
SQY_VIEW_HD inline RangeRun range_run(uint64_t t, uint32_t wpt, uint64_t w0, uint64_t w1)
{
    const uint64_t first = t * wpt;
    const uint32_t lo = w0 > first ? (w0 - first < wpt ? (uint32_t)(w0 - first) : wpt) : 0u;
    const uint32_t hi = w1 > first ? (w1 - first < wpt ? (uint32_t)(w1 - first) : wpt) : 0u;
    return RangeRun{first, lo, hi > lo ? hi : lo};
}

// Many boxes of one blob in one launch (SQYAMD_Decode_Boxes_*): job j owns range_job_groups workgroups of 256 threads -- its threads in
// order, at least one workgroup (the job's first one also moves the tail voxels) -- and workgroup `own` of a job is the single-box
// grid's block `own`: its thread tid is range_first_thread + own 256 + tid.  first_tile holds the prefix sums of the groups.
SQY_VIEW_HD inline uint64_t range_job_groups(uint64_t w0, uint64_t w1, uint32_t wpt)
{
    const uint64_t g = (range_thread_count(w0, w1, wpt) + 255) / 256;
    return g ? g : 1;
}
// the job of workgroup `group`: first_tile[lo] <= group < first_tile[lo + 1] (the kernels' batch_job_of_tile; njobs >= 1)
SQY_VIEW_HD inline uint32_t range_job_of_group(const uint32_t* first_tile, uint32_t njobs, uint32_t group)
{
    uint32_t lo = 0, hi = njobs;
    while (hi - lo > 1u) {
        const uint32_t mid = (lo + hi) >> 1;
        if (first_tile[mid] <= group) lo = mid; else hi = mid;
    }
    return lo;
}

// ---- the update of a window in the bit-plane layout (SQYAMD_Update_BatchWindow_*) ----
// A voxel has the same bit position in every plane: with W voxels to a plane word (16 for 16-bit voxels, 8 for 8-bit ones), plane
// W - 1 - b, word w, bit W - 1 - k is bit b of voxel W w + k.  A run of 128 voxels that begins at a word is 16 bytes of every plane -- four
// 32-bit words m[0..3] as they lie in memory, plane word i of the run at bit W i of them --, and ONE mask says which of those bits a
// window replaces, whatever the plane.

// the bits of the voxels [off, off + len) of the run (off + len <= 128), or-ed into m
SQY_VIEW_HD inline void window_run_mask(uint32_t W, uint32_t off, uint32_t len, uint32_t m[4])
{
    for (uint32_t w = off / W; w * W < off + len; ++w) {
        const uint32_t lo = off > w * W ? off - w * W : 0, hi = off + len < (w + 1) * W ? off + len - w * W : W;
        // voxels [lo, hi) of word w: its bits [W - hi, W - lo)
        const uint32_t bits = ((1u << (hi - lo)) - 1u) << (W - hi), at = w * W;             // (hi - lo <= W <= 16)
        m[at >> 5] |= bits << (at & 31u);
    }
}

// a piece of a plane (a plane word, or several side by side) with the window's bits replaced; `mask` is the same piece of the run's mask
template <class T>
SQY_VIEW_HD inline T window_merge_word(T old_bits, T new_bits, T mask)
{
    return (T)((old_bits & (T)~mask) | (new_bits & mask));
}

// ---- the compare of a window with a view of its shape (SQYAMD_Compare_BatchWindow_*) ----
// What a thread gathers over its voxels: a = the blob's decoded voxel, b = the view's.  A thread owns at most 128 voxels, so every sum
// but sum_sq fits 32 bits there (128 x 65535 < 2^23); 128 x 65535^2 does not.  The neutral element: compare_sums_neutral().
struct CompareSums {
    uint64_t sum_sq;                 // sum (a - b)^2
    uint32_t n;                      // voxels compared
    uint32_t ndiff, sum_abs, max_abs;            // a != b; sum |a - b|; max |a - b|
    uint32_t view_sum, view_min, view_max;       // of b
};
SQY_VIEW_HD inline CompareSums compare_sums_neutral() { return CompareSums{0, 0, 0, 0, 0, 0, 0xffffffffu, 0}; }

SQY_VIEW_HD inline void compare_voxel(CompareSums* s, uint32_t a, uint32_t b)
{
    const uint32_t d = a > b ? a - b : b - a;
    ++s->n;
    s->ndiff += d != 0u;
    s->sum_abs += d;
    s->sum_sq += (uint64_t)(d * d);                                     // (d <= 65535: the square fits 32 bits)
    s->max_abs = d > s->max_abs ? d : s->max_abs;
    s->view_sum += b;
    s->view_min = b < s->view_min ? b : s->view_min;
    s->view_max = b > s->view_max ? b : s->view_max;
}

// sixteen bytes as they lie in memory, on the 16-byte grid
struct alignas(16) WindowBytes16 { uint32_t w[4]; };

template <int ELEM>
SQY_VIEW_HD inline uint32_t window_voxel_load(const uint8_t* base, uint64_t off)
{
    if constexpr (ELEM == 2) return reinterpret_cast<const uint16_t*>(base)[off];
    else return base[off];
}

// voxels [lo, hi) of two pieces of sixteen bytes, each packed as in a dense copy (hi <= 16 / ELEM)
template <int ELEM>
SQY_VIEW_HD inline void compare_piece(CompareSums* s, const uint32_t a[4], const uint32_t b[4], uint32_t lo, uint32_t hi)
{
    constexpr uint32_t G = 16 / ELEM, M = ELEM == 2 ? 0xffffu : 0xffu;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (uint32_t k = 0; k < G; ++k)
        if (k >= lo && k < hi) {
            const uint32_t sh = 8u * ((k * ELEM) & 3u);
            compare_voxel(s, (a[k * ELEM / 4] >> sh) & M, (b[k * ELEM / 4] >> sh) & M);
        }
}

// The windowed transposer's scatter with loads where its stores were: the piece `a` holds the n decoded voxels (n <= 16 / ELEM) at offset p
// of the thread's run; those inside the current sub-run `cur` -- and the ones behind it that the piece reaches, have: there is one -- are
// compared with the view's voxels of the same places.  The view is read sixteen bytes at a time where the full piece lies in one sub-run
// (so in one row) and on the view's 16-byte grid, voxel by voxel where not; nothing else of it is read.  Pieces come in ascending p.
template <int ELEM>
SQY_VIEW_HD inline void window_compare16(const uint8_t* view, const WindowGeometry& g, WindowClip& c, WindowPiece& cur, bool& have, const uint32_t a[4], uint32_t p, uint32_t n,
                                         CompareSums* s)
{
    constexpr uint32_t G = 16 / ELEM;
    while (have && cur.run_off < (uint64_t)p + n) {
        const uint64_t end = cur.run_off + cur.len;                  // (> p: a sub-run that ends in front of the piece has been left)
        const uint32_t lo = cur.run_off > p ? (uint32_t)(cur.run_off - p) : 0u, hi = end < (uint64_t)p + n ? (uint32_t)(end - p) : n;
        const uint64_t off = cur.dst_off + ((uint64_t)p + lo - cur.run_off);          // where voxel lo of the piece lies in the view
        const uint8_t* q = view + off * ELEM;
        uint32_t b[4] = {0, 0, 0, 0};
        if (lo == 0 && hi == G && (reinterpret_cast<uintptr_t>(q) & 15u) == 0) {
            const WindowBytes16 r = *reinterpret_cast<const WindowBytes16*>(q);
            b[0] = r.w[0]; b[1] = r.w[1]; b[2] = r.w[2]; b[3] = r.w[3];
        } else {
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
            for (uint32_t k = 0; k < G; ++k)
                if (k >= lo && k < hi) b[k * ELEM / 4] |= window_voxel_load<ELEM>(view, off + (k - lo)) << (8u * ((k * ELEM) & 3u));
        }
        compare_piece<ELEM>(s, a, b, lo, hi);
        if (end > (uint64_t)p + n) break;                             // the sub-run goes on in the next piece
        have = window_clip_next(g, &c, &cur);
    }
}

// ---- the projection of a box along an axis (SQYAMD_Project_Boxes_*) ----
// The range transposer's scatter with a combine where its stores were: every decoded voxel of the box is combined -- max, min or sum in
// 32 unsigned bits -- into the element of the output image that its place with the projected axis removed names.  The clip computes that
// element: the job's WindowGeometry is filled (sqy::admit_projection) so that dst_off drops the projected axis --
//   axis 0 (frames):  sz = 0, sy = the image's row pitch:   element = cur.dst_off + (p + k - cur.run_off)
//   axis 1 (rows):    sy = 0, sz = the image's row pitch:   the same expression
//   axis 2 (columns): sy = K, sz = K x the image's row pitch, K the power of two >= X: a sub-run lies within one row of the box, so ALL
//                     its voxels go to the one element cur.dst_off >> log2(K) (the bits below hold x - ox); the thread reduces them
//                     itself and sends ONE combine per sub-run -- rows longer than a thread's 128 voxels and rows that straddle two
//                     threads' runs meet in the sink.
// tests/sanitize/project_boxes_test.cpp holds it against a triple loop with an array for the sink.
constexpr uint32_t kProjectMax = 0, kProjectMin = 1, kProjectSum = 2, kProjectOps = 3;

SQY_VIEW_HD inline uint32_t project_neutral(uint32_t op) { return op == kProjectMin ? 0xffffffffu : 0u; }
SQY_VIEW_HD inline uint32_t project_combine(uint32_t op, uint32_t a, uint32_t b)
{
    return op == kProjectMax ? (a > b ? a : b) : op == kProjectMin ? (a < b ? a : b) : a + b;
}
// log2 of the power of two K that axis 2's geometry holds in sy
SQY_VIEW_HD inline uint32_t project_row_shift(const WindowGeometry& g) { return (uint32_t)__builtin_ctzll(g.sy | (1ull << 63)); }

// what a thread has reduced of the sub-run it stands in (axis 2): `any` false, nothing
struct ProjectPending { uint64_t off; uint32_t v; bool any; };

// The piece `a` holds the n decoded voxels (n <= 16 / ELEM, packed as in a dense copy) at offset p of the thread's run; those inside the
// current sub-run `cur` -- and the ones behind it that the piece reaches, have: there is one -- are combined into `sink`
// (sink.combine(element, value)).  Pieces come in ascending p; what `pend` still holds behind the run's last piece is the caller's to send.
template <int ELEM, class Sink>
SQY_VIEW_HD inline void window_project16(Sink& sink, const WindowGeometry& g, WindowClip& c, WindowPiece& cur, bool& have, const uint32_t a[4], uint32_t p, uint32_t n,
                                         uint32_t op, uint32_t axis, ProjectPending* pend)
{
    constexpr uint32_t G = 16 / ELEM, M = ELEM == 2 ? 0xffffu : 0xffu;
    const uint32_t shift = axis == 2 ? project_row_shift(g) : 0u;
    while (have && cur.run_off < (uint64_t)p + n) {
        const uint64_t end = cur.run_off + cur.len;                  // (> p: a sub-run that ends in front of the piece has been left)
        const uint32_t lo = cur.run_off > p ? (uint32_t)(cur.run_off - p) : 0u, hi = end < (uint64_t)p + n ? (uint32_t)(end - p) : n;
        const uint64_t off = cur.dst_off + ((uint64_t)p + lo - cur.run_off);          // axes 0, 1: the element of voxel lo of the piece
        if (axis == 2 && !pend->any) *pend = ProjectPending{cur.dst_off >> shift, project_neutral(op), true};
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
        for (uint32_t k = 0; k < G; ++k)
            if (k >= lo && k < hi) {
                const uint32_t v = (a[k * ELEM / 4] >> (8u * ((k * ELEM) & 3u))) & M;
                if (axis == 2) pend->v = project_combine(op, pend->v, v);
                else sink.combine(off + (k - lo), v);
            }
        if (end > (uint64_t)p + n) break;                             // the sub-run goes on in the next piece
        if (axis == 2) { sink.combine(pend->off, pend->v); pend->any = false; }
        have = window_clip_next(g, &c, &cur);
    }
}

// ---- boxes read at a coarser resolution (SQYAMD_Bin_Boxes_*) ----
// A box of extent (Z, Y, X) under bins (bz, by, bx) -- clamped to the extent by sqy::admit_binning, so a bin never exceeds its dimension --
// has the cell grid C = ceil(extent / bins); cell c reduces the box's voxels [c bins, min((c + 1) bins, extent)).  The bit-plane kernel
// gives every workgroup a BLOCK of cells (sqy::bin_boxes_plan states the tiling): ONE cell layer cz, the cell rows [cy0, cy0 + ncy), the
// cell columns [cx0, cx0 + ncx) -- at most kBinBlockCells accumulators in LDS, and a footprint in a frame that is a band of rows of the
// blob cut to the strip's columns.  Block `own` of a box is layer own / (nbands nstrips), band .. / nstrips, strip .. % nstrips.
// The workgroup's threads share the ITEMS of the block: item t is one 32-voxel run of the blob's dense order on the absolute grid
// (run r holds the voxels [32 r, 32 r + 32): four bytes of every plane) in one frame of the footprint; where a frame is a whole number
// of runs (`zreg`) an item is the run in the layer's FIRST frame and the thread reduces the same positions of the layer's other frames
// into it in registers first.  The clip (window_clip_*, the footprint's geometry with Z = 1 at the item's frame, sy = K the power of
// two >= the footprint's width, sz = 0) names the run's voxels inside the footprint: dst_off = (y - oy) K + (x - ox).  bin_run_cells
// reduces the neighbouring voxels of one cell in registers and sends ONE combine per piece of a cell's row to the sink -- the kernel's
// sink is an LDS atomic on the block's accumulators, the host test's an array (tests/sanitize/bin_boxes_test.cpp holds the whole walk
// against a triple loop).
constexpr uint32_t kBinBlockCells = 8192;               // the accumulators of a block: 32 KiB of LDS, well under the CU's 160 KiB
constexpr uint64_t kBinBlockVoxels = 1u << 16;          // the footprint a block is sized for (256 threads x 8 runs) where the cells allow it

struct BinPlan { uint64_t C[3]; uint64_t band, strip, nbands, nstrips, blocks; };
struct BinBlock { uint64_t cz, cy0, ncy, cx0, ncx; };
SQY_VIEW_HD inline BinBlock bin_block_of(const BinPlan& p, uint64_t own)
{
    const uint64_t per_layer = p.nbands * p.nstrips, cz = own / per_layer, r = own - cz * per_layer, b = r / p.nstrips, s = r - b * p.nstrips;
    const uint64_t cy0 = b * p.band, cx0 = s * p.strip;
    return BinBlock{cz, cy0, p.C[1] - cy0 < p.band ? p.C[1] - cy0 : p.band, cx0, p.C[2] - cx0 < p.strip ? p.C[2] - cx0 : p.strip};
}

// a block's footprint: the frames [z0, z0 + nz) of its cell layer and, in each, the clip's geometry (g.oz is the caller's to step)
struct BinFootprint { WindowGeometry g; uint64_t z0, nz; };
SQY_VIEW_HD inline BinFootprint bin_block_footprint(const WindowGeometry& box, const uint64_t bins[3], const BinBlock& b)
{
    const uint64_t z = b.cz * bins[0], y = b.cy0 * bins[1], x = b.cx0 * bins[2];
    const uint64_t nz = box.Z - z < bins[0] ? box.Z - z : bins[0];
    const uint64_t Y = box.Y - y < b.ncy * bins[1] ? box.Y - y : b.ncy * bins[1], X = box.X - x < b.ncx * bins[2] ? box.X - x : b.ncx * bins[2];
    uint64_t K = 1;
    while (K < X) K <<= 1;
    return BinFootprint{WindowGeometry{box.bY, box.bX, box.oz + z, box.oy + y, box.ox + x, 1, Y, X, 0, K}, box.oz + z, nz};
}
// the runs that hold a voxel of the footprint in frame z, and a bound on their number that holds for every frame
SQY_VIEW_HD inline uint64_t bin_frame_first_run(const WindowGeometry& g, uint64_t z) { return ((z * g.bY + g.oy) * g.bX + g.ox) / 32; }
SQY_VIEW_HD inline uint64_t bin_frame_last_run(const WindowGeometry& g, uint64_t z) { return ((z * g.bY + g.oy + g.Y - 1) * g.bX + g.ox + g.X - 1) / 32; }
SQY_VIEW_HD inline uint64_t bin_frame_runs(const WindowGeometry& g) { return ((g.Y - 1) * g.bX + g.X + 31) / 32 + 1; }
SQY_VIEW_HD inline uint64_t bin_block_items(const BinFootprint& f, bool zreg) { return (zreg ? 1 : f.nz) * bin_frame_runs(f.g); }
// item t of a block: its frame and run (false: the frame has no such run)
SQY_VIEW_HD inline bool bin_block_item(const BinFootprint& f, bool zreg, uint64_t t, uint64_t* z, uint64_t* run)
{
    const uint64_t nr = bin_frame_runs(f.g), zi = zreg ? 0 : t / nr, k = t - zi * nr;
    *z = f.z0 + zi;
    *run = bin_frame_first_run(f.g, *z) + k;
    return *run <= bin_frame_last_run(f.g, *z);
}

SQY_VIEW_HD inline uint64_t bin_div(uint64_t a, uint64_t b) { return ((a | b) >> 32) == 0 ? (uint64_t)((uint32_t)a / (uint32_t)b) : a / b; }

// The 32 values v of a run whose clip stands at its first sub-run `cur` (`have`: there is one): every piece of a cell's row inside the
// run is reduced here and sent once -- sink.combine(cell, value), cell = (cy - cy0) ncx + (cx - cx0) within the block.  by, bx: the
// bins along y and x; ncx: the block's cell columns.
template <class Sink>
SQY_VIEW_HD inline void bin_run_cells(Sink& sink, const WindowGeometry& g, WindowClip& c, WindowPiece& cur, bool& have, const uint32_t (&v)[32], uint64_t by, uint64_t bx,
                                      uint64_t ncx, uint32_t op)
{
    const uint32_t shift = project_row_shift(g);
    uint64_t cell = 0, left = 0;                                        // the cell the walk stands in, what is left of its row piece
    uint32_t acc = project_neutral(op);
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (uint32_t i = 0; i < 32; ++i)
        if (have && i >= cur.run_off) {                                 // (sub-runs in ascending order: i is inside `cur` or in front of it)
            if (i == cur.run_off) {
                const uint64_t y = cur.dst_off >> shift, x = cur.dst_off & (g.sy - 1), cx = bin_div(x, bx);
                cell = bin_div(y, by) * ncx + cx;
                left = bx - (x - cx * bx);
            }
            acc = project_combine(op, acc, v[i]);
            const bool last = i + 1 == cur.run_off + cur.len;
            if (--left == 0 || last) {
                sink.combine(cell, acc);
                acc = project_neutral(op);
                ++cell;
                left = bx;
            }
            if (last) have = window_clip_next(g, &c, &cur);
        }
}

// ---- the intensity histograms of boxes (SQYAMD_Histogram_Boxes_*) ----
// Voxel v of a box falls into bin v >> shift of the box's nbins = R >> shift counters (R = 65536 for 16-bit voxels, 256 for 8-bit ones).
// A workgroup counts into a private array of hist_window_bins(nbins) counters in LDS: the whole histogram up to kHistWindowBins bins
// (64 KiB), else ONE window of that many bins -- window k holds the bins [k kHistWindowBins, (k + 1) kHistWindowBins) -- voted from the
// first voxel each thread counts (hist_vote_window, hist_best_window: the first of the windows with the most votes); a bin outside the
// window goes straight to the output.  Whatever window wins, the counts are the same.  Stacks have long constant runs, and 64 lanes
// adding 1 to one LDS address serialise, so equal neighbours can go in one add (MERGE, below): hist_count merges equal consecutive bins
// of a thread's whole walk -- what `run` still holds behind the walk's last voxel is the caller's to send with hist_flush --, hist_piece
// a full piece of sixteen bytes whose bins are all equal.  The sink: sink.add(bin, n) -- the kernels' routes a
// bin with hist_window_slot to an LDS atomic or a global one, the host test's (tests/sanitize/histogram_boxes_test.cpp, which holds the
// whole walk against a triple loop) to two arrays.
constexpr uint32_t kHistWindowBins = 16384;

SQY_VIEW_HD inline uint32_t hist_bin(uint32_t v, uint32_t shift) { return v >> shift; }
SQY_VIEW_HD inline uint32_t hist_window_bins(uint32_t nbins) { return nbins < kHistWindowBins ? nbins : kHistWindowBins; }
SQY_VIEW_HD inline uint32_t hist_windows(uint32_t nbins) { return nbins / hist_window_bins(nbins ? nbins : 1u); }
SQY_VIEW_HD inline uint32_t hist_vote_window(uint32_t bin) { return bin / kHistWindowBins; }
// the first of the nwin (<= 4) windows with the most votes
SQY_VIEW_HD inline uint32_t hist_best_window(const uint32_t votes[4], uint32_t nwin)
{
    uint32_t best = 0;
    for (uint32_t q = 1; q < 4; ++q)
        if (q < nwin && votes[q] > votes[best]) best = q;
    return best;
}
// true: `bin` is counter *slot of the window that begins at bin wbase and holds wbins bins
SQY_VIEW_HD inline bool hist_window_slot(uint32_t bin, uint32_t wbase, uint32_t wbins, uint32_t* slot)
{
    *slot = bin - wbase;
    return *slot < wbins;                                               // (bin < wbase wraps far above wbins)
}

// the equal bins a thread has seen in a row and not sent yet (n == 0: none)
struct HistRun { uint32_t bin, n; };

// MERGE: kHistMergeNone, one add per voxel; kHistMergeRuns, equal consecutive bins of the thread's whole walk in one add;
// kHistMergePieces, a full piece of sixteen bytes whose bins are all equal in one add, voxel by voxel otherwise (hist_piece)
constexpr int kHistMergeNone = 0, kHistMergeRuns = 1, kHistMergePieces = 2;

template <int MERGE, class Sink>
SQY_VIEW_HD inline void hist_count(Sink& sink, HistRun* run, uint32_t bin)
{
    if constexpr (MERGE != kHistMergeRuns) sink.add(bin, 1u);
    else {
        if (run->n != 0 && run->bin == bin) { ++run->n; return; }
        if (run->n != 0) sink.add(run->bin, run->n);
        run->bin = bin;
        run->n = 1;
    }
}
template <class Sink>
SQY_VIEW_HD inline void hist_flush(Sink& sink, HistRun* run)
{
    if (run->n != 0) sink.add(run->bin, run->n);
    run->n = 0;
}

// voxels [lo, hi) of a piece of sixteen bytes packed as in a dense copy (hi <= 16 / ELEM), counted
template <int ELEM, int MERGE, class Sink>
SQY_VIEW_HD inline void hist_piece(Sink& sink, HistRun* run, const uint32_t a[4], uint32_t lo, uint32_t hi, uint32_t shift)
{
    constexpr uint32_t G = 16 / ELEM, M = ELEM == 2 ? 0xffffu : 0xffu;
    if constexpr (MERGE == kHistMergePieces) {
        if (lo == 0 && hi == G) {                                       // the bins of all G voxels at once: each voxel's field shifted in place
            const uint32_t m = (M >> shift) * (ELEM == 2 ? 0x00010001u : 0x01010101u);
            const uint32_t b0 = (a[0] >> shift) & m, b1 = (a[1] >> shift) & m, b2 = (a[2] >> shift) & m, b3 = (a[3] >> shift) & m;
            const uint32_t turned = (b0 >> (8u * ELEM)) | (b0 << (32u - 8u * ELEM));      // (equal to b0: all its fields are equal)
            if (b0 == b1 && b0 == b2 && b0 == b3 && b0 == turned) { sink.add(b0 & M, G); return; }
        }
    }
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (uint32_t k = 0; k < G; ++k)
        if (k >= lo && k < hi) hist_count<MERGE>(sink, run, hist_bin((a[k * ELEM / 4] >> (8u * ((k * ELEM) & 3u))) & M, shift));
}

// window_compare16 with a count where it compares: the piece `a` holds the n decoded voxels (n <= 16 / ELEM) at offset p of the thread's
// run; those inside the current sub-run `cur` -- and the ones behind it that the piece reaches, have: there is one -- are counted.
// Pieces come in ascending p.
template <int ELEM, int MERGE, class Sink>
SQY_VIEW_HD inline void window_histogram16(Sink& sink, const WindowGeometry& g, WindowClip& c, WindowPiece& cur, bool& have, const uint32_t a[4], uint32_t p, uint32_t n,
                                           uint32_t shift, HistRun* run)
{
    while (have && cur.run_off < (uint64_t)p + n) {
        const uint64_t end = cur.run_off + cur.len;                  // (> p: a sub-run that ends in front of the piece has been left)
        const uint32_t lo = cur.run_off > p ? (uint32_t)(cur.run_off - p) : 0u, hi = end < (uint64_t)p + n ? (uint32_t)(end - p) : n;
        hist_piece<ELEM, MERGE>(sink, run, a, lo, hi, shift);
        if (end > (uint64_t)p + n) break;                             // the sub-run goes on in the next piece
        have = window_clip_next(g, &c, &cur);
    }
}

// ---- a resolution pyramid of boxes (SQYAMD_Pyramid_Boxes_*) ----
// Level l of a box is its binning under the bins of row l; the rows nest (sqy::admit_pyramid), so with r = bins[l] / bins[l - 1] a cell c
// of level l is the reduction of the level-(l - 1) cells [c r, min((c + 1) r, C[l - 1])) per dimension -- partial cells at the far edge
// and bins beyond the extent included, for C[l] = ceil(C[l - 1] / min(r, C[l - 1])).  The bit-plane kernel gives every workgroup a BLOCK
// of cells of the top fused level T (sqy::pyramid_boxes_plan states T and the tiling): ONE level-T cell layer, a band of level-T cell
// rows, a strip of level-T cell columns.  Below it lie, per level l <= T, q[l] cells of level l per level-T cell and dimension; the
// block's accumulators of level l -- ONE layer of its level-l cells -- stand at off[l] in LDS.  The workgroup walks the level-0 cell
// layers of the block one after another (the walk of a Bin_Boxes block: bin_block_footprint, bin_block_item, bin_run_cells); behind a
// barrier it stores the layer and folds it into level 1 (pyramid_fold_cell, a thread per level-1 cell), a completed level-1 layer is
// stored and folded into level 2, and so on.  tests/sanitize/pyramid_boxes_test.cpp holds the whole walk against a triple loop per level.
constexpr uint32_t kPyramidMaxLevels = 8;
constexpr uint32_t kPyramidLdsCells = 10240;            // all fused levels' accumulators of a block: 40 KiB -- level 0's 8192 and a quarter more; four workgroups fit a CU
constexpr uint64_t kPyramidBlockVoxels = 1u << 15;      // the voxels a block is sized for where the cells allow it (DESIGN.md 5 says against what)

struct PyramidPlan {
    uint32_t levels, T;                                 // the call's levels; the top fused one
    uint32_t off[kPyramidMaxLevels];                    // level l's accumulators in LDS (l <= T)
    uint64_t C[kPyramidMaxLevels][3];                   // the cell grids
    uint64_t r[kPyramidMaxLevels][3];                   // level-(l - 1) cells per level-l cell, clamped to C[l - 1] (r[0]: ones)
    uint64_t q[kPyramidMaxLevels][3];                   // level-l cells per level-T cell, clamped to C[l] (l <= T); above T: level-T cells per level-l cell, clamped to C[T]
    uint64_t band, strip, nbands, nstrips, blocks;      // the tiling of the level-T grid (BinPlan's fields)
};
SQY_VIEW_HD inline BinPlan pyramid_top_plan(const PyramidPlan& p)
{
    return BinPlan{{p.C[p.T][0], p.C[p.T][1], p.C[p.T][2]}, p.band, p.strip, p.nbands, p.nstrips, p.blocks};
}
// the level-l cells (l <= T) of dimension d under the level-T cells [c0, c0 + n)
SQY_VIEW_HD inline void pyramid_level_span(const PyramidPlan& p, uint32_t l, int d, uint64_t c0, uint64_t n, uint64_t* first, uint64_t* count)
{
    const uint64_t q = p.q[l][d], f = c0 * q, rest = p.C[l][d] - f;      // (c0 q < C[l]: C[T] = ceil(C[l] / q))
    *first = f;
    *count = n * q < rest ? n * q : rest;
}
// cell (ly, lx) of a level's layer from the layer below it, ncy x ncx cells at `lo`: its children [l r, min((l + 1) r, nc)) reduced
SQY_VIEW_HD inline uint32_t pyramid_fold_cell(const uint32_t* lo, uint64_t ncy, uint64_t ncx, uint64_t ry, uint64_t rx, uint64_t ly, uint64_t lx, uint32_t op)
{
    const uint64_t y0 = ly * ry, x0 = lx * rx, y1 = ncy - y0 < ry ? ncy : y0 + ry, x1 = ncx - x0 < rx ? ncx : x0 + rx;
    uint32_t acc = project_neutral(op);
    for (uint64_t y = y0; y < y1; ++y)
        for (uint64_t x = x0; x < x1; ++x) acc = project_combine(op, acc, lo[y * ncx + x]);
    return acc;
}
// cell (cz, cy, cx) of a level above T from the STORED cells of a finer level (grid Cs, pitches spz, spy in elements): the cells
// [c r, min((c + 1) r, Cs)) per dimension reduced -- what a thread of pyramid_reduce_kernel computes
SQY_VIEW_HD inline uint32_t pyramid_reduce_cell(const uint32_t* src, const uint64_t Cs[3], uint64_t spz, uint64_t spy, const uint64_t r[3], uint64_t cz, uint64_t cy,
                                                uint64_t cx, uint32_t op)
{
    const uint64_t z1 = (cz + 1) * r[0] < Cs[0] ? (cz + 1) * r[0] : Cs[0], y1 = (cy + 1) * r[1] < Cs[1] ? (cy + 1) * r[1] : Cs[1];
    const uint64_t x1 = (cx + 1) * r[2] < Cs[2] ? (cx + 1) * r[2] : Cs[2];
    uint32_t acc = project_neutral(op);
    for (uint64_t z = cz * r[0]; z < z1; ++z)
        for (uint64_t y = cy * r[1]; y < y1; ++y) {
            const uint64_t at = z * spz + y * spy;
            for (uint64_t x = cx * r[2]; x < x1; ++x) acc = project_combine(op, acc, src[at + x]);
        }
    return acc;
}

} // namespace sqy
#endif
