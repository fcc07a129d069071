// The box decode on the host (tests/test_host_decode_box.py builds and runs this with g++, sanitizers on): sqy::decode_box_path against its
// table; and the range transposer of SQYAMD_Decode_Box_* run by run as bitswap1_decode_range_window_kernel drives it -- sqy::range_run's
// threads over the ABSOLUTE plane words, the clip of csrc/sqy_batch_window.hpp (the text the kernel compiles) on each thread's run, every
// word read at Bitswap1Range's address in a buffer of exactly the bytes sqy::frame_range_plan says the pruned LZ4 decode leaves, the tail
// voxel by voxel.  Ranges begin and end inside a thread's 128 voxels, plane segments straddle chunks.  The view must equal a triple
// loop's, every byte of it.  Prints "decode_box ok" and returns 0.
#include "../../sqeazy_amd/csrc/sqy_batch_window.hpp"
#include "../../sqeazy_amd/csrc/sqy_pipeline.hpp"

#include <algorithm>
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

int test_path()
{
    const struct { RangeForm form; BoxPath on; } table[] = {{RangeForm::plain, BoxPath::subset_copy}, {RangeForm::planes, BoxPath::subset_transposer},
                                                            {RangeForm::planes_lut, BoxPath::subset_transposer}, {RangeForm::shuffle, BoxPath::subset_copy}};
    for (const auto& row : table) {
        CHECK(sqy::decode_box_path(true, row.form, true) == row.on);
        CHECK(sqy::decode_box_path(true, row.form, false) == BoxPath::whole_copy);         // the option off
        CHECK(sqy::decode_box_path(false, row.form, true) == BoxPath::whole_copy);         // a blob the frame-range plan does not take
        CHECK(sqy::decode_box_path(false, row.form, false) == BoxPath::whole_copy);
    }
    return 0;
}

int test_runs()
{
    // every thread's words are its share of [w0, w1), the shares tile the range in order
    for (uint32_t wpt : {8u, 16u})
        for (uint64_t w0 = 0; w0 < 40; ++w0)
            for (uint64_t w1 = w0; w1 < 60; ++w1) {
                const uint64_t t0 = sqy::range_first_thread(w0, wpt), nt = sqy::range_thread_count(w0, w1, wpt);
                CHECK((w1 == w0) == (nt == 0));
                uint64_t at = w0;
                for (uint64_t t = t0; t < t0 + nt; ++t) {
                    const sqy::RangeRun r = sqy::range_run(t, wpt, w0, w1);
                    CHECK(r.first == t * wpt && r.first % wpt == 0 && r.lo < r.hi && r.hi <= wpt && r.first + r.lo == at);
                    at = r.first + r.hi;
                }
                CHECK(at == w1 || nt == 0);
                if (t0 > 0) { const sqy::RangeRun r = sqy::range_run(t0 - 1, wpt, w0, w1); CHECK(r.lo == r.hi); }
                const sqy::RangeRun behind = sqy::range_run(t0 + nt, wpt, w0, w1);
                CHECK(behind.lo == behind.hi);
            }
    return 0;
}

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

struct Counts { uint64_t boxes = 0, partial_first = 0, partial_last = 0, tails = 0, straddles = 0; } counts;

// Every z-range of a blob of (bZ, bY, bX) voxels with a sample of the boxes in it, for the stream form `form` in chunks of `chunk` bytes
int box_blob(RangeForm form, uint64_t bZ, uint64_t bY, uint64_t bX, uint64_t chunk)
{
    const int elem = form == RangeForm::planes_lut ? 2 : (bX % 2 ? 1 : 2);        // (odd rows: the 8-bit planes)
    const uint64_t n = bZ * bY * bX;
    const uint32_t we = form == RangeForm::planes ? (uint32_t)elem : 1u, W = 8 * we, wpt = 128 / W;
    std::vector<uint32_t> stored(n), volume(n);                      // what the planes hold; what the decode gives
    for (uint64_t i = 0; i < n; ++i) {
        stored[i] = (uint32_t)((i * 2654435761u) >> 7) & (we == 2 ? 0xffffu : 0xffu);
        volume[i] = form == RangeForm::planes_lut ? stored[i] * 257u + 1u : stored[i];      // (the look-up: a table of 16-bit values)
    }
    const std::vector<uint8_t> stream = plane_stream(stored, we);
    const uint64_t total = stream.size();
    const uint32_t nframes = (uint32_t)((total + chunk - 1) / chunk);
    for (uint64_t oz = 0; oz < bZ; ++oz) for (uint64_t Z = 1; oz + Z <= bZ; ++Z) {
        const sqy::FrameRangePlan p = sqy::frame_range_plan(form, n, elem, bZ, oz, Z, chunk, total, nframes);
        CHECK(p.ok && p.we == (int)we && p.v0 == oz * bY * bX && p.v1 == (oz + Z) * bY * bX);
        // what the pruned LZ4 decode leaves: the chunks of p.ids back to back, exactly p.out_bytes of them
        std::vector<uint8_t> in;
        for (uint32_t f : p.ids) in.insert(in.end(), stream.begin() + (size_t)(f * chunk), stream.begin() + (size_t)std::min<uint64_t>((f + 1) * chunk, total));
        CHECK(in.size() == p.out_bytes);
        const uint64_t seg = n / W;
        for (uint64_t s = 0; s + 1 < W && p.w0 < p.w1; ++s)
            if (((s * seg + p.w0) * we) / chunk != ((s * seg + p.w1) * we - 1) / chunk) ++counts.straddles;
        for (uint64_t oy : {(uint64_t)0, (uint64_t)1, bY - 1}) for (uint64_t Y : {(uint64_t)1, bY - oy})
        for (uint64_t ox : {(uint64_t)0, (uint64_t)3, bX - 1}) for (uint64_t X : {(uint64_t)1, (uint64_t)5, bX - ox}) {
            if (oy >= bY || ox >= bX || ox + X > bX) continue;
            const sqy::WindowGeometry g{bY, bX, oz, oy, ox, Z, Y, X, Y * (X + 3) + 5, X + 3};
            std::vector<uint32_t> view((size_t)(Z * g.sz), 0xfffffffu), want(view);
            for (uint64_t z = 0; z < Z; ++z) for (uint64_t y = 0; y < Y; ++y) for (uint64_t x = 0; x < X; ++x)
                want[(size_t)(z * g.sz + y * g.sy + x)] = volume[(size_t)(((oz + z) * bY + oy + y) * bX + ox + x)];
            auto store = [&](uint64_t dst_off, uint32_t v) -> bool {
                if (dst_off >= view.size() || view[(size_t)dst_off] != 0xfffffffu) return false;      // inside the view, once
                view[(size_t)dst_off] = form == RangeForm::planes_lut ? v * 257u + 1u : v;
                return true;
            };
            sqy::WindowPiece piece;
            // block 0's tail voxels
            const uint64_t tail0 = p.v0 > p.L ? p.v0 : p.L;
            for (uint64_t t = 0; tail0 + t < p.v1; ++t) {
                CHECK(t < 256);
                sqy::WindowClip ct = sqy::window_clip_start(g, tail0 + t, 1);
                if (!sqy::window_clip_next(g, &ct, &piece)) continue;
                uint32_t v = 0;
                for (uint32_t i = 0; i < we; ++i) v |= (uint32_t)in.at((size_t)(p.tail + t * we + i)) << (8 * i);
                CHECK(piece.len == 1 && store(piece.dst_off, v));
                ++counts.tails;
            }
            // the grid's threads
            const uint64_t t0 = sqy::range_first_thread(p.w0, wpt), nt = sqy::range_thread_count(p.w0, p.w1, wpt);
            for (uint64_t t = t0; t < t0 + nt; ++t) {
                const sqy::RangeRun run = sqy::range_run(t, wpt, p.w0, p.w1);
                if (run.lo == run.hi) continue;
                if (run.lo > 0) ++counts.partial_first;
                if (run.hi < wpt) ++counts.partial_last;
                sqy::WindowClip c = sqy::window_clip_start(g, run.first * W, (uint64_t)run.hi * W);
                while (sqy::window_clip_next(g, &c, &piece)) {
                    CHECK(piece.len >= 1 && piece.run_off + piece.len <= (uint64_t)run.hi * W);
                    for (uint64_t k = 0; k < piece.len; ++k) {
                        const uint64_t i = piece.run_off + k, w = run.first + i / W, bit = W - 1 - i % W;
                        CHECK(i / W >= run.lo && i / W < run.hi && w >= p.w0 && w < p.w1);      // a voxel of the box lies in a word the thread owns
                        uint32_t v = 0;
                        for (uint32_t b = 0; b < W; ++b) {
                            uint32_t word = 0;
                            for (uint32_t j = 0; j < we; ++j) word |= (uint32_t)in.at((size_t)(p.plane[W - 1 - b] + (w - p.w0) * we + j)) << (8 * j);
                            v |= ((word >> bit) & 1u) << b;
                        }
                        CHECK(store(piece.dst_off + k, v));
                    }
                }
            }
            CHECK(view == want);
            ++counts.boxes;
        }
    }
    return 0;
}

int test_boxes()
{
    for (RangeForm form : {RangeForm::planes, RangeForm::planes_lut}) {
        // chunks of 64 and 48 bytes (no multiple of 16 words a segment, no power of two): ranges begin and end inside threads, segments
        // straddle chunks; (3, 8, 16): every frame 128 voxels, the runs whole; (2, 3, 300): rows longer than a run
        CHECK(box_blob(form, 5, 7, 9, 64) == 0);
        CHECK(box_blob(form, 5, 7, 9, 48) == 0);
        CHECK(box_blob(form, 4, 6, 10, 64) == 0);
        CHECK(box_blob(form, 7, 5, 22, 48) == 0);
        CHECK(box_blob(form, 3, 8, 16, 64) == 0);
        CHECK(box_blob(form, 2, 3, 300, 128) == 0);
        CHECK(box_blob(form, 6, 16, 24, 256) == 0);
    }
    return 0;
}

} // namespace

int main()
{
    if (test_path() || test_runs() || test_boxes()) return 1;
    std::printf("boxes %llu partial_first %llu partial_last %llu tails %llu straddles %llu\n", (unsigned long long)counts.boxes, (unsigned long long)counts.partial_first,
                (unsigned long long)counts.partial_last, (unsigned long long)counts.tails, (unsigned long long)counts.straddles);
    std::printf("decode_box ok\n");
    return 0;
}
