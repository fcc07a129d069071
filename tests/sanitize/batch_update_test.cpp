// The window update on the host (tests/test_host_batch_update.py builds and runs this with g++, sanitizers on).  The mask and the merge of
// csrc/sqy_batch_window.hpp -- the text the patch kernel compiles -- patch a window into the bit planes of a blob the way a thread of
// that kernel does, run of 128 voxels by run, and the result must be the bit-plane transpose of the pasted volume.  The transpose is
// restated here from the layout rule (plane W - 1 - b, word w, bit W - 1 - k = bit b of voxel W w + k; the voxels behind the last whole
// word verbatim) and tied to tests/golden/synth_u16_4x16x32 (argv[1]: the golden directory).  Every window of two small blobs, windows of
// (2, 3, 300) whose rows cross the runs, both voxel sizes.  Then sqy::update_batch_plan against a table written out by hand.
// Prints "batch_update ok" and returns 0.
#include "../../sqeazy_amd/csrc/sqy_batch_window.hpp"
#include "../../sqeazy_amd/csrc/sqy_kernels.h"
#include "../../sqeazy_amd/csrc/sqy_pipeline.hpp"

#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#define CHECK(cond)                                                                   \
    do {                                                                              \
        if (!(cond)) { std::fprintf(stderr, "line %d: %s\n", __LINE__, #cond); return 1; } \
    } while (0)

namespace {

// the plane stream of `len` voxels of `elem` bytes (voxels and plane words as the host stores them: little endian)
template <class T>
std::vector<T> planes_of(const std::vector<T>& vol)
{
    const uint64_t W = 8 * sizeof(T), len = vol.size(), seg = len / W, L = seg * W;
    std::vector<T> out(len, 0);
    for (uint64_t b = 0; b < W; ++b)
        for (uint64_t w = 0; w < seg; ++w) {
            unsigned word = 0;
            for (uint64_t k = 0; k < W; ++k) word |= ((unsigned)(vol[W * w + k] >> b) & 1u) << (W - 1 - k);
            out[(W - 1 - b) * seg + w] = (T)word;
        }
    for (uint64_t v = L; v < len; ++v) out[v] = vol[v];
    return out;
}

struct Box { uint64_t oz, oy, ox, Z, Y, X; };

// the window's new voxels in a pitched view (rows X + 3, frames Y (X + 3) + 5 voxels apart), a value that tells the place
template <class T>
std::vector<T> view_of(const Box& w, uint64_t* sz, uint64_t* sy)
{
    *sy = w.X + 3;
    *sz = w.Y * *sy + 5;
    std::vector<T> view((size_t)(w.Z * *sz), (T)0x5a);
    for (uint64_t z = 0; z < w.Z; ++z)
        for (uint64_t y = 0; y < w.Y; ++y)
            for (uint64_t x = 0; x < w.X; ++x) view[z * *sz + y * *sy + x] = (T)(0x9e37u * (z * 131 + y * 17 + x + 1) >> 3);
    return view;
}

// what a thread of bitswap1_batch_patch_kernel does for every run of the blob, with the header's clip, mask and merge
template <class T>
std::vector<T> patch_planes(const std::vector<T>& old_planes, uint64_t bY, uint64_t bX, const Box& w, const std::vector<T>& view, uint64_t sz, uint64_t sy,
                            uint64_t* runs_outside, uint64_t* runs_inside, uint64_t* runs_partly)
{
    const uint32_t W = 8 * sizeof(T), WPT = 128 / W;
    const uint64_t len = old_planes.size(), seg = len / W, L = seg * W;
    const sqy::WindowGeometry g{bY, bX, w.oz, w.oy, w.ox, w.Z, w.Y, w.X, sz, sy};
    std::vector<T> out(len, (T)0xee);
    sqy::WindowPiece cur;
    for (uint64_t v = L; v < len; ++v) {
        sqy::WindowClip ct = sqy::window_clip_start(g, v, 1);
        out[v] = sqy::window_clip_next(g, &ct, &cur) ? view[cur.dst_off] : old_planes[v];
    }
    for (uint64_t w0 = 0; w0 < seg; w0 += WPT) {
        const uint32_t nw = (uint32_t)(seg - w0 < WPT ? seg - w0 : WPT);
        sqy::WindowClip c = sqy::window_clip_start(g, w0 * W, (uint64_t)nw * W);
        uint32_t mask[4] = {0, 0, 0, 0}, inside = 0;
        T vox[128];
        std::memset(vox, 0, sizeof(vox));
        while (sqy::window_clip_next(g, &c, &cur)) {
            sqy::window_run_mask(W, (uint32_t)cur.run_off, (uint32_t)cur.len, mask);
            inside += (uint32_t)cur.len;
            for (uint64_t t = 0; t < cur.len; ++t) vox[cur.run_off + t] = view[cur.dst_off + t];
        }
        ++*(inside == 0 ? runs_outside : inside == nw * W ? runs_inside : runs_partly);
        for (uint32_t i = 0; i < nw; ++i) {
            const T m = (T)(mask[(i * W) >> 5] >> ((i * W) & 31u));
            for (uint32_t b = 0; b < W; ++b) {
                unsigned word = 0;
                for (uint32_t k = 0; k < W; ++k) word |= ((unsigned)(vox[W * i + k] >> b) & 1u) << (W - 1 - k);
                const uint64_t at = (uint64_t)(W - 1 - b) * seg + w0 + i;
                out[at] = sqy::window_merge_word<T>(old_planes[at], (T)word, m);
            }
        }
    }
    return out;
}

template <class T>
int one_window(const std::vector<T>& vol, const std::vector<T>& old_planes, uint64_t bY, uint64_t bX, const Box& w, uint64_t counts[3])
{
    uint64_t sz, sy;
    const std::vector<T> view = view_of<T>(w, &sz, &sy);
    std::vector<T> pasted = vol;
    for (uint64_t z = 0; z < w.Z; ++z)                                  // the plain triple loop
        for (uint64_t y = 0; y < w.Y; ++y)
            for (uint64_t x = 0; x < w.X; ++x) pasted[((w.oz + z) * bY + w.oy + y) * bX + w.ox + x] = view[z * sz + y * sy + x];
    const std::vector<T> got = patch_planes(old_planes, bY, bX, w, view, sz, sy, &counts[0], &counts[1], &counts[2]);
    CHECK(got == planes_of(pasted));
    return 0;
}

template <class T>
std::vector<T> blob_of(uint64_t len, unsigned salt)
{
    std::vector<T> vol((size_t)len);
    uint32_t s = 12345u + salt;
    for (T& v : vol) { s = s * 1664525u + 1013904223u; v = (T)(s >> 11); }
    return vol;
}

// every window of a blob of bZ x bY x bX voxels
template <class T>
int every_window(uint64_t bZ, uint64_t bY, uint64_t bX, uint64_t counts[3])
{
    const std::vector<T> vol = blob_of<T>(bZ * bY * bX, (unsigned)bX), old_planes = planes_of(vol);
    for (uint64_t oz = 0; oz < bZ; ++oz) for (uint64_t Z = 1; oz + Z <= bZ; ++Z)
    for (uint64_t oy = 0; oy < bY; ++oy) for (uint64_t Y = 1; oy + Y <= bY; ++Y)
    for (uint64_t ox = 0; ox < bX; ++ox) for (uint64_t X = 1; ox + X <= bX; ++X)
        if (one_window(vol, old_planes, bY, bX, Box{oz, oy, ox, Z, Y, X}, counts)) return 1;
    return 0;
}

// windows of (2, 3, 300) whose rows begin and end at, one in front of and one behind the borders of the runs of 128 voxels
template <class T>
int crossing_windows(uint64_t counts[3])
{
    const uint64_t bZ = 2, bY = 3, bX = 300;
    const std::vector<T> vol = blob_of<T>(bZ * bY * bX, 77), old_planes = planes_of(vol);
    const uint64_t edges[] = {0, 1, 27, 28, 29, 84, 127, 128, 129, 172, 212, 255, 256, 257, 299, 300};
    for (uint64_t oz = 0; oz < bZ; ++oz) for (uint64_t Z = 1; oz + Z <= bZ; ++Z)
    for (uint64_t oy = 0; oy < bY; ++oy) for (uint64_t Y = 1; oy + Y <= bY; ++Y)
    for (uint64_t a : edges) for (uint64_t b : edges)
        if (a < b && one_window(vol, old_planes, bY, bX, Box{oz, oy, a, Z, Y, b - a}, counts)) return 1;
    return 0;
}

bool read_file(const std::string& path, std::vector<uint16_t>* out)
{
    std::FILE* f = std::fopen(path.c_str(), "rb");
    if (!f) return false;
    std::vector<unsigned char> raw;
    unsigned char buf[4096];
    for (size_t n; (n = std::fread(buf, 1, sizeof buf, f)) > 0;) raw.insert(raw.end(), buf, buf + n);
    std::fclose(f);
    out->resize(raw.size() / 2);
    std::memcpy(out->data(), raw.data(), out->size() * 2);
    return raw.size() % 2 == 0;
}

// the restatement against the golden planes, and the golden planes patched
int test_golden(const std::string& dir)
{
    std::vector<uint16_t> vol, planes;
    CHECK(read_file(dir + "/synth_u16_4x16x32.in.bin", &vol) && read_file(dir + "/synth_u16_4x16x32.bitswap1.bin", &planes));
    CHECK(vol.size() == 4 * 16 * 32 && planes.size() == vol.size());
    CHECK(planes_of(vol) == planes);
    uint64_t counts[3] = {0, 0, 0};
    CHECK(one_window(vol, planes, 16, 32, Box{1, 3, 5, 2, 9, 20}, counts) == 0);
    CHECK(one_window(vol, planes, 16, 32, Box{0, 0, 0, 4, 16, 32}, counts) == 0);
    CHECK(one_window(vol, planes, 16, 32, Box{3, 15, 31, 1, 1, 1}, counts) == 0);
    CHECK(counts[0] && counts[1] && counts[2]);
    return 0;
}

int test_mask()
{
    // 16-bit voxels: voxel 0 is bit 15 of plane word 0, voxel 17 bit 14 of word 1 (the high half of m[0]), voxel 127 bit 0 of word 7
    uint32_t m[4] = {0, 0, 0, 0};
    sqy::window_run_mask(16, 0, 1, m);
    CHECK(m[0] == 0x8000u && !m[1] && !m[2] && !m[3]);
    sqy::window_run_mask(16, 17, 1, m);
    CHECK(m[0] == (0x8000u | 0x4000u << 16));
    sqy::window_run_mask(16, 127, 1, m);
    CHECK(m[3] == 0x0001u << 16);
    uint32_t all[4] = {0, 0, 0, 0};
    sqy::window_run_mask(16, 0, 128, all);
    CHECK(all[0] == ~0u && all[1] == ~0u && all[2] == ~0u && all[3] == ~0u);
    // 8-bit voxels: voxels 6 .. 9 are bits 1, 0 of byte 0 and bits 7, 6 of byte 1
    uint32_t b[4] = {0, 0, 0, 0};
    sqy::window_run_mask(8, 6, 4, b);
    CHECK(b[0] == (0x03u | 0xc0u << 8) && !b[1]);
    uint32_t e[4] = {0, 0, 0, 0};
    sqy::window_run_mask(8, 5, 0, e);
    CHECK(!e[0] && !e[1] && !e[2] && !e[3]);
    CHECK(sqy::window_merge_word<uint16_t>(0xffff, 0x0000, 0x00f0) == 0xff0f && sqy::window_merge_word<uint8_t>(0x00, 0xff, 0x81) == 0x81);
    CHECK(sqy::window_merge_word<uint32_t>(0x12345678u, 0xabcdef01u, 0xffff0000u) == 0xabcd5678u);
    return 0;
}

int test_plan()
{
    using sqy::EncodeBatchForm;
    using sqy::DecodeBatchForm;
    const std::vector<uint64_t> raw = {100, 256, 257, 70000};
    const std::vector<int32_t> group_of = {0, -1, 0, 1};
    sqy::UpdateBatchPlan u = sqy::update_batch_plan(raw, EncodeBatchForm::bitswap1_lz4, group_of, true);
    CHECK((u.keep_planes == std::vector<uint8_t>{1, 0, 1, 1}) && (u.place_at == std::vector<uint64_t>{0, 256, 512, 1024}) && u.bytes == 1024 + 70144);
    u = sqy::update_batch_plan(raw, EncodeBatchForm::bitswap1_lz4, group_of, false);
    CHECK((u.keep_planes == std::vector<uint8_t>{0, 0, 0, 0}) && (u.place_at == std::vector<uint64_t>{0, 256, 512, 1024}) && u.bytes == 71168);
    for (EncodeBatchForm f : {EncodeBatchForm::none, EncodeBatchForm::lz4, EncodeBatchForm::quantiser_bitswap1_lz4})
        CHECK((sqy::update_batch_plan(raw, f, group_of, true).keep_planes == std::vector<uint8_t>{0, 0, 0, 0}));
    CHECK((sqy::update_batch_plan(raw, EncodeBatchForm::bitswap1_lz4, {}, true).keep_planes == std::vector<uint8_t>{0, 0, 0, 0}));   // (no plan: no group)
    u = sqy::update_batch_plan({}, EncodeBatchForm::bitswap1_lz4, {}, true);
    CHECK(u.keep_planes.empty() && u.place_at.empty() && u.bytes == 0);
    // patched: asked, found as planes, kept on the joint path -- all three
    CHECK(sqy::update_blob_patched(true, DecodeBatchForm::planes, true));
    CHECK(!sqy::update_blob_patched(false, DecodeBatchForm::planes, true) && !sqy::update_blob_patched(true, DecodeBatchForm::planes, false));
    for (DecodeBatchForm f : {DecodeBatchForm::stages, DecodeBatchForm::plain, DecodeBatchForm::quantised, DecodeBatchForm::diff_planes, DecodeBatchForm::diff_plain})
        CHECK(!sqy::update_blob_patched(true, f, true));
    // the LZ4 output straight into the place: the option on and the planned form `plain`; a group: every member, and it has one
    CHECK(sqy::update_lz4_into_place(true, DecodeBatchForm::plain) && !sqy::update_lz4_into_place(false, DecodeBatchForm::plain));
    for (DecodeBatchForm f : {DecodeBatchForm::stages, DecodeBatchForm::planes, DecodeBatchForm::quantised, DecodeBatchForm::diff_planes, DecodeBatchForm::diff_plain})
        CHECK(!sqy::update_lz4_into_place(true, f));
    const std::vector<uint8_t> into = {1, 0, 1, 1};
    CHECK(sqy::update_group_into_places({0, 2, 3}, into) && sqy::update_group_into_places({3}, into));
    CHECK(!sqy::update_group_into_places({0, 1}, into) && !sqy::update_group_into_places({1}, into) && !sqy::update_group_into_places({}, into));
    // the patch launch's tables: the window launches' layout, the kernels' job struct
    CHECK(sizeof(sqy::BatchPatchJob) == sqy::kBatchPatchJobBytes && sqy::kBatchPatchJobBytes == sqy::kBatchWindowJobBytes);
    const sqy::BatchWindowLayout l = sqy::batch_window_layout(3);
    CHECK(l.tiles_at == 336 && l.total == 352);
    return 0;
}

} // namespace

int main(int argc, char** argv)
{
    if (argc < 2) { std::fprintf(stderr, "usage: batch_update_test <golden directory>\n"); return 2; }
    if (test_mask() || test_plan() || test_golden(argv[1])) return 1;
    uint64_t counts[3] = {0, 0, 0}, crossing[3] = {0, 0, 0};
    if (every_window<uint16_t>(3, 5, 7, counts) || every_window<uint8_t>(3, 5, 7, counts)) return 1;
    if (every_window<uint16_t>(2, 3, 9, counts) || every_window<uint8_t>(2, 3, 9, counts)) return 1;
    if (crossing_windows<uint16_t>(crossing) || crossing_windows<uint8_t>(crossing)) return 1;
    CHECK(counts[2] && crossing[0] && crossing[1] && crossing[2]);      // runs outside, inside and partly inside were all seen
    std::printf("runs outside %llu inside %llu partly %llu\n", (unsigned long long)(counts[0] + crossing[0]), (unsigned long long)(counts[1] + crossing[1]),
                (unsigned long long)(counts[2] + crossing[2]));
    std::printf("batch_update ok\n");
    return 0;
}
