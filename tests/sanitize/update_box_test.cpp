// The box update of one large blob on the host (tests/test_host_update_box.py builds and runs this with g++, sanitizers on):
// sqy::update_box_path over every combination of its inputs against the rule written out here; sqy::pipelines_same_stages and
// sqy::update_box_form_ok on pipeline strings; and the splice plan's arithmetic (sqy::lz4_splice_plan, the functions the splice kernels
// compile) against frame layouts worked out by hand: stored and compressed replaced frames, the first and the last (short) frame
// replaced, a payload length that crosses a power of ten, an old frame outside its payload, a capacity one byte short.
// Prints "update_box ok" and returns 0.
#include "../../sqeazy_amd/csrc/sqy_pipeline.hpp"

#include <cstdio>
#include <string>
#include <vector>

#define CHECK(cond)                                                                   \
    do {                                                                              \
        if (!(cond)) { std::fprintf(stderr, "line %d: %s\n", __LINE__, #cond); return 1; } \
    } while (0)

using sqy::Lz4LayoutKind;
using sqy::UpdateBoxFacts;
using sqy::UpdateBoxPath;

namespace {

long n_subset = 0, n_whole = 0, n_stored = 0, n_compressed = 0, n_digits = 0;

int test_path()
{
    const Lz4LayoutKind kinds[] = {Lz4LayoutKind::chunked, Lz4LayoutKind::serial, Lz4LayoutKind::linked_chunks};
    for (int option = 0; option < 2; ++option)
        for (int same = 0; same < 2; ++same)
            for (int form = 0; form < 2; ++form)
                for (Lz4LayoutKind kind : kinds)
                    for (uint32_t accel : {1u, 2u, 3u})
                        for (uint64_t nchunks : {0ull, 1ull, 2ull, 7ull})
                            for (int taken = 0; taken < 2; ++taken)
                                for (uint64_t frames : {1ull, 2ull, 7ull})
                                    for (uint64_t blocks : {1ull, 2ull, 7ull, 14ull})
                                        for (uint64_t fchunk : {4096ull, 262144ull}) {
                                            UpdateBoxFacts f;
                                            f.option_on = option; f.same_stages = same; f.form_ok = form;
                                            f.layout.kind = kind; f.layout.accel = accel; f.layout.nchunks = nchunks; f.layout.chunk = 4096;
                                            f.subset_taken = taken; f.frames = frames; f.blocks = blocks; f.frame_chunk = fchunk;
                                            const bool want = option && same && form && kind == Lz4LayoutKind::chunked && accel == 1 && nchunks > 1 && taken &&
                                                              frames == nchunks && blocks == frames && fchunk == 4096;
                                            CHECK((sqy::update_box_path(f) == UpdateBoxPath::subset_patch) == want);
                                            ++(want ? n_subset : n_whole);
                                        }
    return 0;
}

int test_pipelines()
{
    auto P = [](const char* s, int e = 2) { return sqy::Pipeline::from_string(s, e); };
    CHECK(sqy::pipelines_same_stages(P("bitswap1->lz4"), P("bitswap1->lz4(accel=1,blocksize_kb=256,framestep_kb=256,n_chunks_of_input=0)")));
    CHECK(sqy::pipelines_same_stages(P("lz4(framestep_kb=4,blocksize_kb=4)"), P("lz4(blocksize_kb=4,framestep_kb=4)")));
    CHECK(!sqy::pipelines_same_stages(P("lz4"), P("bitswap1->lz4")));
    CHECK(!sqy::pipelines_same_stages(P("bitswap1->lz4"), P("bitswap1->lz4(blocksize_kb=4,framestep_kb=4)")));
    CHECK(!sqy::pipelines_same_stages(P("lz4"), P("lz4(accel=2)")));
    CHECK(!sqy::pipelines_same_stages(P("bitswap1->lz4"), P("diff3x3x1->bitswap1->lz4")));
    CHECK(!sqy::pipelines_same_stages(P("bitswap1->lz4"), P("bitswap1")));
    CHECK(sqy::update_box_form_ok(P("lz4")) && sqy::update_box_form_ok(P("bitswap1->lz4(framestep_kb=4)")));
    for (const char* s : {"quantiser->bitswap1->lz4", "frame_shuffle->lz4", "rmestbkrd->bitswap1->lz4", "diff3x3x1->bitswap1->lz4", "bitswap1", "diff3x3x1->lz4", "quantiser"})
        CHECK(!sqy::update_box_form_ok(P(s)));
    CHECK(!sqy::update_box_form_ok(sqy::Pipeline()));
    return 0;
}

// a blob of frames: old frames by (data offset, size field), the replaced ones by (csize, n); the plan against sums written out
int test_splice()
{
    const uint32_t OLD = sqy::kSpliceOldFrame, RAW = 0x80000000u;
    CHECK(sqy::kLz4FrameHead == 11 && sqy::kLz4FrameGap == 15);
    CHECK(sqy::decimal_digits(0) == 1 && sqy::decimal_digits(9) == 1 && sqy::decimal_digits(10) == 2 && sqy::decimal_digits(99999) == 5 && sqy::decimal_digits(100000) == 6 &&
          sqy::decimal_digits(~0ull) == 20);
    // the header: prefix 40, suffix 7, voxels of 2 bytes -- 40 + 4 + 7 = 51 -> 52; 40 + 5 + 7 = 52 -> 52; of 1 byte no padding
    CHECK(sqy::lz4_splice_header_bytes(40, 7, 9999, 2) == 52 && sqy::lz4_splice_header_bytes(40, 7, 10000, 2) == 52 && sqy::lz4_splice_header_bytes(40, 7, 100000, 2) == 54);
    CHECK(sqy::lz4_splice_header_bytes(40, 7, 9999, 1) == 51 && sqy::lz4_splice_header_bytes(40, 7, 10000, 1) == 52);
    // four old frames of a 4 KiB layout, the last one short (1000 bytes): compressed 100, stored 4096, compressed 3000, stored 1000
    const std::vector<uint32_t> old_size = {100, 4096 | RAW, 3000, 1000 | RAW};
    std::vector<uint64_t> old_off(4);
    uint64_t at = 0;
    for (int f = 0; f < 4; ++f) { old_off[f] = at + 11; at += 11 + (old_size[f] & ~RAW) + 4; }
    const uint64_t src_payload = at;
    CHECK(src_payload == 15 * 4 + 100 + 4096 + 3000 + 1000);
    struct Case { std::vector<uint32_t> slot_of, csize, n; std::vector<uint64_t> sizes; };
    const std::vector<Case> cases = {
        {{OLD, OLD, OLD, OLD}, {}, {}, {115, 4111, 3015, 1015}},                                      // nothing replaced: the old payload
        {{0, OLD, OLD, OLD}, {0}, {4096}, {4111, 4111, 3015, 1015}},                                  // the first frame, stored
        {{0, OLD, OLD, OLD}, {17}, {4096}, {32, 4111, 3015, 1015}},                                   // the first frame, compressed
        {{OLD, OLD, OLD, 0}, {0}, {1000}, {115, 4111, 3015, 1015}},                                   // the last, short frame, stored: its own n
        {{OLD, OLD, OLD, 0}, {999}, {1000}, {115, 4111, 3015, 1014}},                                 // .. compressed
        {{OLD, 0, 1, OLD}, {4000, 0}, {4096, 4096}, {115, 4015, 4111, 1015}},                         // the middle: one shrinks, one becomes stored
        {{0, 1, 2, 3}, {1, 2, 3, 4}, {4096, 4096, 4096, 1000}, {16, 17, 18, 19}},                      // all of them
    };
    for (const Case& c : cases) {
        const sqy::Lz4SplicePlan p = sqy::lz4_splice_plan(old_off, old_size, c.slot_of, c.csize, c.n, src_payload, 40, 7, 2, 1 << 20);
        CHECK(p.status == sqy::kSpliceDone && p.frame_off.size() == 5 && p.frame_off[0] == 0);
        uint64_t sum = 0;
        for (int f = 0; f < 4; ++f) { CHECK(p.frame_off[f] == sum); sum += c.sizes[f]; }
        CHECK(p.frame_off[4] == sum && p.payload == sum);
        CHECK(p.header_bytes == 40 + sqy::decimal_digits(sum) + 7 + (40 + sqy::decimal_digits(sum) + 7) % 2);
        for (size_t k = 0; k < c.csize.size(); ++k) ++(c.csize[k] ? n_compressed : n_stored);
        // the capacity: exactly the blob succeeds, one byte less does not and changes nothing else
        CHECK(sqy::lz4_splice_plan(old_off, old_size, c.slot_of, c.csize, c.n, src_payload, 40, 7, 2, p.header_bytes + sum).status == sqy::kSpliceDone);
        const sqy::Lz4SplicePlan q = sqy::lz4_splice_plan(old_off, old_size, c.slot_of, c.csize, c.n, src_payload, 40, 7, 2, p.header_bytes + sum - 1);
        CHECK(q.status == sqy::kSpliceNoRoom && q.payload == sum && q.header_bytes == p.header_bytes && q.frame_off == p.frame_off);
    }
    // the payload length crosses a power of ten: 8156 bytes besides the first frame's body, whose csize moves it from 9999 to 10000
    for (uint32_t cs : {1843u, 1844u, 1845u}) {
        const sqy::Lz4SplicePlan p = sqy::lz4_splice_plan(old_off, old_size, {0, OLD, OLD, OLD}, {cs}, {4096}, src_payload, 40, 7, 1, 1 << 20);
        const uint64_t payload = 15 + cs + 4111 + 3015 + 1015;
        CHECK(p.status == sqy::kSpliceDone && p.payload == payload);
        CHECK(p.header_bytes == (payload >= 10000 ? 52u : 51u));
        CHECK((payload >= 10000) == (cs >= 1844));
        ++n_digits;
    }
    // an int's worth of payload: the reference's limit
    CHECK(sqy::lz4_splice_status(52, 0x7fffffffull, ~0ull) == sqy::kSpliceDone && sqy::lz4_splice_status(52, 0x80000000ull, ~0ull) == sqy::kSplicePayloadTooLong);
    // old frames that do not lie inside the payload, slots out of order or out of range: refused
    CHECK(sqy::lz4_splice_plan(old_off, old_size, {OLD, OLD, OLD, OLD}, {}, {}, src_payload - 1, 40, 7, 2, 1 << 20).status == sqy::kSpliceBadIndex);
    {
        std::vector<uint64_t> off = old_off;
        off[0] = 10;                                                    // a frame head in front of the payload
        CHECK(sqy::lz4_splice_plan(off, old_size, {OLD, OLD, OLD, OLD}, {}, {}, src_payload, 40, 7, 2, 1 << 20).status == sqy::kSpliceBadIndex);
        CHECK(sqy::lz4_splice_plan(off, old_size, {0, OLD, OLD, OLD}, {5}, {4096}, src_payload, 40, 7, 2, 1 << 20).status == sqy::kSpliceDone);    // (replaced: not read)
    }
    CHECK(!sqy::lz4_splice_old_frame_ok(11, 0x7fffffffu, 100) && sqy::lz4_splice_old_frame_ok(11, 85, 100) && !sqy::lz4_splice_old_frame_ok(11, 86, 100) &&
          !sqy::lz4_splice_old_frame_ok(~0ull, 1, 100));
    CHECK(sqy::lz4_splice_ok({OLD, 0, 1, OLD}, 2) && sqy::lz4_splice_ok({OLD}, 0) && !sqy::lz4_splice_ok({}, 0) && !sqy::lz4_splice_ok({1, 0}, 2) &&
          !sqy::lz4_splice_ok({0, 0}, 1) && !sqy::lz4_splice_ok({0, OLD}, 2) && !sqy::lz4_splice_ok({0, 2}, 2) && !sqy::lz4_splice_ok({0}, 2));
    CHECK(sqy::lz4_splice_plan(old_off, old_size, {1, 0, OLD, OLD}, {1, 2}, {4096, 4096}, src_payload, 40, 7, 2, 1 << 20).status == sqy::kSpliceBadIndex);
    return 0;
}

} // namespace

int main()
{
    if (test_path() || test_pipelines() || test_splice()) return 1;
    std::printf("subset %ld whole %ld stored %ld compressed %ld digits %ld\n", n_subset, n_whole, n_stored, n_compressed, n_digits);
    std::printf("update_box ok\n");
    return 0;
}
