// Many boxes of one blob on the host (tests/test_host_decode_boxes.py builds and runs this with g++, sanitizers on): sqy::decode_boxes_path
// against its table; sqy::frame_ranges_plan -- the LZ4 frames of several z-ranges united -- against sqy::frame_range_plan of every range
// on its own, for every form, over all pairs and triples of z-ranges of small streams (disjoint, touching, nested, identical): the ids are
// the union, and every range reads the same bytes out of the union's compaction as out of its own; and the workgroup -> job mapping of
// bitswap1_decode_range_windows_kernel, walked over first_tile as the kernel walks it, with sqy::range_run per job: every word of every
// job exactly once; and the pure helpers every boxes driver shares (a box's range for the transposers, a window in its own frames, the
// outputs' offsets table, the smallest shape that holds a box).  Prints "decode_boxes ok" and returns 0.
#include "../../sqeazy_amd/csrc/sqy_batch_window.hpp"
#include "../../sqeazy_amd/csrc/sqy_pipeline.hpp"

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <set>
#include <vector>

#define CHECK(cond)                                                                   \
    do {                                                                              \
        if (!(cond)) { std::fprintf(stderr, "line %d: %s\n", __LINE__, #cond); return 1; } \
    } while (0)

using sqy::BoxesPath;
using sqy::RangeForm;
typedef std::pair<uint64_t, uint64_t> Range;

namespace {

struct Counts { uint64_t sets = 0, gaps = 0, shared = 0, tails = 0, struck = 0, zero_runs = 0, groups = 0; } counts;

int test_path()
{
    const struct { RangeForm form; BoxesPath on; } table[] = {{RangeForm::plain, BoxesPath::subset_copy}, {RangeForm::planes, BoxesPath::subset_transposer},
                                                              {RangeForm::planes_lut, BoxesPath::subset_transposer}, {RangeForm::shuffle, BoxesPath::subset_copy}};
    for (const auto& row : table) {
        CHECK(sqy::decode_boxes_path(true, row.form, true, true) == row.on);
        CHECK(sqy::decode_boxes_path(true, row.form, false, true) == BoxesPath::whole_copy);      // decode_box_subset off
        CHECK(sqy::decode_boxes_path(false, row.form, true, true) == BoxesPath::whole_copy);      // a blob the frame-range plan does not take
        CHECK(sqy::decode_boxes_path(false, row.form, false, true) == BoxesPath::whole_copy);
        for (int subset_form = 0; subset_form < 2; ++subset_form)
            for (int subset = 0; subset < 2; ++subset) CHECK(sqy::decode_boxes_path(subset_form, row.form, subset, false) == BoxesPath::box_by_box);
    }
    return 0;
}

bool same_plan(const sqy::FrameRangePlan& a, const sqy::FrameRangePlan& b)
{
    return a.ok == b.ok && a.ids == b.ids && a.out_bytes == b.out_bytes && a.range_at == b.range_at && a.coff == b.coff && std::equal(a.plane, a.plane + 16, b.plane) &&
           a.tail == b.tail && a.v0 == b.v0 && a.v1 == b.v1 && a.w0 == b.w0 && a.w1 == b.w1 && a.L == b.L && a.we == b.we && a.remap == b.remap && a.pa == b.pa &&
           a.pb == b.pb && a.direct == b.direct && a.zero_runs == b.zero_runs;
}

std::vector<uint8_t> synthetic(uint64_t total)
{
    std::vector<uint8_t> s(total);
    for (uint64_t i = 0; i < total; ++i) s[i] = (uint8_t)(((i + 1) * 2654435761u) >> 11);
    return s;
}

// the chunks of `ids` back to back: what the pruned LZ4 decode leaves (plain, planes)
std::vector<uint8_t> compaction(const std::vector<uint8_t>& stream, const std::vector<uint32_t>& ids, uint64_t chunk)
{
    std::vector<uint8_t> out;
    for (uint32_t f : ids) out.insert(out.end(), stream.begin() + (size_t)(f * chunk), stream.begin() + (size_t)std::min<uint64_t>((f + 1) * chunk, stream.size()));
    return out;
}

bool same_bytes(const std::vector<uint8_t>& a, uint64_t a_at, const std::vector<uint8_t>& b, uint64_t b_at, uint64_t len)
{
    return a_at + len <= a.size() && b_at + len <= b.size() && (len == 0 || std::memcmp(a.data() + a_at, b.data() + b_at, (size_t)len) == 0);
}

std::vector<Range> all_ranges(uint64_t shape0)
{
    std::vector<Range> r;
    for (uint64_t z0 = 0; z0 < shape0; ++z0) for (uint64_t nz = 1; z0 + nz <= shape0; ++nz) r.push_back({z0, nz});
    return r;
}

// the kernel's grid over the jobs (w0, w1): workgroup -> job by the binary search over first_tile, range_run per thread; every word of
// every job exactly once, no thread of a job outside its words
int walk_groups(const std::vector<Range>& words, uint32_t wpt)
{
    const uint32_t njobs = (uint32_t)words.size();
    std::vector<uint32_t> first_tile;
    uint32_t ntiles = 0;
    for (const Range& w : words) { first_tile.push_back(ntiles); ntiles += (uint32_t)sqy::range_job_groups(w.first, w.second, wpt); }
    first_tile.push_back(ntiles);
    std::vector<std::vector<uint8_t>> seen(njobs);
    for (uint32_t j = 0; j < njobs; ++j) seen[j].assign((size_t)(words[j].second - words[j].first), 0);
    std::vector<uint32_t> first_groups(njobs, 0);
    for (uint32_t group = 0; group < ntiles; ++group) {
        const uint32_t j = sqy::range_job_of_group(first_tile.data(), njobs, group);
        CHECK(j < njobs && first_tile[j] <= group && group < first_tile[j + 1]);
        const uint32_t own = group - first_tile[j];
        if (own == 0) ++first_groups[j];                              // (the workgroup that moves the job's tail)
        const uint64_t w0 = words[j].first, w1 = words[j].second, t0 = sqy::range_first_thread(w0, wpt);
        for (uint32_t tid = 0; tid < 256; ++tid) {
            const sqy::RangeRun run = sqy::range_run(t0 + (uint64_t)own * 256u + tid, wpt, w0, w1);
            CHECK(run.lo <= run.hi && run.hi <= wpt);
            for (uint32_t i = run.lo; i < run.hi; ++i) {
                const uint64_t w = run.first + i;
                CHECK(w >= w0 && w < w1 && seen[j][(size_t)(w - w0)] == 0);
                seen[j][(size_t)(w - w0)] = 1;
            }
        }
        ++counts.groups;
    }
    for (uint32_t j = 0; j < njobs; ++j) {
        CHECK(first_groups[j] == 1);                                   // every job has a first workgroup, a job without words too
        CHECK(std::count(seen[j].begin(), seen[j].end(), 1) == (long)seen[j].size());
    }
    return 0;
}

int check_set(RangeForm form, uint64_t n, int elem, uint64_t shape0, uint64_t chunk, const std::vector<uint8_t>& stream, const std::vector<Range>& set,
              const std::vector<sqy::FrameRangePlan>& single, const std::vector<std::vector<uint8_t>>& single_in, const std::vector<size_t>& which)
{
    const uint64_t total = stream.size();
    const uint32_t nframes = (uint32_t)((total + chunk - 1) / chunk);
    const sqy::FrameRangesPlan u = sqy::frame_ranges_plan(form, n, elem, shape0, set, chunk, total, nframes);
    CHECK(u.ok && u.boxes.size() == set.size());
    // the ids: ascending, unique, the union of the single plans'
    std::set<uint32_t> want;
    for (size_t k : which) want.insert(single[k].ids.begin(), single[k].ids.end());
    CHECK(std::vector<uint32_t>(want.begin(), want.end()) == u.ids);
    for (size_t i = 1; i < u.ids.size(); ++i) { CHECK(u.ids[i - 1] < u.ids[i]); if (u.ids[i] != u.ids[i - 1] + 1) ++counts.gaps; }
    const std::vector<uint8_t> in = compaction(stream, u.ids, chunk);
    CHECK(in.size() == u.out_bytes);
    for (uint32_t f : u.ids) CHECK(same_bytes(in, u.coff[f], stream, f * chunk, std::min<uint64_t>(chunk, total - f * chunk)));
    uint64_t single_sum = 0;
    const uint64_t we = (uint64_t)u.we, W = 8 * we;
    for (size_t i = 0; i < set.size(); ++i) {
        const sqy::FrameRangePlan& s = single[which[i]];
        const sqy::FrameRangesBox& b = u.boxes[i];
        const std::vector<uint8_t>& own = single_in[which[i]];
        single_sum += s.ids.size();
        CHECK(s.we == u.we && b.v0 == s.v0 && b.v1 == s.v1 && b.w0 == s.w0 && b.w1 == s.w1 && b.L == s.L);
        if (form == RangeForm::plain) {
            CHECK(same_bytes(in, b.range_at, own, s.range_at, (b.v1 - b.v0) * (uint64_t)elem));
            CHECK(same_bytes(in, b.range_at, stream, b.v0 * (uint64_t)elem, (b.v1 - b.v0) * (uint64_t)elem));
        } else {
            const uint64_t seg = n / W;
            for (uint64_t p = 0; p < W && b.w0 < b.w1; ++p) {
                CHECK(same_bytes(in, b.plane[p], own, s.plane[p], (b.w1 - b.w0) * we));
                CHECK(same_bytes(in, b.plane[p], stream, (p * seg + b.w0) * we, (b.w1 - b.w0) * we));
            }
            if (b.v1 > b.L) {
                const uint64_t tail0 = std::max(b.v0, b.L);
                CHECK(same_bytes(in, b.tail, own, s.tail, (b.v1 - tail0) * we));
                CHECK(same_bytes(in, b.tail, stream, tail0 * we, (b.v1 - tail0) * we));
                ++counts.tails;
            }
        }
    }
    if (single_sum > u.ids.size()) ++counts.shared;                    // a frame that two ranges need is there once
    if (form != RangeForm::plain) {
        std::vector<Range> words;
        for (const auto& b : u.boxes) words.push_back({b.w0, b.w1});
        CHECK(walk_groups(words, (uint32_t)(128 / W)) == 0);
    }
    ++counts.sets;
    return 0;
}

int test_union(RangeForm form, int elem, uint64_t shape0, uint64_t frame_voxels, uint64_t chunk)
{
    const uint64_t n = shape0 * frame_voxels, total = n * (uint64_t)(form == RangeForm::planes_lut ? 1 : elem);
    const uint32_t nframes = (uint32_t)((total + chunk - 1) / chunk);
    const std::vector<uint8_t> stream = synthetic(total);
    const std::vector<Range> ranges = all_ranges(shape0);
    std::vector<sqy::FrameRangePlan> single;
    std::vector<std::vector<uint8_t>> single_in;
    for (const Range& r : ranges) {
        single.push_back(sqy::frame_range_plan(form, n, elem, shape0, r.first, r.second, chunk, total, nframes));
        CHECK(single.back().ok);
        single_in.push_back(compaction(stream, single.back().ids, chunk));
        CHECK(single_in.back().size() == single.back().out_bytes);
        // one range: frame_range_plan's result, field for field
        const sqy::FrameRangesPlan u = sqy::frame_ranges_plan(form, n, elem, shape0, {r}, chunk, total, nframes);
        CHECK(same_plan(sqy::frame_range_plan_of(u, 0), single.back()) && u.ids == single.back().ids && u.out_bytes == single.back().out_bytes);
    }
    const size_t R = ranges.size();
    for (size_t a = 0; a < R; ++a)
        for (size_t b = 0; b < R; ++b) {
            CHECK(check_set(form, n, elem, shape0, chunk, stream, {ranges[a], ranges[b]}, single, single_in, {a, b}) == 0);
            for (size_t c = (a + b) % 3; c < R; c += 3)                 // (a third of the triples: every kind is among them)
                CHECK(check_set(form, n, elem, shape0, chunk, stream, {ranges[a], ranges[b], ranges[c]}, single, single_in, {a, b, c}) == 0);
        }
    // ranges that name no range of the stream: nothing is planned
    CHECK(!sqy::frame_ranges_plan(form, n, elem, shape0, {}, chunk, total, nframes).ok);
    CHECK(!sqy::frame_ranges_plan(form, n, elem, shape0, {{0, 1}, {shape0, 1}}, chunk, total, nframes).ok);
    CHECK(!sqy::frame_ranges_plan(form, n, elem, shape0, {{0, 1}, {1, shape0}}, chunk, total, nframes).ok);
    CHECK(!sqy::frame_ranges_plan(form, n, elem, shape0, {{0, 0}}, chunk, total, nframes).ok);
    CHECK(!sqy::frame_ranges_plan(form, n, elem, shape0, {{~0ull, 2}}, chunk, total, nframes).ok);
    return 0;
}

// frame_shuffle->lz4: 6 places of 64 bytes in chunks of 32, 12 frames of 32 one-byte voxels (two to a place); the map names place 4 twice
// (the earlier slot is struck) and place 1 not at all (it decodes to zeros)
int test_shuffle()
{
    const uint64_t places = 6, place_bytes = 64, chunk = 32, shape0 = 12, n = places * place_bytes, total = n, fb = n / shape0;
    const uint32_t nframes = (uint32_t)(total / chunk);
    const uint64_t raw_map[6] = {2, 4, 0, 5, 4, 3};
    std::vector<unsigned char> map(places * 8);
    std::memcpy(map.data(), raw_map, sizeof raw_map);
    std::vector<uint64_t> unnamed;
    bool permutation = true;
    CHECK(sqy::frame_shuffle_decode_map(&map, places, &unnamed, &permutation) && !permutation && unnamed == std::vector<uint64_t>{1});
    const std::vector<uint8_t> stream = synthetic(total);              // the sorted stream: slot i at i place_bytes
    std::vector<uint8_t> volume(n, 0);                                 // what the full decode gives
    for (uint64_t i = 0; i < places; ++i) {
        uint64_t v;
        std::memcpy(&v, map.data() + 8 * i, 8);
        if (v == ~0ull) { ++counts.struck; continue; }
        std::copy(stream.begin() + (size_t)(i * place_bytes), stream.begin() + (size_t)((i + 1) * place_bytes), volume.begin() + (size_t)(v * place_bytes));
    }
    // what the subset decode leaves for a plan: the zero runs cleared, subset frame k at remap[k chunk / place_bytes] place_bytes + the rest
    auto decoded = [&](const std::vector<uint32_t>& ids, const std::vector<uint64_t>& remap, const std::vector<Range>& zero_runs, uint64_t out_bytes,
                       std::vector<uint8_t>* out) -> bool {
        out->assign((size_t)out_bytes, 0xEE);
        std::vector<char> written((size_t)out_bytes, 0);
        for (const Range& z : zero_runs) {
            if (z.second * place_bytes > out_bytes || z.first >= z.second) return false;
            std::fill(out->begin() + (size_t)(z.first * place_bytes), out->begin() + (size_t)(z.second * place_bytes), 0);
            std::fill(written.begin() + (size_t)(z.first * place_bytes), written.begin() + (size_t)(z.second * place_bytes), 1);
            ++counts.zero_runs;
        }
        for (size_t k = 0; k < ids.size(); ++k) {
            const uint64_t o = k * chunk;
            if (o / place_bytes >= remap.size() || (ids[k] + 1) * chunk > total) return false;
            const uint64_t at = remap[(size_t)(o / place_bytes)] * place_bytes + o % place_bytes;
            if (at + chunk > out_bytes) return false;
            for (uint64_t i = 0; i < chunk; ++i) {
                if (written[(size_t)(at + i)]++) return false;         // no byte is written twice
                (*out)[(size_t)(at + i)] = stream[(size_t)(ids[k] * chunk + i)];
            }
        }
        return std::count(written.begin(), written.end(), 1) == (long)out_bytes;                  // .. and every byte once: decoded or cleared
    };
    const std::vector<Range> ranges = all_ranges(shape0);
    std::vector<sqy::FrameRangePlan> single;
    for (const Range& r : ranges) {
        single.push_back(sqy::frame_range_plan(RangeForm::shuffle, n, 1, shape0, r.first, r.second, chunk, total, nframes, map, place_bytes, places));
        CHECK(single.back().ok);
        const sqy::FrameRangesPlan u = sqy::frame_ranges_plan(RangeForm::shuffle, n, 1, shape0, {r}, chunk, total, nframes, map, place_bytes, places);
        CHECK(same_plan(sqy::frame_range_plan_of(u, 0), single.back()));
    }
    const size_t R = ranges.size();
    for (size_t a = 0; a < R; ++a)
        for (size_t b = 0; b < R; ++b)
            for (size_t c = (a + b) % 5; c <= R; c += 5) {              // c == R: the pair alone
                std::vector<Range> set = {ranges[a], ranges[b]};
                std::vector<size_t> which = {a, b};
                if (c < R) { set.push_back(ranges[c]); which.push_back(c); }
                const sqy::FrameRangesPlan u = sqy::frame_ranges_plan(RangeForm::shuffle, n, 1, shape0, set, chunk, total, nframes, map, place_bytes, places);
                CHECK(u.ok && u.boxes.size() == set.size());
                std::set<uint32_t> want;
                for (size_t k : which) want.insert(single[k].ids.begin(), single[k].ids.end());
                CHECK(std::vector<uint32_t>(want.begin(), want.end()) == u.ids);      // (slot order is ascending frame order)
                std::vector<uint8_t> in, own;
                CHECK(decoded(u.ids, u.remap, u.zero_runs, u.out_bytes, &in));
                for (size_t i = 0; i < set.size(); ++i) {
                    const sqy::FrameRangePlan& s = single[which[i]];
                    CHECK(decoded(s.ids, s.remap, s.zero_runs, s.out_bytes, &own));
                    const uint64_t len = set[i].second * fb;
                    CHECK(u.boxes[i].pa == s.pa && u.boxes[i].pb == s.pb);
                    CHECK(same_bytes(in, u.boxes[i].range_at, own, s.range_at, len));
                    CHECK(same_bytes(in, u.boxes[i].range_at, volume, set[i].first * fb, len));
                }
                ++counts.sets;
            }
    return 0;
}

int test_groups()
{
    // jobs of several workgroups, of one, of none of their own words; first and last threads that own a part of their words
    for (uint32_t wpt : {8u, 16u}) {
        CHECK(walk_groups({{0, 256u * wpt}}, wpt) == 0);
        CHECK(walk_groups({{3, 3}, {5, 256u * wpt * 2 + 9}, {7, 7}, {256u * wpt - 1, 256u * wpt + 1}, {0, 1}}, wpt) == 0);
        CHECK(walk_groups({{wpt * 700 + 3, wpt * 700 + 3 + 256u * wpt * 3}, {wpt * 700 + 3, wpt * 700 + 3 + 256u * wpt * 3}, {11, 4000}}, wpt) == 0);
        CHECK(walk_groups({{5, 5}}, wpt) == 0);
    }
    return 0;
}

// the fields of sqy::Bitswap1Range (sqy_kernels.h, which this program does not need): what sqy::bitswap1_range_of fills
struct PlaneRange { uint64_t plane[16]; uint64_t tail; uint64_t w0, w1, v0, v1, L; };

// the pure helpers of the boxes drivers (sqy_pipeline.hpp)
int test_driver_helpers()
{
    // a box's range: every value to the field of its name, nothing else of the box
    sqy::FrameRangesBox b;
    for (int s = 0; s < 16; ++s) b.plane[s] = 1000 + 7 * (uint64_t)s;
    b.range_at = 1; b.tail = 2; b.v0 = 3; b.v1 = 4; b.w0 = 5; b.w1 = 6; b.L = 7; b.pa = 8; b.pb = 9; b.direct = true;
    const PlaneRange r = sqy::bitswap1_range_of<PlaneRange>(b);
    for (int s = 0; s < 16; ++s) CHECK(r.plane[s] == 1000 + 7 * (uint64_t)s);
    CHECK(r.tail == 2 && r.v0 == 3 && r.v1 == 4 && r.w0 == 5 && r.w1 == 6 && r.L == 7);

    // a window in its own frames, ranks 1 to 3: every voxel lies where it lay in the blob, less the frames in front of the window
    const std::vector<uint64_t> shapes[3] = {{40}, {9, 11}, {5, 6, 7}};
    const long origins[3][3] = {{13}, {4, 3}, {2, 1, 3}}, extents[3][3] = {{20}, {5, 7}, {3, 4, 2}};
    for (unsigned rank = 1; rank <= 3; ++rank) {
        sqy::BatchWindow w;
        CHECK(sqy::admit_window(shapes[rank - 1], origins[rank - 1], extents[rank - 1], rank, &w));
        uint64_t frame = 1;
        for (unsigned k = 1; k < rank; ++k) frame *= shapes[rank - 1][k];
        const uint64_t in_front = (uint64_t)origins[rank - 1][0] * frame, own = (uint64_t)extents[rank - 1][0] * frame;
        const sqy::BatchWindow f = sqy::window_in_own_frames(w, rank);
        CHECK(f.Z == w.Z && f.Y == w.Y && f.X == w.X && f.bZ * f.bY * f.bX == own);
        for (uint64_t z = 0; z < w.Z; ++z)
            for (uint64_t y = 0; y < w.Y; ++y)
                for (uint64_t x = 0; x < w.X; ++x) {
                    const uint64_t in_blob = ((w.oz + z) * w.bY + w.oy + y) * w.bX + w.ox + x, in_frames = ((f.oz + z) * f.bY + f.oy + y) * f.bX + f.ox + x;
                    CHECK(in_blob >= in_front && in_frames == in_blob - in_front && in_frames < own);
                }
        const sqy::WindowGeometry g = sqy::window_geometry(f, 77, 5);
        CHECK(g.bY == f.bY && g.bX == f.bX && g.oz == f.oz && g.oy == f.oy && g.ox == f.ox && g.Z == f.Z && g.Y == f.Y && g.X == f.X && g.sz == 77 && g.sy == 5);
    }

    // the outputs' offsets: prefix sums; a total that exceeds the capacity by one byte is refused, the same total fits; no room below 0
    std::vector<uint64_t> at;
    CHECK(sqy::output_offsets({3, 0, 5}, 8, &at) && at == (std::vector<uint64_t>{0, 3, 3, 8}));
    CHECK(!sqy::output_offsets({3, 0, 5}, 7, &at) && at.back() == 8);
    CHECK(!sqy::output_offsets({1}, 0, &at) && !sqy::output_offsets({1}, -1, &at) && !sqy::output_offsets({1}, -0x7fffffffffffffffl - 1, &at));
    CHECK(sqy::output_offsets({}, -1, &at) && at == std::vector<uint64_t>{0});
    CHECK(sqy::output_offsets({0x7fffffffffffffffull}, 0x7fffffffffffffffl, &at) && !sqy::output_offsets({0x7fffffffffffffffull, 1}, 0x7fffffffffffffffl, &at));

    // the smallest shape that holds a box: origin + extent; an extent below 1 adds nothing (and no admission takes the box); no wrap
    const long o[3] = {2, 0, 5}, e[3] = {3, -4, 1}, good[3] = {3, 4, 1}, far[1] = {0x7fffffffffffffffl};
    CHECK(sqy::smallest_holding_shape(o, e, 3) == (std::vector<uint64_t>{5, 0, 6}));
    CHECK(sqy::smallest_holding_shape(far, far, 1) == std::vector<uint64_t>{0xfffffffffffffffeull});
    sqy::BatchWindow w;
    CHECK(!sqy::admit_window(sqy::smallest_holding_shape(o, e, 3), o, e, 3, &w));
    CHECK(sqy::admit_window(sqy::smallest_holding_shape(o, good, 3), o, good, 3, &w) && w.bZ == 5 && w.bY == 4 && w.bX == 6 && w.oz + w.Z == w.bZ && w.ox + w.X == w.bX);
    return 0;
}

} // namespace

int main()
{
    if (test_path() || test_groups() || test_shuffle() || test_driver_helpers()) return 1;
    // n = 7 * 33 * 31 in chunks of 4096: tails of 9 voxels (16-bit planes) and of 1 (8-bit planes); 6 * 384 voxels in chunks of 256: no tail,
    // many frames between two ranges' words; 5 * 63 in chunks of 48: plane segments that straddle chunks
    const struct { uint64_t shape0, frame_voxels, chunk; } streams[] = {{7, 33 * 31, 4096}, {6, 16 * 24, 256}, {5, 7 * 9, 48}};
    for (const auto& s : streams) {
        if (test_union(RangeForm::plain, 2, s.shape0, s.frame_voxels, s.chunk) || test_union(RangeForm::plain, 1, s.shape0, s.frame_voxels, s.chunk) ||
            test_union(RangeForm::planes, 2, s.shape0, s.frame_voxels, s.chunk) || test_union(RangeForm::planes, 1, s.shape0, s.frame_voxels, s.chunk) ||
            test_union(RangeForm::planes_lut, 2, s.shape0, s.frame_voxels, s.chunk))
            return 1;
    }
    std::printf("sets %llu gaps %llu shared %llu tails %llu struck %llu zero_runs %llu groups %llu\n", (unsigned long long)counts.sets, (unsigned long long)counts.gaps,
                (unsigned long long)counts.shared, (unsigned long long)counts.tails, (unsigned long long)counts.struck, (unsigned long long)counts.zero_runs,
                (unsigned long long)counts.groups);
    std::printf("decode_boxes ok\n");
    return 0;
}
