// The plan of SQYAMD_Update_Boxes_* on the host (tests/test_host_update_boxes.py builds and runs this with g++, sanitizers on):
// sqy::update_boxes_plan over small shapes and box sets -- every pair of z-ranges where the shape is small, random sets of up to six
// boxes otherwise -- held against what is written out here by brute force:
//   the invariant: no plane word, no tail voxel and no byte of the stream in front of lz4 belongs to two segments;
//   the segments are ascending and neither overlap nor abut; every box lies inside its segment and in no other; the box lists ascend;
//   the segments are the connected components of "overlap or abut, or (planes) the word intervals intersect" (union-find over the boxes);
//   the layers are runs of consecutive boxes, pairwise voxel-disjoint (voxel by voxel), and each one but the first begins with a box
//   that shares a voxel with the layer in front, so a box never moves in front of an earlier box it overlaps;
//   the LZ4 frames of the segments united equal the union of sqy::frame_range_plan's frames of each segment's hull.
// Prints the situations it met (their counts must all be above zero) and "update_boxes ok", and returns 0.
#include "../../sqeazy_amd/csrc/sqy_pipeline.hpp"

#include <algorithm>
#include <cstdio>
#include <numeric>
#include <random>
#include <set>
#include <vector>

#define CHECK(cond)                                                                   \
    do {                                                                              \
        if (!(cond)) { std::fprintf(stderr, "line %d: %s\n", __LINE__, #cond); return 1; } \
    } while (0)

using sqy::BatchWindow;
using sqy::RangeForm;
typedef std::vector<std::pair<uint64_t, uint64_t>> Ranges;

namespace {

unsigned long long n_overlap = 0, n_word = 0, n_tail = 0, n_layers = 0, n_plans = 0;

struct Shape { uint64_t Z, Y, X; };

int find(std::vector<int>& up, int i) { return up[i] == i ? i : up[i] = find(up, up[i]); }

int check(RangeForm form, const Shape& sh, int elem, uint64_t chunk, const std::vector<BatchWindow>& ws)
{
    const uint64_t n = sh.Z * sh.Y * sh.X, vpf = sh.Y * sh.X, e = (uint64_t)elem, W = 8 * e, seg = n / W, L = seg * W, total = n * e;
    const bool planes = form == RangeForm::planes;
    const size_t K = ws.size();
    Ranges ranges(K);
    for (size_t i = 0; i < K; ++i) ranges[i] = {ws[i].oz, ws[i].Z};
    const sqy::UpdateBoxesPlan p = sqy::update_boxes_plan(form, n, elem, sh.Z, ranges, ws);
    CHECK(p.ok && !p.segments.empty());
    ++n_plans;
    n_overlap += p.merged_overlap; n_word += p.merged_word; n_tail += p.merged_tail;
    CHECK(p.merged_overlap + p.merged_word + p.merged_tail + p.segments.size() == K);
    // ascending, apart; every box in exactly one segment, inside it; the lists ascend
    std::vector<int> seg_of(K, -1);
    for (size_t s = 0; s < p.segments.size(); ++s) {
        const sqy::UpdateBoxesSegment& sg = p.segments[s];
        CHECK(sg.nz >= 1 && sg.z0 + sg.nz <= sh.Z && !sg.boxes.empty());
        if (s) CHECK(p.segments[s - 1].z0 + p.segments[s - 1].nz < sg.z0);
        uint64_t lo = ~0ull, hi = 0;
        for (size_t k = 0; k < sg.boxes.size(); ++k) {
            const uint32_t i = sg.boxes[k];
            CHECK(i < K && seg_of[i] == -1);
            if (k) CHECK(sg.boxes[k - 1] < i);
            seg_of[i] = (int)s;
            CHECK(ranges[i].first >= sg.z0 && ranges[i].first + ranges[i].second <= sg.z0 + sg.nz);
            lo = std::min(lo, ranges[i].first); hi = std::max(hi, ranges[i].first + ranges[i].second);
        }
        CHECK(lo == sg.z0 && hi == sg.z0 + sg.nz);                       // the hull, no more
    }
    for (size_t i = 0; i < K; ++i) CHECK(seg_of[i] >= 0);
    // the invariant, by brute force: an owner per word, per tail voxel, per stream byte
    std::vector<int> word(seg + 1, -1), tail(n + 1, -1), byte(total + 1, -1);
    auto own = [](std::vector<int>& owner, uint64_t at, int s) { if (owner[at] != -1 && owner[at] != s) return false; owner[at] = s; return true; };
    for (size_t s = 0; s < p.segments.size(); ++s) {
        const uint64_t v0 = p.segments[s].z0 * vpf, v1 = (p.segments[s].z0 + p.segments[s].nz) * vpf;
        if (!planes) {
            for (uint64_t b = v0 * e; b < v1 * e; ++b) CHECK(own(byte, b, (int)s));
            continue;
        }
        for (uint64_t v = v0; v < v1; ++v) {
            if (v >= L) {
                CHECK(own(tail, v, (int)s));
                for (uint64_t b = 0; b < e; ++b) CHECK(own(byte, v * e + b, (int)s));
            } else {
                CHECK(own(word, v / W, (int)s));
                for (uint64_t pl = 0; pl < W; ++pl) for (uint64_t b = 0; b < e; ++b) CHECK(own(byte, (pl * seg + v / W) * e + b, (int)s));
            }
        }
    }
    // the segments are the connected components of the merge relation
    std::vector<int> up(K);
    std::iota(up.begin(), up.end(), 0);
    for (size_t i = 0; i < K; ++i)
        for (size_t j = i + 1; j < K; ++j) {
            const uint64_t a0 = ranges[i].first, a1 = a0 + ranges[i].second, b0 = ranges[j].first, b1 = b0 + ranges[j].second;
            bool join = a0 <= b1 && b0 <= a1;                            // overlap or abut
            if (planes && !join) {
                const uint64_t aw0 = std::min(a0 * vpf / W, seg), aw1 = std::min((a1 * vpf + W - 1) / W, seg), bw0 = std::min(b0 * vpf / W, seg),
                               bw1 = std::min((b1 * vpf + W - 1) / W, seg);
                join = aw0 < bw1 && bw0 < aw1;
            }
            if (join) up[find(up, (int)i)] = find(up, (int)j);
        }
    // (a chain a - gap - b whose hull swallows a third range c between them: c overlaps the hull, not a or b; close the relation over hulls)
    for (bool moved = true; moved;) {
        moved = false;
        for (size_t i = 0; i < K; ++i)
            for (size_t j = 0; j < K; ++j) {
                if (find(up, (int)i) == find(up, (int)j)) continue;
                uint64_t lo = ~0ull, hi = 0;
                for (size_t k = 0; k < K; ++k)
                    if (find(up, (int)k) == find(up, (int)i)) { lo = std::min(lo, ranges[k].first); hi = std::max(hi, ranges[k].first + ranges[k].second); }
                if (ranges[j].first <= hi && lo <= ranges[j].first + ranges[j].second) { up[find(up, (int)i)] = find(up, (int)j); moved = true; }
            }
    }
    for (size_t i = 0; i < K; ++i) for (size_t j = 0; j < K; ++j) CHECK((find(up, (int)i) == find(up, (int)j)) == (seg_of[i] == seg_of[j]));
    // layers
    if (!planes) {
        const std::vector<uint32_t>& lf = p.layer_first;
        CHECK(lf.size() >= 2 && lf.front() == 0 && lf.back() == K && lf == sqy::update_boxes_layers(ws));
        if (lf.size() > 2) ++n_layers;
        std::vector<int> stamp(n, -1);
        for (size_t l = 0; l + 1 < lf.size(); ++l) {
            CHECK(lf[l] < lf[l + 1]);
            bool first_meets_previous = false;
            for (uint32_t i = lf[l]; i < lf[l + 1]; ++i)
                for (uint64_t z = ws[i].oz; z < ws[i].oz + ws[i].Z; ++z)
                    for (uint64_t y = ws[i].oy; y < ws[i].oy + ws[i].Y; ++y)
                        for (uint64_t x = ws[i].ox; x < ws[i].ox + ws[i].X; ++x) {
                            int& st = stamp[(z * sh.Y + y) * sh.X + x];
                            CHECK(st != (int)l);                        // pairwise disjoint inside a layer
                            if (i == lf[l] && l && st == (int)l - 1) first_meets_previous = true;
                            st = (int)l;
                        }
            if (l) CHECK(first_meets_previous);                           // maximal: the layer had to end
        }
    } else
        CHECK(p.layer_first.empty());
    // the united frames
    const uint32_t nframes = (uint32_t)((total + chunk - 1) / chunk);
    Ranges segs;
    for (const sqy::UpdateBoxesSegment& sg : p.segments) segs.push_back({sg.z0, sg.nz});
    const sqy::FrameRangesPlan u = sqy::frame_ranges_plan(form, n, elem, sh.Z, segs, chunk, total, nframes);
    CHECK(u.ok && u.boxes.size() == segs.size());
    std::set<uint32_t> want;
    for (const auto& r : segs) {
        const sqy::FrameRangePlan one = sqy::frame_range_plan(form, n, elem, sh.Z, r.first, r.second, chunk, total, nframes);
        CHECK(one.ok);
        want.insert(one.ids.begin(), one.ids.end());
    }
    CHECK(std::vector<uint32_t>(want.begin(), want.end()) == u.ids);
    // (planes: a segment's words and tail as the patch kernel addresses them lie apart from the next one's)
    for (size_t s = 1; planes && s < u.boxes.size(); ++s) CHECK(u.boxes[s - 1].w1 <= u.boxes[s].w0 && u.boxes[s - 1].v1 <= u.boxes[s].v0);
    return 0;
}

BatchWindow window(const Shape& sh, uint64_t oz, uint64_t Z, uint64_t oy, uint64_t Y, uint64_t ox, uint64_t X)
{
    return BatchWindow{sh.Z, sh.Y, sh.X, oz, oy, ox, Z, Y, X, false};
}

int run()
{
    const Shape shapes[] = {{5, 1, 3}, {6, 2, 3}, {3, 1, 5}, {9, 1, 7}, {7, 3, 5}, {40, 2, 3}, {4, 4, 4}, {12, 1, 1}};
    std::mt19937_64 rng(20261020);
    for (const Shape& sh : shapes)
        for (int elem : {1, 2})
            for (RangeForm form : {RangeForm::plain, RangeForm::planes})
                for (uint64_t chunk : {8ull, 64ull}) {
                    // every pair of z-ranges (both orders come up), the boxes whole frames
                    if (sh.Z <= 9 && chunk == 8)
                        for (uint64_t a = 0; a < sh.Z; ++a) for (uint64_t na = 1; a + na <= sh.Z; ++na)
                            for (uint64_t b = 0; b < sh.Z; ++b) for (uint64_t nb = 1; b + nb <= sh.Z; ++nb)
                                if (check(form, sh, elem, chunk, {window(sh, a, na, 0, sh.Y, 0, sh.X), window(sh, b, nb, 0, sh.Y, 0, sh.X)})) return 1;
                    // random sets; short ranges, so that gaps stay
                    for (int round = 0; round < 300; ++round) {
                        std::vector<BatchWindow> ws(1 + rng() % 6);
                        for (BatchWindow& w : ws) {
                            const uint64_t Z = 1 + rng() % std::min<uint64_t>(sh.Z, 3), Y = 1 + rng() % sh.Y, X = 1 + rng() % sh.X;
                            w = window(sh, rng() % (sh.Z - Z + 1), Z, rng() % (sh.Y - Y + 1), Y, rng() % (sh.X - X + 1), X);
                        }
                        if (check(form, sh, elem, chunk, ws)) return 1;
                    }
                }
    // what the plan refuses
    const Shape sh{4, 2, 2};
    const std::vector<BatchWindow> one{window(sh, 0, 1, 0, 2, 0, 2)};
    CHECK(!sqy::update_boxes_plan(RangeForm::plain, 16, 2, 4, {}, {}).ok);
    CHECK(!sqy::update_boxes_plan(RangeForm::plain, 16, 2, 4, {{0, 1}, {1, 1}}, one).ok);
    CHECK(!sqy::update_boxes_plan(RangeForm::plain, 16, 2, 4, {{4, 1}}, one).ok);
    CHECK(!sqy::update_boxes_plan(RangeForm::plain, 16, 2, 4, {{3, 2}}, one).ok);
    CHECK(!sqy::update_boxes_plan(RangeForm::plain, 16, 2, 4, {{0, 0}}, one).ok);
    CHECK(!sqy::update_boxes_plan(RangeForm::shuffle, 16, 2, 4, {{0, 1}}, one).ok);
    CHECK(!sqy::update_boxes_plan(RangeForm::planes, 16, 4, 4, {{0, 1}}, one).ok);
    CHECK(sqy::update_boxes_plan(RangeForm::planes, 16, 2, 4, {{0, 1}}, one).ok);
    CHECK(sqy::update_boxes_layers({}).empty());
    return 0;
}

} // namespace

int main()
{
    if (run()) return 1;
    std::printf("plans %llu merged_overlap %llu merged_word %llu merged_tail %llu layers %llu\n", n_plans, n_overlap, n_word, n_tail, n_layers);
    std::printf("update_boxes ok\n");
    return 0;
}
