// decode_batch_plan of csrc/sqy_pipeline.cpp with the forms behind a filter stage (tests/test_host_decode_batch_stages.py builds and runs this
// with g++, sanitizers on): random mixes of all six forms, bounds from one byte to none, a `dropped` list.  Every blob that is not `stages`
// has its job in exactly one table of its group -- `planes`, `plain`, `quantised`, or `diff`, and a diff_planes blob one more in `planes`,
// the transpose in front of its diff inverse --; the tables send every workgroup to the (job, tile) or (job, strip) a brute-force walk finds,
// every chain step covers the frames it must; the workspace regions lie apart and within the bound (a group of at least one blob).
// Prints "decode_batch_stage_plan ok" and returns 0.
#include "../../sqeazy_amd/csrc/sqy_pipeline.hpp"

#include <algorithm>
#include <cstdio>
#include <utility>
#include <vector>

#define CHECK(cond)                                                                   \
    do {                                                                              \
        if (!(cond)) { std::fprintf(stderr, "line %d: %s\n", __LINE__, #cond); return 1; } \
    } while (0)

using sqy::DecodeBatchBlob;
using sqy::DecodeBatchForm;
using sqy::DecodeBatchPlan;

namespace {

// the kernels' search: first[lo] <= block < first[hi]
uint32_t job_of(const std::vector<uint32_t>& first, uint32_t njobs, uint32_t block)
{
    uint32_t lo = 0, hi = njobs;
    while (hi - lo > 1u) {
        const uint32_t mid = (lo + hi) >> 1;
        if (first[mid] <= block) lo = mid; else hi = mid;
    }
    return lo;
}

bool is_diff(DecodeBatchForm f) { return f == DecodeBatchForm::diff_planes || f == DecodeBatchForm::diff_plain; }
uint64_t up256(uint64_t v) { return (v + 255) / 256 * 256; }

// a table of `per(job)` entries per job: prefix sums, and the search finds every entry's job
template <class F>
int check_table(const std::vector<uint32_t>& jobs, const std::vector<uint32_t>& first, uint32_t total, F&& per)
{
    CHECK(first.size() == jobs.size() + 1 && first[0] == 0 && first.back() == total);
    uint32_t block = 0;
    for (size_t j = 0; j < jobs.size(); ++j) {
        const uint64_t n = per(jobs[j]);
        CHECK(n >= 1 && first[j + 1] - first[j] == n);
        for (uint64_t k = 0; k < n; ++k, ++block) {
            CHECK(job_of(first, (uint32_t)jobs.size(), block) == j);
            CHECK(block - first[j] == k);
        }
    }
    CHECK(block == total);
    return 0;
}

int check_plan(const DecodeBatchPlan& plan, const std::vector<DecodeBatchBlob>& blobs, uint64_t group_bytes, const std::vector<uint8_t>* dropped = nullptr)
{
    CHECK(plan.group_of.size() == blobs.size());
    auto tiles_of = [&](uint32_t b) { return std::max<uint64_t>((blobs[b].len + sqy::kBatchTileVoxels - 1) / sqy::kBatchTileVoxels, 1); };
    auto strips_of = [&](uint32_t b) { return ((uint64_t)blobs[b].Y + sqy::kDiffStripRows - 1) / sqy::kDiffStripRows; };
    std::vector<int> seen(blobs.size(), 0);
    for (size_t i = 0; i < blobs.size(); ++i) CHECK((plan.group_of[i] >= 0) == blobs[i].eligible);
    for (size_t gi = 0; gi < plan.groups.size(); ++gi) {
        const sqy::DecodeBatchGroup& g = plan.groups[gi];
        CHECK(!g.blobs.empty() && g.out_at.size() == g.blobs.size());
        // what every table must hold, in blob order
        std::vector<uint32_t> want[4], want_planes;
        for (uint32_t b : g.blobs) {
            CHECK(b < blobs.size() && plan.group_of[b] == (int32_t)gi && !seen[b]);
            seen[b] = 1;
            CHECK(blobs[b].block_bytes == g.block_bytes);
            const DecodeBatchForm f = blobs[b].form;
            if (f == DecodeBatchForm::stages || (dropped && (*dropped)[b])) continue;
            want[f == DecodeBatchForm::planes ? 0 : f == DecodeBatchForm::plain ? 1 : f == DecodeBatchForm::quantised ? 2 : 3].push_back(b);
            if (f == DecodeBatchForm::planes || f == DecodeBatchForm::diff_planes) want_planes.push_back(b);
        }
        // exactly one table each: the lists are the blobs of their forms, once, and nothing else
        CHECK(g.planes.jobs == want_planes && g.plain.jobs == want[1] && g.quantised.jobs == want[2] && g.diff.jobs == want[3]);
        if (check_table(g.planes.jobs, g.planes.first_tile, g.planes.ntiles, tiles_of)) return 1;
        if (check_table(g.plain.jobs, g.plain.first_tile, g.plain.ntiles, tiles_of)) return 1;
        if (check_table(g.quantised.jobs, g.quantised.first_tile, g.quantised.ntiles, tiles_of)) return 1;
        if (check_table(g.diff.jobs, g.diff.first_tile, g.diff.ntiles, tiles_of)) return 1;
        if (check_table(g.diff.jobs, g.diff.first_strip, g.diff.nstrips, strips_of)) return 1;
        // the tiles cover the voxels, the strips the rows
        for (uint32_t b : g.diff.jobs) {
            CHECK(tiles_of(b) * sqy::kBatchTileVoxels >= blobs[b].len && strips_of(b) * sqy::kDiffStripRows >= blobs[b].Y);
            CHECK((strips_of(b) - 1) * sqy::kDiffStripRows < blobs[b].Y);
        }
        // the chain: the steps of the group take every job through frames 1 .. min(X, Z) - 1, the last step is some job's
        CHECK(g.diff.res_at.size() == g.diff.jobs.size());
        uint64_t deepest = 1;
        uint32_t widest = 0;
        for (uint32_t b : g.diff.jobs) {
            const uint64_t zlim = std::min<uint64_t>(blobs[b].X, blobs[b].Z);
            CHECK(1 + (uint64_t)g.diff.steps * sqy::kDiffChainFrames >= zlim);
            deepest = std::max(deepest, zlim);
            widest = std::max(widest, blobs[b].chain_columns);
        }
        CHECK(g.diff.steps == (deepest - 1 + sqy::kDiffChainFrames - 1) / sqy::kDiffChainFrames);
        CHECK(g.diff.max_columns == widest);
        // the workspace: every blob's LZ4 output, a diff_planes job's residual volume behind its own -- 256-byte aligned, apart, inside
        std::vector<std::pair<uint64_t, uint64_t>> regions;
        for (size_t j = 0; j < g.blobs.size(); ++j) {
            CHECK(g.out_at[j] % 256 == 0);
            regions.push_back({g.out_at[j], g.out_at[j] + blobs[g.blobs[j]].total});
        }
        for (size_t j = 0; j < g.diff.jobs.size(); ++j) {
            const uint32_t b = g.diff.jobs[j];
            const size_t k = (size_t)(std::find(g.blobs.begin(), g.blobs.end(), b) - g.blobs.begin());
            CHECK(g.diff.res_at[j] % 256 == 0);
            if (blobs[b].form == DecodeBatchForm::diff_plain) CHECK(g.diff.res_at[j] == g.out_at[k]);
            else regions.push_back({g.diff.res_at[j], g.diff.res_at[j] + blobs[b].total});
        }
        std::sort(regions.begin(), regions.end());
        for (size_t r = 0; r < regions.size(); ++r) {
            CHECK(regions[r].second <= g.out_bytes);
            if (r) CHECK(regions[r - 1].second <= regions[r].first);
        }
        CHECK(g.out_bytes <= group_bytes || g.blobs.size() == 1);
        // a group is only closed when it has to be
        if (gi + 1 < plan.groups.size()) {
            const DecodeBatchBlob& next = blobs[plan.groups[gi + 1].blobs[0]];
            const uint64_t need = up256(next.total) * (next.form == DecodeBatchForm::diff_planes ? 2 : 1);
            CHECK(next.block_bytes != g.block_bytes || g.out_bytes + need > group_bytes);
        }
    }
    for (size_t i = 0; i < blobs.size(); ++i) CHECK(seen[i] == (blobs[i].eligible ? 1 : 0));
    return 0;
}

DecodeBatchBlob diff_blob(uint32_t Z, uint32_t Y, uint32_t X, uint64_t block, bool planes)
{
    DecodeBatchBlob b;
    b.len = (uint64_t)Z * Y * X; b.total = b.len * 2; b.block_bytes = block; b.eligible = true;
    b.form = planes ? DecodeBatchForm::diff_planes : DecodeBatchForm::diff_plain;
    b.Z = Z; b.Y = Y; b.X = X;
    b.chain_columns = std::min<uint32_t>(X, (Z + 7) / 8 * 8);          // (2 + hx = Z for Z >= 2: the chain geometry's count)
    return b;
}

}  // namespace

int main()
{
    const uint64_t kNoBound = 4ull << 30, k256 = 256 << 10;
    {   // one diff blob of each kind: strips, tiles, steps, the second region
        std::vector<DecodeBatchBlob> v{diff_blob(10, 70, 24, k256, true)};
        DecodeBatchPlan plan = sqy::decode_batch_plan(v, kNoBound);
        if (check_plan(plan, v, kNoBound)) return 1;
        const sqy::DecodeBatchGroup& g = plan.groups[0];
        CHECK(g.diff.nstrips == 3 && g.diff.ntiles == 1 && g.diff.steps == 2 && g.planes.ntiles == 1 && g.out_bytes == 2 * up256(10 * 70 * 24 * 2));
        CHECK(g.diff.res_at[0] == up256(10 * 70 * 24 * 2) && g.diff.max_columns == 16);
        v[0] = diff_blob(9, 5, 16, k256, false);
        plan = sqy::decode_batch_plan(v, kNoBound);
        if (check_plan(plan, v, kNoBound)) return 1;
        CHECK(plan.groups[0].diff.steps == 1 && plan.groups[0].planes.ntiles == 0 && plan.groups[0].out_bytes == up256(9 * 5 * 16 * 2) && plan.groups[0].diff.res_at[0] == 0);
        v[0] = diff_blob(1, 8, 8, k256, true);                          // one frame: no chain step at all
        plan = sqy::decode_batch_plan(v, kNoBound);
        if (check_plan(plan, v, kNoBound)) return 1;
        CHECK(plan.groups[0].diff.steps == 0 && plan.groups[0].diff.nstrips == 1);
        // the second region counts against the bound: two blobs whose LZ4 outputs alone would share a group
        std::vector<DecodeBatchBlob> two{diff_blob(16, 128, 128, k256, true), diff_blob(16, 128, 128, k256, true)};
        CHECK(sqy::decode_batch_plan(two, 3 * 524288).groups.size() == 2 && sqy::decode_batch_plan(two, 4 * 524288).groups.size() == 1);
        two[0].form = two[1].form = DecodeBatchForm::diff_plain;
        CHECK(sqy::decode_batch_plan(two, 2 * 524288).groups.size() == 1);
    }
    {   // random mixes of all forms and eligibility; bounds from one byte to none; a dropped list
        for (uint64_t seed : {(uint64_t)12345, (uint64_t)777, (uint64_t)99991}) {
            std::vector<DecodeBatchBlob> v;
            const uint64_t blocks[3] = {k256, 64 << 10, 4 << 20};
            uint64_t x = seed;
            auto rnd = [&](uint64_t m) { x = x * 6364136223846793005ull + 1442695040888963407ull; return (x >> 33) % m; };
            for (int i = 0; i < 240; ++i) {
                const DecodeBatchForm form = (DecodeBatchForm)rnd(6);
                const uint64_t block = blocks[(i / 9) % 3];
                DecodeBatchBlob b;
                if (is_diff(form)) {
                    const uint32_t X = 8 * (1 + (uint32_t)rnd(40)), Z = 1 + (uint32_t)rnd(X), Y = 1 + (uint32_t)rnd(200);      // (Z - 2 <= X - 2)
                    b = diff_blob(Z, Y, X, block, form == DecodeBatchForm::diff_planes);
                } else {
                    b.len = rnd(200000);                                  // (0 as well: one tile, nothing in it)
                    b.total = form == DecodeBatchForm::plain || form == DecodeBatchForm::quantised ? b.len : b.len * (1 + rnd(2));
                    b.block_bytes = block; b.form = form;
                }
                b.eligible = rnd(5) != 0;
                v.push_back(b);
            }
            for (uint64_t bound : {(uint64_t)1, (uint64_t)65536, (uint64_t)300000, (uint64_t)1 << 22, kNoBound}) {
                const DecodeBatchPlan plan = sqy::decode_batch_plan(v, bound);
                if (check_plan(plan, v, bound)) return 1;
                // blobs the ranking refused keep their place and lose their jobs, in every table
                std::vector<uint8_t> dropped(v.size(), 0);
                for (size_t i = seed % 3; i < v.size(); i += 3) dropped[i] = 1;
                const DecodeBatchPlan again = sqy::decode_batch_plan(v, bound, &dropped);
                if (check_plan(again, v, bound, &dropped)) return 1;
                CHECK(again.group_of == plan.group_of && again.groups.size() == plan.groups.size());
                for (size_t g = 0; g < plan.groups.size(); ++g) {
                    CHECK(again.groups[g].out_at == plan.groups[g].out_at && again.groups[g].out_bytes == plan.groups[g].out_bytes);
                    for (size_t j = 0; j < again.groups[g].diff.jobs.size(); ++j) {       // a job that stays keeps its residual region
                        const auto& pj = plan.groups[g].diff.jobs;
                        const size_t k = (size_t)(std::find(pj.begin(), pj.end(), again.groups[g].diff.jobs[j]) - pj.begin());
                        CHECK(k < pj.size() && plan.groups[g].diff.res_at[k] == again.groups[g].diff.res_at[j]);
                    }
                }
            }
        }
    }
    std::printf("decode_batch_stage_plan ok\n");
    return 0;
}
