// decode_batch_plan of csrc/sqy_pipeline.cpp on the host (tests/test_host_decode_batch.py builds and runs this with g++, sanitizers on):
// which blobs of a batch take the joint path, how they are dealt to groups, where their LZ4 output lies in a group's workspace, and that
// the tile tables send every workgroup to the job and tile a brute-force walk finds.  Prints "decode_batch_plan ok" and returns 0.
#include "../../sqeazy_amd/csrc/sqy_pipeline.hpp"

#include <cstdio>
#include <vector>

#define CHECK(cond)                                                                   \
    do {                                                                              \
        if (!(cond)) { std::fprintf(stderr, "line %d: %s\n", __LINE__, #cond); return 1; } \
    } while (0)

using sqy::DecodeBatchBlob;
using sqy::DecodeBatchForm;
using sqy::DecodeBatchPlan;
using sqy::DecodeBatchTiles;

namespace {

// the kernels' search: first_tile[lo] <= block < first_tile[hi]
uint32_t job_of(const std::vector<uint32_t>& first_tile, uint32_t njobs, uint32_t block)
{
    uint32_t lo = 0, hi = njobs;
    while (hi - lo > 1u) {
        const uint32_t mid = (lo + hi) >> 1;
        if (first_tile[mid] <= block) lo = mid; else hi = mid;
    }
    return lo;
}

int check_tiles(const DecodeBatchTiles& t, const std::vector<DecodeBatchBlob>& blobs, const std::vector<uint32_t>& members, DecodeBatchForm form,
                const std::vector<uint8_t>* dropped)
{
    std::vector<uint32_t> want;
    for (uint32_t b : members)
        if (blobs[b].form == form && !(dropped && (*dropped)[b])) want.push_back(b);
    CHECK(t.jobs == want);
    CHECK(t.first_tile.size() == t.jobs.size() + 1 && t.first_tile[0] == 0 && t.first_tile.back() == t.ntiles);
    // brute force: every tile of every job, in order
    uint32_t block = 0;
    for (size_t j = 0; j < t.jobs.size(); ++j) {
        const uint64_t len = blobs[t.jobs[j]].len;
        const uint64_t tiles = len ? (len + sqy::kBatchTileVoxels - 1) / sqy::kBatchTileVoxels : 1;
        CHECK(t.first_tile[j + 1] - t.first_tile[j] == tiles);
        for (uint64_t k = 0; k < tiles; ++k, ++block) {
            CHECK(job_of(t.first_tile, (uint32_t)t.jobs.size(), block) == j);
            CHECK(block - t.first_tile[j] == k);
            CHECK(k * sqy::kBatchTileVoxels < len || (len == 0 && k == 0));           // the tile holds voxels of the job
        }
        CHECK(tiles * sqy::kBatchTileVoxels >= len);                                  // .. and the tiles cover it
    }
    CHECK(block == t.ntiles);
    return 0;
}

int check_plan(const DecodeBatchPlan& plan, const std::vector<DecodeBatchBlob>& blobs, uint64_t group_bytes, const std::vector<uint8_t>* dropped = nullptr)
{
    CHECK(plan.group_of.size() == blobs.size());
    int32_t last_group = -1;
    for (size_t i = 0; i < blobs.size(); ++i) {
        CHECK((plan.group_of[i] >= 0) == blobs[i].eligible);
        if (plan.group_of[i] < 0) continue;
        CHECK(plan.group_of[i] == last_group || plan.group_of[i] == last_group + 1);      // dealt in order
        last_group = plan.group_of[i];
    }
    CHECK(last_group + 1 == (int32_t)plan.groups.size());                                 // no empty group
    std::vector<int> seen(blobs.size(), 0);
    for (size_t gi = 0; gi < plan.groups.size(); ++gi) {
        const sqy::DecodeBatchGroup& g = plan.groups[gi];
        CHECK(!g.blobs.empty() && g.out_at.size() == g.blobs.size());
        uint64_t end = 0;
        for (size_t j = 0; j < g.blobs.size(); ++j) {
            const uint32_t b = g.blobs[j];
            CHECK(b < blobs.size() && plan.group_of[b] == (int32_t)gi && !seen[b]);
            seen[b] = 1;
            if (j) CHECK(g.blobs[j - 1] < b);
            CHECK(blobs[b].block_bytes == g.block_bytes);                                 // one block size per group
            CHECK(g.out_at[j] % 256 == 0 && g.out_at[j] >= end);                          // the outputs do not overlap
            end = g.out_at[j] + blobs[b].total;
            CHECK(end <= g.out_bytes);
        }
        // within the bound, unless it is a group of one
        CHECK(g.out_bytes <= group_bytes || g.blobs.size() == 1);
        // a group is only closed when it has to be: the next eligible blob did not fit or has another block size
        if (gi + 1 < plan.groups.size()) {
            const DecodeBatchBlob& next = blobs[plan.groups[gi + 1].blobs[0]];
            CHECK(next.block_bytes != g.block_bytes || g.out_bytes + (next.total + 255) / 256 * 256 > group_bytes);
        }
        if (check_tiles(g.planes, blobs, g.blobs, DecodeBatchForm::planes, dropped)) return 1;
        if (check_tiles(g.plain, blobs, g.blobs, DecodeBatchForm::plain, dropped)) return 1;
    }
    return 0;
}

DecodeBatchBlob blob(uint64_t total, uint64_t block, uint64_t len, bool eligible, DecodeBatchForm form)
{
    DecodeBatchBlob b;
    b.total = total; b.block_bytes = block; b.len = len; b.eligible = eligible; b.form = form;
    return b;
}

}  // namespace

int main()
{
    const uint64_t kNoBound = 4ull << 30, k256 = 256 << 10;
    {   // empty input
        const DecodeBatchPlan plan = sqy::decode_batch_plan({}, kNoBound);
        CHECK(plan.group_of.empty() && plan.groups.empty());
    }
    {   // one blob; one blob that is not eligible
        std::vector<DecodeBatchBlob> one{blob(105 * 2, k256, 105, true, DecodeBatchForm::planes)};
        DecodeBatchPlan plan = sqy::decode_batch_plan(one, kNoBound);
        if (check_plan(plan, one, kNoBound)) return 1;
        CHECK(plan.groups.size() == 1 && plan.groups[0].planes.ntiles == 1 && plan.groups[0].plain.ntiles == 0 && plan.groups[0].out_bytes == 256);
        one[0].eligible = false;
        plan = sqy::decode_batch_plan(one, kNoBound);
        if (check_plan(plan, one, kNoBound)) return 1;
        CHECK(plan.groups.empty() && plan.group_of[0] == -1);
    }
    {   // a blob larger than the bound: a group of one, wherever it stands
        std::vector<DecodeBatchBlob> v{blob(1000, k256, 500, true, DecodeBatchForm::planes), blob(5000000, k256, 2500000, true, DecodeBatchForm::planes),
                                       blob(1000, k256, 1000, true, DecodeBatchForm::plain)};
        for (uint64_t bound : {(uint64_t)1, (uint64_t)300000, (uint64_t)1 << 20}) {
            const DecodeBatchPlan plan = sqy::decode_batch_plan(v, bound);
            if (check_plan(plan, v, bound)) return 1;
            CHECK(plan.groups.size() == 3 && plan.groups[1].blobs.size() == 1);
        }
        const DecodeBatchPlan all = sqy::decode_batch_plan(v, kNoBound);
        if (check_plan(all, v, kNoBound)) return 1;
        CHECK(all.groups.size() == 1 && all.groups[0].planes.ntiles == 1 + 77 && all.groups[0].plain.ntiles == 1);
    }
    {   // mixed block sizes, forms and eligibility; bounds from one byte to none
        std::vector<DecodeBatchBlob> v;
        const uint64_t blocks[3] = {k256, 64 << 10, 4 << 20};
        uint64_t x = 12345;
        for (int i = 0; i < 200; ++i) {
            x = x * 6364136223846793005ull + 1442695040888963407ull;
            const uint64_t len = (x >> 33) % 200000;                              // (0 as well: one tile, nothing in it)
            const DecodeBatchForm form = (DecodeBatchForm)((x >> 20) % 3);
            const int elem = 1 + (int)((x >> 24) & 1);
            v.push_back(blob(form == DecodeBatchForm::plain ? len : len * elem, blocks[(i / 7) % 3], len, (x >> 28) % 5 != 0, form));
        }
        for (uint64_t bound : {(uint64_t)1, (uint64_t)65536, (uint64_t)300000, (uint64_t)1 << 22, kNoBound}) {
            const DecodeBatchPlan plan = sqy::decode_batch_plan(v, bound);
            if (check_plan(plan, v, bound)) return 1;
            // blobs the ranking refused keep their place and lose their job
            std::vector<uint8_t> dropped(v.size(), 0);
            for (size_t i = 0; i < v.size(); i += 3) dropped[i] = 1;
            const DecodeBatchPlan again = sqy::decode_batch_plan(v, bound, &dropped);
            if (check_plan(again, v, bound, &dropped)) return 1;
            CHECK(again.group_of == plan.group_of && again.groups.size() == plan.groups.size());
            for (size_t g = 0; g < plan.groups.size(); ++g) CHECK(again.groups[g].out_at == plan.groups[g].out_at && again.groups[g].out_bytes == plan.groups[g].out_bytes);
        }
    }
    std::printf("decode_batch_plan ok\n");
    return 0;
}
