// What the host-only planner says about the diff3x3x1 chain (tests/test_diff_seams_host.py builds and runs this with g++, sanitizers on, and
// holds tests/diff_seam_cases.py to the output): the constants kDiffStripRows and kDiffChainFrames, and decode_batch_plan's strip and step
// counts for every "Z Y X w" given on the command line -- each blob alone, then all of them in one group.
#include "../../sqeazy_amd/csrc/sqy_pipeline.hpp"

#include <cstdio>
#include <cstdlib>
#include <vector>

int main(int argc, char** argv)
{
    if (argc < 2 || (argc - 1) % 4 != 0) { std::fprintf(stderr, "usage: %s (Z Y X w)...\n", argv[0]); return 2; }
    std::printf("consts %u %u\n", sqy::kDiffStripRows, sqy::kDiffChainFrames);
    std::vector<sqy::DecodeBatchBlob> all;
    for (int i = 1; i < argc; i += 4) {
        sqy::DecodeBatchBlob b;
        b.Z = (uint32_t)std::strtoul(argv[i], nullptr, 10);
        b.Y = (uint32_t)std::strtoul(argv[i + 1], nullptr, 10);
        b.X = (uint32_t)std::strtoul(argv[i + 2], nullptr, 10);
        b.chain_columns = (uint32_t)std::strtoul(argv[i + 3], nullptr, 10);
        b.len = (uint64_t)b.Z * b.Y * b.X;
        b.total = b.len * 2;
        b.block_bytes = 256 << 10;
        b.eligible = true;
        b.form = sqy::DecodeBatchForm::diff_plain;
        all.push_back(b);
        const sqy::DecodeBatchPlan plan = sqy::decode_batch_plan({b}, 4ull << 30);
        if (plan.groups.size() != 1 || plan.groups[0].diff.jobs.size() != 1) { std::fprintf(stderr, "blob %d: not one diff job\n", (i - 1) / 4); return 1; }
        const sqy::DecodeBatchDiff& d = plan.groups[0].diff;
        std::printf("blob %u %u %u %u %u %u\n", b.Z, b.Y, b.X, d.nstrips, d.steps, d.max_columns);
    }
    const sqy::DecodeBatchPlan plan = sqy::decode_batch_plan(all, 4ull << 30);
    if (plan.groups.size() != 1) { std::fprintf(stderr, "the blobs do not share a group\n"); return 1; }
    const sqy::DecodeBatchDiff& d = plan.groups[0].diff;
    std::printf("group %zu %u %u %u\n", d.jobs.size(), d.nstrips, d.steps, d.max_columns);
    std::printf("diff_seam_plan ok\n");
    return 0;
}
