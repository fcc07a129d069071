// lz4_batch_plan of csrc/sqy_pipeline.cpp on the host (tests/test_host_batch_plan.py builds and runs this with g++, sanitizers on): which
// volumes of a batch are joint-eligible, how they are dealt to groups, and that every group's chunk table tiles every volume's stream
// exactly once.  Prints "batch_plan ok" and returns 0.
#include "../../sqeazy_amd/csrc/sqy_pipeline.hpp"

#include <cstdio>
#include <vector>

#define CHECK(cond)                                                                   \
    do {                                                                              \
        if (!(cond)) { std::fprintf(stderr, "line %d: %s\n", __LINE__, #cond); return 1; } \
    } while (0)

using sqy::Lz4BatchPlan;
using sqy::Lz4Params;

namespace {
const uint64_t kNoBound = ~(uint64_t)0;

// every invariant the driver and the kernels rely on; 0 when they hold
int check_plan(const Lz4BatchPlan& plan, const Lz4Params& p, const std::vector<uint64_t>& totals, unsigned nthreads, uint64_t group_bytes)
{
    CHECK(plan.group_of.size() == totals.size());
    std::vector<int> seen(totals.size(), 0);
    int32_t last_group = -1;
    for (size_t i = 0; i < totals.size(); ++i) {
        if (plan.group_of[i] < 0) continue;
        CHECK((size_t)plan.group_of[i] < plan.groups.size());
        CHECK(plan.group_of[i] == last_group || plan.group_of[i] == last_group + 1);      // dealt in order
        last_group = plan.group_of[i];
    }
    CHECK(last_group + 1 == (int32_t)plan.groups.size());                                 // no empty group
    for (size_t gi = 0; gi < plan.groups.size(); ++gi) {
        const sqy::Lz4BatchGroup& g = plan.groups[gi];
        CHECK(!g.vols.empty() && g.stream_at.size() == g.vols.size() && g.first_chunk.size() == g.vols.size() + 1);
        CHECK(g.first_chunk[0] == 0 && g.first_chunk.back() == g.chunks.size());
        uint64_t sum = 0, end = 0;
        for (size_t j = 0; j < g.vols.size(); ++j) {
            const uint32_t v = g.vols[j];
            CHECK(v < totals.size() && plan.group_of[v] == (int32_t)gi && !seen[v]);
            seen[v] = 1;
            if (j) CHECK(g.vols[j - 1] < v);
            const sqy::Lz4EncodeLayout lay = sqy::lz4_encode_layout(p, totals[v], nthreads);
            CHECK(lay.chunked() && lay.accel == 1 && totals[v] > 0);
            CHECK(g.stream_at[j] % 16 == 0 && g.stream_at[j] >= end);                     // streams do not overlap
            end = g.stream_at[j] + totals[v];
            CHECK(end <= g.stream_bytes);
            CHECK(g.first_chunk[j + 1] - g.first_chunk[j] == lay.nchunks);
            // the entries tile the stream exactly once, in order; only the last may be short
            uint64_t at = g.stream_at[j];
            for (uint32_t e = g.first_chunk[j]; e < g.first_chunk[j + 1]; ++e) {
                const sqy::Lz4BatchChunkPlan& c = g.chunks[e];
                CHECK(c.vol == v && c.off == at && c.n > 0 && c.n <= lay.chunk && c.n <= g.max_chunk);
                CHECK(c.n == lay.chunk || e + 1 == g.first_chunk[j + 1]);
                CHECK(c.off >= g.stream_at[j] && c.off + c.n <= g.stream_at[j] + totals[v]);      // inside its volume's stream
                CHECK(c.slot == e && (uint64_t)c.n <= g.scratch_stride);                       // a slot of its own, large enough
                at += c.n;
            }
            CHECK(at == g.stream_at[j] + totals[v]);
            sum += totals[v];
        }
        CHECK(g.scratch_stride % 16 == 0);
        CHECK(g.vols.size() == 1 || sum <= group_bytes);                                       // a group over the bound holds one volume
    }
    return 0;
}
}

int main()
{
    const Lz4Params dflt("");                   // 256 KiB chunks
    const uint64_t C = 256u << 10;
    {   // single-chunk volumes, a short last chunk in mid-table, an exact multiple of the chunk, tiny volumes
        const std::vector<uint64_t> totals = {C, C + 65536, 210, 10, 2 * C, 1, 3 * C + 1};
        const Lz4BatchPlan plan = sqy::lz4_batch_plan(dflt, totals, 4, 1u << 30, kNoBound);
        CHECK(check_plan(plan, dflt, totals, 4, 1u << 30) == 0);
        CHECK(plan.groups.size() == 1 && plan.groups[0].chunks.size() == 1 + 2 + 1 + 1 + 2 + 1 + 4);
        CHECK(plan.groups[0].chunks[2].n == 65536 && plan.groups[0].chunks[2].vol == 1);      // the short chunk, entries behind it
        CHECK(plan.groups[0].chunks[3].vol == 2 && plan.groups[0].chunks[3].n == 210);
        CHECK(plan.groups[0].chunks[5].n == C && plan.groups[0].chunks[6].n == C);           // the exact multiple: no empty entry behind it
        CHECK(plan.groups[0].max_chunk == C && plan.groups[0].scratch_stride == C);
    }
    {   // an empty volume is refused upstream; the plan leaves it out rather than making entries of no bytes
        const std::vector<uint64_t> totals = {0, 100, 0};
        const Lz4BatchPlan plan = sqy::lz4_batch_plan(dflt, totals, 4, 1u << 30, kNoBound);
        CHECK(check_plan(plan, dflt, totals, 4, 1u << 30) == 0);
        CHECK(plan.group_of[0] == -1 && plan.group_of[1] == 0 && plan.group_of[2] == -1 && plan.groups[0].chunks.size() == 1);
    }
    {   // n_chunks_of_input = 7 on lengths that make misaligned chunk starts
        const Lz4Params seven("n_chunks_of_input=7,framestep_kb=0");
        const Lz4Params p = seven.n_chunks == 7 && seven.framestep_kb == 0 ? seven : Lz4Params("n_chunks_of_input=7");
        const std::vector<uint64_t> totals = {16384, 14322, 105, 6, 7, 8, 1000003};
        const Lz4BatchPlan plan = sqy::lz4_batch_plan(p, totals, 2, 1u << 30, kNoBound);
        CHECK(check_plan(plan, p, totals, 2, 1u << 30) == 0);
        for (size_t i = 0; i < totals.size(); ++i) CHECK(plan.group_of[i] == 0);
        const sqy::Lz4EncodeLayout lay = sqy::lz4_encode_layout(p, 14322, 2);
        CHECK(lay.chunk == 14322 / 7 && lay.nchunks == 7);
        bool misaligned = false;
        for (const sqy::Lz4BatchChunkPlan& c : plan.groups[0].chunks) misaligned = misaligned || (c.off % 16 != 0);
        CHECK(misaligned);
    }
    {   // group cuts at group_bytes; a volume larger than the bound gets a group of its own
        const std::vector<uint64_t> totals = {C, C + 65536, 210, 10, 2 * C, 5 * C, 100};
        const Lz4BatchPlan plan = sqy::lz4_batch_plan(dflt, totals, 4, 600000, kNoBound);
        CHECK(check_plan(plan, dflt, totals, 4, 600000) == 0);
        const int32_t want[] = {0, 0, 0, 0, 1, 2, 3};             // (the two tiny volumes still fit behind the first two)
        for (size_t i = 0; i < totals.size(); ++i) CHECK(plan.group_of[i] == want[i]);
        CHECK(plan.groups[2].vols.size() == 1 && plan.groups[2].stream_bytes == 5 * C && plan.groups[0].stream_bytes == 2 * C + 65536 + 224 + 10);
        const Lz4BatchPlan one = sqy::lz4_batch_plan(dflt, totals, 4, 1, kNoBound);                // every volume alone
        CHECK(check_plan(one, dflt, totals, 4, 1) == 0 && one.groups.size() == totals.size());
    }
    {   // nthreads = 1 with more than one chunk is the serial layout: not eligible; single chunks still are
        const std::vector<uint64_t> totals = {C, C + 1, 10, 4 * C};
        const Lz4BatchPlan plan = sqy::lz4_batch_plan(dflt, totals, 1, 1u << 30, kNoBound);
        CHECK(check_plan(plan, dflt, totals, 1, 1u << 30) == 0);
        CHECK(plan.group_of[0] == 0 && plan.group_of[1] == -1 && plan.group_of[2] == 0 && plan.group_of[3] == -1);
    }
    {   // the size bound, acceleration, chunks of several LZ4 blocks
        const std::vector<uint64_t> totals = {C, 8 * C, 8 * C + 1};
        const Lz4BatchPlan plan = sqy::lz4_batch_plan(dflt, totals, 4, 1u << 30, 8 * C);
        CHECK(check_plan(plan, dflt, totals, 4, 1u << 30) == 0);
        CHECK(plan.group_of[0] == 0 && plan.group_of[1] == 0 && plan.group_of[2] == -1);
        const Lz4Params accel("accel=-3");
        CHECK(sqy::lz4_batch_plan(accel, totals, 4, 1u << 30, kNoBound).groups.empty());
        const Lz4Params linked("framestep_kb=1024");                                               // 1 MiB chunks of 256 KiB blocks
        const Lz4BatchPlan lp = sqy::lz4_batch_plan(linked, {C, 2 * C, 8 * C}, 4, 1u << 30, kNoBound);
        CHECK(lp.group_of[0] == 0 && lp.group_of[1] == -1 && lp.group_of[2] == -1);
        CHECK(sqy::lz4_batch_plan(dflt, {}, 4, 1u << 30, kNoBound).groups.empty());
    }
    std::printf("batch_plan ok\n");
    return 0;
}
