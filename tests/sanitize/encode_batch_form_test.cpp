// The batch encode's planning on the host (csrc/sqy_pipeline.cpp): which joint form a pipeline takes (encode_batch_form), what a volume
// of that form puts in front of the LZ4 stage and takes besides (encode_batch_stream_bytes, encode_batch_extra_bytes), and lz4_batch_plan
// with those extra bytes -- the group cut when the tables, not the streams, reach the bound; the five-argument call as before.
// tests/test_host_encode_batch_stages.py builds and runs this with g++, sanitizers on.  Prints "encode_batch_form ok" and returns 0.
#include "../../sqeazy_amd/csrc/sqy_pipeline.hpp"

#include <cstdio>
#include <string>
#include <vector>

#define CHECK(cond)                                                                   \
    do {                                                                              \
        if (!(cond)) { std::fprintf(stderr, "line %d: %s\n", __LINE__, #cond); return 1; } \
    } while (0)

using sqy::EncodeBatchForm;
using sqy::Lz4BatchPlan;
using sqy::Lz4Params;
using sqy::Pipeline;

namespace {
EncodeBatchForm form_of(const std::string& s, int elem) { return sqy::encode_batch_form(Pipeline::from_string(s, elem), elem); }

bool same_plan(const Lz4BatchPlan& a, const Lz4BatchPlan& b)
{
    if (a.group_of != b.group_of || a.groups.size() != b.groups.size()) return false;
    for (size_t g = 0; g < a.groups.size(); ++g) {
        const sqy::Lz4BatchGroup &x = a.groups[g], &y = b.groups[g];
        if (x.vols != y.vols || x.stream_at != y.stream_at || x.first_chunk != y.first_chunk || x.stream_bytes != y.stream_bytes ||
            x.scratch_stride != y.scratch_stride || x.max_chunk != y.max_chunk || x.chunks.size() != y.chunks.size())
            return false;
        for (size_t e = 0; e < x.chunks.size(); ++e)
            if (x.chunks[e].off != y.chunks[e].off || x.chunks[e].n != y.chunks[e].n || x.chunks[e].vol != y.chunks[e].vol || x.chunks[e].slot != y.chunks[e].slot)
                return false;
    }
    return true;
}
}

int main()
{
    // every form
    CHECK(form_of("lz4", 2) == EncodeBatchForm::lz4 && form_of("lz4", 1) == EncodeBatchForm::lz4);
    CHECK(form_of("lz4(n_chunks_of_input=7)", 2) == EncodeBatchForm::lz4);
    CHECK(form_of("bitswap1->lz4", 2) == EncodeBatchForm::bitswap1_lz4 && form_of("bitswap1->lz4", 1) == EncodeBatchForm::bitswap1_lz4);
    CHECK(form_of("quantiser->bitswap1->lz4", 2) == EncodeBatchForm::quantiser_bitswap1_lz4);
    CHECK(form_of("quantiser->bitswap1->lz4(blocksize_kb=4,framestep_kb=4)", 2) == EncodeBatchForm::quantiser_bitswap1_lz4);
    // .. and what stays on the single-call path
    CHECK(form_of("quantiser(weighting_function=power_of_1_2)->bitswap1->lz4", 2) == EncodeBatchForm::none);
    CHECK(form_of("quantiser(weighting_function=none)->bitswap1->lz4", 2) == EncodeBatchForm::none);          // (the rule is "no weighting_function")
    CHECK(form_of("quantiser(decode_lut_path=/tmp/a.lut)->bitswap1->lz4", 2) == EncodeBatchForm::none);
    CHECK(form_of("quantiser->lz4", 2) == EncodeBatchForm::none);
    CHECK(form_of("diff3x3x1->bitswap1->lz4", 2) == EncodeBatchForm::none);
    CHECK(form_of("diff3x3x1->lz4", 2) == EncodeBatchForm::none);
    CHECK(form_of("bitswap1", 2) == EncodeBatchForm::none);
    CHECK(form_of("bitswap1->bitswap1->lz4", 2) == EncodeBatchForm::none);
    CHECK(form_of("quantiser->diff3x3x1->lz4", 2) == EncodeBatchForm::none);
    CHECK(sqy::encode_batch_form(Pipeline(), 2) == EncodeBatchForm::none);

    // the bytes in front of the LZ4 stage, and the tables
    CHECK(sqy::encode_batch_stream_bytes(EncodeBatchForm::lz4, 1000, 2) == 2000 && sqy::encode_batch_stream_bytes(EncodeBatchForm::bitswap1_lz4, 1000, 1) == 1000);
    CHECK(sqy::encode_batch_stream_bytes(EncodeBatchForm::quantiser_bitswap1_lz4, 1000, 2) == 1000);
    CHECK(sqy::kQuantiserBatchTableBytes == (256u << 10) + (64u << 10) + 512);
    CHECK(sqy::encode_batch_extra_bytes(EncodeBatchForm::quantiser_bitswap1_lz4) == sqy::kQuantiserBatchTableBytes);
    CHECK(sqy::encode_batch_extra_bytes(EncodeBatchForm::lz4) == 0 && sqy::encode_batch_extra_bytes(EncodeBatchForm::bitswap1_lz4) == 0 &&
          sqy::encode_batch_extra_bytes(EncodeBatchForm::none) == 0);

    const Lz4Params dflt("");
    const uint64_t C = 256u << 10, T = sqy::kQuantiserBatchTableBytes;
    {   // the five-argument call: the plan of before, and the same as extra_bytes = 0
        const std::vector<uint64_t> totals = {C, C + 65536, 210, 10, 2 * C, 5 * C, 100};
        const Lz4BatchPlan old5 = sqy::lz4_batch_plan(dflt, totals, 4, 600000, ~(uint64_t)0);
        const int32_t want[] = {0, 0, 0, 0, 1, 2, 3};
        for (size_t i = 0; i < totals.size(); ++i) CHECK(old5.group_of[i] == want[i]);
        CHECK(old5.groups[0].stream_bytes == 2 * C + 65536 + 224 + 10);
        CHECK(same_plan(old5, sqy::lz4_batch_plan(dflt, totals, 4, 600000, ~(uint64_t)0, 0)));
    }
    {   // tiny streams: the tables reach the bound, the streams never would
        const std::vector<uint64_t> totals = {105, 5, 7161, 49152, 100, 100, 100};
        const uint64_t bound = 3 * T + 60000;                   // three volumes' tables and a little
        const Lz4BatchPlan one = sqy::lz4_batch_plan(dflt, totals, 4, bound, ~(uint64_t)0);
        CHECK(one.groups.size() == 1);                          // (without the tables: one group)
        const Lz4BatchPlan p = sqy::lz4_batch_plan(dflt, totals, 4, bound, ~(uint64_t)0, T);
        const int32_t want[] = {0, 0, 0, 1, 1, 1, 2};           // 3 T + 7271 | + 49152 + T is over; 3 T + 49352 | 100 + T
        for (size_t i = 0; i < totals.size(); ++i) CHECK(p.group_of[i] == want[i]);
        CHECK(p.groups.size() == 3 && p.groups[1].vols.size() == 3 && p.groups[1].stream_at[0] == 0 && p.groups[1].chunks[0].off == 0);
        // exactly at the bound is inside it
        const Lz4BatchPlan edge = sqy::lz4_batch_plan(dflt, {100, 200}, 4, 2 * T + 300, ~(uint64_t)0, T);
        CHECK(edge.groups.size() == 1);
        const Lz4BatchPlan over = sqy::lz4_batch_plan(dflt, {100, 200}, 4, 2 * T + 299, ~(uint64_t)0, T);
        CHECK(over.groups.size() == 2);
        // a bound below one volume's tables: every volume alone, none refused
        const Lz4BatchPlan alone = sqy::lz4_batch_plan(dflt, totals, 4, 1000, ~(uint64_t)0, T);
        CHECK(alone.groups.size() == totals.size());
    }
    {   // joint_max looks at the stream only; the layout rules are untouched by the extra bytes
        const Lz4BatchPlan p = sqy::lz4_batch_plan(dflt, {C, C + 1, 4 * C}, 4, 1u << 30, C, T);
        CHECK(p.group_of[0] == 0 && p.group_of[1] == -1 && p.group_of[2] == -1);
        const Lz4BatchPlan serial = sqy::lz4_batch_plan(dflt, {C, C + 1}, 1, 1u << 30, ~(uint64_t)0, T);
        CHECK(serial.group_of[0] == 0 && serial.group_of[1] == -1);
        CHECK(sqy::lz4_batch_plan(Lz4Params("accel=-3"), {C}, 4, 1u << 30, ~(uint64_t)0, T).groups.empty());
    }
    std::printf("encode_batch_form ok\n");
    return 0;
}
