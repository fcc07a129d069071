// The device table layouts of the batch and slab-set drivers and the slab set's grouping (csrc/sqy_pipeline.cpp) on the host
// (tests/test_host_batch_layout.py builds and runs this with g++, sanitizers on): every region at its alignment, the regions ascending and
// disjoint with room for what they are declared to hold -- the sizes worked out here from the counts --, `total` the end of the last one;
// the pinned staging area of an encode group large enough whatever the header text turns out to be; every joint blob of a slab set in
// exactly one group, in order, under the bounds.  Prints "batch_layout ok" and returns 0.
#include "../../sqeazy_amd/csrc/sqy_pipeline.hpp"

#include <cstdio>
#include <vector>

#define CHECK(cond)                                                                   \
    do {                                                                              \
        if (!(cond)) { std::fprintf(stderr, "line %d: %s\n", __LINE__, #cond); return 1; } \
    } while (0)

using sqy::DecodeBatchBlob;
using sqy::DecodeBatchForm;

namespace {

uint64_t g_x = 88172645463325252ull;
uint64_t rnd(uint64_t n)        // [0, n)
{
    g_x = g_x * 6364136223846793005ull + 1442695040888963407ull;
    return (g_x >> 33) % n;
}
uint64_t round_up(uint64_t v, uint64_t a) { return (v + a - 1) / a * a; }

// a region as the test expects it: where the layout puts it, the bytes it must hold, the alignment of its start
struct Region { uint64_t at, bytes, align; };

// ascending, disjoint, aligned, each starting where the one before ends but for the padding of its alignment; *end: the end of the last one
int check_regions(const std::vector<Region>& r, uint64_t* end)
{
    *end = 0;
    for (const Region& x : r) {
        CHECK(x.at % x.align == 0);
        CHECK(x.at >= *end && x.at - *end < x.align);
        *end = x.at + x.bytes;
    }
    return 0;
}

int check_rank(const std::vector<sqy::DecodeRankBlob>& blobs, uint64_t desc_bytes)
{
    const sqy::DecodeRankLayout l = sqy::decode_rank_layout(blobs, desc_bytes);
    CHECK(l.blobs.size() == blobs.size());
    std::vector<Region> r;
    for (size_t k = 0; k < blobs.size(); ++k) {
        r.push_back({l.blobs[k].scratch_at, blobs[k].scratch_bytes, 256});
        r.push_back({l.blobs[k].blk_at, blobs[k].max_blocks * 16, 256});                  // 16 bytes per LZ4 block
        r.push_back({l.blobs[k].frame_first_at, (blobs[k].max_blocks + 2) * 4, 256});     // a word per block and two
    }
    r.push_back({l.counts_at, blobs.size() * 16 * 4, 256});                               // 16 words per blob
    r.push_back({l.flag_at, 64, 4});
    r.push_back({l.desc_at, desc_bytes, 256});
    uint64_t end = 0;
    if (check_regions(r, &end)) return 1;
    CHECK(l.total == end);
    return 0;
}

// the joint tables of `g` with nparts of its blobs left, as a batch group (g != nullptr) or as a slab set's
int check_joint(uint64_t nparts, uint64_t map_bytes, uint64_t nframes, const sqy::DecodeBatchGroup* g)
{
    const sqy::DecodeJointLayout l = sqy::decode_joint_layout(nparts, map_bytes, nframes, g);
    std::vector<Region> r;
    r.push_back({l.parts_at, nparts * 64, 256});                      // Lz4JointPart: 64 bytes, holds pointers
    r.push_back({l.maps_at, map_bytes, 256});
    const uint64_t host_end = l.maps_at + map_bytes;
    r.push_back({l.jblk_at, nframes * 16, 256});
    r.push_back({l.jff_at, (nframes + 1) * 4, 4});
    r.push_back({l.jout_at, nframes * 16, 256});
    CHECK(l.parts_at == 0 && l.upload_bytes == host_end);
    uint64_t end = 0;
    if (!g) {
        if (check_regions(r, &end)) return 1;
        CHECK(l.total == end && l.jobs_bytes == 0 && l.jobs_upload_at == end);
        return 0;
    }
    const sqy::DecodeJointLayout::Family* f[3] = {&l.planes, &l.plain, &l.quantised};
    const uint64_t nj[3] = {g->planes.jobs.size(), g->plain.jobs.size(), g->quantised.jobs.size()};
    for (int k = 0; k < 3; ++k) {
        r.push_back({f[k]->jobs_at, nj[k] * 24, 256});                // Bitswap1Job: two pointers and a length
        r.push_back({f[k]->tiles_at, (nj[k] + 1) * 4, 4});
        r.push_back({f[k]->extra_at, k == 2 ? nj[k] * 512 : 0, 256}); // the quantised blobs' decode LUTs: 256 16-bit values each
    }
    const uint64_t nd = g->diff.jobs.size();
    r.push_back({l.diff.jobs_at, nd * 32, 256});                      // DiffBatchJob: two pointers, four words
    r.push_back({l.diff.tiles_at, (nd + 1) * 4, 4});                  // first_strip
    r.push_back({l.diff.extra_at, (nd + 1) * 4, 4});                  // first_tile
    if (check_regions(r, &end)) return 1;
    CHECK(l.total == end);
    CHECK(l.jobs_upload_at == l.planes.jobs_at && l.jobs_upload_at >= l.jout_at + nframes * 16 && l.jobs_bytes == end - l.jobs_upload_at);
    for (const Region& x : r) CHECK(x.at % 8 == 0 || x.align == 4);   // arrays of structs with pointers on 8 bytes
    return 0;
}

DecodeBatchBlob blob(DecodeBatchForm form, uint64_t block = 256 << 10)
{
    DecodeBatchBlob b;
    b.eligible = true;
    b.form = form;
    b.block_bytes = block;
    b.Z = 1 + (uint32_t)rnd(12); b.Y = 1 + (uint32_t)rnd(100); b.X = 8 + (uint32_t)rnd(60);
    b.len = (uint64_t)b.Z * b.Y * b.X;
    b.chain_columns = 8;
    b.total = form == DecodeBatchForm::plain || form == DecodeBatchForm::quantised ? b.len : b.len * 2;
    return b;
}

// every group of the plan of `blobs`, whole and with `dropped` blobs refused by the ranking
int check_joint_of_plan(const std::vector<DecodeBatchBlob>& blobs, const std::vector<uint8_t>* dropped)
{
    const sqy::DecodeBatchPlan plan = sqy::decode_batch_plan(blobs, 4ull << 30, dropped);
    for (const sqy::DecodeBatchGroup& g : plan.groups) {
        uint64_t left = 0, frames = 0;
        for (uint32_t b : g.blobs)
            if (!(dropped && (*dropped)[b])) { ++left; frames += 1 + rnd(5); }
        if (!left) continue;                                          // (nobody stays: the driver leaves before the tables)
        if (check_joint(left, 8 * rnd(40), frames, &g)) return 1;
        if (check_joint(left, 8 * rnd(40), frames, nullptr)) return 1;
    }
    return 0;
}

int check_encode(uint64_t nc, uint64_t nv, bool quantised, uint64_t text)
{
    const sqy::EncodeBatchLayout l = sqy::encode_batch_layout(nc, nv, quantised, text);
    std::vector<Region> r;
    r.push_back({l.table_at, nc * 24, 16});                           // Lz4BatchChunk
    r.push_back({l.volof_at, nc * 4, 16});
    r.push_back({l.jobs_at, nv * 24, 16});                            // Bitswap1Job
    r.push_back({l.tiles_at, (nv + 1) * 4, 16});
    r.push_back({l.vols_at, nv * 48, 16});                            // Lz4BatchVolume
    r.push_back({l.text_at, text, 16});
    uint64_t end = 0;
    if (check_regions(r, &end)) return 1;
    CHECK(l.upload == round_up(end, 16) && l.table_at == 0);
    // the staging area: the upload, behind it the decode LUTs of a quantised group
    CHECK(l.decode_at % 16 == 0 && l.decode_at >= end && l.decode_at - end < 16);
    CHECK(l.staging_bytes == l.decode_at + (quantised ? nv * 512 : 0) && l.staging_bytes >= l.upload);
    // the device tables: the upload, behind it what the kernels hand each other
    r.push_back({l.csize_at, nc * 4, 16});
    r.push_back({l.redo_at, (nc + 1) * 4, 16});
    r.push_back({l.foff_at, nc * 8, 16});
    r.push_back({l.vinfo_at, nv * 16, 16});
    if (check_regions(r, &end)) return 1;
    CHECK(l.tables == end && l.csize_at == l.upload);
    // what the driver pins for the group -- the layout at the worst-case text -- holds this one
    const sqy::EncodeBatchLayout worst = sqy::encode_batch_layout(nc, nv, quantised, nv * sqy::kBatchHeaderTextMax);
    CHECK(text > nv * sqy::kBatchHeaderTextMax || worst.staging_bytes >= l.staging_bytes);
    if (quantised) CHECK(worst.staging_bytes >= worst.decode_at + nv * 512 && worst.staging_bytes >= l.decode_at + nv * 512);
    return 0;
}

int check_slab_groups(const std::vector<sqy::SlabJointBlob>& joint, uint64_t bound, int inflight)
{
    const std::vector<std::vector<size_t>> groups = sqy::decode_slab_groups(joint, bound, inflight);
    size_t next = 0;
    for (size_t gi = 0; gi < groups.size(); ++gi) {
        const std::vector<size_t>& g = groups[gi];
        CHECK(!g.empty());
        uint64_t bytes = 0;
        for (size_t j : g) {
            CHECK(j == next++);                                                           // every blob once, in order
            CHECK(joint[j].block_bytes == joint[g[0]].block_bytes);                       // one block size
            bytes += round_up(joint[j].total, 256);
        }
        CHECK(inflight <= 0 || g.size() <= (size_t)inflight);
        CHECK(bytes <= bound || g.size() == 1);
        // a group is only closed when it has to be
        if (gi + 1 < groups.size()) {
            const sqy::SlabJointBlob& nx = joint[groups[gi + 1][0]];
            CHECK(nx.block_bytes != joint[g[0]].block_bytes || bytes + round_up(nx.total, 256) > bound || (inflight > 0 && g.size() == (size_t)inflight));
        }
    }
    CHECK(next == joint.size());
    return 0;
}

}  // namespace

int main()
{
    const DecodeBatchForm kForms[6] = {DecodeBatchForm::stages, DecodeBatchForm::planes, DecodeBatchForm::plain, DecodeBatchForm::quantised,
                                       DecodeBatchForm::diff_planes, DecodeBatchForm::diff_plain};
    // ---- the ranking workspace: one blob, one chunk; random groups
    if (check_rank({{0, 1}}, 0)) return 1;
    if (check_rank({{1, 1}}, 1)) return 1;
    if (check_rank({{4096, 3}, {255, 257}, {257, 64}}, 3 * 80)) return 1;
    for (int it = 0; it < 2000; ++it) {
        std::vector<sqy::DecodeRankBlob> blobs(1 + rnd(it % 10 ? 8 : 200));
        for (sqy::DecodeRankBlob& b : blobs) { b.scratch_bytes = rnd(3) ? rnd(100000) : 256 * rnd(40); b.max_blocks = 1 + rnd(rnd(4) ? 70 : 5000); }
        if (check_rank(blobs, rnd(2) ? blobs.size() * 80 : rnd(5000))) return 1;
    }
    // ---- the joint tables: a slab set's, one blob, one frame
    if (check_joint(1, 0, 1, nullptr)) return 1;
    if (check_joint(3, 8 * 17, 40, nullptr)) return 1;
    {   // zero jobs in every family (`stages` blobs only), each family alone, all four at once -- each also with every other blob dropped
        for (int only = 0; only < 7; ++only) {
            std::vector<DecodeBatchBlob> v;
            for (int i = 0; i < 9; ++i) v.push_back(blob(only < 6 ? kForms[only] : kForms[i % 6]));
            if (check_joint_of_plan(v, nullptr)) return 1;
            std::vector<uint8_t> dropped(v.size(), 0);
            for (size_t i = 0; i < v.size(); i += 2) dropped[i] = 1;
            if (check_joint_of_plan(v, &dropped)) return 1;
            const std::vector<DecodeBatchBlob> one(1, v[0]);          // one blob
            if (check_joint_of_plan(one, nullptr)) return 1;
        }
    }
    for (int it = 0; it < 2000; ++it) {     // random groups: mixed forms and block sizes, some blobs not eligible, some dropped
        std::vector<DecodeBatchBlob> v(1 + rnd(it % 10 ? 12 : 150));
        for (size_t i = 0; i < v.size(); ++i) {
            v[i] = blob(kForms[rnd(6)], (i / 5) % 2 ? 64 << 10 : 256 << 10);
            v[i].eligible = rnd(6) != 0;
        }
        std::vector<uint8_t> dropped(v.size(), 0);
        for (uint8_t& d : dropped) d = rnd(4) == 0;
        if (check_joint_of_plan(v, it % 2 ? &dropped : nullptr)) return 1;
    }
    // ---- the tables of an encode group: nv = 1, one chunk, no text and the longest, quantised and not; random groups
    for (int q = 0; q < 2; ++q) {
        for (uint64_t nv : {(uint64_t)1, (uint64_t)2, (uint64_t)7, (uint64_t)256})
            for (uint64_t per : {(uint64_t)1, (uint64_t)3})
                for (uint64_t text : {(uint64_t)0, (uint64_t)1, nv * 700 + 5, nv * sqy::kBatchHeaderTextMax - 1, nv * sqy::kBatchHeaderTextMax})
                    if (check_encode(nv * per, nv, q != 0, text)) return 1;
    }
    for (int it = 0; it < 3000; ++it) {
        const uint64_t nv = 1 + rnd(it % 10 ? 20 : 3000), nc = nv + rnd(4 * nv);
        if (check_encode(nc, nv, rnd(2) != 0, rnd(nv * sqy::kBatchHeaderTextMax + 1))) return 1;
    }
    // ---- the slab set's groups
    if (check_slab_groups({}, 4ull << 30, 0)) return 1;
    if (check_slab_groups({{1000, 262144}}, 1, 1)) return 1;
    for (int it = 0; it < 2000; ++it) {
        std::vector<sqy::SlabJointBlob> joint(1 + rnd(60));
        const uint64_t blocks[3] = {64 << 10, 256 << 10, 4 << 20};
        for (size_t j = 0; j < joint.size(); ++j) joint[j] = sqy::SlabJointBlob{1 + rnd(rnd(3) ? 100000 : 6000000), blocks[(j / (1 + it % 9)) % 3]};
        const uint64_t bounds[5] = {1, 65536, 300000, 1 << 22, 4ull << 30};
        const int inflights[6] = {-1, 0, 1, 2, 3, 100};
        if (check_slab_groups(joint, bounds[rnd(5)], inflights[rnd(6)])) return 1;
    }
    std::printf("batch_layout ok\n");
    return 0;
}
