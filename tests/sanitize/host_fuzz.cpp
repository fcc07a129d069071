// Host side of libsqeazy_amd under AddressSanitizer + UndefinedBehaviorSanitizer (CPU only, no HIP): the pipeline grammar, the
// configuration strings, the sqy header (pack / unpack of untrusted bytes), base64, the LZ4 block planner, the quantiser's host LUTs
// and file readers, the frame / tile ordering, the decode and encode planners -- everything sqy_pipeline.cpp holds -- driven with valid inputs, systematic
// truncations and seeded random mutations.  Built and run by tests/test_host_sanitizers.py:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all host_fuzz.cpp ../../sqeazy_amd/csrc/sqy_pipeline.cpp
// Exit code 0 and no sanitizer report = pass.  ("race detection / sanitizers".)
#include "../../sqeazy_amd/csrc/sqy_pipeline.hpp"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <random>
#include <string>
#include <vector>

using namespace sqy;

static unsigned long g_checks = 0;
#define CHECK(c) do { ++g_checks; if (!(c)) { std::fprintf(stderr, "CHECK failed %s:%d: %s\n", __FILE__, __LINE__, #c); std::exit(2); } } while (0)

static std::string mutate(const std::string& s, std::mt19937& rng)
{
    std::string t = s;
    const char alphabet[] = "->(),=<>/verbatim_0123456789abcxyz \t\"\\{}[]:;";
    const int ops = 1 + (int)(rng() % 4);
    for (int i = 0; i < ops; ++i) {
        const unsigned op = rng() % 5;
        const size_t at = t.empty() ? 0 : rng() % (t.size() + 1);
        if (op == 0 && !t.empty()) t.erase(at % t.size(), 1 + rng() % 3);
        else if (op == 1) t.insert(at, 1, alphabet[rng() % (sizeof(alphabet) - 1)]);
        else if (op == 2 && !t.empty()) t[at % t.size()] = (char)(rng() & 0xff);
        else if (op == 3) t.insert(at, t.substr(0, rng() % (t.size() + 1)));
        else if (!t.empty()) t.resize(rng() % (t.size() + 1));
    }
    return t;
}

static void pipelines(std::mt19937& rng)
{
    const char* good[] = {
        "bitswap1->lz4", "lz4", "diff3x3x1->bitswap1->lz4", "frame_shuffle->lz4", "quantiser->bitswap1->lz4", "quantiser->lz4",
        "bitswap1->lz4(accel=1,blocksize_kb=64,framestep_kb=64)", "lz4(n_chunks_of_input=3)", "raster_reorder(tile_size=8)->lz4",
        "zcurve_reorder(tile_size=4)->bitswap1->lz4", "tile_shuffle(tile_size=16)->lz4", "bitshuffle(block_size=4096)->lz4",
        "pass_through->bitswap1->lz4", "quantiser(weighting_function=power_of_1_2)->lz4", "frame_shuffle(frame_chunk_size=4)->lz4",
        "quantiser(decode_lut_string=<verbatim>AAAA</verbatim>)->lz4", "rmbkrd_neighbor5x5x5->lz4", "remove_background->bitswap1->lz4",
        "", "->", "lz4->lz4", "bitswap1->", "(", "lz4(", "lz4()", "lz4(=)", "lz4(a=)", "lz4(=b)", "<verbatim>", "</verbatim>", "a<verbatim>b->c",
    };
    for (const char* g : good) {
        for (int round = 0; round < 400; ++round) {
            const std::string s = round == 0 ? std::string(g) : mutate(g, rng);
            bool ok = false;
            (void)split_outside_verbatim(s, "->", &ok);
            const pairs_t pr = parse_pairs(s);
            for (const auto& p : pr) (void)parse_minors(p.second);
            (void)Pipeline::reference_accepts(s);
            for (int elem = 1; elem <= 2; ++elem) {
                std::string why;
                if (Pipeline::supported(s, elem, &why)) {
                    Pipeline p = Pipeline::from_string(s, elem);
                    const std::string name = p.name();
                    CHECK(Pipeline::supported(name, elem));                       // a pipeline's own name parses again
                    // ... to the same pipeline, unless a value is empty: "key=" parses to the value "key=" (string_parsers.hpp:455-459, kept)
                    if (name.find("=,") == std::string::npos && name.find("=)") == std::string::npos)
                        CHECK(Pipeline::from_string(name, elem).name() == name);
                    else
                        (void)Pipeline::from_string(name, elem).name();
                    p.set_n_threads((int)(rng() % 70) - 3);
                    for (uint64_t nbytes : {0ull, 1ull, 12345ull, 1ull << 20, (1ull << 31) - 2, 1ull << 33})
                        (void)p.max_encoded_size(nbytes, elem);
                    for (const Stage& st : p.stages) { (void)st.config(); (void)st.full_name(); }
                }
            }
        }
    }
}

static void headers(std::mt19937& rng)
{
    const std::vector<std::vector<uint64_t>> shapes = {{1}, {7, 3}, {512, 1024, 1024}, {1, 1, 5}, {2, 3, 4, 5}, {}, {0, 1, 2}, {1ull << 40, 3, 3}};
    const char* names[] = {"bitswap1->lz4", "lz4(accel=1,blocksize_kb=256,framestep_kb=256,n_chunks_of_input=0)", "",
                           "quantiser(decode_lut_string=<verbatim>AAECAwQF\"\\\n</verbatim>)->lz4", "x"};
    for (const auto& shp : shapes)
        for (const char* nm : names)
            for (int elem = 1; elem <= 2; ++elem) {
                const uint64_t payload = rng() % (1u << 30);
                const std::string h = header_pack(elem, elem == 1 && (rng() & 1), shp, nm, payload);
                HeaderInfo hi = header_unpack(h.data(), h.data() + h.size());
                if (hi.valid) {
                    CHECK(hi.size == h.size());
                    CHECK(hi.payload_bytes == payload);
                    CHECK(hi.shape == shp);
                    (void)hi.elem_size();
                }
                // every prefix, and mutations: untrusted bytes
                for (size_t cut = 0; cut <= h.size(); cut += (h.size() > 200 ? 7 : 1)) (void)header_unpack(h.data(), h.data() + cut);
                for (int round = 0; round < 200; ++round) {
                    std::string m = mutate(h, rng);
                    HeaderInfo x = header_unpack(m.data(), m.data() + m.size());
                    if (x.valid) { (void)x.elem_size(); (void)Pipeline::supported(x.pipename, x.elem_size() > 0 ? x.elem_size() : 1); }
                }
            }
    {
        // The one escaping vector the reference holds (tests/test_header_tag_impl.cpp:87, "property_tag_cant_do_this"): what Boost's
        // JSON writer made of a quantiser LUT of raw bytes 00 40 00 80 00 and of the '/' of the closing verbatim tag -- NUL as
        // \u0000, '/' as \/, a byte >= 0x80 and '@' as they are.  The raw pipename goes in, the reference's 71 bytes must come out.
        const std::string raw = std::string("quantiser(decode_lut_string=<verbatim>") + std::string("\0@\0\200\0", 5) + "</verbatim>)";
        const std::string want("quantiser(decode_lut_string=<verbatim>\\u0000@\\u0000\200\\u0000<\\/verbatim>)", 71);
        const std::string h = header_pack(2, false, {1, 2, 3}, raw, 100);
        CHECK(h.find("\"pipename\": \"" + want + "\",\n") != std::string::npos);
        HeaderInfo hi = header_unpack(h.data(), h.data() + h.size());
        CHECK(hi.valid && hi.pipename == raw && hi.payload_bytes == 100);
        // .. and the reader takes the writer's other form of the same text (an unescaped '/') as well
        std::string h2 = h;
        const size_t at = h2.find("<\\/verbatim>");
        CHECK(at != std::string::npos);
        h2.erase(at + 1, 1);
        if (h2.size() % 2) h2.insert(0, 1, ' ');
        HeaderInfo hj = header_unpack(h2.data(), h2.data() + h2.size());
        CHECK(hj.valid && hj.pipename == raw);
    }
    std::vector<char> noise(4096);
    for (int round = 0; round < 300; ++round) {
        for (char& c : noise) c = (char)(rng() & 0xff);
        const size_t n = rng() % noise.size();
        (void)header_unpack(noise.data(), noise.data() + n);
    }
    (void)header_unpack(nullptr, nullptr);
}

static void base64(std::mt19937& rng)
{
    for (int round = 0; round < 2000; ++round) {
        std::vector<unsigned char> raw(rng() % 300);
        for (auto& c : raw) c = (unsigned char)(rng() & 0xff);
        const std::string e = base64_encode(raw.data(), raw.size());
        CHECK(base64_decode(e) == raw);
        (void)base64_decode(mutate(e, rng));
        const std::string v = to_verbatim(raw.data(), raw.size());
        CHECK(raw.empty() ? v.empty() : v.find("<verbatim>") == 0);
        std::vector<unsigned char> back;
        if (!raw.empty()) CHECK(from_verbatim(v, &back) && back == raw);
        const std::string m = mutate(v, rng);
        const bool ok = from_verbatim(m, &back);
        CHECK(ok == (m.size() >= 21));                                       // shorter than the two tags: refused, else decoded
        CHECK(!from_verbatim(v.substr(0, rng() % 21), &back));
    }
}

static void lz4_plans(std::mt19937& rng)
{
    const uint64_t blocks[] = {64u << 10, 256u << 10, 1u << 20, 4u << 20};
    for (int round = 0; round < 3000; ++round) {
        const uint64_t bb = blocks[rng() % 4];
        const uint64_t total = (rng() % 8 == 0) ? rng() % 100 : (uint64_t)rng() % (40u << 20);
        uint64_t step = (rng() % 3 == 0) ? bb : 1 + (uint64_t)rng() % (8u << 20);
        const bool serial = rng() & 1;
        const Lz4Plan p = lz4_plan_blocks(total, step, bb, serial);
        if (!p.ok || total == 0) continue;
        uint64_t at = 0;
        for (const Lz4BlockPlan& b : p.blocks) {
            CHECK(b.start == at);
            CHECK(b.n > 0 && b.n <= bb && b.n <= p.max_block);
            CHECK(b.low_in <= (int64_t)b.start && b.low_dict <= b.low_in + (int64_t)bb + 65536);
            at += b.n;
        }
        CHECK(at == total);
        CHECK(!p.frame_first.empty() && p.frame_first.front() == 0 && p.frame_first.back() == p.blocks.size());
        for (size_t f = 0; f + 1 < p.frame_first.size(); ++f) {
            CHECK(p.frame_first[f] < p.frame_first[f + 1]);
            CHECK(p.blocks[p.frame_first[f]].flags & 1u);
            CHECK(p.blocks[p.frame_first[f + 1] - 1].flags & 2u);
        }
    }
    for (const char* cfg : {"", "accel=1", "accel=-3", "accel=99", "blocksize_kb=0", "blocksize_kb=99999999", "framestep_kb=0", "n_chunks_of_input=4294967295",
                            "blocksize_kb=-1", "framestep_kb=abc", "accel=", "=", ",,,"}) {
        Lz4Params p(cfg);
        (void)p.config(); (void)p.block_bytes();
        for (uint64_t n : {0ull, 1ull, 262144ull, 262145ull, 1ull << 31, 1ull << 40}) { (void)p.bytes_per_chunk(n); (void)p.max_encoded_size(n, (unsigned)(rng() % 9)); }
    }
}

static void quantiser(std::mt19937& rng)
{
    const char* wf[] = {"none", "power_of_1_2", "offset_power_of_3_2", "power_of_2", "power_of", "power_of_1_0", "power_of_1_2_3", "offset", "",
                        "power_of_99999999999999999999_1", "power_of_-1_2", "nonepower_of_1_1"};
    std::vector<uint32_t> histo(65536);
    std::vector<unsigned char> enc(65536);
    uint16_t dec[256];
    for (const char* w : wf) {
        QuantiserWeighting q;
        const bool ok = quantiser_parse_weighting(w, &q);
        for (int kind = 0; kind < 6; ++kind) {
            std::fill(histo.begin(), histo.end(), 0u);
            if (kind == 1) histo[rng() % 65536] = 1u << 30;
            else if (kind == 2) for (auto& h : histo) h = rng() % 1000;
            else if (kind == 3) for (int i = 0; i < 200; ++i) histo[rng() % 65536] += rng() % 100000;
            else if (kind == 4) for (int i = 0; i < 300; ++i) histo[i * 7] = 0xffffffffu;
            else if (kind == 5) histo[65535] = 1, histo[0] = 1;
            if (ok) quantiser_build_luts(histo.data(), histo.size(), enc.data(), dec, q);
        }
    }
    // LUT files: well-formed, short, garbled, missing
    const std::string dir = std::getenv("SQY_SAN_TMP") ? std::getenv("SQY_SAN_TMP") : "/tmp";
    const std::string path = dir + "/sqy_san_lut.txt";
    uint16_t lut[256], back[256];
    for (int i = 0; i < 256; ++i) lut[i] = (uint16_t)(i * 257);
    CHECK(quantiser_lut_to_file(path, lut, 256));
    CHECK(quantiser_lut_from_file(path, back, 256));
    CHECK(std::memcmp(lut, back, sizeof(lut)) == 0);
    for (const char* body : {"", "1\n2\n3\n", "abc\ndef\n", "99999999999999999999\n-5\n", "1 2 3 4 5 6 7 8 9", "\0\0\0\0"}) {
        FILE* f = std::fopen(path.c_str(), "wb");
        CHECK(f != nullptr);
        std::fwrite(body, 1, std::strlen(body), f);
        std::fclose(f);
        (void)quantiser_lut_from_file(path, back, 256);
    }
    std::remove(path.c_str());
    (void)quantiser_lut_from_file(dir + "/does/not/exist", back, 256);
    (void)quantiser_lut_to_file(dir + "/does/not/exist/x", lut, 256);
}

static void orderings(std::mt19937& rng)
{
    for (int round = 0; round < 300; ++round) {
        const size_t Z = 1 + rng() % 200;
        std::vector<float> sums(Z);
        for (auto& s : sums) s = (rng() % 4 == 0) ? 0.0f : (float)(rng() % 100000) * (rng() % 2 ? 1.0f : 0.25f);
        std::vector<uint64_t> map(Z, ~0ull);
        frame_shuffle_order(sums.data(), Z, 1 + rng() % 5000, map.data());
        for (uint64_t m : map) CHECK(m < Z);
        for (int elem = 1; elem <= 2; ++elem) {
            std::fill(map.begin(), map.end(), ~0ull);
            tile_shuffle_order(sums.data(), Z, 1 + rng() % 5000, elem, map.data());
            for (uint64_t m : map) CHECK(m < Z);
        }
    }
    for (uint64_t Z : {1ull, 2ull, 16ull, 17ull, 100ull})
        for (uint64_t Y : {1ull, 16ull, 33ull})
            for (uint64_t X : {1ull, 8ull, 16ull, 100ull})
                for (uint64_t ts : {0ull, 1ull, 2ull, 3ull, 8ull, 16ull, 64ull, 128ull, 256ull, ~0ull}) {
                    for (int elem = 1; elem <= 2; ++elem) (void)raster_geometry_defined(Z, Y, X, ts, elem);
                    (void)zcurve_geometry_defined(Z, Y, X, ts);
                    (void)tile_shuffle_geometry_defined(Z, Y, X, ts);
                }
    for (uint64_t bs : {0ull, 1ull, 7ull, 8ull, 4096ull, ~0ull}) { (void)bitshuffle_block_elems(1, bs); (void)bitshuffle_block_elems(2, bs); }
    for (int n : {-5, 0, 1, 2, 1000000}) (void)clean_number_of_threads(n);
    std::vector<unsigned char> buf(1000);
    for (auto& c : buf) c = (unsigned char)(rng() & 0xff);
    for (size_t n = 0; n <= buf.size(); n += 13) (void)xxh32(buf.data(), n, (uint32_t)rng());
    // xxh32 known answers (the LZ4 frame descriptor's header checksum byte is taken from it)
    CHECK(xxh32(nullptr, 0, 0) == 0x02CC5D05u);
}

// ---- the decode planners (host arithmetic on untrusted input: a header's LZ4 parameters, shape and reorder_map, a caller's range) ----
static void lz4_geometry(std::mt19937&)
{
    for (const char* cfg : {"", "blocksize_kb=64", "accel=1,blocksize_kb=256,framestep_kb=256,n_chunks_of_input=0", "blocksize_kb=64,framestep_kb=64",
                            "blocksize_kb=64,framestep_kb=256", "n_chunks_of_input=7", "n_chunks_of_input=3", "blocksize_kb=64,n_chunks_of_input=2",
                            "framestep_kb=0,n_chunks_of_input=3", "framestep_kb=0", "blocksize_kb=4096,framestep_kb=1024"}) {
        const Lz4Params p(cfg);
        const uint64_t c = lz4_decode_geometry(p, 1ull << 30).chunk;
        for (uint64_t total : {(uint64_t)0, (uint64_t)1, c - 1, c, c + 1, 3 * c, 3 * c + 5, (uint64_t)((3ull << 30) + 12345)}) {
            const Lz4DecodeGeometry g = lz4_decode_geometry(p, total);
            CHECK(g.chunk >= 1 && g.block_bytes == p.block_bytes());
            if (total == 0) { CHECK(g.nchunks == 0 && g.max_blocks >= 1); continue; }
            CHECK(g.nchunks * g.chunk >= total && total > (g.nchunks - 1) * g.chunk);
            const Lz4Plan plan = lz4_plan_blocks(total, g.chunk, g.block_bytes, false);
            if (plan.ok) CHECK(g.max_blocks >= plan.blocks.size());
        }
    }
}

static std::vector<unsigned char> map_bytes(const std::vector<uint64_t>& m)
{
    std::vector<unsigned char> b(m.size() * 8);
    if (!m.empty()) std::memcpy(b.data(), m.data(), b.size());
    return b;
}

static void shuffle_maps(std::mt19937& rng)
{
    for (int round = 0; round < 4000; ++round) {
        const uint64_t Z = rng() % 40;
        std::vector<uint64_t> m(Z);
        for (uint64_t i = 0; i < Z; ++i) m[i] = i;
        const unsigned kind = rng() % 4;
        if (kind == 0) std::shuffle(m.begin(), m.end(), rng);                        // a permutation
        else for (uint64_t i = 0; i < Z; ++i) if (rng() % 3 == 0) m[i] = rng() % Z;  // repeated places
        bool bad = false;
        if (kind == 2 && Z) { m[rng() % Z] = Z + rng() % 3 + (rng() % 2 ? 0 : ~0ull - Z - 3); bad = true; }    // an entry >= Z
        std::vector<unsigned char> bytes = map_bytes(m);
        if (kind == 3) { bytes.resize(rng() % (Z * 8 + 20)); bad = bytes.size() != Z * 8; }                    // wrong length
        std::vector<uint64_t> unnamed = {99};
        bool permutation = false;
        const bool ok = frame_shuffle_decode_map(&bytes, Z, &unnamed, &permutation);
        CHECK(ok == !bad);
        if (!ok) continue;
        // the model: walk the slots in order, the last writer of a place wins
        std::vector<uint64_t> winner(Z, ~0ull);
        for (uint64_t i = 0; i < Z; ++i) winner[m[i]] = i;
        std::vector<uint64_t> want_unnamed;
        for (uint64_t v = 0; v < Z; ++v) if (winner[v] == ~0ull) want_unnamed.push_back(v);
        CHECK(permutation == want_unnamed.empty());
        CHECK(unnamed == want_unnamed);
        for (uint64_t i = 0; i < Z; ++i) {
            uint64_t v; std::memcpy(&v, bytes.data() + 8 * i, 8);
            CHECK(v == (winner[m[i]] == i ? m[i] : ~0ull));
        }
    }
}

// one frame-range plan against brute force over the range's voxels; `map`: the shuffle's reorder_map as the header has it
static void check_range_plan(RangeForm form, uint64_t n, int elem, uint64_t shape0, uint64_t z0, uint64_t nz, uint64_t chunk, const std::vector<uint64_t>& map,
                             uint64_t place_bytes)
{
    const uint64_t e = (uint64_t)elem, we = form == RangeForm::planes ? e : 1, total = n * (form == RangeForm::planes_lut ? 1 : e);
    const uint32_t nframes = (uint32_t)((total + chunk - 1) / chunk);
    std::vector<unsigned char> struck = map_bytes(map);
    std::vector<uint64_t> unnamed;
    bool permutation = true;
    if (form == RangeForm::shuffle) CHECK(frame_shuffle_decode_map(&struck, map.size(), &unnamed, &permutation));
    const FrameRangePlan p = frame_range_plan(form, n, elem, shape0, z0, nz, chunk, total, nframes, struck, place_bytes, map.size());
    if (nz == 0 || z0 >= shape0 || nz > shape0 - z0) { CHECK(!p.ok); return; }       // (what the drivers refuse before planning)
    CHECK(p.ok);
    for (size_t i = 0; i < p.ids.size(); ++i) CHECK(p.ids[i] < nframes && (i == 0 || p.ids[i - 1] < p.ids[i]));
    std::vector<char> sel(nframes, 0);
    for (uint32_t f : p.ids) sel[f] = 1;
    const uint64_t vpf = n / shape0, v0 = z0 * vpf, v1 = (z0 + nz) * vpf, fb = vpf * e;
    if (form == RangeForm::shuffle) {
        const uint64_t P = map.size(), np = p.pb - p.pa, cpf = place_bytes / chunk;
        CHECK(p.pa * place_bytes <= z0 * fb && (z0 + nz) * fb <= p.pb * place_bytes && p.pb <= P && p.out_bytes == np * place_bytes);
        CHECK(p.range_at + nz * fb <= p.out_bytes && p.direct == (np * place_bytes == nz * fb));
        CHECK(p.ids.size() == p.remap.size() * cpf);
        std::vector<int> cover(np, 0);
        for (uint64_t v : p.remap) { CHECK(v < np); cover[v] += 1; }
        for (const auto& run : p.zero_runs) { CHECK(run.first < run.second && run.second <= np); for (uint64_t k = run.first; k < run.second; ++k) cover[k] += 2; }
        std::vector<uint64_t> winner(P, ~0ull);
        for (uint64_t i = 0; i < P; ++i) winner[map[i]] = i;
        // every byte of the range: in a place the last slot named for it fills -- that slot's frames are decoded, to that place -- or zeroed
        for (uint64_t b = v0 * e; b < v1 * e; ++b) {
            const uint64_t place = b / place_bytes, slot = winner[place];
            CHECK(place >= p.pa && place < p.pb && cover[place - p.pa] == (slot == ~0ull ? 2 : 1));
            if (slot == ~0ull) continue;
            const uint64_t f = (slot * place_bytes + b % place_bytes) / chunk;
            CHECK(sel[f]);
            const size_t at = std::lower_bound(p.ids.begin(), p.ids.end(), (uint32_t)f) - p.ids.begin();
            CHECK(p.remap[at / cpf] == place - p.pa);
        }
        for (uint64_t k = 0; k < np; ++k) CHECK(cover[k] == 1 || cover[k] == 2);
        return;
    }
    // the selected frames back to back: where every byte of them came from
    std::vector<uint64_t> from;
    for (uint32_t f : p.ids) {
        CHECK(p.coff[f] == from.size());
        for (uint64_t b = (uint64_t)f * chunk; b < std::min<uint64_t>(total, ((uint64_t)f + 1) * chunk); ++b) from.push_back(b);
    }
    CHECK(p.out_bytes == from.size());
    if (form == RangeForm::plain) {
        CHECK(p.range_at + nz * fb <= p.out_bytes);
        for (uint64_t b = v0 * e; b < v1 * e; ++b) { CHECK(sel[b / chunk]); CHECK(from[p.range_at + (b - v0 * e)] == b); }
        return;
    }
    // the bit-plane layout: W = 8 * we plane segments of n / W words, then the verbatim tail
    const uint64_t W = 8 * we, seg = n / W, L = seg * W;
    CHECK(p.we == (int)we && p.v0 == v0 && p.v1 == v1 && p.L == L && p.w0 <= p.w1 && p.w1 <= seg);
    for (uint64_t v = v0; v < v1; ++v) {
        if (v >= L) {
            for (uint64_t k = 0; k < we; ++k) CHECK(sel[(v * we + k) / chunk]);
            CHECK(p.tail + (v1 - std::max(v0, L)) * we <= p.out_bytes);
            for (uint64_t k = 0; k < we; ++k) CHECK(from[p.tail + (v - std::max(v0, L)) * we + k] == v * we + k);
            continue;
        }
        const uint64_t w = v / W;
        CHECK(w >= p.w0 && w < p.w1);
        for (uint64_t s = 0; s < W; ++s) {
            CHECK(p.plane[s] + (p.w1 - p.w0) * we <= p.out_bytes);
            for (uint64_t k = 0; k < we; ++k) {
                CHECK(sel[((s * seg + w) * we + k) / chunk]);
                CHECK(from[p.plane[s] + (w - p.w0) * we + k] == (s * seg + w) * we + k);
            }
        }
    }
}

static void range_plans(std::mt19937& rng)
{
    const RangeForm forms[] = {RangeForm::plain, RangeForm::planes, RangeForm::planes_lut, RangeForm::shuffle};
    for (int round = 0; round < 6000; ++round) {
        const RangeForm form = forms[round % 4];
        const int elem = form == RangeForm::planes_lut ? 2 : 1 + (int)(rng() % 2);
        const uint64_t shape0 = 1 + rng() % 12, vpf = 1 + rng() % 40, n = shape0 * vpf;
        const uint64_t total = n * (uint64_t)(form == RangeForm::planes_lut ? 1 : elem);
        // hostile ranges: the volume's ends, single frames, and now and then what the drivers refuse (nz = 0, past the end)
        uint64_t z0 = rng() % shape0, nz = 1 + rng() % (shape0 - z0);
        switch (rng() % 8) {
            case 0: nz = shape0 - z0; break;
            case 1: z0 = 0; nz = 1; break;
            case 2: z0 = shape0 - 1; nz = 1; break;
            case 3: if (rng() % 4 == 0) nz = rng() % 3 ? shape0 - z0 + 1 + rng() % 3 : 0; break;
            case 4: if (rng() % 4 == 0) { z0 = shape0 + rng() % 2; nz = 1; } break;
            default: break;
        }
        uint64_t chunk = rng() % 3 == 0 ? total + rng() % 3 : 1 + rng() % total;       // (one-chunk streams among them)
        std::vector<uint64_t> map;
        uint64_t place_bytes = 0;
        if (form == RangeForm::shuffle) {
            // frame_chunk_size consecutive frames are one place; whole chunks inside whole places, more than one chunk
            uint64_t fcs = 1 + rng() % shape0;
            while (shape0 % fcs) --fcs;
            place_bytes = vpf * (uint64_t)elem * fcs;
            chunk = 1 + rng() % place_bytes;
            while (place_bytes % chunk) --chunk;
            if (total / chunk < 2) continue;
            map.resize(shape0 / fcs);
            for (uint64_t i = 0; i < map.size(); ++i) map[i] = i;
            if (rng() % 2) std::shuffle(map.begin(), map.end(), rng);
            else for (uint64_t& v : map) if (rng() % 3 == 0) v = rng() % map.size();
        }
        check_range_plan(form, n, elem, shape0, z0, nz, chunk, map, place_bytes);
    }
    // fewer voxels than a plane word holds, a volume that is no whole number of words, one frame, one chunk
    for (RangeForm form : {RangeForm::planes, RangeForm::planes_lut})
        for (int elem : {1, 2})
            for (uint64_t shape0 : {(uint64_t)1, (uint64_t)3, (uint64_t)5})
                for (uint64_t vpf : {(uint64_t)1, (uint64_t)2, (uint64_t)7, (uint64_t)16})
                    for (uint64_t z0 = 0; z0 < shape0; ++z0)
                        for (uint64_t chunk : {(uint64_t)1, (uint64_t)3, (uint64_t)16, (uint64_t)1000}) {
                            if (form == RangeForm::planes_lut && elem != 2) continue;
                            check_range_plan(form, shape0 * vpf, elem, shape0, z0, 1, chunk, {}, 0);
                            check_range_plan(form, shape0 * vpf, elem, shape0, z0, shape0 - z0, chunk, {}, 0);
                        }
    // arguments that name no range of such a stream are refused, not followed
    CHECK(!frame_range_plan(RangeForm::plain, 0, 1, 0, 0, 1, 1, 0, 0).ok);
    CHECK(!frame_range_plan(RangeForm::plain, 12, 2, 3, 0, 1, 0, 24, 1).ok);                               // no chunk size
    CHECK(!frame_range_plan(RangeForm::plain, 12, 2, 3, 0, 1, 8, 24, 2).ok);                               // not one frame per chunk
    CHECK(!frame_range_plan(RangeForm::planes, 12, 2, 3, ~0ull, 2, 8, 24, 3).ok);                          // z0 + nz wraps
    CHECK(!frame_range_plan(RangeForm::planes, 12, 4, 3, 0, 1, 8, 48, 6).ok);                              // no such voxel type
    CHECK(!frame_range_plan(RangeForm::shuffle, 12, 2, 3, 0, 1, 8, 24, 3, std::vector<unsigned char>(8), 8, 3).ok);   // a map of the wrong length
    CHECK(!frame_range_plan(RangeForm::shuffle, 12, 2, 3, 0, 1, 8, 24, 3, std::vector<unsigned char>(24), 12, 2).ok); // chunks across places
    CHECK(lz4_folds_into_shuffle(3, 3, 24, 8, 3, 8) && !lz4_folds_into_shuffle(1, 1, 24, 24, 1, 24) && !lz4_folds_into_shuffle(3, 3, 24, 8, 3, 0) &&
          !lz4_folds_into_shuffle(3, 3, 24, 8, 2, 8) && !lz4_chunks_whole(3, 3, 25, 9) && !lz4_chunks_whole(2, 3, 24, 8) && !lz4_chunks_whole(0, 0, 0, 0));
}

// ---- the encode planners (sqy_capi.cpp's EncodeCall asks them; each is checked against a brute-force model of its own) ----
static Lz4Params random_lz4(std::mt19937& rng)
{
    const char* const blocksizes[] = {"64", "256", "1024", "4096"};
    std::string cfg = std::string("blocksize_kb=") + blocksizes[rng() % 4];
    switch (rng() % 4) {
        case 0: break;                                                                   // framestep_kb = 256
        case 1: cfg += ",framestep_kb=" + std::to_string(1u << (rng() % 14)); break;
        case 2: cfg += ",framestep_kb=" + std::to_string(1 + rng() % 9000); break;
        default: cfg += ",framestep_kb=0,n_chunks_of_input=" + std::to_string(rng() % 40); break;
    }
    if (rng() % 3 == 0) cfg += ",accel=" + std::to_string((int)(rng() % 200) - 100);
    return Lz4Params(cfg);
}

static void encode_layouts(std::mt19937& rng)
{
    for (int round = 0; round < 200000; ++round) {
        const Lz4Params lz = random_lz4(rng);
        const unsigned nthreads = (unsigned)(rng() % 4);
        const uint64_t sizes[] = {0, 1, (uint64_t)rng() % 5000, (uint64_t)rng() % (64u << 20), ((uint64_t)rng() % 2048 + 1) << 10, lz.block_bytes() + rng() % 3 - 1,
                                  lz.bytes_per_chunk(1ull << 40) * (rng() % 5) + rng() % 3 - 1};
        const uint64_t total = sizes[rng() % 7] & 0xffffffffull;
        const Lz4EncodeLayout lay = lz4_encode_layout(lz, total, nthreads);
        const Lz4DecodeGeometry g = lz4_decode_geometry(lz, total);
        CHECK(lay.chunk == g.chunk && lay.nchunks == g.nchunks && lay.chunk >= 1);
        {   // EncodeCall::lz4_stage as it was
            const uint64_t chunk = total ? lz.bytes_per_chunk(total) : 1;
            const uint64_t nchunks = total ? (total + chunk - 1) / chunk : 0;
            const bool serial = nthreads == 1 && nchunks > 1;
            const Lz4LayoutKind want = !serial && chunk <= lz.block_bytes() ? Lz4LayoutKind::chunked : serial ? Lz4LayoutKind::serial : Lz4LayoutKind::linked_chunks;
            CHECK(lay.chunk == chunk && lay.nchunks == nchunks && lay.kind == want);
            CHECK(total || lay.chunked());                          // (the linked layouts are never asked for an empty stream)
        }
        if (total) {      // (no stage sees an empty stream: a call of zero voxels is refused)
            // EncodeCall::bitswap1 as it was
            const uint64_t chunk = lz.bytes_per_chunk(total);
            const bool chunked = chunk <= lz.block_bytes() && !(nthreads == 1 && total > chunk);
            CHECK(lay.chunked() == chunked && lay.chunk == chunk);
            CHECK((lay.nchunks > 1) == (total > chunk) && lay.nchunks == (total + chunk - 1) / chunk);
            // EncodeCall::frame_shuffle as it was
            const uint64_t frame_bytes = rng() % 3 ? chunk * (1 + rng() % 3) : 1 + rng() % (2 * chunk);
            const bool fused = chunk && frame_bytes % chunk == 0 && chunk <= lz.block_bytes() && !(nthreads == 1 && total > chunk);
            CHECK((lay.chunked() && frame_bytes % lay.chunk == 0) == fused);
        }
        CHECK(lay.accel == (lz.accel < 0 ? (uint32_t)(1 - lz.accel) : 1u));
    }
    const struct { int accel; uint32_t want; } edges[] = {{0, 1}, {1, 1}, {-1, 2}, {-65535, 65536}, {-65536, 65537}, {-65537, 65537}, {-2147483647 - 1, 65537}, {2147483647, 1}};
    for (const auto& e : edges) {
        Lz4Params lz;
        lz.accel = e.accel;
        CHECK(lz4_encode_layout(lz, 1u << 20, 0).accel == e.want);
    }
}

static void dedupe_and_inplace_plans(std::mt19937& rng)
{
    for (int round = 0; round < 200000; ++round) {
        const Lz4Params lz = random_lz4(rng);
        const unsigned nthreads = (unsigned)(rng() % 3);
        const uint64_t total = rng() % 4 ? ((uint64_t)rng() % 4096 + 1) << 13 : (uint64_t)rng() % (32u << 20);      // (bitswap1's tiles: 8192 voxels)
        const uint64_t words = rng() % 5 ? total / 16384 * 64 : 0;
        const Lz4EncodeLayout lay = lz4_encode_layout(lz, total, nthreads);
        const uint64_t nch = lay.nchunks, chunk = lay.chunk;
        // the duplicate search's workspace: EncodeCall::bitswap1's condition and sum as they were
        const Lz4DedupeLayout d = lz4_dedupe_layout(lay, words);
        const bool searched = words && lay.chunked() && chunk % 1024 == 0 && total > chunk;
        CHECK((d.total != 0) == searched);
        if (searched) {
            uint64_t tab = 64;
            while (tab < 2 * nch) tab <<= 1;
            CHECK(d.table == tab && (d.table & (d.table - 1)) == 0 && d.table >= 64 && d.table >= 2 * nch);
            const uint64_t ph_bytes = (words * 4 + 63) & ~(uint64_t)63, work_bytes = nch * 8 + tab * 8 + tab * 4 + 64;
            const uint64_t dup_bytes = (nch * 4 + 7) & ~(uint64_t)7, holes_bytes = nch * (1u + ((uint64_t)((uint32_t)chunk >> 10) + 63u) / 64u) * 8u;
            CHECK(d.total == ph_bytes + work_bytes + dup_bytes + holes_bytes);
            // regions: ascending, disjoint, aligned as they were (64 / 8 / 8), inside the total; each holds what is kept there
            CHECK(d.work_at >= words * 4 && d.work_at == ph_bytes && d.work_at % 64 == 0);
            CHECK(d.tab_key_at == d.work_at + nch * 8 && d.tab_val_at == d.tab_key_at + d.table * 8 && d.tab_val_at + d.table * 4 <= d.dup_at);
            CHECK(d.dup_at == d.work_at + work_bytes && d.dup_at % 8 == 0 && d.dup_at + nch * 4 <= d.holes_at);
            CHECK(d.holes_at == d.dup_at + dup_bytes && d.holes_at % 8 == 0 && d.holes_at + holes_bytes == d.total && holes_bytes >= nch * (8 + ((chunk >> 10) + 7) / 8));
        }
        // frames in place
        const bool last = rng() % 8 != 0, offset = rng() % 8 != 0;
        const unsigned mod16 = (unsigned)(rng() % 16);
        const uint64_t hdr_max = 100 + rng() % 400;
        uint64_t t0 = hdr_max;
        while ((mod16 + t0 + 11) % 16) ++t0;
        const uint64_t need = t0 + nch * (chunk + 15);
        const uint64_t capacity = rng() % 3 == 0 ? need : rng() % 3 == 0 ? need - 1 : need + (int64_t)(rng() % 4096) - 2048;
        const Lz4InplacePlan p = lz4_inplace_plan(lay, words, last, offset, mod16, capacity, hdr_max);
        const bool want = searched && last && offset && (chunk & (chunk - 1)) == 0 && need <= capacity;
        CHECK(p.on == want);
        if (p.on) {
            CHECK(kLz4FrameHead == 11 && kLz4FrameGap == 15);
            CHECK((mod16 + p.body0) % 16 == 0 && p.body0 == p.t0 + kLz4FrameHead && p.t0 >= hdr_max && p.t0 - hdr_max < 16 && p.t0 == t0);
            CHECK(p.chunk == chunk && p.in_stride == chunk + kLz4FrameGap && p.t0 + nch * (chunk + kLz4FrameGap) <= capacity);
            CHECK(!lz4_inplace_plan(lay, words, last, offset, mod16, need - 1, hdr_max).on && lz4_inplace_plan(lay, words, last, offset, mod16, need, hdr_max).on);
            CHECK(!lz4_inplace_plan(lay, 0, last, offset, mod16, capacity, hdr_max).on && !lz4_inplace_plan(lay, words, false, offset, mod16, capacity, hdr_max).on &&
                  !lz4_inplace_plan(lay, words, last, false, mod16, capacity, hdr_max).on);
        } else {
            CHECK(p.chunk == 0 && p.t0 == 0 && p.in_stride == 0 && p.body0 == 0);
        }
        // the noise digest: EncodeCall::bitswap1's test as it was, the stride from the probes of liblz4's step schedule over a chunk (from probe
        // 961 on, in whole 64-word rows; chunks of 16 KiB and more that are powers of two)
        const bool option = rng() % 8 != 0;
        const uint64_t segment = total / 16;
        static std::map<uint64_t, uint32_t> strides;
        if (chunk >= 16384 && !(chunk & (chunk - 1)) && !strides.count(chunk)) {
            uint64_t probes = 0;
            for (uint64_t pos = 1, step = 1, attempts = 64; ; pos += step, step = attempts++ >> 6) { ++probes; if (pos + step > chunk - 11) break; }
            strides[chunk] = probes > 961 ? (uint32_t)((probes - 960 + 63) / 64 * 64) : 0u;
        }
        const uint32_t stride = strides.count(chunk) ? strides[chunk] : 0u;
        CHECK(lz4_noise_digest_words(lz, lay, option, segment) == (option && stride && segment % chunk == 0 && lz.accel >= 0 ? stride : 0u));
    }
}

static void block_parallel_plans(std::mt19937& rng)
{
    const uint64_t blocks[] = {64u << 10, 256u << 10, 1u << 20};
    for (int round = 0; round < 3000; ++round) {
        const uint64_t bb = blocks[rng() % 3];
        const uint64_t total = 1 + (uint64_t)rng() % (24u << 20);
        const uint64_t step = rng() % 2 ? bb * (1 + rng() % 6) : 1 + (uint64_t)rng() % (4u << 20);
        const Lz4Plan plan = lz4_plan_blocks(total, step, bb, rng() % 3 == 0);
        if (!plan.ok || plan.blocks.empty()) continue;
        const size_t nblocks = plan.blocks.size(), nframes = plan.frame_first.size() - 1;
        std::vector<uint32_t> frame_of(nblocks);
        uint64_t longest_frame = 0;
        for (size_t f = 0; f < nframes; ++f) {
            for (uint32_t k = plan.frame_first[f]; k < plan.frame_first[f + 1]; ++k) frame_of[k] = (uint32_t)f;
            longest_frame = std::max<uint64_t>(longest_frame, plan.frame_first[f + 1] - plan.frame_first[f]);
        }
        CHECK(lz4_spec_wanted(plan) == (longest_frame >= 3 && nframes < 1024));
        // warm-up windows: inside the frame, enough bytes or from the frame's first block, and not one block more than that
        const uint64_t warmups[] = {0, 1, 65536, bb, 1 + (uint64_t)rng() % (3 * bb)};
        const uint64_t warmup = warmups[rng() % 5];
        std::vector<uint32_t> first, last;
        lz4_warmup_windows(plan, warmup, &first, &last);
        CHECK(first.size() == nblocks && last.size() == nblocks);
        for (size_t k = 0; k < nblocks; ++k) {
            const uint32_t f0 = plan.frame_first[frame_of[k]];
            CHECK(last[k] == k && first[k] <= k && first[k] >= f0);
            uint64_t have = 0;
            for (size_t j = first[k]; j < k; ++j) have += plan.blocks[j].n;
            CHECK(have >= warmup || first[k] == f0);
            if (first[k] < k) CHECK(have - plan.blocks[first[k]].n < warmup);
        }
        // redo runs
        const uint64_t run_max = 1 + rng() % 40;
        std::vector<uint32_t> ok(nblocks);
        const unsigned density = 1 + rng() % 8;
        for (size_t k = 0; k < nblocks; ++k) ok[k] = round % 50 == 0 ? 1u : (rng() % density != 0 ? 0u : 1u);
        std::vector<uint32_t> rf(nblocks, ~0u), rl(nblocks, ~0u);
        const Lz4RedoRuns r = lz4_redo_runs(plan, ok, run_max, &rf, &rl);
        CHECK(r.nruns <= nblocks);
        std::vector<unsigned char> starts(nblocks, 0);
        for (uint64_t i = 0; i < r.nruns; ++i) {
            CHECK(rf[i] <= rl[i] && rl[i] < nblocks && rl[i] - rf[i] + 1 <= run_max);
            if (i) CHECK(rf[i] > rl[i - 1]);
            for (uint32_t k = rf[i]; k <= rl[i]; ++k) { CHECK(!ok[k] && frame_of[k] == frame_of[rf[i]]); if (k > rf[i]) CHECK(!(plan.blocks[k].flags & 1u)); }
            starts[rf[i]] = 1;
        }
        for (uint64_t i = r.nruns; i < nblocks; ++i) CHECK(rf[i] == ~0u && rl[i] == ~0u);
        // model: the maximal stretches of failed blocks of one frame; each starts exactly one run
        uint64_t stretches = 0, longest = 0;
        for (size_t k = 0; k < nblocks; ++k) {
            if (ok[k] || (k > 0 && !ok[k - 1] && frame_of[k - 1] == frame_of[k])) continue;
            size_t e = k;
            while (e + 1 < nblocks && !ok[e + 1] && frame_of[e + 1] == frame_of[k]) ++e;
            ++stretches; longest = std::max<uint64_t>(longest, e - k + 1);
            CHECK(starts[k]);
        }
        CHECK(r.nruns == stretches && r.longest == longest);
        if (round % 50 == 0) CHECK(r.nruns == 0 && r.longest == 0);
    }
}


int main(int argc, char** argv)
{
    std::mt19937 rng(argc > 1 ? (unsigned)std::atoi(argv[1]) : 20261004u);
    pipelines(rng);
    headers(rng);
    base64(rng);
    lz4_plans(rng);
    quantiser(rng);
    orderings(rng);
    lz4_geometry(rng);
    shuffle_maps(rng);
    range_plans(rng);
    encode_layouts(rng);
    dedupe_and_inplace_plans(rng);
    block_parallel_plans(rng);
    std::printf("host_fuzz ok: %lu checks\n", g_checks);
    return 0;
}
