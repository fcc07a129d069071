// The batch encode's LUT routine (csrc/sqy_quantiser_lut.hpp, the host instantiation of the source the LUT kernel compiles) against
// sqy::quantiser_build_luts with the default weighting: both tables, all 65536 + 256 entries, on constructed histograms and on 1000
// seeded random ones.  tests/test_host_encode_batch_stages.py builds and runs this with g++, sanitizers on.  Prints "quantiser_lut ok"
// and returns 0; else the case (the seed), the table and the first differing entry, and returns 1.
// With a directory as its argument it also reads the histograms of tests/quantiser_cases.py from it (names.txt, <index>.histo as 65536
// uint32, <index>.enc as 65536 bytes, <index>.dec as 256 uint16: the oracle's tables, which tests/test_oracle_reference_quantiser.py
// holds to the reference's own quantiser) and compares BOTH host routines with those tables; prints "quantiser_lut table ok".
#include "../../sqeazy_amd/csrc/sqy_pipeline.hpp"
#include "../../sqeazy_amd/csrc/sqy_quantiser_lut.hpp"

#include <cstdio>
#include <fstream>
#include <random>
#include <string>
#include <vector>

namespace {
const size_t N = 65536;
int g_cases = 0;

int compare(const char* what, long seed, const std::vector<uint32_t>& histo)
{
    std::vector<unsigned char> enc_ref(N, 0xAA), enc(N, 0x55);
    uint16_t dec_ref[256], dec[256];
    for (int i = 0; i < 256; ++i) { dec_ref[i] = 0xAAAA; dec[i] = 0x5555; }
    sqy::quantiser_build_luts(histo.data(), N, enc_ref.data(), dec_ref);
    sqy::quantiser_lut_default_host(histo.data(), enc.data(), dec);
    ++g_cases;
    for (size_t i = 0; i < N; ++i)
        if (enc[i] != enc_ref[i]) {
            std::fprintf(stderr, "%s (seed %ld): lut_encode[%zu] = %u, quantiser_build_luts has %u\n", what, seed, i, (unsigned)enc[i], (unsigned)enc_ref[i]);
            return 1;
        }
    for (size_t i = 0; i < 256; ++i)
        if (dec[i] != dec_ref[i]) {
            std::fprintf(stderr, "%s (seed %ld): lut_decode[%zu] = %u, quantiser_build_luts has %u\n", what, seed, i, (unsigned)dec[i], (unsigned)dec_ref[i]);
            return 1;
        }
    return 0;
}

template <class T>
bool read_file(const std::string& path, std::vector<T>& into, size_t count)
{
    into.assign(count, T());
    std::ifstream f(path, std::ios::binary);
    f.read(reinterpret_cast<char*>(into.data()), (std::streamsize)(count * sizeof(T)));
    return (size_t)f.gcount() == count * sizeof(T);
}

// 0 when both host routines give the tables the directory holds for every histogram in it
int table(const std::string& dir)
{
    std::ifstream names(dir + "/names.txt");
    std::string name;
    int k = 0;
    for (; std::getline(names, name); ++k) {
        std::vector<uint32_t> histo;
        std::vector<unsigned char> enc_want;
        std::vector<uint16_t> dec_want;
        const std::string stem = dir + "/" + std::to_string(k);
        if (!read_file(stem + ".histo", histo, N) || !read_file(stem + ".enc", enc_want, N) || !read_file(stem + ".dec", dec_want, 256)) {
            std::fprintf(stderr, "%s: cannot read the case's files\n", name.c_str());
            return 1;
        }
        for (int routine = 0; routine < 2; ++routine) {
            const char* who = routine ? "quantiser_lut_default_host" : "quantiser_build_luts";
            std::vector<unsigned char> enc(N, 0x55);
            uint16_t dec[256];
            for (int i = 0; i < 256; ++i) dec[i] = 0x5555;
            if (routine) sqy::quantiser_lut_default_host(histo.data(), enc.data(), dec);
            else sqy::quantiser_build_luts(histo.data(), N, enc.data(), dec);
            for (size_t i = 0; i < N; ++i)
                if (enc[i] != enc_want[i]) {
                    std::fprintf(stderr, "%s: %s: lut_encode[%zu] = %u, the oracle has %u\n", name.c_str(), who, i, (unsigned)enc[i], (unsigned)enc_want[i]);
                    return 1;
                }
            for (size_t i = 0; i < 256; ++i)
                if (dec[i] != dec_want[i]) {
                    std::fprintf(stderr, "%s: %s: lut_decode[%zu] = %u, the oracle has %u\n", name.c_str(), who, i, (unsigned)dec[i], (unsigned)dec_want[i]);
                    return 1;
                }
        }
    }
    if (!k) { std::fprintf(stderr, "no histograms in %s\n", dir.c_str()); return 1; }
    std::printf("quantiser_lut table ok (%d histograms)\n", k);
    return 0;
}

std::vector<uint32_t> zeros() { return std::vector<uint32_t>(N, 0); }

// `levels` occupied bins spread over [lo, hi], counts 1 .. max_count
std::vector<uint32_t> spread(std::mt19937_64& rng, uint32_t lo, uint32_t hi, uint32_t levels, uint32_t max_count)
{
    std::vector<uint32_t> h = zeros();
    const uint32_t width = hi - lo + 1;
    if (levels > width) levels = width;
    uint32_t placed = 0;
    while (placed < levels) {
        const uint32_t b = lo + (uint32_t)(rng() % width);
        if (h[b]) continue;
        h[b] = 1 + (uint32_t)(rng() % max_count);
        ++placed;
    }
    return h;
}
}

int main(int argc, char** argv)
{
    if (argc > 1) return table(argv[1]);
    int bad = 0;
    bad += compare("all zero", -1, zeros());
    for (uint32_t at : {0u, 65535u, 31000u, 63u, 64u}) {
        std::vector<uint32_t> h = zeros();
        h[at] = 12345;
        bad += compare("one occupied bin", (long)at, h);
    }
    {   // exactly 256 and exactly 257 levels: the last case of the linear mapping, the first of the Lloyd walk; evenly spaced and packed
        for (uint32_t levels : {255u, 256u, 257u, 258u}) {
            std::vector<uint32_t> even = zeros(), packed = zeros(), top = zeros();
            for (uint32_t i = 0; i < levels; ++i) { even[i * 255] = 1 + i % 7; packed[1000 + i] = 3 + i % 5; top[65535 - i] = 1 + i % 3; }
            bad += compare("levels, evenly spaced", levels, even);
            bad += compare("levels, packed", levels, packed);
            bad += compare("levels, at the top", levels, top);
        }
    }
    {   // bin 65535 occupied / not occupied with at most 256 levels: the decode table's tail
        for (uint32_t levels : {1u, 2u, 77u, 255u, 256u}) {
            std::vector<uint32_t> with_top = zeros(), without = zeros();
            for (uint32_t i = 0; i + 1 < levels; ++i) { with_top[17 + 200 * i] = 5; without[17 + 200 * i] = 5; }
            with_top[65535] = 9;
            without[65534] = 9;
            bad += compare("top bin occupied", levels, with_top);
            bad += compare("top bin empty", levels, without);
        }
    }
    {
        std::vector<uint32_t> h(N, 1);
        bad += compare("every bin occupied, equal", 0, h);
        for (size_t i = 0; i < N; ++i) h[i] = 1 + (uint32_t)((i * 2654435761u) >> 20);
        bad += compare("every bin occupied, varied", 1, h);
    }
    {   // counts the float conversion rounds (above 2^24), in a narrow band and next to small ones
        std::vector<uint32_t> h = zeros();
        h[500] = (1u << 24) + 1;
        bad += compare("count above 2^24, alone", 0, h);
        for (uint32_t i = 0; i < 400; ++i) h[300 + i * 3] = 1 + i;
        h[500] = (1u << 24) + 3;
        h[900] = 0xffffffffu;
        bad += compare("counts above 2^24 among small ones", 1, h);
    }
    if (bad) return 1;
    for (long seed = 0; seed < 1000; ++seed) {
        std::mt19937_64 rng((uint64_t)seed * 0x9E3779B97F4A7C15ull + 1);
        std::vector<uint32_t> h;
        const char* what;
        switch (seed % 5) {
        case 0: {   // a sparse narrow band
            const uint32_t lo = (uint32_t)(rng() % 60000), width = 300 + (uint32_t)(rng() % 5000);
            what = "narrow band";
            h = spread(rng, lo, std::min<uint32_t>(65535, lo + width), 100 + (uint32_t)(rng() % 900), 1 + (uint32_t)(rng() % 100000));
            break;
        }
        case 1:     // wide and uniform
            what = "wide uniform";
            h = spread(rng, 0, 65535, 257 + (uint32_t)(rng() % 20000), 1 + (uint32_t)(rng() % 50));
            break;
        case 2: {   // long runs of empty bins between occupied clusters
            what = "clusters";
            h = zeros();
            const uint32_t clusters = 2 + (uint32_t)(rng() % 40);
            for (uint32_t c = 0; c < clusters; ++c) {
                const uint32_t at = (uint32_t)(rng() % 65000), n = 1 + (uint32_t)(rng() % 60);
                for (uint32_t i = 0; i < n && at + i < N; ++i) if (rng() % 3) h[at + i] = 1 + (uint32_t)(rng() % (c % 2 ? 20 : 2000000));
            }
            break;
        }
        case 3:     // around the boundary between the two mappings
            what = "near 256 levels";
            h = spread(rng, (uint32_t)(rng() % 1000), 65535 - (uint32_t)(rng() % 1000), 240 + (uint32_t)(rng() % 40), 1 + (uint32_t)(rng() % 1000));
            break;
        default: {  // a peak of a few heavy bins over a thin floor: buckets that close on empty bins
            what = "heavy peak";
            h = spread(rng, 0, 65535, 300 + (uint32_t)(rng() % 3000), 3);
            for (int i = 0; i < 5; ++i) h[rng() % N] = 1000000 + (uint32_t)(rng() % 100000000);
            break;
        }
        }
        if (compare(what, seed, h)) return 1;
    }
    std::printf("quantiser_lut ok (%d histograms)\n", g_cases);
    return 0;
}
