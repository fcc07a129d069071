// The reference driver (oracle/ref_driver.cpp, compiled into this program) over the whole stage case table under AddressSanitizer +
// UndefinedBehaviorSanitizer, on the CPU.  tests/test_oracle_reference_stages_san.py writes the table's inputs with
// oracle.gen_golden.dump_stage_cases (cases.txt + <index>.bin) and runs this on the directory: every case the goldens were taken from
// runs with 1 and 3 threads (1 only where the table says so), the two outputs must be equal, and the lossless stages must decode back.
// Behind them come the cases of tests/golden/ref_shuffles.json (frame_shuffle, tile_shuffle; see shuffle_case below), in the same format.
// The same directory holds two volumes of tests/quantiser_cases.py (quantiser.txt: name and voxel count per line, quantiser_<index>.bin):
// the reference's quantiser builds its LUTs from them and encodes them, with the default weighting and both weighting functors, 1 and 3
// threads; the tables must not depend on the thread count and every code must be the encode LUT's entry of its voxel.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

extern "C" {
int ref_diff3x3x1(int dtype, const void* in, void* out, const size_t* shape, int decode, int nthreads);
int ref_rmestbkrd(int dtype, const void* in, void* out, const size_t* shape, int nthreads, float* supports4, double* threshold);
int ref_rmbkrd_neighbor5x5x5(int dtype, const void* in, void* out, const size_t* shape, long threshold, float fraction, int nthreads);
int ref_zcurve_reorder(int dtype, const void* in, void* out, const size_t* shape, size_t tile, int decode, int nthreads);
int ref_raster_reorder(int dtype, const void* in, void* out, const size_t* shape, size_t tile, int decode, int nthreads);
int ref_bitswap1(int dtype, const void* in, void* out, size_t len, int decode, int nthreads);
int ref_hist_stats(int dtype, const void* in, size_t n, uint32_t* bins, double* stats);
int ref_quantiser_luts(const uint16_t* in, size_t n, int mode, int a, int b, int nthreads, uint8_t* lut_encode, uint16_t* lut_decode);
int ref_quantiser_encode(const uint16_t* in, size_t n, int mode, int a, int b, int nthreads, uint8_t* codes, uint16_t* lut_decode);
int ref_frame_shuffle_encode(int dtype, const void* in, void* out, const size_t* shape, size_t frame_chunk_size, int nthreads, size_t* map, size_t map_cap);
int ref_frame_shuffle_decode(int dtype, const void* in, void* out, const size_t* shape, size_t frame_chunk_size, const size_t* map, size_t n_map, int nthreads);
int ref_tile_shuffle_encode(int dtype, const void* in, void* out, const size_t* shape, size_t tile_size, int nthreads, size_t* map, size_t map_cap);
int ref_tile_shuffle_decode(int dtype, const void* in, void* out, const size_t* shape, size_t tile_size, const size_t* map, size_t n_map, int nthreads);
}

namespace {

// `bytes` bytes that start exactly `offset` bytes behind a 64-byte boundary and end where the block ends, so that the sanitizer's red
// zone follows the last of them.
struct buffer {
    unsigned char* block;
    unsigned char* first;
    buffer(size_t bytes, size_t offset) : block(nullptr), first(nullptr)
    {
        void* p = nullptr;
        if (posix_memalign(&p, 64, offset + bytes ? offset + bytes : 1)) std::abort();
        block = static_cast<unsigned char*>(p);
        first = block + offset;
        std::memset(block, 0, offset + bytes);
    }
    ~buffer() { std::free(block); }
    buffer(const buffer&) = delete;
    buffer& operator=(const buffer&) = delete;
    unsigned char* data() { return first; }
};

int run(const std::string& stage, int dt, const void* in, void* out, const size_t* shape, long p0, float p1, int decode, int nthreads)
{
    const size_t len = shape[0] * shape[1] * shape[2];
    if (stage == "diff3x3x1") return ref_diff3x3x1(dt, in, out, shape, decode, nthreads);
    if (stage == "rmestbkrd") {
        float sup[4];
        double thr;
        return ref_rmestbkrd(dt, in, out, shape, nthreads, sup, &thr);
    }
    if (stage == "rmbkrd_neighbor5x5x5") return ref_rmbkrd_neighbor5x5x5(dt, in, out, shape, p0, p1, nthreads);
    if (stage == "zcurve_reorder") return ref_zcurve_reorder(dt, in, out, shape, (size_t)p0, decode, nthreads);
    if (stage == "raster_reorder") return ref_raster_reorder(dt, in, out, shape, (size_t)p0, decode, nthreads);
    if (stage == "bitswap1") return ref_bitswap1(dt, in, out, len, decode, nthreads);
    return -1;
}

// frame_shuffle / tile_shuffle, a case of tests/golden/ref_shuffles.json: p is frame_chunk_size or tile_size.  A case the table calls
// refused must be answered with 4 (remainder) -- the stand-in median behind the reference's remainder path stops the program, so getting
// here at all says it was not reached.  Every other case is encoded with 1 and 3 threads, output and map must be equal, and the decode
// from that map must restore the input where the map is a permutation.  The map's buffer holds exactly one entry per unit.
int shuffle_case(bool frames, int dt, const void* in, const size_t* shape, size_t bytes, size_t p, bool refused)
{
    const size_t units = !p ? 0 : frames ? shape[0] / p : (shape[0] / p) * (shape[1] / p) * (shape[2] / p);
    buffer out1(bytes, 0), out3(bytes, 0), back(bytes, 0), map1(units * sizeof(size_t), 0), map3(units * sizeof(size_t), 0);
    size_t* m1 = reinterpret_cast<size_t*>(map1.data());
    size_t* m3 = reinterpret_cast<size_t*>(map3.data());
    const auto encode = frames ? ref_frame_shuffle_encode : ref_tile_shuffle_encode;
    const auto decode = frames ? ref_frame_shuffle_decode : ref_tile_shuffle_decode;
    int rc = encode(dt, in, out1.data(), shape, p, 1, m1, units);
    if (refused) return rc == 4 && encode(dt, in, out3.data(), shape, p, 3, m3, units) == 4 ? 0 : 30;
    if (rc) return rc;
    if ((rc = encode(dt, in, out3.data(), shape, p, 3, m3, units))) return rc;
    if (std::memcmp(out1.data(), out3.data(), bytes) || std::memcmp(m1, m3, units * sizeof(size_t))) return 10;
    std::memset(back.data(), 0xA5, bytes);                     // the driver zero-fills what the map does not name
    if ((rc = decode(dt, out1.data(), back.data(), shape, p, m1, units, 1))) return rc;
    std::vector<char> named(units, 0);
    size_t distinct = 0;
    for (size_t i = 0; i < units; ++i)
        if (m1[i] >= units) return 31;
        else if (!named[m1[i]]) { named[m1[i]] = 1; ++distinct; }
    if (distinct == units && std::memcmp(back.data(), in, bytes)) return 11;
    return 0;
}

// 0, or what went wrong with one volume under one weighting (mode 0: none, 1: power_of_a_b, 2: offset_power_of_a_b)
int quantiser_case(const uint16_t* vox, size_t n, int mode, int a, int b)
{
    buffer enc1(65536, 0), enc3(65536, 0), dec1(512, 0), dec3(512, 0), dec_e(512, 0), codes1(n, 0), codes3(n, 0);
    uint16_t* d1 = reinterpret_cast<uint16_t*>(dec1.data());
    uint16_t* d3 = reinterpret_cast<uint16_t*>(dec3.data());
    uint16_t* de = reinterpret_cast<uint16_t*>(dec_e.data());
    if (ref_quantiser_luts(vox, n, mode, a, b, 1, enc1.data(), d1)) return 20;
    if (ref_quantiser_luts(vox, n, mode, a, b, 3, enc3.data(), d3)) return 21;
    if (std::memcmp(enc1.data(), enc3.data(), 65536) || std::memcmp(d1, d3, 512)) return 22;
    if (ref_quantiser_encode(vox, n, mode, a, b, 1, codes1.data(), de) || std::memcmp(d1, de, 512)) return 23;
    if (ref_quantiser_encode(vox, n, mode, a, b, 3, codes3.data(), de) || std::memcmp(d1, de, 512)) return 24;
    for (size_t i = 0; i < n; ++i)
        if (codes1.data()[i] != enc1.data()[vox[i]] || codes3.data()[i] != codes1.data()[i]) return 25;
    return 0;
}

}  // namespace

int main(int argc, char** argv)
{
    if (argc < 2) return 2;
    const std::string dir = argv[1];
    std::ifstream table(dir + "/cases.txt");
    std::string line;
    int k = 0, bad = 0;
    for (; std::getline(table, line); ++k) {
        std::istringstream is(line);
        std::string id, stage, dtype;
        size_t shape[3];
        long p0;
        double p1;
        size_t offset;
        int serial_only;
        if (!(is >> id >> stage >> dtype >> shape[0] >> shape[1] >> shape[2] >> p0 >> p1 >> offset >> serial_only)) return 3;
        const int dt = dtype == "uint16" ? 1 : dtype == "uint8" ? 0 : 2;
        const size_t len = shape[0] * shape[1] * shape[2], bytes = len * (dt == 1 ? 2 : 1);
        buffer in(bytes, offset);
        std::ifstream f(dir + "/" + std::to_string(k) + ".bin", std::ios::binary);
        f.read(reinterpret_cast<char*>(in.data()), (std::streamsize)bytes);
        if ((size_t)f.gcount() != bytes) return 4;
        if (stage == "histogram") {
            std::vector<uint32_t> bins(dt == 1 ? 65536 : 256);
            double stats[10];
            if (ref_hist_stats(dt, in.data(), len, bins.data(), stats)) { std::printf("FAILED %s\n", id.c_str()); ++bad; }
            continue;
        }
        if (stage == "frame_shuffle" || stage == "tile_shuffle") {
            const int rc = shuffle_case(stage == "frame_shuffle", dt, in.data(), shape, bytes, (size_t)p0, p1 != 0.0);
            if (rc) { std::printf("FAILED %s rc=%d\n", id.c_str(), rc); ++bad; }
            continue;
        }
        buffer out1(bytes, 0), out3(bytes, 0), back(bytes, 0);
        std::memset(out1.data(), 0, bytes);
        std::memset(out3.data(), 0, bytes);
        int rc = run(stage, dt, in.data(), out1.data(), shape, p0, (float)p1, 0, 1);
        if (!rc && !serial_only) {
            rc = run(stage, dt, in.data(), out3.data(), shape, p0, (float)p1, 0, 3);
            if (!rc && std::memcmp(out1.data(), out3.data(), bytes)) rc = 10;
        }
        if (!rc && stage != "rmestbkrd" && stage != "rmbkrd_neighbor5x5x5") {
            rc = run(stage, dt, out1.data(), back.data(), shape, p0, (float)p1, 1, 1);
            if (!rc && std::memcmp(back.data(), in.data(), bytes)) rc = 11;
        }
        if (rc) { std::printf("FAILED %s rc=%d\n", id.c_str(), rc); ++bad; }
    }
    std::printf("ref_stages_san: %d cases, %d failed\n", k, bad);
    std::ifstream qtable(dir + "/quantiser.txt");
    int q = 0, qbad = 0;
    for (; std::getline(qtable, line); ++q) {
        std::istringstream is(line);
        std::string name;
        size_t n;
        if (!(is >> name >> n) || !n) return 5;
        buffer vox(n * 2, 0);
        std::ifstream f(dir + "/quantiser_" + std::to_string(q) + ".bin", std::ios::binary);
        f.read(reinterpret_cast<char*>(vox.data()), (std::streamsize)(n * 2));
        if ((size_t)f.gcount() != n * 2) return 6;
        const int weightings[3][3] = {{0, 1, 1}, {1, 1, 2}, {2, 2, 3}};
        for (const auto& w : weightings) {
            const int rc = quantiser_case(reinterpret_cast<const uint16_t*>(vox.data()), n, w[0], w[1], w[2]);
            if (rc) { std::printf("FAILED quantiser %s mode=%d rc=%d\n", name.c_str(), w[0], rc); ++qbad; }
        }
    }
    std::printf("ref_stages_san: %d quantiser volumes, %d failed\n", q, qbad);
    bad += qbad;
    return bad ? 1 : 0;
}
