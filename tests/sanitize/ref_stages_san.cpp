// The reference driver (oracle/ref_driver.cpp, compiled into this program) over the whole stage case table under AddressSanitizer +
// UndefinedBehaviorSanitizer, on the CPU.  tests/test_oracle_reference_stages_san.py writes the table's inputs with
// oracle.gen_golden.dump_stage_cases (cases.txt + <index>.bin) and runs this on the directory: every case the goldens were taken from
// runs with 1 and 3 threads (1 only where the table says so), the two outputs must be equal, and the lossless stages must decode back.
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
    return bad ? 1 : 0;
}
