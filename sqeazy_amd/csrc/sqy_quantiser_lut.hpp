// sqy_quantiser_lut.hpp -- the quantiser's encode and decode LUT from a 65536-bin histogram, default weighting (weights 1), written once
// for two callers: the batch encode's LUT kernel (sqy_kernels.hip: one wavefront per histogram) and plain host C++ (no HIP header needed:
// tests/sanitize/quantiser_lut_test.cpp holds the host form against sqy::quantiser_build_luts, entry by entry).
//
// Same results as sqy::quantiser_build_luts (sqy_pipeline.cpp; encoders/quantiser_utils.hpp:386-418, :227-306 of the reference), the
// arithmetic in the reference's statement order, IEEE binary32 with the one double-precision total.  The numeric rules:
//   no fused multiply-add (fp contract off inside the routine; the host build has no FMA target), correctly rounded division (the
//   compiler's default for both callers; no fast-math), roundf for std::round.
//
// The walk sees the histogram through a `Blocks` object, 64 bins at a time (a wavefront: lane k holds bin k of the current block):
//   double   total()                       sum of double(float(count)) over all bins -- every term an integer below 2^32, the sum below 2^48:
//                                          exact in any order, so a caller may add in parallel
//   uint32_t levels()                      the bins with a count
//   uint64_t enter(uint32_t b)             bins [64 b, 64 b + 64) become the current block; bit k of the result: bin 64 b + k has a count
//   uint32_t count(uint32_t k)             the count of bin k of the current block (only asked for bins with a count)
//   void     codes_begin(uint32_t c)       every bin of the current block gets the code c ..
//   void     codes_from(uint32_t k, uint32_t c)   .. bins k, k + 1, .. of it the code c (k may be 64: none)
//   void     codes_write()                 the block's 64 codes go to the encode LUT
// Every value the walk computes is the same in all lanes of the wavefront (wave-uniform).
//
// Empty bins.  A bin without a count takes the walk's `else` branch as a no-op: quantile_sum + 0, the weighted sum + raw_idx * 0, the
// integral + 0 change nothing, and the rounded mean is recomputed from unchanged operands.  It changes the state only when it is the bin
// that closes a bucket (the `if` branch).  So an empty bin is looked at once: when the closing condition does not hold for it, it does not
// hold for the empty bins behind it either (same state), and the walk goes on at the next bin with a count.
#ifndef SQY_QUANTISER_LUT_HPP_
#define SQY_QUANTISER_LUT_HPP_

#include <cmath>
#include <cstdint>
#include <cstring>

#if defined(__HIP__) || defined(__HIPCC__)
#define SQY_QLUT_HD __host__ __device__
#else
#define SQY_QLUT_HD
#endif

namespace sqy {

constexpr uint32_t kQlutBins = 65536, kQlutLevels = 256, kQlutBlockBins = 64, kQlutBlocks = kQlutBins / kQlutBlockBins;

SQY_QLUT_HD inline float qlut_importance(uint32_t count) { return (float)count; }      // computeImportance with weights of 1.f

// lut_decode: kQlutLevels entries, written and read back by the walk (every lane of a wavefront writes the same values)
template <class Blocks>
SQY_QLUT_HD inline void quantiser_lut_default(Blocks& io, uint16_t* lut_decode)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const uint32_t max_compressed = kQlutLevels;
    for (uint32_t i = 0; i < max_compressed; ++i) lut_decode[i] = 0;
    const float importanceSum = (float)io.total();
    if (!(importanceSum != 0)) {
        for (uint32_t b = 0; b < kQlutBlocks; ++b) { io.enter(b); io.codes_begin(0); io.codes_write(); }
        return;
    }
    const uint32_t n_levels = io.levels();

    if (n_levels <= max_compressed) {
        // linear_mapping_quantisation: bin raw_idx gets the number of occupied bins in front of it, lut_decode[c] the last bin with code c;
        // the loop ends with the 256th level (the bins behind it keep code 0)
        uint32_t comp_idx = 0;
        for (uint32_t b = 0; b < kQlutBlocks; ++b) {
            const uint64_t occ = io.enter(b);
            io.codes_begin(comp_idx < max_compressed ? comp_idx : 0);
            if (comp_idx < max_compressed) {
                uint64_t rest = occ;
                while (rest != 0 && comp_idx < max_compressed) {
                    const uint32_t k = (uint32_t)__builtin_ctzll(rest);
                    rest &= rest - 1;
                    lut_decode[comp_idx] = (uint16_t)(b * kQlutBlockBins + k);
                    comp_idx++;
                    io.codes_from(k + 1, comp_idx < max_compressed ? comp_idx : 0);
                }
                // the empty bins up to the block's end share the code that is open now
                if (comp_idx < max_compressed && !(occ >> (kQlutBlockBins - 1))) lut_decode[comp_idx] = (uint16_t)(b * kQlutBlockBins + kQlutBlockBins - 1);
            }
            io.codes_write();
        }
        const uint16_t raw_max = 65535;
        if (comp_idx < max_compressed && comp_idx > 0 && lut_decode[comp_idx] == raw_max)
            for (uint32_t i = comp_idx; i < max_compressed; ++i) lut_decode[i] = lut_decode[comp_idx - 1];
        return;
    }

    // adaptive_lloyd_com
    uint32_t levels_available = max_compressed;
    float bucketSize = importanceSum / (float)levels_available;
    float importanceIntegral = 0, quantile_sum = 0;
    uint32_t comp_idx = 0;
    float weighted_mean_importance_in_bucket = 0;
    float index_weighted_mean_importance = 0;
    for (uint32_t b = 0; b < kQlutBlocks; ++b) {
        const uint64_t occ = io.enter(b);
        io.codes_begin(comp_idx);
        uint32_t k = 0;
        if (b == 0) {           // bin 0 is the walk's starting state
            const float first = (occ & 1u) ? qlut_importance(io.count(0)) : 0.f;
            importanceIntegral = first;
            quantile_sum = first;
            weighted_mean_importance_in_bucket = 0 * first;
            k = 1;
        }
        while (k < kQlutBlockBins) {
            const bool has = (occ >> k) & 1u;
            const bool closes = quantile_sum >= bucketSize && (comp_idx < max_compressed - 1);
            if (!has && !closes) {
                const uint64_t rest = occ >> k;                       // (bit 0 clear)
                if (rest == 0) break;
                k += (uint32_t)__builtin_ctzll(rest);
                continue;
            }
            const uint32_t raw_idx = b * kQlutBlockBins + k;
            const float importance = has ? qlut_importance(io.count(k)) : 0.f;
            if (closes) {
                lut_decode[comp_idx] = static_cast<uint16_t>(index_weighted_mean_importance);
                comp_idx++;
                levels_available--;
                quantile_sum = importance;
                weighted_mean_importance_in_bucket = (float)raw_idx * importance;
                if (importanceIntegral < importanceSum) bucketSize = (importanceSum - importanceIntegral) / (float)levels_available;
                if (quantile_sum != 0.f) index_weighted_mean_importance = ::roundf(weighted_mean_importance_in_bucket / quantile_sum);
                io.codes_from(k, comp_idx);
            } else {
                quantile_sum += importance;
                weighted_mean_importance_in_bucket += (float)raw_idx * importance;
                if (quantile_sum != 0.f) index_weighted_mean_importance = ::roundf(weighted_mean_importance_in_bucket / quantile_sum);
            }
            importanceIntegral += importance;
            ++k;
        }
        io.codes_write();
    }
    lut_decode[comp_idx] = static_cast<uint16_t>(index_weighted_mean_importance);
}

#if !defined(__HIP_DEVICE_COMPILE__)
// the host's view of a histogram: the "wavefront" is a loop
struct QlutHostBlocks {
    const uint32_t* histo;
    unsigned char* lut_encode;
    uint32_t base = 0;
    unsigned char codes[kQlutBlockBins];
    double total() const
    {
        double t = 0.;
        for (uint32_t i = 0; i < kQlutBins; ++i) t = t + qlut_importance(histo[i]);
        return t;
    }
    uint32_t levels() const
    {
        uint32_t n = 0;
        for (uint32_t i = 0; i < kQlutBins; ++i) if (qlut_importance(histo[i]) != 0.f) ++n;
        return n;
    }
    uint64_t enter(uint32_t b)
    {
        base = b * kQlutBlockBins;
        uint64_t occ = 0;
        for (uint32_t k = 0; k < kQlutBlockBins; ++k) if (histo[base + k]) occ |= (uint64_t)1 << k;
        return occ;
    }
    uint32_t count(uint32_t k) const { return histo[base + k]; }
    void codes_begin(uint32_t c) { std::memset(codes, (int)c, sizeof codes); }
    void codes_from(uint32_t k, uint32_t c) { for (; k < kQlutBlockBins; ++k) codes[k] = (unsigned char)c; }
    void codes_write() { std::memcpy(lut_encode + base, codes, sizeof codes); }
};
// lut_encode[65536], lut_decode[256] from histo[65536]
inline void quantiser_lut_default_host(const uint32_t* histo, unsigned char* lut_encode, uint16_t* lut_decode)
{
    QlutHostBlocks io{histo, lut_encode};
    quantiser_lut_default(io, lut_decode);
}
#endif

} // namespace sqy
#endif
