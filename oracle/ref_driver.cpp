/*
 * ref_driver.cpp -- thin driver around the parts of the REAL reference that build in this image
 * (TEST INFRASTRUCTURE ONLY; built into oracle/_ref/, which is git-ignored; never linked into the product).
 * The reference tree is included in place through -I, never quoted.
 *
 *  (1) the reference's utility headers, which hold all of the arithmetic of its filter stages.  They
 *      use Boost for two things only (enable_if_c / is_integral, and Boost.Align); oracle/boost_standin/
 *      maps those names onto <type_traits> and posix_memalign, and oracle/Makefile pre-includes the
 *      standard headers Boost used to drag in.  Compiled unmodified: traits.hpp, neighborhood_utils.hpp,
 *      diff_scheme_utils.hpp, sqeazy_common.hpp, sqeazy_algorithms.hpp, hist_impl.hpp,
 *      encoders/{histogram_utils, background_scheme_utils, zcurve_reorder_utils, morton,
 *      raster_reorder_utils, scalar_utils, bitplane_reorder_scalar, bitplane_reorder_sse, sse_utils,
 *      quantiser_utils, quantiser_weighters, frame_shuffle_utils, tile_shuffle_utils}.hpp and header_utils.hpp.
 *      The two shuffle headers include Boost.Accumulators for ONE thing, the median of encode_with_remainder (shapes that are no
 *      whole number of units).  boost_standin/boost/accumulators/ declares the names they mention, with bodies that stop the
 *      program; the entry points below return REF_REMAINDER for such shapes before the reference is called, so those bodies are
 *      never reached.  Everything else in the two headers -- encode_full: std::accumulate in float, sum / n, std::sort,
 *      std::find -- is plain C++ and runs as the reference wrote it.  quantiser_utils.hpp includes
 *      "string_parsers.hpp" (Boost.StringAlgo) for its two LUT-as-string helpers; oracle/ref_shim/ holds a header
 *      of that name, our own, that declares the two templates those helpers name, and the Makefile puts it on the
 *      include path in front of the reference tree.  The driver never calls the helpers.
 *      The *_scheme_impl.hpp classes around them need the dynamic-stage machinery (Boost proper) and do
 *      not build; they are thin, and the entry points below restate their few lines of CALL SEQUENCE
 *      (cited at each one) while the reference's own templates do the arithmetic.
 *  (2) liblz4 1.9.3 -- the third-party library that holds ALL of the reference's LZ4 arithmetic
 *      (the reference only calls its Frame API).  It is installed in this image
 *      (/usr/lib/x86_64-linux-gnu/liblz4.so.1.9.3, headers /opt/conda/include).  The functions
 *      below drive it with the call sequence and preferences of the reference's call sites:
 *      encoders/lz4.hpp:103-113 (prefs), encoders/lz4_utils.hpp:99-173 (encode_serial),
 *      :193-274 (encode_parallel).
 *
 * Still restated only (oracle/sqy_oracle.*): bitshuffle (its library is not in the reference tree), the sqy header
 * (Boost.PropertyTree) and with it the text form of the quantiser's decode LUT and of the shuffles' reorder_map, and the
 * remainder / median path of frame_shuffle and tile_shuffle (refused by oracle and product, never run here).  The quantiser's
 * LUTs themselves are the reference's (ref_quantiser_* below), and so are the metric, the order and the decode_map of
 * frame_shuffle and tile_shuffle on whole units (ref_frame_shuffle_* / ref_tile_shuffle_* below).
 */
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>
#include <numeric>
#include <algorithm>
#include <iostream>
#include <thread>
#include <climits>
#include <omp.h>

/* from the reference's src/cpp/src via -I */
#include "traits.hpp"
#include "sqeazy_common.hpp"
#include "neighborhood_utils.hpp"
#include "diff_scheme_utils.hpp"
#include "sqeazy_algorithms.hpp"
#include "hist_impl.hpp"
#include "encoders/histogram_utils.hpp"
#include "encoders/background_scheme_utils.hpp"
#include "encoders/morton.hpp"
#include "encoders/zcurve_reorder_utils.hpp"
#include "encoders/raster_reorder_utils.hpp"
#include "encoders/scalar_utils.hpp"
#include "encoders/bitplane_reorder_scalar.hpp"
#include "encoders/sse_utils.hpp"
#include "encoders/bitplane_reorder_sse.hpp"
#include "encoders/quantiser_utils.hpp"         /* its "string_parsers.hpp" is oracle/ref_shim/'s */
#include "encoders/frame_shuffle_utils.hpp"     /* their <boost/accumulators/...> are oracle/boost_standin/'s */
#include "encoders/tile_shuffle_utils.hpp"

#include "lz4.h"
#include "lz4frame.h"

namespace {

typedef std::vector<std::size_t> shape_t;

inline std::size_t voxels(const std::size_t* zyx) { return zyx[0] * zyx[1] * zyx[2]; }

/* The rows a halo-based stage walks: where each row starts and how many voxels it runs. */
struct rows_t {
    std::vector<std::size_t> start;
    std::size_t run;
};

/* Geometry of diff3x3x1 as encoders/diff_scheme_impl.hpp:92-103 (encode) and :154-164 (decode) ask for it: a
 * sqeazy::halo<last_plane_neighborhood<3>> over (width, height, depth), its compute_offsets_in_x, the run taken from
 * axis 0, and the whole rest of the volume as one run when there is a single start. */
typedef sqeazy::last_plane_neighborhood<3> plane3x3;

rows_t diff_rows(const std::size_t* zyx)
{
    rows_t r;
    sqeazy::halo<plane3x3, std::size_t> h(zyx[2], zyx[1], zyx[0]);
    h.compute_offsets_in_x(r.start);
    r.run = h.non_halo_end(0) - h.non_halo_begin(0);
    if (r.start.size() == 1) r.run = voxels(zyx) - r.start[0];
    return r;
}

/* diff3x3x1, both directions.  What decides the arithmetic (diff_scheme_impl.hpp:15-24): the sum of the nine voxels
 * comes from sqeazy::naive_sum<> in the voxel type T, is widened to add_unsigned<twice_as_wide<T>>, divided by
 * num_traversed_pixels<>, and the result is stored through remove_unsigned<T>.
 *   encode (:89-135): dst starts as a copy of src; every walked voxel becomes src - mean(src)
 *   decode (:151-190): dst starts as a copy of src; every walked voxel becomes src + mean(dst), in walk order */
template <typename T, bool Decode>
int diff_walk(const T* src, T* dst, const std::size_t* zyx, int nthreads)
{
    typedef typename sqeazy::remove_unsigned<T>::type signed_t;
    typedef typename sqeazy::add_unsigned<typename sqeazy::twice_as_wide<T>::type>::type wide_t;
    const std::size_t n = voxels(zyx);
    std::memcpy(dst, src, n * sizeof(T));
    const rows_t rows = diff_rows(zyx);
    const unsigned nine = sqeazy::num_traversed_pixels<plane3x3>();
    const T* summed = Decode ? dst : src;
    const signed_t* src_signed = reinterpret_cast<const signed_t*>(src);
    signed_t* dst_signed = reinterpret_cast<signed_t*>(dst);
    const long nrows = (long)rows.start.size();
#pragma omp parallel for num_threads(nthreads)
    for (long r = 0; r < nrows; ++r) {
        for (std::size_t k = 0; k < rows.run; ++k) {
            const std::size_t at = rows.start[r] + k;
            const wide_t sum = sqeazy::naive_sum<plane3x3>(summed, at, zyx[2], zyx[1], zyx[0]);
            if (Decode)
                dst[at] = static_cast<T>(src_signed[at] + sum / nine);
            else
                dst_signed[at] = static_cast<signed_t>(src[at] - sum / nine);
        }
    }
    return 0;
}

/* rmestbkrd (encoders/remove_estimated_background_scheme_impl.hpp:73-103): the four face supports from
 * sqeazy::extract_darkest_face_supports at 0.99f, their minimum as the level, and the level handed to
 * remove_background_scheme<T>, whose constructor narrows the float to T (remove_background_scheme_impl.hpp:41-44)
 * and whose encode (:87-89) keeps what lies above the level, less the level, and zeroes the rest.  That last loop
 * has no template behind it in the reference; it is the one line of arithmetic stated here. */
template <typename T>
int rmestbkrd_encode(const T* in, T* out, const std::size_t* zyx, int nthreads, float* supports4, double* threshold)
{
    const shape_t shape(zyx, zyx + 3);
    const std::vector<float> faces = sqeazy::extract_darkest_face_supports(in, shape, 0.99f, nthreads);
    float lowest = faces[0];
    for (std::size_t f = 0; f < faces.size(); ++f) {
        if (supports4 && f < 4) supports4[f] = faces[f];
        if (faces[f] < lowest) lowest = faces[f];
    }
    const T level = lowest;
    if (threshold) *threshold = (double)level;
    if (!out) return 0;
    const long n = (long)voxels(zyx);
#pragma omp parallel for num_threads(nthreads)
    for (long i = 0; i < n; ++i) out[i] = in[i] > level ? in[i] - level : 0;
    return 0;
}

/* rmbkrd_neighbor5x5x5 (encoders/flatten_to_neighborhood_scheme_impl.hpp:94-149): a sqeazy::halo<cube_neighborhood<5>>
 * built from the shape in the order it comes (:98), rows of non_halo_end(2) - non_halo_begin(2) + 1 voxels (:106).  A
 * walked voxel below the level is left alone; any other is kept or zeroed by whether sqeazy::count_neighbors_if<>
 * finds more neighbours below the level than fraction * (size<>() - 1), compared as float (:112, :142).  Voxels that
 * are not walked, or are left alone, keep what `out` held on entry.
 * With a single row start the reference takes the run from an element its list does not have (:101): returns 3. */
template <typename T>
int neighbor5_encode(const T* in, T* out, const std::size_t* zyx, long threshold, float fraction, int nthreads)
{
    typedef sqeazy::cube_neighborhood<5> cube5;
    const shape_t shape(zyx, zyx + 3);
    const T level = threshold;                     /* the constructor's narrowing of std::stoi's int (:58-60) */
    rows_t rows;
    sqeazy::halo<cube5, std::size_t> h(shape.begin(), shape.end());
    h.compute_offsets_in_x(rows.start);
    if (rows.start.size() == 1) return 3;
    rows.run = h.non_halo_end(sqeazy::row_major::x) - h.non_halo_begin(sqeazy::row_major::x) + 1;
    const float most = fraction * (sqeazy::size<cube5>() - 1);
    const auto below = [level](T v) { return v < level; };
    const long nrows = (long)rows.start.size();
#pragma omp parallel for num_threads(nthreads)
    for (long r = 0; r < nrows; ++r) {
        for (std::size_t k = 0; k < rows.run; ++k) {
            const std::size_t at = rows.start[r] + k;
            if (below(in[at])) continue;
            const unsigned dark = sqeazy::count_neighbors_if<cube5>(in + at, shape, below);
            out[at] = dark > most ? T(0) : in[at];
        }
    }
    return 0;
}

/* zcurve_reorder (encoders/zcurve_reorder_scheme_impl.hpp:43-61, :85-115): a detail::zcurve of the tile size, and
 * its encode or decode over the whole volume; done when it reports the end of the output. */
template <typename T>
int zcurve_run(const T* in, T* out, const std::size_t* zyx, std::size_t tile, int decode, int nthreads)
{
    const shape_t shape(zyx, zyx + 3);
    const std::size_t n = voxels(zyx);
    const sqeazy::detail::zcurve curve(tile);
    const T* stop = decode ? curve.decode(in, in + n, out, shape, nthreads) : curve.encode(in, in + n, out, shape, nthreads);
    return stop == out + n ? 0 : 1;
}

/* raster_reorder (encoders/raster_reorder_scheme_impl.hpp:105-143): the same with a detail::reorder. */
template <typename T>
int raster_run(const T* in, T* out, const std::size_t* zyx, std::size_t tile, int decode, int nthreads)
{
    const shape_t shape(zyx, zyx + 3);
    const std::size_t n = voxels(zyx);
    const sqeazy::detail::reorder tiles(tile);
    const T* stop = decode ? tiles.decode(in, in + n, out, shape, nthreads) : tiles.encode(in, in + n, out, shape, nthreads);
    return stop == out + n ? 0 : 1;
}

/* bitswap1 encode (encoders/bitswap_scheme_impl.hpp:97-145): the elements behind the last whole group of
 * 8 * sizeof(T) are copied as they are; the groups go through sse_bitplane_reorder_encode<1> when T is wider than a
 * byte and sse_valid_length<1,T> accepts the WHOLE length, else through scalar_bitplane_reorder_encode<1>.
 * (platform::use_vectorisation and compass' run-time SSE4 test, the other two conditions of :106-110, hold wherever
 * this driver is built: the Makefile passes -msse4.1.)  The SSE gather loads with _mm_load_si128: the caller keeps
 * 16-byte alignment wherever that branch is taken. */
template <typename T>
int bitswap1_encode(const T* in, T* out, std::size_t n, int nthreads)
{
    const std::size_t group = sizeof(T) * CHAR_BIT;
    const std::size_t whole = n - n % group;
    std::memcpy(out + whole, in + whole, (n - whole) * sizeof(T));
    const bool sse = sizeof(T) > 1 && sqeazy::detail::sse_valid_length<1, T>(n);
    const int failed = sse ? sqeazy::detail::sse_bitplane_reorder_encode<1>(in, out, whole, nthreads)
                           : sqeazy::detail::scalar_bitplane_reorder_encode<1>(in, out, whole, nthreads);
    return failed ? 1 : 0;
}

/* bitswap1 decode (encoders/bitswap_scheme_impl.hpp:181-197): the same tail, then always
 * scalar_bitplane_reorder_decode<1> with its default of one thread */
template <typename T>
int bitswap1_decode(const T* in, T* out, std::size_t n)
{
    const std::size_t group = sizeof(T) * CHAR_BIT;
    const std::size_t whole = n - n % group;
    std::memcpy(out + whole, in + whole, (n - whole) * sizeof(T));
    return sqeazy::detail::scalar_bitplane_reorder_decode<1>(in, out, whole) ? 1 : 0;
}

/* sqeazy::histogram<T>(begin, end) (hist_impl.hpp:162-185 -> fill_from_image -> fill_stats, :216-243) and
 * calc_support(0.99f) (:359-381), the call of extract_darkest_face_supports.
 * stats: smallest / largest populated bin, integral, mean, mean variation, median, median variation, mode,
 * entropy, support. */
template <typename T>
int hist_stats(const T* in, std::size_t n, std::uint32_t* bins, double* stats)
{
    if (!n) return 1;
    sqeazy::histogram<T> h(in, in + n);
    std::copy(h.bins.begin(), h.bins.end(), bins);
    stats[0] = h.smallest_populated_bin();
    stats[1] = h.largest_populated_bin();
    stats[2] = (double)h.integral();
    stats[3] = h.mean();
    stats[4] = h.mean_variation();
    stats[5] = h.median();
    stats[6] = h.median_variation();
    stats[7] = h.mode();
    stats[8] = h.entropy();
    stats[9] = h.calc_support(0.99f);
    return 0;
}

/* quantiser (encoders/quantiser_scheme_impl.hpp:176-226): the scheme holds a default-constructed sqeazy::quantiser (:64, :72), hands it
 * its thread count (:94) and calls setup_com on the voxels -- without a functor when the weighting string contains "none" (:186-187), else
 * with weighters::offset_power_of(a, b) when it contains "offset" and weighters::power_of(a, b) when not (:189-196).  The codes are
 * std::transform, or its OpenMP loop, of applyLUT over lut_encode_ (:206-223).  Histogram, weights, importance, the level count, the
 * linear mapping and the Lloyd walk all run inside the reference's quantiser (quantiser_utils.hpp:386-418, :227-306).
 * mode: 0 none, 1 power_of, 2 offset_power_of.  codes may be null: LUTs only. */
typedef sqeazy::quantiser<std::uint16_t, std::uint8_t> quantiser16;

int quantiser_run(const std::uint16_t* in, std::size_t n, int mode, int a, int b, int nthreads, std::uint8_t* lut_encode,
                  std::uint16_t* lut_decode, std::uint8_t* codes)
{
    if (!in || !n || mode < 0 || mode > 2) return 1;
    quantiser16 shrinker;
    shrinker.set_n_threads(nthreads);
    if (mode == 0)
        shrinker.setup_com(in, in + n);
    else if (mode == 2) {
        sqeazy::weighters::offset_power_of w(a, b);
        shrinker.setup_com(in, in + n, w);
    } else {
        sqeazy::weighters::power_of w(a, b);
        shrinker.setup_com(in, in + n, w);
    }
    if (lut_encode) std::copy(shrinker.lut_encode_.begin(), shrinker.lut_encode_.end(), lut_encode);
    if (lut_decode) std::copy(shrinker.lut_decode_.begin(), shrinker.lut_decode_.end(), lut_decode);
    if (!codes) return 0;
    sqeazy::applyLUT<std::uint16_t, std::uint8_t> lutApplyer(shrinker.lut_encode_);
    if (nthreads == 1)
        std::transform(in, in + n, codes, lutApplyer);
    else {
        const long len = (long)n;
#pragma omp parallel for shared(codes) firstprivate(len, in, lutApplyer) num_threads(nthreads)
        for (long idx = 0; idx < len; idx++) codes[idx] = lutApplyer(in[idx]);
    }
    return 0;
}

/* frame_shuffle and tile_shuffle.  What the entry points answer besides 0, 1 (the reference did not reach the end of its output) and 2
 * (it threw): */
enum {
    REF_REMAINDER = 4,     /* the shape is no whole number of units: the reference would take encode_with_remainder, the median path.  Worked
                              out HERE, before anything of the reference runs: the stand-in median behind that path must stay unreachable */
    REF_BAD_MAP = 5        /* decode: the map has another length than the shape has units, or names a unit the shape does not have (the
                              reference would read or write behind its buffers); encode: the caller's map has no room */
};

inline bool frame_remainder(const std::size_t* zyx, std::size_t chunk) { return zyx[0] % chunk != 0; }

inline bool tile_remainder(const std::size_t* zyx, std::size_t tile)
{
    for (int d = 0; d < 3; ++d)
        if (zyx[d] < tile || zyx[d] % tile) return true;       /* an axis shorter than the tile is all remainder */
    return false;
}

inline std::size_t frame_units(const std::size_t* zyx, std::size_t chunk) { return zyx[0] / chunk; }
inline std::size_t tile_units(const std::size_t* zyx, std::size_t tile) { return (zyx[0] / tile) * (zyx[1] / tile) * (zyx[2] / tile); }

inline bool map_fits(const std::size_t* map, std::size_t n_map, std::size_t units)
{
    if (n_map != units) return false;
    for (std::size_t i = 0; i < n_map; ++i)
        if (map[i] >= units) return false;
    return true;
}

/* frame_shuffle_scheme::encode (encoders/frame_shuffle_scheme_impl.hpp:74-93): a detail::frame_shuffle of frame_chunk_size, its encode
 * over the whole volume with the scheme's thread count, and its decode_map, which the scheme then writes into its config as text (:89;
 * that text form stays with the oracle).  The metric (float std::accumulate over a unit, divided by the size_t voxel count), std::sort and
 * std::find all run inside the reference (frame_shuffle_utils.hpp:92-172). */
template <typename T>
int frame_shuffle_encode(const T* in, T* out, const std::size_t* zyx, std::size_t chunk, int nthreads, std::size_t* map, std::size_t map_cap)
{
    if (!chunk || !voxels(zyx)) return 1;
    if (frame_remainder(zyx, chunk)) return REF_REMAINDER;
    if (map_cap < frame_units(zyx, chunk)) return REF_BAD_MAP;
    const shape_t shape(zyx, zyx + 3);
    const std::size_t n = voxels(zyx);
    sqeazy::detail::frame_shuffle frames_of(chunk);
    const T* stop = frames_of.encode(in, in + n, out, shape, nthreads);
    if (frames_of.decode_map.size() != frame_units(zyx, chunk)) return 1;
    std::copy(frames_of.decode_map.begin(), frames_of.decode_map.end(), map);
    return stop == out + n ? 0 : 1;
}

/* frame_shuffle_scheme::decode (:95-120): a detail::frame_shuffle of frame_chunk_size and the map read back from the config, its decode
 * over the whole volume; SUCCESS when it reports the end of the output.
 * THE DRIVER'S CHOICE, NOT THE REFERENCE'S: `out` is zero-filled first.  The reference copies unit i to slot decode_map[i] and touches
 * nothing else (frame_shuffle_utils.hpp:337-344), so a slot that no map entry names -- every map of an encode with equal metrics has
 * such slots -- keeps whatever the caller's buffer held.  Oracle and product make those slots zero; zero-filling here makes the
 * reference's result a function of payload and map alone, so that the three can be compared. */
template <typename T>
int frame_shuffle_decode(const T* in, T* out, const std::size_t* zyx, std::size_t chunk, const std::size_t* map, std::size_t n_map, int nthreads)
{
    if (!chunk || !voxels(zyx)) return 1;
    if (frame_remainder(zyx, chunk)) return REF_REMAINDER;
    if (!map_fits(map, n_map, frame_units(zyx, chunk))) return REF_BAD_MAP;
    const shape_t shape(zyx, zyx + 3);
    const std::size_t n = voxels(zyx);
    std::memset(out, 0, n * sizeof(T));
    const sqeazy::detail::frame_shuffle frames_of(chunk, std::vector<std::size_t>(map, map + n_map));
    const T* stop = frames_of.decode(in, in + n, out, shape, nthreads);
    return stop == out + n ? 0 : 1;
}

/* tile_shuffle_scheme::encode (encoders/tile_shuffle_scheme_impl.hpp:74-93): the same with a detail::tile_shuffle of tile_size.  The
 * tiles, the float std::accumulate over each, the quotient stored INTO THE VOXEL TYPE, std::sort and std::find are the reference's
 * (tile_shuffle_utils.hpp:104-213). */
template <typename T>
int tile_shuffle_encode(const T* in, T* out, const std::size_t* zyx, std::size_t tile, int nthreads, std::size_t* map, std::size_t map_cap)
{
    if (!tile || !voxels(zyx)) return 1;
    if (tile_remainder(zyx, tile)) return REF_REMAINDER;
    if (map_cap < tile_units(zyx, tile)) return REF_BAD_MAP;
    const shape_t shape(zyx, zyx + 3);
    const std::size_t n = voxels(zyx);
    sqeazy::detail::tile_shuffle tiles_of(tile);
    const T* stop = tiles_of.encode(in, in + n, out, shape, nthreads);
    if (tiles_of.decode_map.size() != tile_units(zyx, tile)) return 1;
    std::copy(tiles_of.decode_map.begin(), tiles_of.decode_map.end(), map);
    return stop == out + n ? 0 : 1;
}

/* tile_shuffle_scheme::decode (:95-120).  The zero fill is again THE DRIVER'S CHOICE, kept for symmetry with frame_shuffle: this decode
 * of the reference writes every voxel of the output from tiles that start out as zeros (tile_shuffle_utils.hpp:466, :529-557), so here a
 * slot nobody names is zero in the reference too. */
template <typename T>
int tile_shuffle_decode(const T* in, T* out, const std::size_t* zyx, std::size_t tile, const std::size_t* map, std::size_t n_map, int nthreads)
{
    if (!tile || !voxels(zyx)) return 1;
    if (tile_remainder(zyx, tile)) return REF_REMAINDER;
    if (!map_fits(map, n_map, tile_units(zyx, tile))) return REF_BAD_MAP;
    const shape_t shape(zyx, zyx + 3);
    const std::size_t n = voxels(zyx);
    std::memset(out, 0, n * sizeof(T));
    const sqeazy::detail::tile_shuffle tiles_of(tile, std::vector<std::size_t>(map, map + n_map));
    const T* stop = tiles_of.decode(in, in + n, out, shape, nthreads);
    return stop == out + n ? 0 : 1;
}

} /* namespace */

extern "C" {

int ref_lz4_version() { return LZ4_versionNumber(); }

/* ---- filter stages: the reference's own templates behind the call sequence of its scheme classes ------------
 * dtype: 0 = uint8, 1 = uint16, 2 = char (the tail-filter form behind a sink).  Every entry point returns 0 on
 * success and 2 when the reference threw (e.g. std::length_error from a reserve() of a wrapped size). */
#define REF_GUARD(expr) try { return (expr); } catch (...) { return 2; }

/* the offsets and halo_size_x of diff_scheme::encode (diff_scheme_impl.hpp:92-103); returns the number of offsets */
long ref_diff3x3x1_offsets(const size_t* shape, size_t* out, size_t cap, size_t* halo_size_x)
{
    try {
        const rows_t rows = diff_rows(shape);
        if (halo_size_x) *halo_size_x = rows.run;
        for (size_t i = 0; i < rows.start.size() && i < cap; ++i) out[i] = rows.start[i];
        return (long)rows.start.size();
    } catch (...) { return -2; }
}

int ref_diff3x3x1(int dtype, const void* in, void* out, const size_t* shape, int decode, int nthreads)
{
    REF_GUARD(dtype == 1 ? (decode ? diff_walk<uint16_t, true>((const uint16_t*)in, (uint16_t*)out, shape, nthreads) : diff_walk<uint16_t, false>((const uint16_t*)in, (uint16_t*)out, shape, nthreads))
            : dtype == 0 ? (decode ? diff_walk<uint8_t, true>((const uint8_t*)in, (uint8_t*)out, shape, nthreads) : diff_walk<uint8_t, false>((const uint8_t*)in, (uint8_t*)out, shape, nthreads))
                         : (decode ? diff_walk<char, true>((const char*)in, (char*)out, shape, nthreads) : diff_walk<char, false>((const char*)in, (char*)out, shape, nthreads)))
}

/* out may be null: supports and threshold only */
int ref_rmestbkrd(int dtype, const void* in, void* out, const size_t* shape, int nthreads, float* supports4, double* threshold)
{
    REF_GUARD(dtype == 1 ? rmestbkrd_encode((const uint16_t*)in, (uint16_t*)out, shape, nthreads, supports4, threshold)
                         : rmestbkrd_encode((const uint8_t*)in, (uint8_t*)out, shape, nthreads, supports4, threshold))
}

/* the L2 size extract_darkest_face_supports compares a frame with (background_scheme_utils.hpp:44-45) */
unsigned ref_cache_l2_bytes() { return compass::runtime::size::cache::level(2); }

int ref_rmbkrd_neighbor5x5x5(int dtype, const void* in, void* out, const size_t* shape, long threshold, float fraction, int nthreads)
{
    REF_GUARD(dtype == 1 ? neighbor5_encode((const uint16_t*)in, (uint16_t*)out, shape, threshold, fraction, nthreads)
                         : neighbor5_encode((const uint8_t*)in, (uint8_t*)out, shape, threshold, fraction, nthreads))
}

int ref_zcurve_reorder(int dtype, const void* in, void* out, const size_t* shape, size_t tile, int decode, int nthreads)
{
    REF_GUARD(dtype == 1 ? zcurve_run((const uint16_t*)in, (uint16_t*)out, shape, tile, decode, nthreads)
                         : zcurve_run((const uint8_t*)in, (uint8_t*)out, shape, tile, decode, nthreads))
}

int ref_raster_reorder(int dtype, const void* in, void* out, const size_t* shape, size_t tile, int decode, int nthreads)
{
    REF_GUARD(dtype == 1 ? raster_run((const uint16_t*)in, (uint16_t*)out, shape, tile, decode, nthreads)
                         : raster_run((const uint8_t*)in, (uint8_t*)out, shape, tile, decode, nthreads))
}

/* any length, any alignment except where the reference's SSE branch is taken (uint16, len % 128 == 0): 16 bytes there */
int ref_bitswap1(int dtype, const void* in, void* out, size_t len, int decode, int nthreads)
{
    REF_GUARD(dtype == 1 ? (decode ? bitswap1_decode((const uint16_t*)in, (uint16_t*)out, len) : bitswap1_encode((const uint16_t*)in, (uint16_t*)out, len, nthreads))
                         : (decode ? bitswap1_decode((const uint8_t*)in, (uint8_t*)out, len) : bitswap1_encode((const uint8_t*)in, (uint8_t*)out, len, nthreads)))
}

/* bitswap_scheme<uint16_t,1>::encode as before this entry point was generalised: 1 when the SSE branch's
 * aligned loads would fault on `in` */
int ref_bitswap1_encode_u16(const uint16_t* in, uint16_t* out, size_t len, int nthreads)
{
    if (len % 128 == 0 && (reinterpret_cast<uintptr_t>(in) & 15u) != 0) return 1;
    return ref_bitswap1(1, in, out, len, 0, nthreads);
}

/* bins: 256 or 65536 counters; stats: 10 doubles (see hist_stats) */
int ref_hist_stats(int dtype, const void* in, size_t n, uint32_t* bins, double* stats)
{
    REF_GUARD(dtype == 1 ? hist_stats((const uint16_t*)in, n, bins, stats) : hist_stats((const uint8_t*)in, n, bins, stats))
}

/* quantiser<uint16_t, uint8_t>: lut_encode 65536 entries, lut_decode 256; mode / a / b as quantiser_run takes them */
int ref_quantiser_luts(const uint16_t* in, size_t n, int mode, int a, int b, int nthreads, uint8_t* lut_encode, uint16_t* lut_decode)
{
    REF_GUARD(quantiser_run(in, n, mode, a, b, nthreads, lut_encode, lut_decode, nullptr))
}

/* the scheme's encode: n codes and the decode LUT that goes into the header */
int ref_quantiser_encode(const uint16_t* in, size_t n, int mode, int a, int b, int nthreads, uint8_t* codes, uint16_t* lut_decode)
{
    REF_GUARD(quantiser_run(in, n, mode, a, b, nthreads, nullptr, lut_decode, codes))
}

/* frame_shuffle / tile_shuffle on whole units.  dtype as above (2: the `char` form behind a sink).  `map` takes the decode_map, one size_t
 * per unit (Z / frame_chunk_size, or the tiles of the volume); 4 for a shape with a remainder -- the reference is not run on it --, 5 for a
 * map that does not fit the shape. */
#define REF_BY_DTYPE(fn, ...) REF_GUARD(dtype == 1 ? fn((const uint16_t*)in, (uint16_t*)out, __VA_ARGS__) \
                                      : dtype == 0 ? fn((const uint8_t*)in, (uint8_t*)out, __VA_ARGS__)   \
                                                   : fn((const char*)in, (char*)out, __VA_ARGS__))

int ref_frame_shuffle_encode(int dtype, const void* in, void* out, const size_t* shape, size_t frame_chunk_size, int nthreads, size_t* map, size_t map_cap)
{
    REF_BY_DTYPE(frame_shuffle_encode, shape, frame_chunk_size, nthreads, map, map_cap)
}

/* `out` is zero-filled before the reference writes to it: see frame_shuffle_decode above */
int ref_frame_shuffle_decode(int dtype, const void* in, void* out, const size_t* shape, size_t frame_chunk_size, const size_t* map, size_t n_map, int nthreads)
{
    REF_BY_DTYPE(frame_shuffle_decode, shape, frame_chunk_size, map, n_map, nthreads)
}

int ref_tile_shuffle_encode(int dtype, const void* in, void* out, const size_t* shape, size_t tile_size, int nthreads, size_t* map, size_t map_cap)
{
    REF_BY_DTYPE(tile_shuffle_encode, shape, tile_size, nthreads, map, map_cap)
}

int ref_tile_shuffle_decode(int dtype, const void* in, void* out, const size_t* shape, size_t tile_size, const size_t* map, size_t n_map, int nthreads)
{
    REF_BY_DTYPE(tile_shuffle_decode, shape, tile_size, map, n_map, nthreads)
}

static LZ4F_preferences_t make_prefs(int accel, int blocksize_id)
{
    /* encoders/lz4.hpp:103-113 */
    LZ4F_preferences_t prefs;
    std::memset(&prefs, 0, sizeof(prefs));
    prefs.frameInfo.blockSizeID = static_cast<LZ4F_blockSizeID_t>(blocksize_id);
    prefs.frameInfo.blockMode = LZ4F_blockLinked;
    prefs.frameInfo.contentChecksumFlag = LZ4F_noContentChecksum;
    prefs.frameInfo.frameType = LZ4F_frame;
    prefs.frameInfo.contentSize = 0;
    prefs.frameInfo.dictID = 0;
    prefs.frameInfo.blockChecksumFlag = LZ4F_noBlockChecksum;
    prefs.compressionLevel = accel;
    prefs.autoFlush = 0;
    prefs.favorDecSpeed = 0;
    return prefs;
}

size_t ref_lz4f_compress_bound(size_t n, int accel, int blocksize_id)
{
    LZ4F_preferences_t prefs = make_prefs(accel, blocksize_id);
    return LZ4F_compressBound(n, &prefs);
}

int ref_lz4f_header_size_max() { return LZ4F_HEADER_SIZE_MAX; }

/* call sequence of lz4::encode_serial (lz4_utils.hpp:99-173); returns bytes written, 0 on error */
size_t ref_lz4_encode_serial(const char* in, size_t n, char* out, size_t out_bytes, size_t framestep,
                             int accel, int blocksize_id)
{
    LZ4F_preferences_t prefs = make_prefs(accel, blocksize_id);
    LZ4F_compressionContext_t ctx;
    size_t rc = LZ4F_createCompressionContext(&ctx, LZ4F_VERSION);
    if (LZ4F_isError(rc)) return 0;
    size_t written = LZ4F_compressBegin(ctx, out, out_bytes, &prefs);
    if (LZ4F_isError(written)) { LZ4F_freeCompressionContext(ctx); return 0; }
    const size_t n_steps = (n + framestep - 1) / framestep;
    const char* src = in;
    const char* src_end = in + n;
    char* dst = out + written;
    for (size_t s = 0; s < n_steps; ++s) {
        const size_t src_size = (size_t)(src_end - src) < framestep ? (size_t)(src_end - src) : framestep;
        const size_t m = LZ4F_compressUpdate(ctx, dst, out_bytes - written, src, src_size, nullptr);
        if (LZ4F_isError(m)) { LZ4F_freeCompressionContext(ctx); return 0; }
        src += src_size;
        written += m;
        dst += m;
    }
    rc = LZ4F_compressEnd(ctx, dst, out_bytes - written, nullptr);
    if (LZ4F_isError(rc)) { LZ4F_freeCompressionContext(ctx); return 0; }
    written += rc;
    LZ4F_freeCompressionContext(ctx);
    return written;
}

/* call sequence of lz4::encode_parallel (lz4_utils.hpp:193-274): chunk k is framed on its own
 * into out + k*maxbytes_encoded_chunk, then the blanks are removed (:175-190). */
size_t ref_lz4_encode_parallel(const char* in, size_t n, char* out, size_t out_bytes, size_t chunk,
                               int accel, int blocksize_id, int nthreads)
{
    const size_t nchunks = (n + chunk - 1) / chunk;
    if (nchunks == 1) return ref_lz4_encode_serial(in, n, out, out_bytes, chunk, accel, blocksize_id);
    if ((size_t)nthreads > nchunks) nthreads = (int)nchunks;
    const size_t stride = ref_lz4f_compress_bound(chunk, accel, blocksize_id) + LZ4F_HEADER_SIZE_MAX;
    if (nchunks * stride > out_bytes) return 0;
    std::vector<size_t> written(nchunks, 0);
#pragma omp parallel for num_threads(nthreads) schedule(static)
    for (long k = 0; k < (long)nchunks; ++k) {
        const char* t_in = in + (size_t)k * chunk;
        const size_t len = std::min(chunk, n - (size_t)k * chunk);
        written[k] = ref_lz4_encode_serial(t_in, len, out + (size_t)k * stride, stride, chunk, accel, blocksize_id);
    }
    char* value = out + written[0];
    for (size_t k = 1; k < nchunks; ++k) {
        std::memmove(value, out + k * stride, written[k]);
        value += written[k];
    }
    return (size_t)(value - out);
}

/* block level: LZ4_compress_fast_continue on a fresh stream (what LZ4F_makeBlock runs for the
 * first block of a block-linked frame), capacity as given. */
int ref_lz4_block_fast_continue(const char* src, int n, char* dst, int cap, int accel)
{
    LZ4_stream_t* s = LZ4_createStream();
    if (!s) return -1;
    const int r = LZ4_compress_fast_continue(s, src, dst, n, cap, accel);
    LZ4_freeStream(s);
    return r;
}

/* decoder: encoders/lz4.hpp:257-339 (LZ4F_decompress over concatenated frames) */
size_t ref_lz4_decode_frames(const char* in, size_t n, char* out, size_t cap)
{
    LZ4F_decompressionContext_t dctx;
    if (LZ4F_isError(LZ4F_createDecompressionContext(&dctx, LZ4F_VERSION))) return (size_t)-1;
    const char* src = in;
    const char* src_end = in + n;
    char* dst = out;
    char* dst_end = out + cap;
    size_t ret = 1;
    while (src < src_end) {
        size_t dsz = (size_t)(dst_end - dst);
        size_t ssz = (size_t)(src_end - src);
        ret = LZ4F_decompress(dctx, dst, &dsz, src, &ssz, nullptr);
        if (LZ4F_isError(ret)) { LZ4F_freeDecompressionContext(dctx); return (size_t)-1; }
        src += ssz;
        dst += dsz;
        if (ssz == 0 && dsz == 0) break;
    }
    LZ4F_freeDecompressionContext(dctx);
    return (size_t)(dst - out);
}

} /* extern "C" */
