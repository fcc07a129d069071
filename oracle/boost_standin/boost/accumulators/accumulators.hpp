// Stand-in for <boost/accumulators/accumulators.hpp> (TEST INFRASTRUCTURE ONLY, see oracle/ref_driver.cpp):
// the names encoders/frame_shuffle_utils.hpp and encoders/tile_shuffle_utils.hpp mention, so that both compile.  They use them in
// encode_with_remainder only -- the median path, which oracle and product refuse and the driver never reaches.  Nothing here
// computes a median: whoever gets here is stopped.
#ifndef SQY_STANDIN_BOOST_ACCUMULATORS_HPP
#define SQY_STANDIN_BOOST_ACCUMULATORS_HPP
#include <cstdio>
#include <cstdlib>

namespace boost {
namespace accumulators {

namespace tag {
struct median;
}

template <typename... Features>
struct stats;

[[noreturn]] inline void standin_median_not_available()
{
    std::fputs("boost_standin: the median path (encode_with_remainder) is not available in this build\n", stderr);
    std::abort();
}

template <typename Sample, typename Features>
struct accumulator_set {
    void operator()(const Sample&) { standin_median_not_available(); }
};

}  // namespace accumulators
}  // namespace boost

#endif
