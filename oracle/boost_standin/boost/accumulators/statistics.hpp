// Stand-in for <boost/accumulators/statistics.hpp> (TEST INFRASTRUCTURE ONLY, see accumulators.hpp next to this file): the one
// extractor the reference's shuffle headers name.  It stops the program; the median path is not available here.
#ifndef SQY_STANDIN_BOOST_ACCUMULATORS_STATISTICS_HPP
#define SQY_STANDIN_BOOST_ACCUMULATORS_STATISTICS_HPP
#include <boost/accumulators/accumulators.hpp>

namespace boost {
namespace accumulators {

template <typename Accumulators>
double median(const Accumulators&)
{
    standin_median_not_available();
}

}  // namespace accumulators
}  // namespace boost

#endif
