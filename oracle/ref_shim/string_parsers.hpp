/*
 * string_parsers.hpp -- stand-in for the reference's header of the same name (TEST INFRASTRUCTURE ONLY; on the include path of
 * oracle/ref_driver.cpp in front of the reference tree, see oracle/Makefile).
 *
 * The reference's encoders/quantiser_utils.hpp includes "string_parsers.hpp", whose own text needs Boost.StringAlgo, and names two
 * things from it, both in the helpers that turn a LUT into a header string and back (lut_to_string, lut_from_string).  The driver
 * calls neither helper, so the two templates are declared here and never defined: a call would not link.  Nothing of the quantiser's
 * arithmetic lives behind them.
 */
#ifndef SQY_ORACLE_REF_SHIM_STRING_PARSERS_HPP_
#define SQY_ORACLE_REF_SHIM_STRING_PARSERS_HPP_

#include <string>

namespace sqeazy {
namespace parsing {

template <typename iter_t>
std::string range_to_verbatim(iter_t first, iter_t last);

template <typename string_t, typename iter_t>
iter_t verbatim_to_range(string_t text, iter_t first, iter_t last);

}
}

#endif
