// Stand-in for <boost/utility/enable_if.hpp> (TEST INFRASTRUCTURE ONLY, see oracle/ref_driver.cpp):
// the one name the reference's utility headers use, on top of <type_traits>.
#ifndef SQY_STANDIN_BOOST_ENABLE_IF_HPP
#define SQY_STANDIN_BOOST_ENABLE_IF_HPP
#include <type_traits>

namespace boost {
template <bool Cond, typename T = void>
using enable_if_c = std::enable_if<Cond, T>;
}

#endif
