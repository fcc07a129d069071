// Stand-in for <boost/type_traits.hpp> (TEST INFRASTRUCTURE ONLY, see oracle/ref_driver.cpp):
// the one trait the reference's utility headers use, on top of <type_traits>.
#ifndef SQY_STANDIN_BOOST_TYPE_TRAITS_HPP
#define SQY_STANDIN_BOOST_TYPE_TRAITS_HPP
#include <type_traits>

namespace boost {
template <typename T>
using is_integral = std::is_integral<T>;
}

#endif
