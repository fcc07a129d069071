// Stand-in for <boost/align/aligned_alloc.hpp> (TEST INFRASTRUCTURE ONLY, see oracle/ref_driver.cpp):
// aligned_alloc / aligned_free on top of posix_memalign.
#ifndef SQY_STANDIN_BOOST_ALIGNED_ALLOC_HPP
#define SQY_STANDIN_BOOST_ALIGNED_ALLOC_HPP
#include <cstddef>
#include <cstdlib>

namespace boost {
namespace alignment {

inline void* aligned_alloc(std::size_t alignment, std::size_t size) noexcept
{
    if (alignment < sizeof(void*)) alignment = sizeof(void*);
    void* p = nullptr;
    return ::posix_memalign(&p, alignment, size ? size : 1) == 0 ? p : nullptr;
}

inline void aligned_free(void* p) noexcept { ::free(p); }

}  // namespace alignment
}  // namespace boost

#endif
