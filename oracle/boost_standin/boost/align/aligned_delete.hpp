// Stand-in for <boost/align/aligned_delete.hpp> (TEST INFRASTRUCTURE ONLY, see oracle/ref_driver.cpp):
// the deleter of a unique_ptr over memory from aligned_alloc.
#ifndef SQY_STANDIN_BOOST_ALIGNED_DELETE_HPP
#define SQY_STANDIN_BOOST_ALIGNED_DELETE_HPP
#include "boost/align/aligned_alloc.hpp"

namespace boost {
namespace alignment {

struct aligned_delete {
    template <typename T>
    void operator()(T* p) const noexcept
    {
        if (p) {
            p->~T();
            aligned_free(p);
        }
    }
};

}  // namespace alignment
}  // namespace boost

#endif
