// Stand-in for <boost/align/aligned_allocator.hpp> (TEST INFRASTRUCTURE ONLY, see oracle/ref_driver.cpp):
// a minimal C++11 allocator whose blocks start on an `Alignment`-byte boundary.
#ifndef SQY_STANDIN_BOOST_ALIGNED_ALLOCATOR_HPP
#define SQY_STANDIN_BOOST_ALIGNED_ALLOCATOR_HPP
#include <cstddef>
#include <new>

#include "boost/align/aligned_alloc.hpp"

namespace boost {
namespace alignment {

template <typename T, std::size_t Alignment = alignof(T)>
struct aligned_allocator {
    typedef T value_type;

    template <typename U>
    struct rebind {
        typedef aligned_allocator<U, Alignment> other;
    };

    aligned_allocator() noexcept {}
    template <typename U>
    aligned_allocator(const aligned_allocator<U, Alignment>&) noexcept {}

    T* allocate(std::size_t n)
    {
        void* p = aligned_alloc(Alignment > alignof(T) ? Alignment : alignof(T), n * sizeof(T));
        if (!p) throw std::bad_alloc();
        return static_cast<T*>(p);
    }

    void deallocate(T* p, std::size_t) noexcept { aligned_free(p); }
};

template <typename T, typename U, std::size_t A>
bool operator==(const aligned_allocator<T, A>&, const aligned_allocator<U, A>&) noexcept { return true; }
template <typename T, typename U, std::size_t A>
bool operator!=(const aligned_allocator<T, A>&, const aligned_allocator<U, A>&) noexcept { return false; }

}  // namespace alignment
}  // namespace boost

#endif
