// sqy_batch_view.hpp -- the index walk of a strided view (SQYAMD_*_BatchStrided_*), written once for two callers: the kernels that gather
// from or scatter into a view (sqy_kernels.hip) and plain host C++ (no HIP header needed: tests/sanitize/batch_view_test.cpp holds it
// against a triple loop, index by index).
//
// A view is Z x Y x X voxels, x innermost with stride 1, rows sy voxels apart, frames sz voxels apart (sqy::BatchView, sqy_pipeline.hpp).
// Its dense order is i = (z Y + y) X + x.  The walk maps i to the voxel's offset in the view (in voxels) and to the voxels left in its
// row from there on, with two divisions at its start and none afterwards: a caller that goes through the dense order in runs asks
// view_walk_advance for the next run.
#ifndef SQY_BATCH_VIEW_HPP_
#define SQY_BATCH_VIEW_HPP_

#include <cstdint>

#if defined(__HIP__) || defined(__HIPCC__)
#define SQY_VIEW_HD __host__ __device__
#else
#define SQY_VIEW_HD
#endif

namespace sqy {

// the geometry the walk needs (a BatchView's, without its flags)
struct ViewGeometry { uint64_t Y, X, sz, sy; };

struct ViewWalk {
    uint64_t off;            // the voxel's offset in the view
    uint64_t left;           // voxels left in its row, itself included (1 .. X)
    uint64_t y;              // its row in its frame
};

// the walk at flat index i of the dense order (i < Z Y X)
SQY_VIEW_HD inline ViewWalk view_walk_start(const ViewGeometry& g, uint64_t i)
{
    uint64_t row, z;
    if (((i | g.X | g.Y) >> 32) == 0) {      // (the cheap division where everything fits 32 bits: every volume an encode call admits)
        row = (uint32_t)i / (uint32_t)g.X;
        z = (uint32_t)row / (uint32_t)g.Y;
    } else {
        row = i / g.X;
        z = row / g.Y;
    }
    const uint64_t x = i - row * g.X, y = row - z * g.Y;
    return ViewWalk{z * g.sz + y * g.sy + x, g.X - x, y};
}

// n voxels on (n <= w->left): to the next row, and the next frame, where the row ends.  Behind the view's last voxel the walk is not
// to be read.
SQY_VIEW_HD inline void view_walk_advance(const ViewGeometry& g, ViewWalk* w, uint64_t n)
{
    w->off += n;
    w->left -= n;
    if (w->left) return;
    w->left = g.X;
    if (++w->y == g.Y) {
        w->y = 0;
        w->off += g.sz - (g.Y - 1) * g.sy - g.X;
    } else
        w->off += g.sy - g.X;
}

} // namespace sqy
#endif
