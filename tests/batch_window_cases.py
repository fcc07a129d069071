"""The boxes read out of a tiled store, shared by tests/test_host_batch_windows.py (box_windows against numpy) and
tests/test_gpu_batch_window.py (the same boxes decoded on the GPU)."""

# (parent shape, tile) -> named boxes (origin, extent): the whole parent | a box that crosses a tile corner in every dimension | exactly
# one tile | the last voxel | the first row across every tile of it
BOX_CASES = {
    ((9, 40, 72), (4, 16, 32)): [((0, 0, 0), (9, 40, 72)), ((3, 15, 31), (2, 2, 2)), ((4, 16, 32), (4, 16, 32)), ((8, 39, 71), (1, 1, 1)), ((0, 0, 0), (9, 1, 72))],
    ((5, 7), (2, 7)): [((0, 0), (5, 7)), ((1, 3), (2, 2)), ((2, 0), (2, 7)), ((4, 6), (1, 1)), ((0, 0), (5, 1))],
    ((10,), (4,)): [((0,), (10,)), ((3,), (2,)), ((4,), (4,)), ((9,), (1,)), ((0,), (1,))],
    ((3, 4, 5), (7, 9, 11)): [((0, 0, 0), (3, 4, 5)), ((1, 1, 1), (2, 2, 2)), ((2, 3, 4), (1, 1, 1)), ((0, 0, 0), (3, 1, 5))],      # a tile larger than the shape
}


def pitched(extent):
    """strides (voxels) of a box buffer with padded rows and frames"""
    strides = [1] * len(extent)
    for k in range(len(extent) - 2, -1, -1):
        strides[k] = strides[k + 1] * extent[k + 1] + (3 if k == len(extent) - 2 else 5)
    return tuple(strides)
