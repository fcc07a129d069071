"""The case table of SQYAMD_Update_Boxes_* (tests/test_gpu_update_boxes.py runs it, tests/test_host_update_boxes.py holds every case to the
property it is named for, on the CPU with numpy).  A case is a blob shape (test_gpu_decode_box.SHAPES with the chunk geometry each is
encoded with, (600, 2, 3) with 4 KiB chunks -- frames of 6 voxels, so a 16-voxel plane word spans three frames -- and a blob of rank 2 and
of rank 1) and its boxes (origin, extent) in the caller's order.  The views and the expected volume are made here too, with numpy alone."""
from collections import namedtuple

import numpy as np

from sqeazy_amd import synth

SMALL_CHUNKS = "(blocksize_kb=4,framestep_kb=4)"

Case = namedtuple("Case", "name kind shape cfg boxes reverse gap u16_only")


def _case(name, kind, shape, cfg, boxes, reverse=False, gap=False, u16_only=False):
    return Case(name, kind, tuple(shape), cfg, [(tuple(o), tuple(e)) for o, e in boxes], reverse, gap, u16_only)


Case.rank = property(lambda c: len(c.shape))

S0, S1, S2, S3, S4, S5 = (7, 33, 31), (2, 3, 300), (3, 128, 128), (23, 131, 151), (16, 128, 128), (600, 2, 3)
_OVERLAP = [((1, 2, 3), (3, 20, 20)), ((2, 10, 10), (3, 20, 20))]
# five voxel-disjoint boxes in frames 10 .. 12 of S3
FIVE = [((10, 0, 0), (3, 40, 40)), ((10, 50, 50), (3, 30, 60)), ((10, 0, 120), (3, 131, 31)), ((10, 90, 0), (3, 41, 100)), ((10, 45, 0), (3, 4, 119))]

CASES = [
    _case("one-as-many", "one", S0, SMALL_CHUNKS, [((2, 3, 4), (3, 20, 20))]),
    _case("same-frames-5", "same_frames", S3, "", FIVE),
    _case("same-frames-small", "same_frames", S0, SMALL_CHUNKS, [((3, 0, 0), (2, 10, 31)), ((3, 12, 0), (2, 5, 7)), ((3, 12, 9), (2, 21, 22))]),
    _case("disjoint-ranges", "disjoint_ranges", S3, "", [((20, 3, 3), (3, 100, 100)), ((1, 0, 0), (2, 131, 151)), ((8, 130, 150), (1, 1, 1))]),
    _case("disjoint-ranges-wide", "disjoint_ranges", S4, "", [((0, 0, 0), (2, 128, 128)), ((12, 1, 1), (4, 100, 17)), ((5, 64, 0), (1, 64, 128))]),
    _case("abutting", "abutting", S0, SMALL_CHUNKS, [((1, 3, 3), (2, 20, 20)), ((3, 0, 0), (2, 33, 31))]),
    _case("abutting-chunks", "abutting", S2, SMALL_CHUNKS, [((0, 0, 0), (1, 128, 128)), ((1, 7, 7), (2, 100, 100))]),
    # voxels 2204 .. 2208 and 2209 .. 2212 of one row: plane word 138 (16-bit) / 276 (8-bit) holds voxels of both
    _case("shared-word-x", "shared_word_x", S0, SMALL_CHUNKS, [((2, 5, 3), (1, 1, 5)), ((2, 5, 8), (1, 1, 4))]),
    # frame 1 begins at voxel 1023, the last voxel of the 16-voxel word 63
    _case("shared-word-frames", "shared_word_frames", S0, SMALL_CHUNKS, [((0, 32, 20), (1, 1, 11)), ((1, 0, 0), (1, 1, 5))]),
    # frames 10 (voxels 60 .. 65) and 12 (72 .. 77): word 4 (64 .. 79) holds voxels of both and all of frame 11
    _case("shared-word-three-frames", "shared_word_frames", S5, SMALL_CHUNKS, [((10, 0, 0), (1, 2, 3)), ((12, 0, 1), (1, 2, 2))], gap=True, u16_only=True),
    # the 16-bit tail is voxels 7152 .. 7160, x = 22 .. 30 of the last row
    _case("shared-tail", "shared_tail", S0, SMALL_CHUNKS, [((6, 32, 22), (1, 1, 4)), ((6, 32, 27), (1, 1, 4))]),
    _case("overlap", "overlap", S0, SMALL_CHUNKS, _OVERLAP),
    _case("overlap-reversed", "overlap", S0, SMALL_CHUNKS, _OVERLAP[::-1], reverse=True),
    _case("coincide", "coincide", S2, SMALL_CHUNKS, [((1, 5, 5), (1, 100, 100)), ((1, 5, 5), (1, 100, 100))]),
    _case("whole-inside", "whole_inside", S1, SMALL_CHUNKS, [((0, 0, 0), S1), ((0, 1, 10), (2, 1, 200))]),
    _case("rank-2", "disjoint_ranges", (40, 300), SMALL_CHUNKS, [((35, 0), (5, 300)), ((3, 17), (30, 200))]),
    _case("rank-1", "disjoint_ranges", (9000,), SMALL_CHUNKS, [((4100,), (4000,)), ((100,), (50,))]),
    _case("unchanged", "unchanged", S0, SMALL_CHUNKS, _OVERLAP + [((2, 5, 3), (1, 1, 5)), ((2, 5, 8), (1, 1, 4)), ((6, 32, 22), (1, 1, 9))]),
]


def cut(full, origin, extent):
    return full[tuple(slice(o, o + n) for o, n in zip(origin, extent))]


def volume(shape, dtype):
    """the old volume of a case of lower rank (the others come from test_gpu_batch_window._blob)"""
    return synth.stack((1, 1, int(np.prod(shape))), dtype, seed=731).reshape(shape)


_made = {}


def tiles(case, dtype, full):
    """the new voxels of every box, box k's own (two boxes of one extent differ); `unchanged`: the old voxels"""
    if case.kind == "unchanged":
        return [np.ascontiguousarray(cut(full, o, e)) for o, e in case.boxes]
    out = []
    for k, (_, e) in enumerate(case.boxes):
        key = (e, np.dtype(dtype).name, k)
        if key not in _made:
            t = synth.stack((1,) * (3 - len(e)) + e, dtype, seed=1300 + k).reshape(e)
            _made[key] = t + np.asarray(k + 1, dtype)                  # (wraps; never the same as another box's tile of this extent)
        out.append(_made[key])
    return out


def pasted(full, boxes, tiles_):
    """the boxes pasted in box order"""
    v = np.array(full, copy=True)
    for (o, _), t in zip(boxes, tiles_):
        v[tuple(slice(a, a + n) for a, n in zip(o, t.shape))] = t
    return v
