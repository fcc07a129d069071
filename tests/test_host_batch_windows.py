"""Windows on the host, under AddressSanitizer + UndefinedBehaviorSanitizer, built with g++ as test_host_batch_views.py builds its target
(tests/sanitize/batch_window_test.cpp, a stand-alone program): sqy::admit_window -- every rule, ranks 1 to 3, an origin + extent that
overflows long --, the clip the window kernels compile (csrc/sqy_batch_window.hpp) against a triple loop for every window of small blobs
and for rows that cross the 128-voxel runs, and the window table's layout.  And box_windows, the pure-Python cut of a box into windows."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from batch_window_cases import BOX_CASES, pitched

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sqeazy_amd", "csrc")
SAN = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:exitcode=97:abort_on_error=0", UBSAN_OPTIONS="halt_on_error=1:exitcode=98:print_stacktrace=1")
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "batch_window_test")
    # (the kernels' job struct lives in sqy_kernels.h, which names HIP's stream type: the runtime's C header, nothing linked)
    subprocess.check_call(["g++"] + SAN + ["-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(ROCM, "include"), os.path.join(ROOT, "tests", "sanitize", "batch_window_test.cpp"),
                                           os.path.join(CSRC, "sqy_pipeline.cpp"), "-o", exe, "-lpthread"])
    r = subprocess.run([exe], env=ENV, capture_output=True, text=True, timeout=120)
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    assert r.returncode == 0 and "batch_window ok" in r.stdout, (r.returncode, r.stdout, r.stderr[-2000:])


def _scatter(parent, tile, origin, extent, strides):
    """the box rebuilt from box_windows' answer with numpy, in a flat buffer of the box's reach; returns (box, times each voxel was written)"""
    import sqeazy_amd
    itemsize, base = parent.itemsize, 1 << 20
    shape = parent.shape
    indices, origins, ptrs, shapes, sts = sqeazy_amd.box_windows(shape, tile, origin, extent, base, strides, itemsize)
    grid = [-(-d // t) for d, t in zip(shape, tile)]
    assert indices == sorted(set(indices)) and len(indices) == len(origins) == len(ptrs) == len(shapes) == len(sts)
    # the tiles as tile_views cuts them, in its order
    tptrs, tshapes, _ = sqeazy_amd.tile_views(0, shape, tile, 1)
    assert len(tptrs) == int(np.prod(grid))
    st = list(strides) if strides is not None else [int(np.prod(extent[k + 1:])) for k in range(len(extent))]
    reach = sum((e - 1) * s for e, s in zip(extent, st)) + 1
    buf = np.zeros(reach, dtype=parent.dtype)
    seen = np.zeros(reach, dtype=np.int32)
    for i, o, p, s, s_st in zip(indices, origins, ptrs, shapes, sts):
        assert tuple(s_st) == tuple(st) and (p - base) % itemsize == 0
        t_origin = np.unravel_index(tptrs[i], shape)                    # (tile_views at base 0, one byte a voxel: the pointer is the flat index)
        assert all(0 <= a and a + n <= ts and n >= 1 for a, n, ts in zip(o, s, tshapes[i]))
        tile_data = parent[tuple(slice(int(a), int(a) + n) for a, n in zip(t_origin, tshapes[i]))]
        window = tile_data[tuple(slice(a, a + n) for a, n in zip(o, s))]
        idx = (p - base) // itemsize + sum(np.arange(n).reshape([-1 if k == j else 1 for k in range(len(s))]) * st[j] for j, n in enumerate(s))
        assert idx.min() >= 0 and idx.max() < reach
        buf[idx.reshape(-1)] = window.reshape(-1)
        seen[idx.reshape(-1)] += 1
    return buf, seen, st, len(indices)


def _check_box(parent, tile, origin, extent, strides):
    buf, seen, st, ntiles = _scatter(parent, tile, origin, extent, strides)
    want = parent[tuple(slice(o, o + e) for o, e in zip(origin, extent))]
    idx = sum(np.arange(n).reshape([-1 if k == j else 1 for k in range(len(extent))]) * st[j] for j, n in enumerate(extent))
    assert np.array_equal(buf[idx], want)
    inside = np.zeros(seen.size, dtype=bool)
    inside[idx.reshape(-1)] = True
    assert np.all(seen[inside] == 1) and np.all(seen[~inside] == 0)    # every box voxel exactly once, the gaps never
    # the tiles are exactly those the box reaches
    assert ntiles == int(np.prod([(o + e - 1) // t - o // t + 1 for o, e, t in zip(origin, extent, tile)]))


@pytest.mark.parametrize("shape, tile", list(BOX_CASES))
def test_box_windows_rebuild_the_box(shape, tile):
    parent = (np.arange(int(np.prod(shape)), dtype=np.uint32) * 2654435761 >> 7).astype(np.uint16).reshape(shape)
    for origin, extent in BOX_CASES[(shape, tile)]:
        _check_box(parent, tile, origin, extent, None)
        _check_box(parent, tile, origin, extent, pitched(extent))
    rng = np.random.default_rng(0)
    for k in range(200):
        origin = tuple(int(rng.integers(0, d)) for d in shape)
        extent = tuple(int(rng.integers(1, d - o + 1)) for d, o in zip(shape, origin))
        _check_box(parent, tile, origin, extent, None if k % 2 else pitched(extent))


def test_box_windows_eight_tiles_at_a_corner():
    import sqeazy_amd
    indices, origins, ptrs, shapes, strides = sqeazy_amd.box_windows((9, 40, 72), (4, 16, 32), (3, 15, 31), (2, 2, 2), 4096, None, 2)
    assert indices == [0, 1, 3, 4, 9, 10, 12, 13] and origins[0] == (3, 15, 31) and origins[-1] == (0, 0, 0)
    assert shapes == [(1, 1, 1)] * 8 and strides == [(4, 2, 1)] * 8 and ptrs == [4096 + 2 * k for k in range(8)]


def test_box_windows_refuses_bad_arguments():
    import sqeazy_amd
    bad = [((9, 40, 72), (4, 16), (0, 0, 0), (1, 1, 1), None),            # ranks that differ
           ((9, 40, 72), (4, 16, 32), (0, 0), (1, 1, 1), None),
           ((9, 40, 72), (4, 16, 32), (0, 0, 0), (1, 1), None),
           ((9, 40, 72), (4, 16, 32), (0, 0, 0), (1, 1, 1), (72, 1)),
           ((1, 2, 3, 4), (1, 1, 1, 1), (0, 0, 0, 0), (1, 1, 1, 1), None),  # a rank outside 1 to 3
           ((), (), (), (), None),
           ((9, 40, 72), (4, 16, 32), (0, 0, 0), (1, 0, 1), None),          # a non-positive extent
           ((9, 40, 72), (4, 16, 32), (0, 0, 0), (1, -1, 1), None),
           ((9, 40, 72), (4, 0, 32), (0, 0, 0), (1, 1, 1), None),
           ((9, 40, 72), (4, 16, 32), (8, 39, 71), (2, 1, 1), None),        # a box outside the parent
           ((9, 40, 72), (4, 16, 32), (0, 40, 0), (1, 1, 1), None),
           ((9, 40, 72), (4, 16, 32), (0, 0, -1), (1, 1, 1), None),
           ((10,), (4,), (5,), (6,), None)]
    for shape, tile, origin, extent, strides in bad:
        with pytest.raises(ValueError):
            sqeazy_amd.box_windows(shape, tile, origin, extent, 0, strides, 2)
