"""Strided views on the host, under AddressSanitizer + UndefinedBehaviorSanitizer, built with g++ as test_host_encode_batch_stages.py builds
its targets (tests/sanitize/batch_view_test.cpp): sqy::admit_view -- every rule, the folding, the dense flag, ranks 1 to 3, overflow of
shape x stride --, the index walk the pack, unpack and strided transposer kernels compile (csrc/sqy_batch_view.hpp) against a triple loop
for every flat index, and the batch planner with the packed copies counted against the group bound.  And tile_views, the pure-Python grid."""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sqeazy_amd", "csrc")
SAN = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:exitcode=97:abort_on_error=0", UBSAN_OPTIONS="halt_on_error=1:exitcode=98:print_stacktrace=1")


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "batch_view_test")
    subprocess.check_call(["g++"] + SAN + [os.path.join(ROOT, "tests", "sanitize", "batch_view_test.cpp"), os.path.join(CSRC, "sqy_pipeline.cpp"), "-o", exe, "-lpthread"])
    r = subprocess.run([exe], env=ENV, capture_output=True, text=True, timeout=120)
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    assert r.returncode == 0 and "batch_view ok" in r.stdout, (r.returncode, r.stdout, r.stderr[-2000:])


@pytest.mark.parametrize("shape, tile", [((9, 40, 72), (4, 16, 32)), ((5, 7), (2, 7)), ((10,), (4,)), ((3, 4, 5), (3, 4, 5)), ((3, 4, 5), (7, 9, 11))])
def test_tile_views_cover_the_volume_once(shape, tile):
    import sqeazy_amd
    itemsize = 2
    vol = np.arange(int(np.prod(shape)), dtype=np.uint16).reshape(shape)
    base = 4096
    ptrs, shapes, strides = sqeazy_amd.tile_views(base, shape, tile, itemsize)
    grid = [-(-d // t) for d, t in zip(shape, tile)]
    assert len(ptrs) == len(shapes) == len(strides) == int(np.prod(grid))
    seen = np.zeros(vol.size, dtype=np.int32)
    flat = vol.reshape(-1)
    for p, s, st in zip(ptrs, shapes, strides):
        assert st[-1] == 1 and tuple(st) == tuple(x // itemsize for x in vol.strides)
        assert all(1 <= a <= t for a, t in zip(s, tile)) and (p - base) % itemsize == 0
        idx = (p - base) // itemsize + sum(np.arange(n).reshape([-1 if k == j else 1 for k in range(len(s))]) * st[j] for j, n in enumerate(s))
        seen[idx.reshape(-1)] += 1
        # the view is the slice numpy cuts at the tile's origin
        origin = np.unravel_index((p - base) // itemsize, shape)
        cut = vol[tuple(slice(o, o + n) for o, n in zip(origin, s))]
        assert cut.shape == tuple(s) and np.array_equal(flat[idx], cut)
    assert np.all(seen == 1)
    # row-major grid order: the tiles' origins ascend as the nested loops over the grid give them; the last tile ends at the last voxel
    origins = [np.unravel_index((p - base) // itemsize, shape) for p in ptrs]
    want = [()]
    for d, t in zip(shape, tile):
        want = [o + (x,) for o in want for x in range(0, d, t)]
    assert [tuple(int(x) for x in o) for o in origins] == want and ptrs[0] == base
    assert tuple(int(o) + n for o, n in zip(origins[-1], shapes[-1])) == tuple(shape)


def test_tile_views_refuses_bad_arguments():
    import sqeazy_amd
    for shape, tile in [((3, 4), (3,)), ((3, 0), (1, 1)), ((3, 4), (0, 4)), ((1, 2, 3, 4), (1, 1, 1, 1)), ((), ())]:
        with pytest.raises(ValueError):
            sqeazy_amd.tile_views(0, shape, tile, 1)
