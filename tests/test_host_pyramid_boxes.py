"""A whole resolution pyramid of boxes of one blob, on the host.  The routing (sqy::pyramid_boxes_path), the admission (sqy::admit_pyramid:
every refusal -- the levels, the nesting, a bad output in any level, the sum bound on the top level), the plan (sqy::pyramid_boxes_plan:
the top fused level T, the tiling of its grid, the accumulators' offsets) and the bit-plane kernel's whole fused walk -- blocks, level-0
layers, sqy::bin_run_cells into arrays standing in for LDS, the folds, the stores, the tail reduce -- under AddressSanitizer +
UndefinedBehaviorSanitizer as a stand-alone program built with g++ (tests/sanitize/pyramid_boxes_test.cpp, as test_host_bin_boxes.py
builds its own).  And what SQYAMD_Pyramid_Boxes_* must do without a GPU: the declarations, the two options, the argument rules that come
before any device is looked for, the Python helper for "mean"."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sqeazy_amd", "csrc")
SAN = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:exitcode=97:abort_on_error=0", UBSAN_OPTIONS="halt_on_error=1:exitcode=98:print_stacktrace=1")
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")
ENTRY_POINTS = ("SQYAMD_Pyramid_Boxes_UI16_Device", "SQYAMD_Pyramid_Boxes_UI8_Device", "SQYAMD_Pyramid_Boxes_UI16", "SQYAMD_Pyramid_Boxes_UI8")
OPTIONS = ("pyramid_boxes_subset", "pyramid_boxes_fused")


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_path_table_admission_plan_and_fused_walk_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "pyramid_boxes_test")
    # (the kernels' job structs live in sqy_kernels.h, which names HIP's stream type: the runtime's C header, nothing linked)
    subprocess.check_call(["g++"] + SAN + ["-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(ROCM, "include"), os.path.join(ROOT, "tests", "sanitize", "pyramid_boxes_test.cpp"),
                                           os.path.join(CSRC, "sqy_pipeline.cpp"), "-o", exe, "-lpthread"])
    r = subprocess.run([exe], env=ENV, capture_output=True, text=True, timeout=300)
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    assert r.returncode == 0 and r.stdout.endswith("pyramid_boxes ok\n"), (r.returncode, r.stdout[-500:], r.stderr[-2000:])
    words = r.stdout.splitlines()[-2].split()
    assert words[0] == "walk" and words[1::2] == ["blocks", "folds", "stored", "tail", "zreg", "above"], r.stdout
    # blocks, folds, cells stored by the walk and by the tail, boxes reduced over z in registers, boxes with a level above T -- all met
    counts = [int(x) for x in words[2::2]]
    assert len(counts) == 6 and min(counts) > 0, r.stdout


def test_the_header_declares_the_entry_points():
    text = open(os.path.join(ROOT, "include", "sqeazy_amd.h")).read()
    for name in ENTRY_POINTS:
        m = re.search(r"SQY_FUNCTION_PREFIX int %s\(([^;]*)\);" % name, text)
        assert m, name
        args = " ".join(m.group(1).split())
        if name.endswith("_Device"):
            assert args == ("const void* d_src, long srclength, long count, const long* origins, const long* extents, unsigned rank, long levels, const long* bins, "
                            "int op, void* const* d_outs, const long* out_strides, void* hip_stream"), args
        else:
            assert args == ("const char* src, long srclength, long count, const long* origins, const long* extents, unsigned rank, long levels, const long* bins, "
                            "int op, char* out, long out_capacity"), args
    # the projection's constants are reused: no new ones but the level bound
    assert len(re.findall(r"#define SQYAMD_PROJECT_", text)) == 3 and not re.search(r"#define SQYAMD_BIN_", text)
    assert re.findall(r"#define SQYAMD_PYRAMID_(\w+) (\d+)", text) == [("MAX_LEVELS", "8")]
    for option in OPTIONS:
        assert '"%s"' % option in text and "SQY_NO_" + option.upper() in text


def test_the_library_exports_the_entry_points(sqy):
    for name in ENTRY_POINTS:
        assert name in sqy.EXPORTED_SYMBOLS and getattr(sqy.lib(), name)
    assert callable(sqy.pyramid_boxes) and callable(sqy.pyramid_boxes_device)


def test_the_options(sqy):
    for option in OPTIONS:
        assert sqy.get_option(option) == 1
        try:
            assert sqy.lib().SQYAMD_Set_Option(option.encode(), 2) == 1 and sqy.get_option(option) == 1
            assert sqy.lib().SQYAMD_Set_Option(option.encode(), -1) == 1 and sqy.get_option(option) == 1
            sqy.set_option(option, 0)
            assert sqy.get_option(option) == 0
            # the other one and the binning's are their own
            assert all(sqy.get_option(o) == 1 for o in OPTIONS + ("bin_boxes_subset", "project_boxes_subset") if o != option)
        finally:
            sqy.set_option(option, 1)


def test_the_environment_switches():
    """SQY_NO_PYRAMID_BOXES_SUBSET=1 and SQY_NO_PYRAMID_BOXES_FUSED=1 are read when the library is loaded: a fresh interpreter"""
    import sys
    code = "import sqeazy_amd; print(*[sqeazy_amd.get_option(o) for o in ('pyramid_boxes_subset', 'pyramid_boxes_fused', 'bin_boxes_subset')])"
    switches = ("SQY_NO_PYRAMID_BOXES_SUBSET", "SQY_NO_PYRAMID_BOXES_FUSED", "SQY_NO_BIN_BOXES_SUBSET")
    for env, want in (({switches[0]: "1"}, ["0", "1", "1"]), ({switches[1]: "1"}, ["1", "0", "1"]), ({switches[0]: "1", switches[1]: "1"}, ["0", "0", "1"]), ({}, ["1", "1", "1"])):
        clean = {k: v for k, v in os.environ.items() if k not in switches}
        r = subprocess.run([sys.executable, "-c", code], env=dict(clean, SQEAZY_AMD_NO_TORCH_PRELOAD="1", **env), cwd=ROOT, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and r.stdout.split()[-3:] == want, (r.stdout, r.stderr[-2000:])


@pytest.mark.parametrize("dtype", [np.uint16, np.uint8])
def test_bad_arguments_return_1_with_the_outputs_untouched_before_a_device_is_looked_for(sqy, dtype):
    """What SQYAMD_Bin_Boxes_* refuses, for a pyramid of three levels -- NULL pointers, count below 1, a negative origin in ANY box, rank 0
    or above 3, srclength <= 0, bins NULL or with an entry below 1 in ANY level, op out of range -- and the pyramid's own: levels 0, 9 and
    negative, a row that is no multiple of the row before in each dimension, a NULL output or one 2 bytes off in ANY level of ANY box, the
    stride rules for any output, the sum bound on the top level's cell, a capacity one byte short: 1, the outputs as they were"""
    sfx = "UI16" if dtype == np.uint16 else "UI8"
    dev, host = getattr(sqy.lib(), "SQYAMD_Pyramid_Boxes_%s_Device" % sfx), getattr(sqy.lib(), "SQYAMD_Pyramid_Boxes_" + sfx)
    src = np.zeros(256, np.uint8)
    outs = np.full((3, 3, 2, 3, 8), 0xABCD1234, np.uint32)               # (3 boxes x 3 levels: room for 2 x 3 x 4 cells with a row pitch of up to 8)
    rows = lambda v: None if v is None else (ctypes.c_long * max(sum(len(r) for r in v), 1))(*[x for r in v for x in r])
    O, S = [(0, 0, 0)] * 3, [(2, 3, 4)] * 3
    BINS = ((1, 1, 1), (2, 1, 2), (2, 3, 4))                             # grids 2 x 3 x 4, 1 x 3 x 2, 1 x 1 x 1
    GOOD = [(24, 8, 1), (24, 8, 1), (24, 8, 1)]

    def call_dev(src_ok=True, srclen=256, count=3, origins=O, ptrs="all", extents=S, strides=None, rank=3, shift=0, bins=BINS, op=0, levels=3, bad=None):
        p = None
        if ptrs is not None:
            p = (ctypes.c_void_p * 9)(*[None if ptrs == (k, l) else outs[k, l].ctypes.data + (shift if bad in (None, (k, l)) else 0) for k in range(3) for l in range(3)])
        return dev(src.ctypes.data if src_ok else None, srclen, count, rows(origins), rows(extents), ctypes.c_uint(rank), levels, rows(bins), op, p, rows(strides), None)

    def call_host(src_ok=True, srclen=256, count=3, origins=O, out_ok=True, extents=S, rank=3, nbytes=outs.nbytes, bins=BINS, op=0, levels=3):
        return host(src.ctypes.data if src_ok else None, srclen, count, rows(origins), rows(extents), ctypes.c_uint(rank), levels, rows(bins), op,
                    outs.ctypes.data if out_ok else None, nbytes)

    def one(row, k, n=3, good=(0, 0, 0)):
        return [row if i == k else good for i in range(n)]

    def level(row, l):
        return tuple(row if i == l else b for i, b in enumerate(BINS))

    common = [dict(src_ok=False), dict(origins=None), dict(extents=None), dict(srclen=0), dict(srclen=-7), dict(rank=0), dict(rank=4), dict(count=0), dict(count=-3)]
    common += [dict(origins=one((0, -1, 0), k)) for k in range(3)] + [dict(origins=one((0, 0, -(2 ** 62)), 2))]
    common += [dict(bins=None), dict(op=3), dict(op=-1)] + [dict(levels=n) for n in (0, 9, -1, -(2 ** 63), 2 ** 62)]
    common += [dict(bins=level(bad, l)) for l in range(3) for bad in ((0, 1, 1), (1, -1, 1), (1, 1, -(2 ** 63)))]
    # the nesting, on the values as given: a non-multiple in each dimension, in level 1 and in level 2
    common += [dict(bins=((2, 2, 2), tuple(4 + (d == k) for k in range(3)), (8, 8, 8))) for d in range(3)]
    common += [dict(bins=((2, 2, 2), (4, 4, 4), tuple(8 + 2 * (d == k) for k in range(3)))) for d in range(3)]
    common += [dict(bins=((2, 2, 2), (4, 4, 4), (4, 2, 4))), dict(bins=((5, 5, 5), (7, 7, 7), (35, 35, 35)))]
    common += [dict(extents=one(bad, k, good=(2, 3, 4))) for k in range(3) for bad in ((2, 0, 4), (2, 3, -4))]
    # the sum bound on the top level's cell: V one above the bound in ONE box, in the top level alone
    big = 65537 if dtype == np.uint16 else 16843010
    common += [dict(extents=one((big, 1, 1), k, good=(2, 3, 4)), bins=((1, 1, 1), (1, 3, 4), (big, 3, 4)), op=2) for k in range(3)]
    dev_only = [dict(ptrs=None)] + [dict(ptrs=(k, l)) for k in range(3) for l in range(3)]
    dev_only += [dict(shift=s, bad=(k, l)) for k in range(3) for l in range(3) for s in (2, 1)]
    for k in range(3):
        for l, bads in enumerate((((24, 8, 2), (24, 3, 1), (24, 0, 1), (23, 8, 1)), ((24, 8, 2), (24, 1, 1), (24, 0, 1)), ((24, 8, 2), (24, 8, 0)))):
            for bad in bads:
                s = [list(GOOD) for _ in range(3)]
                s[k][l] = bad
                dev_only.append(dict(strides=[r for box in s for r in box]))
    for kw in common + dev_only:
        assert call_dev(**kw) == 1, kw
        assert (outs == 0xABCD1234).all(), kw
    for kw in common + [dict(out_ok=False)]:
        assert call_host(**kw) == 1, kw
        assert (outs == 0xABCD1234).all(), kw
    assert call_host() == 1 and (outs == 0xABCD1234).all()               # (no sqy header in the blob: refused on the host as well)
    # out_capacity against a blob with a header of (2, 3, 4) voxels: one byte less than the outputs hold -- refused on the host
    from sqeazy_amd import multi
    blob = np.frombuffer(multi.build_header("lz4", dtype, (2, 3, 4), 64) + bytes(64), np.uint8).copy()
    for bins, cells in ((BINS, 24 + 6 + 1), (((1, 1, 1),), 24), (((2, 2, 2), (2, 2, 2)), 8), (((9, 9, 9), (18, 9, 9)), 2)):
        for nbytes in (3 * cells * 4 - 1, 0, -1):
            rc = host(blob.ctypes.data, len(blob), 3, rows(O), rows(S), ctypes.c_uint(3), len(bins), rows(bins), 0, outs.ctypes.data, nbytes)
            assert rc == 1 and (outs == 0xABCD1234).all(), (bins, nbytes)


def test_the_python_wrapper_refuses_and_divides_by_the_cells_voxel_counts(sqy):
    """pyramid_boxes without a header in the blob, with ragged rows or none: (1, None), nothing called; what "mean" divides level l by is
    bin_counts of its row -- every cell's actual voxel count, and a level's counts are the sums of the counts of the cells under it"""
    assert sqy.pyramid_boxes(bytes(64), [(0, 0, 0)], [(2, 3, 4)], ((1, 1, 1), (2, 2, 2))) == (1, None)
    from sqeazy_amd import multi
    blob = multi.build_header("lz4", np.uint16, (2, 3, 4), 64) + bytes(64)
    for bins in (None, (), ((1, 1), (2, 2)), ((1, 1, 1), (2, 0, 2))):
        assert sqy.pyramid_boxes(blob, [(0, 0, 0)], [(2, 3, 4)], bins) == (1, None)
    assert sqy.pyramid_boxes(blob, [(0, 0, 0)], [], ((1, 1, 1),)) == (1, None)
    extent = (7, 33, 31)
    for pyramid in (((1, 1, 1), (2, 2, 2), (4, 4, 4), (8, 8, 8)), ((3, 5, 7), (6, 5, 21), (12, 10, 42)), ((2, 1, 1), (1000, 1, 1))):
        below = None
        for l, bins in enumerate(pyramid):
            counts = sqy.bin_counts(extent, bins)
            assert counts.shape == sqy.bin_shape(extent, bins) and counts.sum() == np.prod(extent)
            if below is not None:
                ratio = [min(b // a, n) for b, a, n in zip(bins, pyramid[l - 1], below.shape)]
                folded = below
                for ax, r in enumerate(ratio):
                    folded = np.add.reduceat(folded, np.arange(0, folded.shape[ax], r), axis=ax)
                assert np.array_equal(folded, counts), (pyramid, l)
            below = counts
