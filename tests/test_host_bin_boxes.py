"""Boxes of one blob read at a coarser resolution, on the host.  The routing (sqy::bin_boxes_path), the admission (sqy::admit_binning: every
refusal, the sum bound applied to the cell, the clamp of bins beyond the extents), the tiling of a cell grid into a workgroup's blocks
(sqy::bin_boxes_plan) and the bit-plane kernel's cell walk -- blocks, footprints, items, the clip and sqy::bin_run_cells into an array
standing in for the LDS accumulators -- under AddressSanitizer + UndefinedBehaviorSanitizer as a stand-alone program built with g++
(tests/sanitize/bin_boxes_test.cpp, as test_host_project_boxes.py builds its own).  And what SQYAMD_Bin_Boxes_* must do without a GPU:
the declarations, the option, the argument rules that come before any device is looked for, the Python helpers for "mean"."""
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
ENTRY_POINTS = ("SQYAMD_Bin_Boxes_UI16_Device", "SQYAMD_Bin_Boxes_UI8_Device", "SQYAMD_Bin_Boxes_UI16", "SQYAMD_Bin_Boxes_UI8")


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_path_table_admission_plan_and_cell_walk_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "bin_boxes_test")
    # (the kernels' job structs live in sqy_kernels.h, which names HIP's stream type: the runtime's C header, nothing linked)
    subprocess.check_call(["g++"] + SAN + ["-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(ROCM, "include"), os.path.join(ROOT, "tests", "sanitize", "bin_boxes_test.cpp"),
                                           os.path.join(CSRC, "sqy_pipeline.cpp"), "-o", exe, "-lpthread"])
    r = subprocess.run([exe], env=ENV, capture_output=True, text=True, timeout=300)
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    assert r.returncode == 0 and r.stdout.endswith("bin_boxes ok\n"), (r.returncode, r.stdout[-500:], r.stderr[-2000:])
    words = r.stdout.splitlines()[-2].split()
    assert words[0] == "items" and words[1::2] == ["outside", "inside", "partly", "blocks", "zreg"], r.stdout
    # items outside, inside and partly inside a footprint; blocks; boxes reduced over z in registers -- all met
    counts = [int(x) for x in words[2::2]]
    assert len(counts) == 5 and min(counts) > 0, r.stdout


def test_the_header_declares_the_entry_points():
    text = open(os.path.join(ROOT, "include", "sqeazy_amd.h")).read()
    for name in ENTRY_POINTS:
        m = re.search(r"SQY_FUNCTION_PREFIX int %s\(([^;]*)\);" % name, text)
        assert m, name
        args = " ".join(m.group(1).split())
        if name.endswith("_Device"):
            assert args == ("const void* d_src, long srclength, long count, const long* origins, const long* extents, unsigned rank, const long* bins, int op, "
                            "void* const* d_outs, const long* out_strides, void* hip_stream"), args
        else:
            assert args == ("const char* src, long srclength, long count, const long* origins, const long* extents, unsigned rank, const long* bins, int op, "
                            "char* out, long out_capacity"), args
    # the projection's constants are reused: no new ones
    assert len(re.findall(r"#define SQYAMD_PROJECT_", text)) == 3 and not re.search(r"#define SQYAMD_BIN_", text)
    assert '"bin_boxes_subset"' in text and "SQY_NO_BIN_BOXES_SUBSET" in text


def test_the_library_exports_the_entry_points(sqy):
    for name in ENTRY_POINTS:
        assert name in sqy.EXPORTED_SYMBOLS and getattr(sqy.lib(), name)


def test_the_option(sqy):
    assert sqy.get_option("bin_boxes_subset") == 1
    try:
        assert sqy.lib().SQYAMD_Set_Option(b"bin_boxes_subset", 2) == 1 and sqy.get_option("bin_boxes_subset") == 1
        assert sqy.lib().SQYAMD_Set_Option(b"bin_boxes_subset", -1) == 1 and sqy.get_option("bin_boxes_subset") == 1
        sqy.set_option("bin_boxes_subset", 0)
        assert sqy.get_option("bin_boxes_subset") == 0
        # the projection's and the decode's options are their own
        assert sqy.get_option("project_boxes_subset") == 1 and sqy.get_option("project_boxes_walk") == 1 and sqy.get_option("decode_boxes_joint") == 1
    finally:
        sqy.set_option("bin_boxes_subset", 1)


def test_the_environment_switch():
    """SQY_NO_BIN_BOXES_SUBSET=1 is read when the library is loaded: a fresh interpreter"""
    import sys
    code = "import sqeazy_amd; print(sqeazy_amd.get_option('bin_boxes_subset'), sqeazy_amd.get_option('project_boxes_subset'))"
    for env, want in (({"SQY_NO_BIN_BOXES_SUBSET": "1"}, ["0", "1"]), ({}, ["1", "1"])):
        clean = {k: v for k, v in os.environ.items() if k not in ("SQY_NO_BIN_BOXES_SUBSET", "SQY_NO_PROJECT_BOXES_SUBSET")}
        r = subprocess.run([sys.executable, "-c", code], env=dict(clean, SQEAZY_AMD_NO_TORCH_PRELOAD="1", **env), cwd=ROOT, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and r.stdout.split()[-2:] == want, (r.stdout, r.stderr[-2000:])


@pytest.mark.parametrize("dtype", [np.uint16, np.uint8])
def test_bad_arguments_return_1_with_the_outputs_untouched_before_a_device_is_looked_for(sqy, dtype):
    """NULL pointers, count below 1, a NULL output among the outputs, an output 2 bytes off, a negative origin in ANY box, rank 0 or above 3,
    srclength <= 0, bins NULL or with an entry below 1, op out of range, the stride rules for any output, the sum bound on the cell, a
    capacity one byte short: 1, the outputs as they were"""
    sfx = "UI16" if dtype == np.uint16 else "UI8"
    dev, host = getattr(sqy.lib(), "SQYAMD_Bin_Boxes_%s_Device" % sfx), getattr(sqy.lib(), "SQYAMD_Bin_Boxes_" + sfx)
    src = np.zeros(256, np.uint8)
    outs = np.full((3, 2, 3, 8), 0xABCD1234, np.uint32)                  # (room for 3 outputs of 2 x 3 x 4 cells with a row pitch of up to 8)
    rows = lambda v: None if v is None else (ctypes.c_long * max(sum(len(r) for r in v), 1))(*[x for r in v for x in r])
    O, S = [(0, 0, 0)] * 3, [(2, 3, 4)] * 3

    def call_dev(src_ok=True, srclen=256, count=3, origins=O, ptrs="all", extents=S, strides=None, rank=3, shift=0, bins=(1, 1, 1), op=0):
        p = None
        if ptrs is not None:
            p = (ctypes.c_void_p * 3)(*[None if ptrs == k else outs[k].ctypes.data + shift for k in range(3)])
        return dev(src.ctypes.data if src_ok else None, srclen, count, rows(origins), rows(extents), ctypes.c_uint(rank), rows(None if bins is None else [bins]), op, p,
                   rows(strides), None)

    def call_host(src_ok=True, srclen=256, count=3, origins=O, out_ok=True, extents=S, rank=3, nbytes=outs.nbytes, bins=(1, 1, 1), op=0):
        return host(src.ctypes.data if src_ok else None, srclen, count, rows(origins), rows(extents), ctypes.c_uint(rank), rows(None if bins is None else [bins]), op,
                    outs.ctypes.data if out_ok else None, nbytes)

    def one(row, k, n=3, good=(0, 0, 0)):
        return [row if i == k else good for i in range(n)]

    common = [dict(src_ok=False), dict(origins=None), dict(extents=None), dict(srclen=0), dict(srclen=-7), dict(rank=0), dict(rank=4), dict(count=0), dict(count=-3)]
    common += [dict(origins=one((0, -1, 0), k)) for k in range(3)] + [dict(origins=one((0, 0, -(2 ** 62)), 2))]
    common += [dict(bins=None), dict(bins=(0, 1, 1)), dict(bins=(1, -1, 1)), dict(bins=(1, 1, -(2 ** 63))), dict(op=3), dict(op=-1)]
    common += [dict(extents=one(bad, k, good=(2, 3, 4))) for k in range(3) for bad in ((2, 0, 4), (2, 3, -4))]
    # the sum bound on the cell: V one above the bound in ONE box (the others' cells are their whole small extents)
    big = 65537 if dtype == np.uint16 else 16843010
    common += [dict(extents=one((big, 1, 1), k, good=(2, 3, 4)), bins=(big, 3, 4), op=2) for k in range(3)]
    common += [dict(extents=one((4, big // 4 + 1, 1), k, good=(2, 3, 4)), bins=(2 ** 62, 2 ** 62, 2 ** 62), op=2) for k in range(3)]
    dev_only = [dict(ptrs=None), dict(ptrs=0), dict(ptrs=1), dict(ptrs=2), dict(shift=2), dict(shift=1)]
    dev_only += [dict(strides=one(bad, k, good=(24, 8, 1))) for k in range(3) for bad in ((24, 8, 2), (24, 3, 1), (24, 0, 1), (23, 8, 1))]
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
    for bins, cells in (((1, 1, 1), 24), ((2, 2, 2), 4), ((1, 2, 3), 8), ((9, 9, 9), 1)):
        for nbytes in (3 * cells * 4 - 1, 0, -1):
            rc = host(blob.ctypes.data, len(blob), 3, rows(O), rows(S), ctypes.c_uint(3), rows([bins]), 0, outs.ctypes.data, nbytes)
            assert rc == 1 and (outs == 0xABCD1234).all(), (bins, nbytes)


def test_the_python_shapes_and_cell_counts(sqy):
    """what "mean" divides by: every cell's actual voxel count, partial cells at the far edges included"""
    assert sqy.bin_shape((7, 33, 31), (2, 2, 2)) == (4, 17, 16) and sqy.bin_shape((7, 33, 31), (1000, 1, 33)) == (1, 33, 1) and sqy.bin_shape((5,), (5,)) == (1,)
    for extent, bins in (((7, 33, 31), (2, 2, 2)), ((7, 33, 31), (3, 5, 7)), ((4, 6), (9, 2)), ((10,), (3,)), ((2, 3, 4), (1, 1, 1))):
        want = np.zeros(sqy.bin_shape(extent, bins), np.float64)
        for idx in np.ndindex(*extent):
            want[tuple(i // b for i, b in zip(idx, bins))] += 1
        got = sqy.bin_counts(extent, bins)
        assert got.dtype == np.float64 and got.shape == want.shape and np.array_equal(got, want), (extent, bins)
