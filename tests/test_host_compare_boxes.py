"""Many boxes of one blob compared with resident voxels, on the host.  The routing (sqy::compare_boxes_path), the comparing job's layout and
the comparing range transposer's walk -- sqy::range_run, the clip and window_compare16 run by run over ranges of small blobs -- under
AddressSanitizer + UndefinedBehaviorSanitizer as a stand-alone program built with g++ (tests/sanitize/compare_boxes_test.cpp, as
test_host_batch_compare.py builds its own).  And what SQYAMD_Compare_Boxes_* must do without a GPU: the declarations, the option, the
argument rules that come before any device is looked for."""
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
ENTRY_POINTS = ("SQYAMD_Compare_Boxes_UI16_Device", "SQYAMD_Compare_Boxes_UI8_Device", "SQYAMD_Compare_Boxes_UI16", "SQYAMD_Compare_Boxes_UI8")


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_path_table_and_comparing_range_walk_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "compare_boxes_test")
    # (the kernels' job struct lives in sqy_kernels.h, which names HIP's stream type: the runtime's C header, nothing linked)
    subprocess.check_call(["g++"] + SAN + ["-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(ROCM, "include"), os.path.join(ROOT, "tests", "sanitize", "compare_boxes_test.cpp"),
                                           os.path.join(CSRC, "sqy_pipeline.cpp"), "-o", exe, "-lpthread"])
    r = subprocess.run([exe], env=ENV, capture_output=True, text=True, timeout=300)
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    assert r.returncode == 0 and r.stdout.endswith("compare_boxes ok\n"), (r.returncode, r.stdout[-500:], r.stderr[-2000:])
    words = r.stdout.splitlines()[-2].split()
    assert words[0] == "runs" and words[1::2] == ["outside", "inside", "partly", "first", "last"], r.stdout
    # runs outside, inside and partly inside a box; first and last threads of a range -- all met
    counts = [int(x) for x in words[2::2]]
    assert len(counts) == 5 and min(counts) > 0, r.stdout


def test_the_header_declares_the_entry_points():
    text = open(os.path.join(ROOT, "include", "sqeazy_amd.h")).read()
    for name in ENTRY_POINTS:
        m = re.search(r"SQY_FUNCTION_PREFIX int %s\(([^;]*)\);" % name, text)
        assert m, name
        args = " ".join(m.group(1).split())
        if name.endswith("_Device"):
            assert args == ("const void* d_src, long srclength, long count, const long* origins, const void* const* d_views, const long* view_shapes, "
                            "const long* view_strides, unsigned rank, unsigned long long* stats, void* hip_stream"), args
        else:
            assert args == ("const char* src, long srclength, long count, const long* origins, const long* extents, unsigned rank, const char* views, "
                            "long views_bytes, unsigned long long* stats"), args
    assert '"compare_boxes_subset"' in text and "SQY_NO_COMPARE_BOXES_SUBSET" in text


def test_the_library_exports_the_entry_points(sqy):
    for name in ENTRY_POINTS:
        assert name in sqy.EXPORTED_SYMBOLS and getattr(sqy.lib(), name)


def test_the_option(sqy):
    assert sqy.get_option("compare_boxes_subset") == 1
    try:
        assert sqy.lib().SQYAMD_Set_Option(b"compare_boxes_subset", 2) == 1 and sqy.get_option("compare_boxes_subset") == 1
        assert sqy.lib().SQYAMD_Set_Option(b"compare_boxes_subset", -1) == 1 and sqy.get_option("compare_boxes_subset") == 1
        sqy.set_option("compare_boxes_subset", 0)
        assert sqy.get_option("compare_boxes_subset") == 0
    finally:
        sqy.set_option("compare_boxes_subset", 1)
    # the decode's options are its own
    assert sqy.get_option("decode_box_subset") == 1 and sqy.get_option("decode_boxes_joint") == 1


def test_the_environment_switch():
    """SQY_NO_COMPARE_BOXES_SUBSET=1 is read when the library is loaded: a fresh interpreter"""
    import sys
    code = "import sqeazy_amd; print(sqeazy_amd.get_option('compare_boxes_subset'))"
    for env, want in (({"SQY_NO_COMPARE_BOXES_SUBSET": "1"}, "0"), ({}, "1")):
        clean = {k: v for k, v in os.environ.items() if k != "SQY_NO_COMPARE_BOXES_SUBSET"}
        r = subprocess.run([sys.executable, "-c", code], env=dict(clean, SQEAZY_AMD_NO_TORCH_PRELOAD="1", **env), cwd=ROOT, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and r.stdout.split()[-1] == want, (r.stdout, r.stderr[-2000:])


@pytest.mark.parametrize("dtype", [np.uint16, np.uint8])
def test_bad_arguments_return_1_with_stats_zeroed_before_a_device_is_looked_for(sqy, dtype):
    """test_host_decode_boxes' table -- NULL pointers, count below 1, a NULL view among the views, a negative origin in ANY box, rank 0 or
    above 3, srclength <= 0, the view rules for any view -- and stats == NULL, views_bytes one byte off either way: 1, stats zeroed, the
    views as they were"""
    sfx = "UI16" if dtype == np.uint16 else "UI8"
    dev, host = getattr(sqy.lib(), "SQYAMD_Compare_Boxes_%s_Device" % sfx), getattr(sqy.lib(), "SQYAMD_Compare_Boxes_" + sfx)
    src = np.zeros(256, np.uint8)
    views = np.full((3, 2, 3, 4), 9, dtype)
    stats = np.zeros((3, 8), np.uint64)
    rows = lambda v: None if v is None else (ctypes.c_long * max(sum(len(r) for r in v), 1))(*[x for r in v for x in r])
    O, S = [(0, 0, 0)] * 3, [(2, 3, 4)] * 3

    def st(ok):
        stats[:] = 0xDEAD
        return stats.ctypes.data_as(ctypes.POINTER(ctypes.c_ulonglong)) if ok else None

    def call_dev(src_ok=True, srclen=256, count=3, origins=O, ptrs="all", shapes=S, strides=None, rank=3, shift=0, stats_ok=True):
        p = None
        if ptrs is not None:
            p = (ctypes.c_void_p * 3)(*[None if ptrs == k else views[k].ctypes.data + shift for k in range(3)])
        return dev(src.ctypes.data if src_ok else None, srclen, count, rows(origins), p, rows(shapes), rows(strides), ctypes.c_uint(rank), st(stats_ok), None)

    def call_host(src_ok=True, srclen=256, count=3, origins=O, views_ok=True, extents=S, rank=3, nbytes=views.nbytes, stats_ok=True):
        return host(src.ctypes.data if src_ok else None, srclen, count, rows(origins), rows(extents), ctypes.c_uint(rank), views.ctypes.data if views_ok else None, nbytes,
                    st(stats_ok))

    def one(row, k, n=3, good=(0, 0, 0)):
        return [row if i == k else good for i in range(n)]

    def zeroed(kw):
        """the rows of the call's count are zeros (a count that names no rows: nothing to zero)"""
        n = kw.get("count", 3)
        return not stats[:n].any() if 1 <= n <= 3 and kw.get("stats_ok", True) else True
    common = [dict(src_ok=False), dict(origins=None), dict(srclen=0), dict(srclen=-7), dict(rank=0), dict(rank=4), dict(count=0), dict(count=-3), dict(stats_ok=False)]
    common += [dict(origins=one((0, -1, 0), k)) for k in range(3)] + [dict(origins=one((0, 0, -(2 ** 62)), 2))]
    dev_only = [dict(ptrs=None), dict(ptrs=0), dict(ptrs=1), dict(ptrs=2), dict(shapes=None)]
    dev_only += [dict(shapes=one(bad, k, good=(2, 3, 4))) for k in range(3) for bad in ((2, 0, 4), (2, 3, -4))]
    dev_only += [dict(strides=one(bad, k, good=(12, 4, 1))) for k in range(3) for bad in ((12, 4, 2), (12, 3, 1), (11, 4, 1), (12, 0, 1))]
    for kw in common + dev_only + ([dict(shift=1)] if dtype == np.uint16 else []):
        assert call_dev(**kw) == 1, kw
        assert zeroed(kw), kw
    for kw in common + [dict(extents=None), dict(views_ok=False)]:
        assert call_host(**kw) == 1, kw
        assert zeroed(kw), kw
    assert call_host() == 1 and not stats.any()                          # (no sqy header in the blob: refused on the host as well)
    assert (views == 9).all()
    # views_bytes against a blob with a header of (2, 3, 4) voxels: one byte less and one byte more than the boxes hold -- refused on the host
    from sqeazy_amd import multi
    item = np.dtype(dtype).itemsize
    blob = np.frombuffer(multi.build_header("lz4", dtype, (2, 3, 4), 64) + bytes(64), np.uint8).copy()
    total = 3 * 24 * item
    assert views.nbytes == total
    for nbytes in (total - 1, total + 1, 0, -1):
        stats[:] = 0xDEAD
        rc = host(blob.ctypes.data, len(blob), 3, rows(O), rows(S), ctypes.c_uint(3), views.ctypes.data, nbytes, stats.ctypes.data_as(ctypes.POINTER(ctypes.c_ulonglong)))
        assert rc == 1 and not stats.any(), nbytes
    assert (views == 9).all()
