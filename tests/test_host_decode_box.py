"""The box decode on the host.  The routing plan (sqy::decode_box_path) against its table, and the clip and run text of
csrc/sqy_batch_window.hpp, which bitswap1_decode_range_window_kernel compiles, under AddressSanitizer + UndefinedBehaviorSanitizer as a
stand-alone program built with g++ (tests/sanitize/decode_box_test.cpp, as test_host_batch_compare.py builds its own): driven run by run
as the kernel drives it, over word ranges that begin and end inside a thread's 128 voxels, its view must be a triple loop's.  And what
SQYAMD_Decode_Box_* must do without a GPU: the declarations, the option, the argument rules that come before any device is looked for."""
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
ENTRY_POINTS = ("SQYAMD_Decode_Box_UI16_Device", "SQYAMD_Decode_Box_UI8_Device", "SQYAMD_Decode_Box_UI16", "SQYAMD_Decode_Box_UI8")


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_plan_clip_and_runs_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "decode_box_test")
    subprocess.check_call(["g++"] + SAN + [os.path.join(ROOT, "tests", "sanitize", "decode_box_test.cpp"), os.path.join(CSRC, "sqy_pipeline.cpp"), "-o", exe, "-lpthread"])
    r = subprocess.run([exe], env=ENV, capture_output=True, text=True, timeout=300)
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    assert r.returncode == 0 and r.stdout.endswith("decode_box ok\n"), (r.returncode, r.stdout[-500:], r.stderr[-2000:])
    counts = [int(x) for x in r.stdout.splitlines()[-2].split()[1::2]]
    # boxes; threads whose first / last words are not theirs; tail voxels stored; ranges whose plane segments straddle chunks -- all met
    assert len(counts) == 5 and min(counts) > 0, r.stdout


def test_the_header_declares_the_entry_points():
    text = open(os.path.join(ROOT, "include", "sqeazy_amd.h")).read()
    for name in ENTRY_POINTS:
        m = re.search(r"SQY_FUNCTION_PREFIX int %s\(([^;]*)\);" % name, text)
        assert m, name
        args = " ".join(m.group(1).split())
        if name.endswith("_Device"):
            assert args == ("const void* d_src, long srclength, const long* origin, void* d_dst, const long* dst_shape, const long* dst_strides, "
                            "unsigned rank, void* hip_stream"), args
        else:
            assert args == "const char* src, long srclength, const long* origin, const long* extent, unsigned rank, char* dst, long dst_capacity", args
    assert '"decode_box_subset"' in text and "SQY_NO_DECODE_BOX_SUBSET" in text


def test_the_option(sqy):
    assert sqy.get_option("decode_box_subset") == 1
    try:
        assert sqy.lib().SQYAMD_Set_Option(b"decode_box_subset", 2) == 1 and sqy.get_option("decode_box_subset") == 1
        assert sqy.lib().SQYAMD_Set_Option(b"decode_box_subset", -1) == 1 and sqy.get_option("decode_box_subset") == 1
        sqy.set_option("decode_box_subset", 0)
        assert sqy.get_option("decode_box_subset") == 0
    finally:
        sqy.set_option("decode_box_subset", 1)


def test_the_environment_switch():
    """SQY_NO_DECODE_BOX_SUBSET=1 is read when the library is loaded: a fresh interpreter"""
    import sys
    code = "import sqeazy_amd; print(sqeazy_amd.get_option('decode_box_subset'))"
    for env, want in (({"SQY_NO_DECODE_BOX_SUBSET": "1"}, "0"), ({}, "1")):
        clean = {k: v for k, v in os.environ.items() if k != "SQY_NO_DECODE_BOX_SUBSET"}
        r = subprocess.run([sys.executable, "-c", code], env=dict(clean, SQEAZY_AMD_NO_TORCH_PRELOAD="1", **env), cwd=ROOT, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and r.stdout.split()[-1] == want, (r.stdout, r.stderr[-2000:])


@pytest.mark.parametrize("dtype", [np.uint16, np.uint8])
def test_bad_arguments_return_1_before_a_device_is_looked_for(sqy, dtype):
    """NULL pointers, a negative origin, rank 0 or above 3, srclength <= 0, the view rules: 1, nothing written"""
    sfx = "UI16" if dtype == np.uint16 else "UI8"
    dev, host = getattr(sqy.lib(), "SQYAMD_Decode_Box_%s_Device" % sfx), getattr(sqy.lib(), "SQYAMD_Decode_Box_" + sfx)
    src = np.zeros(256, np.uint8)
    dst = np.full((2, 3, 4), 9, dtype)
    longs = lambda v: None if v is None else (ctypes.c_long * max(len(v), 1))(*v)

    def call_dev(src_ok=True, srclen=256, origin=(0, 0, 0), dst_ok=True, shape=(2, 3, 4), strides=None, rank=3, shift=0):
        return dev(src.ctypes.data if src_ok else None, srclen, longs(origin), dst.ctypes.data + shift if dst_ok else None, longs(shape), longs(strides),
                   ctypes.c_uint(rank), None)

    def call_host(src_ok=True, srclen=256, origin=(0, 0, 0), dst_ok=True, extent=(2, 3, 4), rank=3, cap=dst.nbytes):
        return host(src.ctypes.data if src_ok else None, srclen, longs(origin), longs(extent), ctypes.c_uint(rank), dst.ctypes.data if dst_ok else None, cap)
    common = [dict(src_ok=False), dict(dst_ok=False), dict(origin=None), dict(srclen=0), dict(srclen=-7), dict(rank=0), dict(rank=4), dict(origin=(0, -1, 0)),
              dict(origin=(-1, 0, 0)), dict(origin=(0, 0, -(2 ** 62)))]
    for kw in common + [dict(shape=None), dict(shape=(2, 0, 4)), dict(shape=(2, 3, -4)), dict(strides=(12, 4, 2)), dict(strides=(12, 3, 1)), dict(strides=(11, 4, 1)),
                        dict(strides=(12, 0, 1))] + ([dict(shift=1)] if dtype == np.uint16 else []):
        assert call_dev(**kw) == 1, kw
    for kw in common + [dict(extent=None)]:
        assert call_host(**kw) == 1, kw
    assert call_host() == 1                                              # (no sqy header in the blob: refused on the host as well)
    assert (dst == 9).all()
