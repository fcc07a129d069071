"""A box written into one large blob, on the host.  The routing (sqy::update_box_path over every combination of its inputs), the pipeline
comparison and the splice plan's arithmetic (sqy::lz4_splice_plan: the functions the splice kernels compile) under AddressSanitizer +
UndefinedBehaviorSanitizer as a stand-alone program built with g++ (tests/sanitize/update_box_test.cpp, as test_host_decode_boxes.py builds
its own).  And what SQYAMD_Update_Box_* must do without a GPU: the declarations, the option, the argument rules that come before any
device is looked for."""
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
ENTRY_POINTS = ("SQYAMD_Update_Box_UI16_Device", "SQYAMD_Update_Box_UI8_Device")


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_path_and_splice_plan_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "update_box_test")
    subprocess.check_call(["g++"] + SAN + [os.path.join(ROOT, "tests", "sanitize", "update_box_test.cpp"), os.path.join(CSRC, "sqy_pipeline.cpp"), "-o", exe, "-lpthread"])
    r = subprocess.run([exe], env=ENV, capture_output=True, text=True, timeout=300)
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    assert r.returncode == 0 and r.stdout.endswith("update_box ok\n"), (r.returncode, r.stdout[-500:], r.stderr[-2000:])
    counts = [int(x) for x in r.stdout.splitlines()[-2].split()[1::2]]
    # input combinations that give either path; stored and compressed replaced frames; payload lengths around a power of ten -- all met
    assert len(counts) == 5 and min(counts) > 0, r.stdout


def test_the_header_declares_the_entry_points():
    text = open(os.path.join(ROOT, "include", "sqeazy_amd.h")).read()
    for name in ENTRY_POINTS:
        m = re.search(r"SQY_FUNCTION_PREFIX int %s\(([^;]*)\);" % name, text)
        assert m, name
        args = " ".join(m.group(1).split())
        assert args == ("const char* pipeline, const void* d_src, long srclength, const long* origin, const void* d_view, const long* view_shape, "
                        "const long* view_strides, unsigned rank, void* d_dst, long dst_capacity, long* dstlength, int nthreads, void* hip_stream"), args
    assert '"update_box_subset"' in text


def test_the_option(sqy):
    assert sqy.get_option("update_box_subset") == 1
    try:
        sqy.set_option("update_box_subset", 0)
        assert sqy.get_option("update_box_subset") == 0
    finally:
        sqy.set_option("update_box_subset", 1)


def test_the_environment_switch():
    """SQY_NO_UPDATE_BOX_SUBSET=1 is read when the library is loaded: a fresh interpreter"""
    import sys
    code = "import sqeazy_amd; print(sqeazy_amd.get_option('update_box_subset'))"
    for env, want in (({"SQY_NO_UPDATE_BOX_SUBSET": "1"}, "0"), ({}, "1")):
        clean = {k: v for k, v in os.environ.items() if k != "SQY_NO_UPDATE_BOX_SUBSET"}
        r = subprocess.run([sys.executable, "-c", code], env=dict(clean, SQEAZY_AMD_NO_TORCH_PRELOAD="1", **env), cwd=ROOT, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and r.stdout.split()[-1] == want, (r.stdout, r.stderr[-2000:])


@pytest.mark.parametrize("dtype", [np.uint16, np.uint8])
def test_bad_arguments_return_1_before_a_device_is_looked_for(sqy, dtype):
    """NULL pointers, rank 0 or above 3, srclength <= 0, dst_capacity <= 0, a negative origin, a pipeline that is not admitted for the voxel
    type, the view rules: 1, *dstlength = 0, nothing written"""
    fn = getattr(sqy.lib(), "SQYAMD_Update_Box_%s_Device" % ("UI16" if dtype == np.uint16 else "UI8"))
    src = np.zeros(256, np.uint8)
    view = np.full((2, 3, 4), 9, dtype)
    dst = np.full(4096, 0x5A, np.uint8)
    longs = lambda v: None if v is None else (ctypes.c_long * max(len(v), 1))(*v)

    def call(pipeline=b"bitswap1->lz4", src_ok=True, srclen=256, origin=(0, 0, 0), view_ok=True, shape=(2, 3, 4), strides=None, rank=3, dst_ok=True, cap=4096, len_ok=True,
             shift=0):
        n = ctypes.c_long(77)
        rc = fn(pipeline, src.ctypes.data if src_ok else None, srclen, longs(origin), view.ctypes.data + shift if view_ok else None, longs(shape), longs(strides),
                ctypes.c_uint(rank), dst.ctypes.data if dst_ok else None, cap, ctypes.byref(n) if len_ok else None, 0, None)
        assert not len_ok or n.value == 0, n.value
        return rc
    bad = [dict(pipeline=None), dict(src_ok=False), dict(origin=None), dict(view_ok=False), dict(shape=None), dict(dst_ok=False), dict(len_ok=False), dict(rank=0), dict(rank=4),
           dict(srclen=0), dict(srclen=-7), dict(cap=0), dict(cap=-1), dict(origin=(0, -1, 0)), dict(origin=(0, 0, -(2 ** 62))), dict(pipeline=b"no_such_stage->lz4"),
           dict(pipeline=b""), dict(shape=(2, 0, 4)), dict(shape=(2, 3, -4)), dict(strides=(12, 4, 2)), dict(strides=(12, 3, 1)), dict(strides=(11, 4, 1)), dict(strides=(12, 0, 1))]
    if dtype == np.uint16:
        bad.append(dict(shift=1))                                       # a view off the voxel grid
    else:
        bad.append(dict(pipeline=b"quantiser->bitswap1->lz4"))          # a 16-bit pipeline
    for kw in bad:
        assert call(**kw) == 1, kw
    assert (dst == 0x5A).all() and (view == 9).all()
