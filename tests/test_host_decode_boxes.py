"""Many boxes of one blob on the host.  The union plan (sqy::frame_ranges_plan), the routing (sqy::decode_boxes_path) and the workgroup ->
job walk of bitswap1_decode_range_windows_kernel under AddressSanitizer + UndefinedBehaviorSanitizer as a stand-alone program built with g++
(tests/sanitize/decode_boxes_test.cpp, as test_host_decode_box.py builds its own).  And what SQYAMD_Decode_Boxes_* must do without a GPU: the
declarations, the option, the argument rules that come before any device is looked for."""
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
ENTRY_POINTS = ("SQYAMD_Decode_Boxes_UI16_Device", "SQYAMD_Decode_Boxes_UI8_Device", "SQYAMD_Decode_Boxes_UI16", "SQYAMD_Decode_Boxes_UI8")


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_union_plan_and_job_walk_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "decode_boxes_test")
    subprocess.check_call(["g++"] + SAN + [os.path.join(ROOT, "tests", "sanitize", "decode_boxes_test.cpp"), os.path.join(CSRC, "sqy_pipeline.cpp"), "-o", exe, "-lpthread"])
    r = subprocess.run([exe], env=ENV, capture_output=True, text=True, timeout=300)
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    assert r.returncode == 0 and r.stdout.endswith("decode_boxes ok\n"), (r.returncode, r.stdout[-500:], r.stderr[-2000:])
    counts = [int(x) for x in r.stdout.splitlines()[-2].split()[1::2]]
    # sets of ranges; unions with a gap of unneeded frames; frames that two ranges share; tails; a struck slot; zero runs; workgroups -- all met
    assert len(counts) == 7 and min(counts) > 0, r.stdout


def test_the_header_declares_the_entry_points():
    text = open(os.path.join(ROOT, "include", "sqeazy_amd.h")).read()
    for name in ENTRY_POINTS:
        m = re.search(r"SQY_FUNCTION_PREFIX int %s\(([^;]*)\);" % name, text)
        assert m, name
        args = " ".join(m.group(1).split())
        if name.endswith("_Device"):
            assert args == ("const void* d_src, long srclength, long count, const long* origins, void* const* d_dsts, const long* dst_shapes, "
                            "const long* dst_strides, unsigned rank, void* hip_stream"), args
        else:
            assert args == "const char* src, long srclength, long count, const long* origins, const long* extents, unsigned rank, char* dst, long dst_capacity", args
    assert '"decode_boxes_joint"' in text and "SQY_NO_DECODE_BOXES_JOINT" in text


def test_the_option(sqy):
    assert sqy.get_option("decode_boxes_joint") == 1
    try:
        assert sqy.lib().SQYAMD_Set_Option(b"decode_boxes_joint", 2) == 1 and sqy.get_option("decode_boxes_joint") == 1
        assert sqy.lib().SQYAMD_Set_Option(b"decode_boxes_joint", -1) == 1 and sqy.get_option("decode_boxes_joint") == 1
        sqy.set_option("decode_boxes_joint", 0)
        assert sqy.get_option("decode_boxes_joint") == 0
    finally:
        sqy.set_option("decode_boxes_joint", 1)


def test_the_environment_switch():
    """SQY_NO_DECODE_BOXES_JOINT=1 is read when the library is loaded: a fresh interpreter"""
    import sys
    code = "import sqeazy_amd; print(sqeazy_amd.get_option('decode_boxes_joint'))"
    for env, want in (({"SQY_NO_DECODE_BOXES_JOINT": "1"}, "0"), ({}, "1")):
        clean = {k: v for k, v in os.environ.items() if k != "SQY_NO_DECODE_BOXES_JOINT"}
        r = subprocess.run([sys.executable, "-c", code], env=dict(clean, SQEAZY_AMD_NO_TORCH_PRELOAD="1", **env), cwd=ROOT, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and r.stdout.split()[-1] == want, (r.stdout, r.stderr[-2000:])


@pytest.mark.parametrize("dtype", [np.uint16, np.uint8])
def test_bad_arguments_return_1_before_a_device_is_looked_for(sqy, dtype):
    """NULL pointers, count below 1, a NULL view among the views, a negative origin in ANY box, rank 0 or above 3, srclength <= 0, the view
    rules for any view: 1, nothing written"""
    sfx = "UI16" if dtype == np.uint16 else "UI8"
    dev, host = getattr(sqy.lib(), "SQYAMD_Decode_Boxes_%s_Device" % sfx), getattr(sqy.lib(), "SQYAMD_Decode_Boxes_" + sfx)
    src = np.zeros(256, np.uint8)
    dst = np.full((3, 2, 3, 4), 9, dtype)
    rows = lambda v: None if v is None else (ctypes.c_long * max(sum(len(r) for r in v), 1))(*[x for r in v for x in r])
    O, S = [(0, 0, 0)] * 3, [(2, 3, 4)] * 3

    def call_dev(src_ok=True, srclen=256, count=3, origins=O, ptrs="all", shapes=S, strides=None, rank=3, shift=0):
        p = None
        if ptrs is not None:
            p = (ctypes.c_void_p * 3)(*[None if ptrs == k else dst[k].ctypes.data + shift for k in range(3)])
        return dev(src.ctypes.data if src_ok else None, srclen, count, rows(origins), p, rows(shapes), rows(strides), ctypes.c_uint(rank), None)

    def call_host(src_ok=True, srclen=256, count=3, origins=O, dst_ok=True, extents=S, rank=3, cap=dst.nbytes):
        return host(src.ctypes.data if src_ok else None, srclen, count, rows(origins), rows(extents), ctypes.c_uint(rank), dst.ctypes.data if dst_ok else None, cap)

    def one(row, k, n=3, good=(0, 0, 0)):
        return [row if i == k else good for i in range(n)]
    common = [dict(src_ok=False), dict(origins=None), dict(srclen=0), dict(srclen=-7), dict(rank=0), dict(rank=4), dict(count=0), dict(count=-3)]
    common += [dict(origins=one((0, -1, 0), k)) for k in range(3)] + [dict(origins=one((0, 0, -(2 ** 62)), 2))]
    dev_only = [dict(ptrs=None), dict(ptrs=0), dict(ptrs=1), dict(ptrs=2), dict(shapes=None)]
    dev_only += [dict(shapes=one(bad, k, good=(2, 3, 4))) for k in range(3) for bad in ((2, 0, 4), (2, 3, -4))]
    dev_only += [dict(strides=one(bad, k, good=(12, 4, 1))) for k in range(3) for bad in ((12, 4, 2), (12, 3, 1), (11, 4, 1), (12, 0, 1))]
    for kw in common + dev_only + ([dict(shift=1)] if dtype == np.uint16 else []):
        assert call_dev(**kw) == 1, kw
    for kw in common + [dict(extents=None), dict(dst_ok=False)]:
        assert call_host(**kw) == 1, kw
    assert call_host() == 1                                              # (no sqy header in the blob: refused on the host as well)
    assert (dst == 9).all()
