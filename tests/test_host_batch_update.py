"""The window update on the host.  The mask and the merge of csrc/sqy_batch_window.hpp, which the patch kernel compiles, and the host-only
plan (sqy::update_batch_plan, csrc/sqy_pipeline.cpp) under AddressSanitizer + UndefinedBehaviorSanitizer as a stand-alone program built
with g++ (tests/sanitize/batch_update_test.cpp, as test_host_batch_packed.py builds its own): planes patched run by run must be the
bit-plane transpose of the pasted volume for every window of small blobs, and the restated transpose must reproduce the golden planes.
And what SQYAMD_Update_BatchWindow_* must do without a GPU: the argument rules, which come before any device is looked for."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sqeazy_amd", "csrc")
SAN = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:exitcode=97:abort_on_error=0", UBSAN_OPTIONS="halt_on_error=1:exitcode=98:print_stacktrace=1")
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_mask_merge_and_plan_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "batch_update_test")
    # (the kernels' job struct lives in sqy_kernels.h, which names HIP's stream type: the runtime's C header, nothing linked)
    subprocess.check_call(["g++"] + SAN + ["-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(ROCM, "include"), os.path.join(ROOT, "tests", "sanitize", "batch_update_test.cpp"),
                                           os.path.join(CSRC, "sqy_pipeline.cpp"), "-o", exe, "-lpthread"])
    r = subprocess.run([exe, os.path.join(ROOT, "tests", "golden")], env=ENV, capture_output=True, text=True, timeout=300)
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    assert r.returncode == 0 and r.stdout.endswith("batch_update ok\n"), (r.returncode, r.stdout[-500:], r.stderr[-2000:])
    counts = [int(x) for x in r.stdout.splitlines()[-2].split()[2::2]]
    assert len(counts) == 3 and min(counts) > 0, r.stdout              # runs outside, inside and partly inside the window were all patched


@pytest.mark.parametrize("dtype", [np.uint16, np.uint8])
def test_bad_arguments_return_1_with_zeroed_tables(sqy, dtype):
    """1, offsets and lengths zeroed, nothing written, no device needed"""
    fn = getattr(sqy.lib(), "SQYAMD_Update_BatchWindow_%s_Device" % ("UI16" if dtype == np.uint16 else "UI8"))
    src = np.zeros(256, np.uint8)
    wins = [np.zeros((2, 3, 4), dtype), np.zeros((1, 2, 3), dtype)]
    dst = np.zeros(4096, np.uint8)

    def call(pipeline=b"bitswap1->lz4", src_ok=True, offs=(0, 128), lens=(100, 100), n=2, origins=((0, 0, 0), (1, 1, 1)), wins_ok=(True, True), ptrs_ok=True,
             shapes=((2, 3, 4), (1, 2, 3)), strides=None, rank=3, dst_ok=True, cap=2048, tables=True):
        ptrs = (ctypes.c_void_p * 2)(*[w.ctypes.data if ok else None for w, ok in zip(wins, wins_ok)]) if ptrs_ok else None
        longs = lambda rows: (ctypes.c_long * 6)(*[x for r in rows for x in r]) if rows else None
        out_offs = (ctypes.c_long * 2)(7, 7)
        out_lens = (ctypes.c_long * 2)(7, 7)
        rc = fn(pipeline, src.ctypes.data if src_ok else None, (ctypes.c_long * 2)(*offs) if offs else None, (ctypes.c_long * 2)(*lens) if lens else None, ctypes.c_int(n),
                longs(origins), ptrs, longs(shapes), longs(strides), ctypes.c_uint(rank), dst.ctypes.data if dst_ok else None, ctypes.c_long(cap),
                out_offs if tables else None, out_lens if tables else None, ctypes.c_int(0), None)
        return rc, list(out_offs), list(out_lens)
    assert call(n=0) == (1, [7, 7], [7, 7])                              # (no blob: no table entry to zero)
    assert call(n=-3)[0] == 1
    assert call(tables=False)[0] == 1
    other = b"quantiser->bitswap1->lz4" if dtype == np.uint8 else b"bitswap1->"                              # not admitted for the voxel type / malformed
    assert not sqy.pipeline_possible(other.decode(), dtype)
    bad = [dict(pipeline=None), dict(src_ok=False), dict(offs=None), dict(lens=None), dict(ptrs_ok=False), dict(wins_ok=(True, False)), dict(shapes=None),
           dict(dst_ok=False), dict(rank=0), dict(rank=4), dict(cap=0), dict(cap=-2048), dict(pipeline=b"no_such_stage->lz4"), dict(pipeline=other),
           dict(shapes=((2, 3, 4), (1, 0, 3))), dict(origins=((0, 0, 0), (1, -1, 1))), dict(offs=(0, -128)), dict(lens=(100, 0)), dict(lens=(-5, 100)),
           dict(strides=((12, 4, 2), (6, 3, 1))), dict(strides=((12, 3, 1), (6, 3, 1)))]      # an innermost stride of 2; rows that overlap
    for kw in bad:
        assert call(**kw) == (1, [0, 0], [0, 0]), kw
    assert (dst == 0).all()
