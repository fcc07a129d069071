"""The window compare on the host.  The accumulate routine of csrc/sqy_batch_window.hpp, which the comparing kernels compile, under
AddressSanitizer + UndefinedBehaviorSanitizer as a stand-alone program built with g++ (tests/sanitize/batch_compare_test.cpp, as
test_host_batch_update.py builds its own): driven run by run as the comparing transposer drives it, its sums must be a triple loop's for
every window of small blobs.  And what SQYAMD_Compare_BatchWindow_* must do without a GPU: the argument rules, which come before any
device is looked for."""
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
FIELDS = 8


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_accumulate_routine_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "batch_compare_test")
    # (the kernels' job struct lives in sqy_kernels.h, which names HIP's stream type: the runtime's C header, nothing linked)
    subprocess.check_call(["g++"] + SAN + ["-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(ROCM, "include"), os.path.join(ROOT, "tests", "sanitize", "batch_compare_test.cpp"),
                                           os.path.join(CSRC, "sqy_pipeline.cpp"), "-o", exe, "-lpthread"])
    r = subprocess.run([exe], env=ENV, capture_output=True, text=True, timeout=300)
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    assert r.returncode == 0 and r.stdout.endswith("batch_compare ok\n"), (r.returncode, r.stdout[-500:], r.stderr[-2000:])
    counts = [int(x) for x in r.stdout.splitlines()[-2].split()[2::2]]
    assert len(counts) == 3 and min(counts) > 0, r.stdout              # runs outside, inside and partly inside the window were all compared


def test_the_header_names_the_fields():
    text = open(os.path.join(ROOT, "include", "sqeazy_amd.h")).read()
    names = ("VOXELS", "NDIFF", "SUM_ABS", "SUM_SQ", "MAX_ABS", "VIEW_SUM", "VIEW_MIN", "VIEW_MAX")
    assert "#define SQYAMD_COMPARE_FIELDS %d" % FIELDS in text
    for k, name in enumerate(names):
        assert "#define SQYAMD_COMPARE_%s %d " % (name, k) in text, name


def test_the_option(sqy):
    assert sqy.get_option("batch_compare_fused") == 1
    try:
        assert sqy.lib().SQYAMD_Set_Option(b"batch_compare_fused", 2) == 1 and sqy.get_option("batch_compare_fused") == 1
        sqy.set_option("batch_compare_fused", 0)
        assert sqy.get_option("batch_compare_fused") == 0
    finally:
        sqy.set_option("batch_compare_fused", 1)


@pytest.mark.parametrize("dtype", [np.uint16, np.uint8])
def test_bad_arguments_return_1_with_zeroed_stats(sqy, dtype):
    """1, stats zeroed, no device needed"""
    fn = getattr(sqy.lib(), "SQYAMD_Compare_BatchWindow_%s_Device" % ("UI16" if dtype == np.uint16 else "UI8"))
    src = np.zeros(256, np.uint8)
    views = [np.full((2, 3, 4), 9, dtype), np.full((1, 2, 3), 9, dtype)]
    before = [v.copy() for v in views]

    def call(src_ok=True, offs=(0, 128), lens=(100, 100), n=2, origins=((0, 0, 0), (1, 1, 1)), views_ok=(True, True), ptrs_ok=True, shapes=((2, 3, 4), (1, 2, 3)),
             strides=None, rank=3, stats_ok=True):
        ptrs = (ctypes.c_void_p * 2)(*[v.ctypes.data if ok else None for v, ok in zip(views, views_ok)]) if ptrs_ok else None
        longs = lambda rows: (ctypes.c_long * 6)(*[x for r in rows for x in r]) if rows else None
        stats = (ctypes.c_ulonglong * (2 * FIELDS))(*([7] * (2 * FIELDS)))
        rc = fn(src.ctypes.data if src_ok else None, (ctypes.c_long * 2)(*offs) if offs else None, (ctypes.c_long * 2)(*lens) if lens else None, ctypes.c_int(n),
                longs(origins), ptrs, longs(shapes), longs(strides), ctypes.c_uint(rank), stats if stats_ok else None, None)
        return rc, list(stats)
    assert call(n=0) == (1, [7] * (2 * FIELDS))                           # (no blob: no row to zero)
    assert call(n=-3) == (1, [7] * (2 * FIELDS))
    assert call(stats_ok=False)[0] == 1                                   # a NULL stats
    bad = [dict(src_ok=False), dict(offs=None), dict(lens=None), dict(ptrs_ok=False), dict(views_ok=(True, False)), dict(views_ok=(False, True)), dict(shapes=None),
           dict(rank=0), dict(rank=4), dict(shapes=((2, 3, 4), (1, 0, 3))), dict(origins=((0, 0, 0), (1, -1, 1))), dict(offs=(0, -128)), dict(lens=(100, 0)),
           dict(lens=(-5, 100)), dict(strides=((12, 4, 2), (6, 3, 1))), dict(strides=((12, 3, 1), (6, 3, 1)))]      # an innermost stride of 2; rows that overlap
    for kw in bad:
        assert call(**kw) == (1, [0] * (2 * FIELDS)), kw
    assert all(np.array_equal(v, b) for v, b in zip(views, before))


def test_compare_metrics_is_plain_float64(sqy):
    """the definitions, on integers too large for float32 and with the denominators that vanish"""
    row = [1000, 10, 12345, 2 ** 40 + 1, 65535, 1000 * 300, 100, 900]
    m = sqy.compare_metrics(row, np.uint16)
    mse = np.float64(2 ** 40 + 1) / np.float64(1000)
    want = dict(mse=mse, rms=np.sqrt(mse), nrmse=np.sqrt(mse) / np.float64(800), mnmse=np.sqrt(mse) / np.float64(300), l1norm=np.float64(12345),
                l2norm=np.float64(2 ** 40 + 1), psnr=np.float64(20) * np.log10(np.float64(65535)) - np.float64(10) * np.log10(mse), drange=np.float64(800))
    assert sorted(m) == sorted(want)
    for k, v in want.items():
        assert abs(m[k] - v) <= 1e-12 * abs(v), k
    m = sqy.compare_metrics([64, 0, 0, 0, 0, 64 * 5, 5, 5], np.uint8)      # an equal pair on a constant view
    assert m["mse"] == 0 and m["rms"] == 0 and np.isnan(m["nrmse"]) and m["mnmse"] == 0 and m["psnr"] == np.inf and m["drange"] == 0
    m = sqy.compare_metrics([64, 64, 64, 64, 1, 0, 0, 0], np.uint8)        # a view of zeros
    assert m["mse"] == 1 and m["nrmse"] == np.inf and m["mnmse"] == np.inf
