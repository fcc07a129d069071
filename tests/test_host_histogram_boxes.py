"""The intensity histograms of boxes of one blob, on the host.  The routing (sqy::histogram_boxes_path), the admission
(sqy::admit_histogram: every refusal, the shift at its bounds, origins near 2^63) and the range transposer's counting walk -- workgroups
of 256 threads, the vote for a window, the clip and sqy::window_histogram16 into an array standing in for the LDS window plus the output
for what misses it -- under AddressSanitizer + UndefinedBehaviorSanitizer as a stand-alone program built with g++
(tests/sanitize/histogram_boxes_test.cpp, as test_host_bin_boxes.py builds its own).  And what SQYAMD_Histogram_Boxes_* must do without a
GPU: the declarations, the option, the argument rules that come before any device is looked for, the Python helpers."""
import ctypes
import math
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
ENTRY_POINTS = ("SQYAMD_Histogram_Boxes_UI16_Device", "SQYAMD_Histogram_Boxes_UI8_Device", "SQYAMD_Histogram_Boxes_UI16", "SQYAMD_Histogram_Boxes_UI8")


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_path_table_admission_and_counting_walk_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "histogram_boxes_test")
    # (the kernels' job structs live in sqy_kernels.h, which names HIP's stream type: the runtime's C header, nothing linked)
    subprocess.check_call(["g++"] + SAN + ["-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(ROCM, "include"), os.path.join(ROOT, "tests", "sanitize", "histogram_boxes_test.cpp"),
                                           os.path.join(CSRC, "sqy_pipeline.cpp"), "-o", exe, "-lpthread"])
    r = subprocess.run([exe], env=ENV, capture_output=True, text=True, timeout=300)
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    assert r.returncode == 0 and r.stdout.endswith("histogram_boxes ok\n"), (r.returncode, r.stdout[-500:], r.stderr[-2000:])
    words = r.stdout.splitlines()[-2].split()
    assert words[0] == "runs" and words[1::2] == ["outside", "inside", "partly", "window0", "window1", "window2", "window3", "offwindow", "merged", "pieces", "groups2"], r.stdout
    # runs outside, inside and partly inside a box; workgroups that voted for each of the four windows; adds that missed the window; adds
    # of several equal voxels and of whole pieces; jobs of more than one workgroup -- all met
    counts = [int(x) for x in words[2::2]]
    assert len(counts) == 11 and min(counts) > 0, r.stdout


def test_the_header_declares_the_entry_points():
    text = open(os.path.join(ROOT, "include", "sqeazy_amd.h")).read()
    for name in ENTRY_POINTS:
        m = re.search(r"SQY_FUNCTION_PREFIX int %s\(([^;]*)\);" % name, text)
        assert m, name
        args = " ".join(m.group(1).split())
        if name.endswith("_Device"):
            assert args == ("const void* d_src, long srclength, long count, const long* origins, const long* extents, unsigned rank, int shift, "
                            "void* const* d_hists, void* hip_stream"), args
        else:
            assert args == ("const char* src, long srclength, long count, const long* origins, const long* extents, unsigned rank, int shift, "
                            "char* out, long out_capacity"), args
    # no constants of its own, none under the projection's or the binning's names
    assert len(re.findall(r"#define SQYAMD_PROJECT_", text)) == 3 and not re.search(r"#define SQYAMD_(BIN|HISTOGRAM)_", text)
    assert '"histogram_boxes_subset"' in text and "SQY_NO_HISTOGRAM_BOXES_SUBSET" in text


def test_the_library_exports_the_entry_points(sqy):
    for name in ENTRY_POINTS:
        assert name in sqy.EXPORTED_SYMBOLS and getattr(sqy.lib(), name)


def test_the_option(sqy):
    assert sqy.get_option("histogram_boxes_subset") == 1
    try:
        assert sqy.lib().SQYAMD_Set_Option(b"histogram_boxes_subset", 2) == 1 and sqy.get_option("histogram_boxes_subset") == 1
        assert sqy.lib().SQYAMD_Set_Option(b"histogram_boxes_subset", -1) == 1 and sqy.get_option("histogram_boxes_subset") == 1
        sqy.set_option("histogram_boxes_subset", 0)
        assert sqy.get_option("histogram_boxes_subset") == 0
        # the binning's, the projection's and the decode's options are their own
        assert sqy.get_option("bin_boxes_subset") == 1 and sqy.get_option("project_boxes_subset") == 1 and sqy.get_option("decode_boxes_joint") == 1
    finally:
        sqy.set_option("histogram_boxes_subset", 1)


def test_the_environment_switch():
    """SQY_NO_HISTOGRAM_BOXES_SUBSET=1 is read when the library is loaded: a fresh interpreter"""
    import sys
    code = "import sqeazy_amd; print(sqeazy_amd.get_option('histogram_boxes_subset'), sqeazy_amd.get_option('bin_boxes_subset'))"
    for env, want in (({"SQY_NO_HISTOGRAM_BOXES_SUBSET": "1"}, ["0", "1"]), ({}, ["1", "1"])):
        clean = {k: v for k, v in os.environ.items() if k not in ("SQY_NO_HISTOGRAM_BOXES_SUBSET", "SQY_NO_BIN_BOXES_SUBSET")}
        r = subprocess.run([sys.executable, "-c", code], env=dict(clean, SQEAZY_AMD_NO_TORCH_PRELOAD="1", **env), cwd=ROOT, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and r.stdout.split()[-2:] == want, (r.stdout, r.stderr[-2000:])


@pytest.mark.parametrize("dtype", [np.uint16, np.uint8])
def test_bad_arguments_return_1_with_the_outputs_untouched_before_a_device_is_looked_for(sqy, dtype):
    """NULL pointers, count below 1, a NULL histogram among the histograms, a histogram 1, 2 or 3 bytes off, a negative origin in ANY box,
    an extent below 1, rank 0 or above 3, srclength <= 0, the shift below 0 or at the voxel's bits, a capacity one byte short: 1, the
    outputs as they were"""
    sfx, bits = ("UI16", 16) if dtype == np.uint16 else ("UI8", 8)
    dev, host = getattr(sqy.lib(), "SQYAMD_Histogram_Boxes_%s_Device" % sfx), getattr(sqy.lib(), "SQYAMD_Histogram_Boxes_" + sfx)
    src = np.zeros(256, np.uint8)
    SHIFT = bits - 3                                                    # eight bins
    outs = np.full((3, 16), 0xABCD1234, np.uint32)                      # (room for 3 histograms of 8 counters, up to 3 bytes off)
    rows = lambda v: None if v is None else (ctypes.c_long * max(sum(len(r) for r in v), 1))(*[x for r in v for x in r])
    O, S = [(0, 0, 0)] * 3, [(2, 3, 4)] * 3

    def call_dev(src_ok=True, srclen=256, count=3, origins=O, ptrs="all", extents=S, rank=3, off=0, shift=SHIFT):
        p = None
        if ptrs is not None:
            p = (ctypes.c_void_p * 3)(*[None if ptrs == k else outs[k].ctypes.data + off for k in range(3)])
        return dev(src.ctypes.data if src_ok else None, srclen, count, rows(origins), rows(extents), ctypes.c_uint(rank), shift, p, None)

    def call_host(src_ok=True, srclen=256, count=3, origins=O, out_ok=True, extents=S, rank=3, nbytes=outs.nbytes, shift=SHIFT):
        return host(src.ctypes.data if src_ok else None, srclen, count, rows(origins), rows(extents), ctypes.c_uint(rank), shift, outs.ctypes.data if out_ok else None, nbytes)

    def one(row, k, n=3, good=(0, 0, 0)):
        return [row if i == k else good for i in range(n)]

    common = [dict(src_ok=False), dict(origins=None), dict(extents=None), dict(srclen=0), dict(srclen=-7), dict(rank=0), dict(rank=4), dict(count=0), dict(count=-3)]
    common += [dict(origins=one((0, -1, 0), k)) for k in range(3)] + [dict(origins=one((0, 0, -(2 ** 62)), 2))]
    common += [dict(shift=bits), dict(shift=-1), dict(shift=bits + 1), dict(shift=2 ** 31 - 1), dict(shift=-(2 ** 31))]
    common += [dict(extents=one(bad, k, good=(2, 3, 4))) for k in range(3) for bad in ((2, 0, 4), (2, 3, -4))]
    dev_only = [dict(ptrs=None), dict(ptrs=0), dict(ptrs=1), dict(ptrs=2), dict(off=1), dict(off=2), dict(off=3)]
    for kw in common + dev_only:
        assert call_dev(**kw) == 1, kw
        assert (outs == 0xABCD1234).all(), kw
    for kw in common + [dict(out_ok=False)]:
        assert call_host(**kw) == 1, kw
        assert (outs == 0xABCD1234).all(), kw
    assert call_host() == 1 and (outs == 0xABCD1234).all()               # (no sqy header in the blob: refused on the host as well)
    # out_capacity against a blob with a header of (2, 3, 4) voxels: one byte less than the histograms hold -- refused on the host
    from sqeazy_amd import multi
    blob = np.frombuffer(multi.build_header("lz4", dtype, (2, 3, 4), 64) + bytes(64), np.uint8).copy()
    for shift in (SHIFT, bits - 1, bits - 2):
        for nbytes in (3 * ((1 << bits) >> shift) * 4 - 1, 0, -1):
            rc = host(blob.ctypes.data, len(blob), 3, rows(O), rows(S), ctypes.c_uint(3), shift, outs.ctypes.data, nbytes)
            assert rc == 1 and (outs == 0xABCD1234).all(), (shift, nbytes)


def test_histogram_bins(sqy):
    assert sqy.histogram_bins(np.uint16, 0) == 65536 and sqy.histogram_bins(np.uint16, 1) == 32768 and sqy.histogram_bins(np.uint16, 15) == 2
    assert sqy.histogram_bins(np.uint8, 0) == 256 and sqy.histogram_bins(np.uint8, 3) == 32 and sqy.histogram_bins(np.uint8, 7) == 2
    for dtype, shift in ((np.uint16, 16), (np.uint16, -1), (np.uint8, 8), (np.uint8, -1), (np.uint32, 0), (np.float32, 0)):
        with pytest.raises(ValueError):
            sqy.histogram_bins(dtype, shift)


def _nearest_rank(x, q):
    return int(np.sort(x)[max(1, math.ceil(q * x.size)) - 1])


def test_histogram_quantile(sqy):
    """the nearest-rank quantile: np.sort(x)[max(1, ceil(q N)) - 1] at shift 0, that value with its low `shift` bits cleared above"""
    rng = np.random.default_rng(5)
    draws = [rng.integers(0, 65536, 1000), rng.integers(900, 1100, 37), rng.integers(0, 256, 513), np.full(77, 12345), np.array([0]), np.array([65535, 0, 65535]),
             (rng.normal(3000, 400, 5000).clip(0, 65535)).astype(np.int64)]
    for x in draws:
        for shift in (0, 1, 4, 15):
            hist = np.bincount(x >> shift, minlength=65536 >> shift).astype(np.uint32)
            for q in (0.0, 1.0, 0.5, 0.01, 0.99, 1.0 / 3, 0.999, 1e-9) + tuple(rng.random(5)):
                want = _nearest_rank(x, q) >> shift << shift
                assert sqy.histogram_quantile(hist, q, shift) == want, (x.size, shift, q)
        assert sqy.histogram_quantile(np.bincount(x, minlength=65536), 0.0) == int(x.min()) and sqy.histogram_quantile(np.bincount(x, minlength=65536), 1.0) == int(x.max())
    const = np.bincount(np.full(77, 12345), minlength=65536)
    assert all(sqy.histogram_quantile(const, q) == 12345 for q in (0.0, 0.3, 1.0))
    # counts whose sum passes 2^32: the cumulative count is 64 bits wide
    big = np.zeros(256, np.uint32)
    big[3] = big[200] = 0xFFFFFFFF
    assert sqy.histogram_quantile(big, 0.5) == 3 and sqy.histogram_quantile(big, 0.51) == 200
    for bad in (np.zeros(256, np.uint32), np.zeros(0, np.uint32)):
        with pytest.raises(ValueError):
            sqy.histogram_quantile(bad, 0.5)
    for q in (-0.01, 1.01, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            sqy.histogram_quantile(const, q)
