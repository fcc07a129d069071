"""Batch encode on the host: lz4_batch_plan (csrc/sqy_pipeline.cpp) under AddressSanitizer + UndefinedBehaviorSanitizer, built with g++ as
test_host_sanitizers.py builds its targets; and what the loaded library must do without a GPU -- the three options and the four entry
points' argument checks, which come before any device is looked for."""
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


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_batch_plan_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "batch_plan_test")
    subprocess.check_call(["g++"] + SAN + [os.path.join(ROOT, "tests", "sanitize", "batch_plan_test.cpp"), os.path.join(CSRC, "sqy_pipeline.cpp"), "-o", exe,
                                          "-lpthread"])
    r = subprocess.run([exe], env=ENV, capture_output=True, text=True, timeout=120)
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    assert r.returncode == 0 and "batch_plan ok" in r.stdout, (r.returncode, r.stdout, r.stderr[-2000:])


def test_options(sqy, options):
    assert sqy.get_option("encode_batch_joint") == 1
    options("encode_batch_joint", 0)
    assert sqy.get_option("encode_batch_joint") == 0
    with pytest.raises(ValueError):
        sqy.set_option("encode_batch_joint", 2)
    assert sqy.get_option("encode_batch_group_bytes") == 1 << 30
    for name, lowest in (("encode_batch_group_bytes", 1), ("encode_batch_joint_max_bytes", 0)):
        for value in (lowest, 12345, (1 << 32) - 1):
            options(name, value)
            assert sqy.get_option(name) == value
        for value in (lowest - 1, 1 << 32):
            with pytest.raises(ValueError):
                sqy.set_option(name, value)
            assert sqy.get_option(name) == (1 << 32) - 1


@pytest.mark.parametrize("dtype", [np.uint16, np.uint8])
@pytest.mark.parametrize("host", [False, True])
def test_bad_arguments_return_1_with_zeroed_tables(sqy, dtype, host):
    """nvolumes = 0, a NULL table, a zero extent and an unsupported pipeline: 1, offsets and lengths zeroed, no device needed"""
    sfx = "UI16" if dtype == np.uint16 else "UI8"
    fn = getattr(sqy.lib(), "SQYAMD_PipelineEncode_Batch_%s%s" % (sfx, "" if host else "_Device"))
    vols = [np.zeros((2, 3, 4), dtype), np.zeros((1, 2, 3), dtype)]
    dst = np.zeros(4096, np.uint8)

    def call(pipeline=b"bitswap1->lz4", srcs=True, shapes=((2, 3, 4), (1, 2, 3)), n=2, dst_ok=True, tables=True):
        ptrs = (ctypes.c_void_p * 2)(*[v.ctypes.data for v in vols]) if srcs else None
        shp = (ctypes.c_long * 6)(*[x for s in shapes for x in s]) if shapes else None
        offs = (ctypes.c_long * 2)(7, 7)
        lens = (ctypes.c_long * 2)(7, 7)
        args = [pipeline, ptrs, shp, ctypes.c_uint(3), ctypes.c_int(n), dst.ctypes.data if dst_ok else None, ctypes.c_long(2048),
                offs if tables else None, lens if tables else None, ctypes.c_int(0)]
        if not host:
            args.append(None)
        return fn(*args), list(offs), list(lens)
    assert call(n=0) == (1, [7, 7], [7, 7])                              # (no volume: nothing to zero)
    assert call(n=-3)[0] == 1
    assert call(tables=False)[0] == 1
    for kw in (dict(srcs=False), dict(shapes=None), dict(dst_ok=False), dict(shapes=((2, 3, 4), (1, 0, 3))), dict(shapes=((2, 3, 4), (1, -2, 3))),
               dict(pipeline=b"no_such_stage->lz4"), dict(pipeline=b"quantiser->lz4") if dtype == np.uint8 else dict(pipeline=b""), dict(pipeline=None)):
        assert call(**kw) == (1, [0, 0], [0, 0]), kw
    assert (dst == 0).all()
