"""Batch decode on the host: decode_batch_plan (csrc/sqy_pipeline.cpp) under AddressSanitizer + UndefinedBehaviorSanitizer as a stand-alone
program, built with g++ as test_host_batch_plan.py builds its target; and what the loaded library must do without a GPU -- the two options
and the four entry points' argument checks, which come before any device is looked for (the host variants read the headers first as well)."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

from sqeazy_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sqeazy_amd", "csrc")
SAN = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:exitcode=97:abort_on_error=0", UBSAN_OPTIONS="halt_on_error=1:exitcode=98:print_stacktrace=1")


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_decode_batch_plan_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "decode_batch_plan_test")
    subprocess.check_call(["g++"] + SAN + [os.path.join(ROOT, "tests", "sanitize", "decode_batch_plan_test.cpp"), os.path.join(CSRC, "sqy_pipeline.cpp"), "-o", exe,
                                          "-lpthread"])
    r = subprocess.run([exe], env=ENV, capture_output=True, text=True, timeout=120)
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    assert r.returncode == 0 and "decode_batch_plan ok" in r.stdout, (r.returncode, r.stdout, r.stderr[-2000:])


def test_options(sqy, options):
    assert sqy.get_option("decode_batch_joint") == 1
    options("decode_batch_joint", 0)
    assert sqy.get_option("decode_batch_joint") == 0
    with pytest.raises(ValueError):
        sqy.set_option("decode_batch_joint", 2)
    assert sqy.get_option("decode_batch_joint") == 0
    assert sqy.get_option("decode_batch_group_bytes") == 1 << 32          # the slab-set decode's 4 GiB bound
    for value in (1, 300000, 1 << 32):
        options("decode_batch_group_bytes", value)
        assert sqy.get_option("decode_batch_group_bytes") == value
    for value in (0, (1 << 32) + 1):
        with pytest.raises(ValueError):
            sqy.set_option("decode_batch_group_bytes", value)
        assert sqy.get_option("decode_batch_group_bytes") == 1 << 32


@pytest.mark.parametrize("dtype", [np.uint16, np.uint8])
@pytest.mark.parametrize("host", [False, True])
def test_bad_arguments_return_1_with_zeroed_lengths(sqy, dtype, host):
    """nblobs 0 and negative, NULL tables, a NULL entry in d_dsts, a negative offset, a zero length: 1, decoded_bytes zeroed, no device needed"""
    sfx = "UI16" if dtype == np.uint16 else "UI8"
    fn = getattr(sqy.lib(), "SQYAMD_Decode_Batch_%s%s" % (sfx, "" if host else "_Device"))
    src = np.zeros(256, np.uint8)
    outs = [np.full(64, 0xA5, np.uint8), np.full(64, 0xA5, np.uint8)]

    def call(n=2, src_ok=True, offs=(0, 100), lens=(100, 100), dsts=(True, True), caps=(64, 64), decoded=True):
        o = (ctypes.c_long * 2)(*offs) if offs is not None else None
        ln = (ctypes.c_long * 2)(*lens) if lens is not None else None
        p = (ctypes.c_void_p * 2)(*[outs[i].ctypes.data if ok else None for i, ok in enumerate(dsts)]) if dsts is not None else None
        c = (ctypes.c_long * 2)(*caps) if caps is not None else None
        d = (ctypes.c_long * 2)(7, 7)
        args = [src.ctypes.data if src_ok else None, o, ln, ctypes.c_int(n), p, c, d if decoded else None]
        if not host:
            args.append(None)
        return fn(*args), list(d)
    assert call(n=0) == (1, [7, 7])                                        # (no blob: nothing to zero)
    assert call(n=-3) == (1, [7, 7])
    if host:
        assert call(decoded=False)[0] == 1                                 # (zeros where a header should be; decoded_bytes may be NULL)
        assert call() == (1, [0, 0])
    assert call(dsts=(False, True), decoded=False)[0] == 1
    for kw in (dict(src_ok=False), dict(offs=None), dict(lens=None), dict(dsts=None), dict(caps=None), dict(dsts=(True, False)), dict(offs=(0, -1)),
               dict(lens=(100, 0)), dict(lens=(-5, 100))):
        assert call(**kw) == (1, [0, 0]), kw
    assert all((o == 0xA5).all() for o in outs)


@pytest.mark.parametrize("dtype", [np.uint16, np.uint8])
def test_host_variant_reads_the_headers_before_it_looks_for_a_device(sqy, oracle, dtype):
    """oracle-made blobs: a capacity one byte short, the other voxel type and a truncated header return 1 with the destinations untouched"""
    sfx = "UI16" if dtype == np.uint16 else "UI8"
    fn = getattr(sqy.lib(), "SQYAMD_Decode_Batch_" + sfx)
    other = np.uint8 if dtype == np.uint16 else np.uint16
    vols = [synth.stack((3, 5, 7), dtype), synth.stack((2, 4, 6), dtype, seed=2)]
    blobs = [oracle.pipeline_encode("bitswap1->lz4", v, nthreads=2) for v in vols]
    alien = oracle.pipeline_encode("bitswap1->lz4", synth.stack((2, 4, 6), other), nthreads=2)

    def call(blobs, caps, cut=None):
        src = np.frombuffer(b"".join(blobs), dtype=np.uint8).copy()
        offs = (ctypes.c_long * 2)(0, len(blobs[0]))
        lens = (ctypes.c_long * 2)(*[len(b) for b in blobs])
        if cut is not None:
            lens[cut] = 40
        outs = [np.full(v.nbytes + 16, 0xA5, np.uint8) for v in vols]
        p = (ctypes.c_void_p * 2)(*[o.ctypes.data for o in outs])
        d = (ctypes.c_long * 2)(7, 7)
        rc = fn(src.ctypes.data, offs, lens, ctypes.c_int(2), p, (ctypes.c_long * 2)(*caps), d)
        assert all((o == 0xA5).all() for o in outs), "written although the call was refused"
        return rc, list(d)
    full = [v.nbytes for v in vols]
    assert call(blobs, [full[0], full[1] - 1]) == (1, [0, 0])
    assert call(blobs, [full[0] - 1, full[1]]) == (1, [0, 0])
    assert call([blobs[0], alien], full) == (1, [0, 0])
    assert call(blobs, full, cut=1) == (1, [0, 0])
