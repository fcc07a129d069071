"""The packed batch encode on the host.  sqy::packed_places (csrc/sqy_pipeline.cpp), the one statement of the placement rule, under
AddressSanitizer + UndefinedBehaviorSanitizer as a stand-alone program built with g++ (tests/sanitize/batch_packed_test.cpp, as
test_host_batch_views.py builds its own): a table written out by hand inside the program, and a grid of cases -- every align from 1 to
65536, lengths that are multiples of it and not, gaps, capacities at the end, one byte short and in mid-table, sums past 2^32, ends at
2^63 -- that it prints line by line and the restatement below must reproduce byte for byte.  And what the four entry points must do
without a GPU: the argument rules, which come before any device is looked for."""
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


def packed_places(lengths, gaps, align, base, capacity):
    """the rule again: (ok, end, first_unfit, places); anything at or above 2^63 is refused"""
    if align < 1 or align > 65536 or align & (align - 1) or (gaps and len(gaps) != len(lengths)) or base >= 1 << 63:
        return 0, 0, 0, []
    at, end, cur, unfit = [], base, base, len(lengths)
    for j, n in enumerate(lengths):
        at.append(cur + (gaps[j] if gaps else 0))
        end = at[-1] + n
        cur = -(-end // align) * align
        if end >= 1 << 63 or (j + 1 < len(lengths) and cur >= 1 << 63):
            return 0, 0, 0, []
        if end > capacity and unfit == len(lengths):
            unfit = j
    return 1, end, unfit, at


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_packed_places_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "batch_packed_test")
    subprocess.check_call(["g++"] + SAN + [os.path.join(ROOT, "tests", "sanitize", "batch_packed_test.cpp"), os.path.join(CSRC, "sqy_pipeline.cpp"), "-o", exe,
                                          "-lpthread"])
    r = subprocess.run([exe], env=ENV, capture_output=True, text=True, timeout=120)
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    assert r.returncode == 0 and r.stdout.endswith("batch_packed ok\n"), (r.returncode, r.stdout[-500:], r.stderr[-2000:])
    lines = r.stdout.splitlines()[:-1]
    aligns, refused, short, past32 = set(), 0, 0, 0
    for line in lines:
        args, got = line.split(" => ")
        head, lens, gaps = [[int(x) for x in part.split()] for part in args.split("|")]
        ok, end, unfit, at = packed_places(lens, gaps, *head)
        want = "%d %d %d |%s" % (ok, end, unfit, "".join(" %d" % x for x in at))
        assert got == want, line
        aligns.add(head[0])
        refused += not ok
        short += bool(ok) and unfit < len(lens)
        past32 += bool(ok) and end > 1 << 32
    # the grid is the one the issue asks for
    assert {1 << k for k in range(17)} <= aligns and refused >= 17 and short >= 17 * 3 and past32 >= 17, (sorted(aligns), refused, short, past32)
    assert len(lines) > 400


def test_the_restatement_on_the_rule_as_the_header_states_it():
    """offsets[0] = 0, offsets[i + 1] = round_up(offsets[i] + lengths[i], align), total = offsets[n - 1] + lengths[n - 1]"""
    lens = [21, 16, 1, 4096, 33]
    for align in (1, 16, 4096):
        ok, end, unfit, at = packed_places(lens, [], align, 0, 1 << 40)
        assert ok and unfit == len(lens) and at[0] == 0 and end == at[-1] + lens[-1]
        for i in range(len(lens) - 1):
            assert at[i + 1] == (at[i] + lens[i] + align - 1) // align * align


@pytest.mark.parametrize("dtype", [np.uint16, np.uint8])
@pytest.mark.parametrize("host", [False, True])
def test_bad_arguments_return_1_with_zeroed_tables(sqy, dtype, host):
    """align 0, 3 and 131072, total == NULL, dst_capacity <= 0 and the Batch call's own refusals: 1, offsets, lengths and *total zeroed, nothing
    written, no device needed"""
    sfx = "UI16" if dtype == np.uint16 else "UI8"
    fn = getattr(sqy.lib(), "SQYAMD_PipelineEncode_BatchPacked_%s%s" % (sfx, "" if host else "_Device"))
    vols = [np.zeros((2, 3, 4), dtype), np.zeros((1, 2, 3), dtype)]
    dst = np.zeros(4096, np.uint8)

    def call(pipeline=b"bitswap1->lz4", srcs=True, shapes=((2, 3, 4), (1, 2, 3)), n=2, dst_ok=True, tables=True, align=1, cap=4096, total_ok=True, strides=None):
        ptrs = (ctypes.c_void_p * 2)(*[v.ctypes.data for v in vols]) if srcs else None
        shp = (ctypes.c_long * 6)(*[x for s in shapes for x in s]) if shapes else None
        offs = (ctypes.c_long * 2)(7, 7)
        lens = (ctypes.c_long * 2)(7, 7)
        total = ctypes.c_long(7)
        args = [pipeline, ptrs, shp]
        if not host:
            args.append((ctypes.c_long * 6)(*[x for s in strides for x in s]) if strides else None)
        args += [ctypes.c_uint(3), ctypes.c_int(n), dst.ctypes.data if dst_ok else None, ctypes.c_long(cap), ctypes.c_long(align),
                 offs if tables else None, lens if tables else None, ctypes.byref(total) if total_ok else None, ctypes.c_int(0)]
        if not host:
            args.append(None)
        return fn(*args), list(offs), list(lens), total.value
    assert call(n=0) == (1, [7, 7], [7, 7], 0)                           # (no volume: no table entry to zero)
    assert call(n=-3)[0] == 1
    assert call(tables=False)[0::3] == (1, 0)
    assert call(total_ok=False) == (1, [0, 0], [0, 0], 7)                # (no total to zero)
    bad = [dict(align=0), dict(align=3), dict(align=131072), dict(align=-16), dict(cap=0), dict(cap=-4096),
           dict(srcs=False), dict(shapes=None), dict(dst_ok=False), dict(shapes=((2, 3, 4), (1, 0, 3))), dict(pipeline=b"no_such_stage->lz4"), dict(pipeline=None)]
    if not host:
        bad += [dict(strides=((12, 4, 2), (6, 3, 1))), dict(strides=((12, 3, 1), (6, 3, 1)))]      # an innermost stride of 2; rows that overlap
    for kw in bad:
        assert call(**kw) == (1, [0, 0], [0, 0], 0), kw
    assert (dst == 0).all()
