"""Many boxes written into one large blob, on the host.  The plan (sqy::update_boxes_plan: segments and layers) under AddressSanitizer +
UndefinedBehaviorSanitizer as a stand-alone program built with g++ (tests/sanitize/update_boxes_test.cpp, as test_host_update_box.py builds
its own; it is never loaded into Python).  The case table of the GPU test (tests/update_boxes_cases.py): every case is what its name says,
checked with numpy.  And what SQYAMD_Update_Boxes_* must do without a GPU: the declarations, the option, the argument rules that come
before any device is looked for."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import update_boxes_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sqeazy_amd", "csrc")
SAN = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:exitcode=97:abort_on_error=0", UBSAN_OPTIONS="halt_on_error=1:exitcode=98:print_stacktrace=1")
DEVICE_ARGS = ("const char* pipeline, const void* d_src, long srclength, long count, const long* origins, const void* const* d_views, const long* view_shapes, "
               "const long* view_strides, unsigned rank, void* d_dst, long dst_capacity, long* dstlength, int nthreads, void* hip_stream")
HOST_ARGS = ("const char* pipeline, const char* src, long srclength, long count, const long* origins, const long* extents, unsigned rank, const char* views, "
             "long views_bytes, char* dst, long dst_capacity, long* dstlength, int nthreads")
ENTRY_POINTS = {"SQYAMD_Update_Boxes_UI16_Device": DEVICE_ARGS, "SQYAMD_Update_Boxes_UI8_Device": DEVICE_ARGS, "SQYAMD_Update_Boxes_UI16": HOST_ARGS,
                "SQYAMD_Update_Boxes_UI8": HOST_ARGS}


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_plan_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "update_boxes_test")
    subprocess.check_call(["g++"] + SAN + [os.path.join(ROOT, "tests", "sanitize", "update_boxes_test.cpp"), os.path.join(CSRC, "sqy_pipeline.cpp"), "-o", exe, "-lpthread"])
    r = subprocess.run([exe], env=ENV, capture_output=True, text=True, timeout=300)
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    assert r.returncode == 0 and r.stdout.endswith("update_boxes ok\n"), (r.returncode, r.stdout[-500:], r.stderr[-2000:])
    words = r.stdout.splitlines()[-2].split()
    counts = dict(zip(words[::2], (int(x) for x in words[1::2])))
    # merged by overlap, by a shared plane word alone, by tail voxels alone; more than one layer -- all met
    assert set(counts) == {"plans", "merged_overlap", "merged_word", "merged_tail", "layers"} and min(counts.values()) > 0, r.stdout


def test_the_header_declares_the_entry_points():
    text = open(os.path.join(ROOT, "include", "sqeazy_amd.h")).read()
    for name, want in ENTRY_POINTS.items():
        m = re.search(r"SQY_FUNCTION_PREFIX int %s\(([^;]*)\);" % name, text)
        assert m, name
        assert " ".join(m.group(1).split()) == want, name
    assert '"update_boxes_subset"' in text and "SQY_NO_UPDATE_BOXES_SUBSET" in text


def test_the_package_names_the_entry_points(sqy):
    for name in ENTRY_POINTS:
        assert name in sqy.EXPORTED_SYMBOLS and getattr(sqy.lib(), name)


def test_the_option(sqy):
    assert sqy.get_option("update_boxes_subset") == 1
    try:
        sqy.set_option("update_boxes_subset", 0)
        assert sqy.get_option("update_boxes_subset") == 0 and sqy.get_option("update_box_subset") == 1
    finally:
        sqy.set_option("update_boxes_subset", 1)


def test_the_environment_switch():
    """SQY_NO_UPDATE_BOXES_SUBSET=1 is read when the library is loaded: a fresh interpreter"""
    import sys
    code = "import sqeazy_amd; print(sqeazy_amd.get_option('update_boxes_subset'))"
    for env, want in (({"SQY_NO_UPDATE_BOXES_SUBSET": "1"}, "0"), ({}, "1")):
        clean = {k: v for k, v in os.environ.items() if k != "SQY_NO_UPDATE_BOXES_SUBSET"}
        r = subprocess.run([sys.executable, "-c", code], env=dict(clean, SQEAZY_AMD_NO_TORCH_PRELOAD="1", **env), cwd=ROOT, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and r.stdout.split()[-1] == want, (r.stdout, r.stderr[-2000:])


def _longs(v):
    return None if v is None else (ctypes.c_long * max(len(v), 1))(*v)


@pytest.mark.parametrize("dtype", [np.uint16, np.uint8])
def test_bad_arguments_return_1_before_a_device_is_looked_for(sqy, dtype):
    """NULL pointers (a NULL in the middle of d_views among them), count < 1, rank 0 or above 3, srclength <= 0, dst_capacity <= 0, a negative
    origin in the LAST row, a pipeline that is not admitted for the voxel type, the view rules in the last row: 1, *dstlength = 0, nothing
    written"""
    fn = getattr(sqy.lib(), "SQYAMD_Update_Boxes_%s_Device" % ("UI16" if dtype == np.uint16 else "UI8"))
    src = np.zeros(256, np.uint8)
    views = [np.full((2, 3, 4), 9 + k, dtype) for k in range(3)]
    dst = np.full(4096, 0x5A, np.uint8)
    O, S = (0, 0, 0) * 3, (2, 3, 4) * 3

    def call(pipeline=b"bitswap1->lz4", src_ok=True, srclen=256, count=3, origins=O, views_ok=True, null_at=None, shapes=S, strides=None, rank=3, dst_ok=True, cap=4096,
             len_ok=True, shift=0):
        n = ctypes.c_long(77)
        ptrs = (ctypes.c_void_p * 3)(*[None if k == null_at else v.ctypes.data + (shift if k == 2 else 0) for k, v in enumerate(views)])
        rc = fn(pipeline, src.ctypes.data if src_ok else None, srclen, count, _longs(origins), ptrs if views_ok else None, _longs(shapes), _longs(strides), ctypes.c_uint(rank),
                dst.ctypes.data if dst_ok else None, cap, ctypes.byref(n) if len_ok else None, 0, None)
        assert not len_ok or n.value == 0, n.value
        return rc
    dense = (12, 4, 1) * 2
    bad = [dict(pipeline=None), dict(src_ok=False), dict(origins=None), dict(views_ok=False), dict(null_at=1), dict(null_at=2), dict(shapes=None), dict(dst_ok=False),
           dict(len_ok=False), dict(rank=0), dict(rank=4), dict(count=0), dict(count=-3), dict(count=2 ** 31), dict(srclen=0), dict(srclen=-7), dict(cap=0), dict(cap=-1),
           dict(origins=O[:6] + (0, -1, 0)), dict(origins=O[:6] + (0, 0, -(2 ** 62))), dict(pipeline=b"no_such_stage->lz4"), dict(pipeline=b""),
           dict(shapes=S[:6] + (2, 0, 4)), dict(shapes=S[:6] + (2, 3, -4)), dict(strides=dense + (12, 4, 2)), dict(strides=dense + (12, 3, 1)), dict(strides=dense + (11, 4, 1)),
           dict(strides=dense + (12, 0, 1))]
    if dtype == np.uint16:
        bad.append(dict(shift=1))                                       # the last view off the voxel grid
    else:
        bad.append(dict(pipeline=b"quantiser->bitswap1->lz4"))          # a 16-bit pipeline
    for kw in bad:
        assert call(**kw) == 1, kw
    assert (dst == 0x5A).all() and all((v == 9 + k).all() for k, v in enumerate(views))


@pytest.mark.parametrize("dtype", [np.uint16, np.uint8])
def test_the_host_variants_check_their_arguments_first(sqy, dtype):
    """.. and views_bytes against the boxes' summed bytes, which needs no header (the blob here has none)"""
    fn = getattr(sqy.lib(), "SQYAMD_Update_Boxes_" + ("UI16" if dtype == np.uint16 else "UI8"))
    item = np.dtype(dtype).itemsize
    src = np.zeros(256, np.uint8)
    views = np.full(3 * 24, 7, dtype)
    dst = np.full(4096, 0x5A, np.uint8)
    O, S = (0, 0, 0) * 3, (2, 3, 4) * 3

    def call(pipeline=b"bitswap1->lz4", src_ok=True, srclen=256, count=3, origins=O, extents=S, rank=3, views_ok=True, nbytes=views.nbytes, dst_ok=True, cap=4096, len_ok=True):
        n = ctypes.c_long(77)
        rc = fn(pipeline, src.ctypes.data if src_ok else None, srclen, count, _longs(origins), _longs(extents), ctypes.c_uint(rank), views.ctypes.data if views_ok else None, nbytes,
                dst.ctypes.data if dst_ok else None, cap, ctypes.byref(n) if len_ok else None, 0)
        assert not len_ok or n.value == 0, n.value
        return rc
    for kw in (dict(pipeline=None), dict(src_ok=False), dict(origins=None), dict(extents=None), dict(views_ok=False), dict(dst_ok=False), dict(len_ok=False), dict(rank=0),
               dict(rank=4), dict(count=0), dict(count=-1), dict(srclen=0), dict(cap=0), dict(origins=O[:6] + (0, -1, 0)), dict(pipeline=b"no_such_stage->lz4"),
               dict(extents=S[:6] + (2, 0, 4)), dict(extents=S[:6] + (2 ** 40, 2 ** 40, 2 ** 40)), dict(nbytes=views.nbytes - 1), dict(nbytes=views.nbytes + 1),
               dict(nbytes=views.nbytes - item), dict(nbytes=-1), dict(nbytes=0)):
        assert call(**kw) == 1, kw
    assert call() == 1                                                  # (no header in the blob: refused behind the checks above, still without a device)
    assert (dst == 0x5A).all() and (views == 7).all()


# ---- the case table: every case is what its name says --------------------------------------------------------------------------------

def _voxels(shape, origin, extent):
    pad = (1,) * (3 - len(shape))
    sh, o, e = pad + tuple(shape), (0,) * (3 - len(shape)) + tuple(origin), pad + tuple(extent)
    z, y, x = np.ogrid[o[0]:o[0] + e[0], o[1]:o[1] + e[1], o[2]:o[2] + e[2]]
    return set(((z * sh[1] + y) * sh[2] + x).reshape(-1).tolist())


def _frames(shape, origin, extent):
    return set(range(origin[0], origin[0] + extent[0]))


@pytest.mark.parametrize("case", C.CASES, ids=[c.name for c in C.CASES])
def test_a_case_is_what_its_name_says(case):
    for dtype in (np.uint16,) if case.u16_only else (np.uint16, np.uint8):
        W = 8 * np.dtype(dtype).itemsize
        n = int(np.prod(case.shape))
        L = n // W * W
        vox = [_voxels(case.shape, o, e) for o, e in case.boxes]
        fr = [_frames(case.shape, o, e) for o, e in case.boxes]
        words = [set(v // W for v in s if v < L) for s in vox]
        assert all(vox), case.name
        disjoint = all(not (vox[i] & vox[j]) for i in range(len(vox)) for j in range(i))
        kind = case.kind
        if kind == "one":
            assert len(vox) == 1
        elif kind == "same_frames":
            assert len(vox) >= 3 and disjoint and all(f == fr[0] for f in fr)
        elif kind == "disjoint_ranges":
            order = sorted(range(len(fr)), key=lambda i: min(fr[i]))
            assert len(fr) >= 2 and all(min(fr[b]) - max(fr[a]) >= 2 for a, b in zip(order, order[1:]))      # an untouched frame between
        elif kind == "abutting":
            assert len(fr) == 2 and max(fr[0]) + 1 == min(fr[1])
        elif kind == "shared_word_x":
            assert len(vox) == 2 and disjoint and fr[0] == fr[1] and dtype_words_shared(words) and len({v // 128 for v in vox[0] | vox[1]}) == 1
        elif kind == "shared_word_frames":
            if dtype == np.uint16:                                      # (named for the 16-voxel word)
                assert len(vox) == 2 and not (fr[0] & fr[1]) and dtype_words_shared(words)
                if case.gap:
                    assert min(fr[1]) - max(fr[0]) >= 2                 # the word spans the frames between
        elif kind == "shared_tail":
            if dtype == np.uint16:                                      # (named for the 16-bit tail: both boxes lie in it, in no plane word)
                tails = [set(v for v in s if v >= L) for s in vox]
                assert n % W and len(vox) == 2 and disjoint and all(tails) and not any(words)
        elif kind == "overlap":
            assert len(vox) == 2 and vox[0] & vox[1] and vox[0] - vox[1] and vox[1] - vox[0]
        elif kind == "coincide":
            assert len(vox) == 2 and vox[0] == vox[1]
        elif kind == "whole_inside":
            assert len(vox) == 2 and len(vox[0]) == n and vox[1] < vox[0]
        elif kind == "unchanged":
            assert len(vox) >= 2
        else:
            raise AssertionError(kind)
        assert len(case.shape) == case.rank


def dtype_words_shared(words):
    return bool(words[0] & words[1])


def test_the_table_holds_every_kind_and_the_ranks():
    kinds = {c.kind for c in C.CASES}
    assert kinds == {"one", "same_frames", "disjoint_ranges", "abutting", "shared_word_x", "shared_word_frames", "shared_tail", "overlap", "coincide", "whole_inside", "unchanged"}
    assert {c.rank for c in C.CASES} == {1, 2, 3}
    assert any(c.kind == "shared_word_frames" and c.shape == (7, 33, 31) for c in C.CASES) and any(c.kind == "shared_word_frames" and c.shape == (600, 2, 3) for c in C.CASES)
    assert any(c.kind == "overlap" and c.reverse for c in C.CASES)


def test_the_overlap_orders_differ():
    """the two orders of the overlap case give different volumes, with the views the GPU test uses"""
    for case in (c for c in C.CASES if c.kind in ("overlap", "coincide")):
        for dtype in (np.uint16, np.uint8):
            full = np.zeros(case.shape, dtype)
            tiles = C.tiles(case, dtype, full)
            a = C.pasted(full, case.boxes, tiles)
            b = C.pasted(full, case.boxes[::-1], tiles[::-1])
            assert not np.array_equal(a, b), case.name
