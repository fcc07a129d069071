"""GPU: SQYAMD_Update_Boxes_* -- many boxes written into ONE large blob in one call (include/sqeazy_amd.h).

The expectation is never the code under test: the old blob is the single call's blob, the boxes are pasted IN BOX ORDER with numpy into
its decode (update_boxes_cases.pasted), and the new blob must be, byte for byte, the single call's blob of the pasted volume
(test_gpu_encode_batch._want, which holds that blob to the oracle).  Every destination lies between canaries; the views are
test_gpu_batch_update.Sources (dense, then pitched and 2 bytes off the 16-byte grid) and must be unchanged afterwards.  The case table is
tests/update_boxes_cases.py; tests/test_host_update_boxes.py holds every case to the property it is named for.  The subset path (every
stage of SQYAMD_Update_Box_* once for all boxes) and the whole path ("update_boxes_subset" = 0) must give the same bytes, and each shows
its launches in the profile -- so the fallback cannot stand in for a broken subset path."""
import ctypes
import hashlib
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import update_boxes_cases as C
from test_gpu_batch_update import Sources
from test_gpu_batch_window import _blob
from test_gpu_decode_box import SHAPES, SMALL_CHUNKS, _case_blob, _to_device
from test_gpu_decode_frames import _damaged, _lz4_frames, _profile_names
from test_gpu_decode_slabs import _profile_names as _profile
from test_gpu_encode_batch import CANARY, GAP, _want
from test_gpu_update_box import OTHERS, SPLICE

pytestmark = pytest.mark.gpu

BSL = "bitswap1->lz4"
PATCH = {BSL: "bitswap1_range_patches", "lz4": "boxes_window_paste"}
SUBSET_ONCE = ("lz4_frames_subset_decode", "lz4_chunks_table") + SPLICE
KINDS = [(BSL, np.uint16), (BSL, np.uint8), ("lz4", np.uint16), ("lz4", np.uint8)]
KIND_IDS = ["%s-%s" % (p, np.dtype(d).name) for p, d in KINDS]
BY_NAME = {c.name: c for c in C.CASES}


def _dev():
    import torch
    return torch.device("cuda", 0)


def test_the_table_uses_the_box_tests_shapes():
    known = {s for s, _ in SHAPES} | {(600, 2, 3)}
    assert SMALL_CHUNKS == C.SMALL_CHUNKS
    for c in C.CASES:
        assert c.rank < 3 or (c.shape in known and (c.shape == (600, 2, 3) or (c.shape, c.cfg) in SHAPES)), c.name


def _old(sqy, oracle, case, pipeline, dtype):
    """(old blob, its decode): the single call's blob of the case's volume"""
    if case.rank == 3:
        return _blob(sqy, oracle, pipeline + case.cfg, case.shape, dtype)
    vol = C.volume(case.shape, dtype)
    return _want(sqy, oracle, pipeline + case.cfg, vol, 0, _dev(), key=("update_boxes_old", case.shape, np.dtype(dtype).name)), vol


def _expect(sqy, oracle, name, full, boxes, tiles, nthreads=0):
    """the single call's blob for the volume with the boxes pasted in box order, held to the oracle"""
    v = C.pasted(full, boxes, tiles)
    return _want(sqy, oracle, name, v, nthreads, _dev(), key=("update_boxes", v.shape, v.dtype.name, hashlib.sha1(v.tobytes()).hexdigest()))


def _update(sqy, pipeline, d_blob, nbytes, origins, S, cap=None, nthreads=0, stream=None, shape=None, ptrs=None, count=None):
    """the call into cap bytes between canaries: (rc, dstlength, blob or None).  The canaries hold whatever rc is, the bytes behind the blob
    too, and every byte when rc is not 0"""
    import torch
    if cap is None:
        cap = sqy.max_compressed_length(pipeline, shape, S.dtype)
    buf = torch.full((2 * GAP + cap,), CANARY, dtype=torch.uint8, device=_dev())
    torch.cuda.synchronize()                                            # (the fill is torch's stream's: the caller's to complete)
    rc, n = sqy.update_boxes_device(pipeline, d_blob.data_ptr(), nbytes, origins, S.ptrs if ptrs is None else ptrs, S.extents, S.strides, S.dtype, buf.data_ptr() + GAP, cap,
                                    nthreads=nthreads, stream=stream, count=count)
    torch.cuda.synchronize()
    h = buf.cpu().numpy()
    if rc:
        assert (h == CANARY).all(), "rc %d and the destination was written" % rc
        return rc, n, None
    assert 0 < n <= cap and (h[:GAP] == CANARY).all() and (h[GAP + n:] == CANARY).all(), "written outside the blob"
    return rc, n, h[GAP:GAP + n].tobytes()


def _unchanged(S):
    assert np.array_equal(S.buf.cpu().numpy(), S.host), "a view was written"


def _both_paths(sqy, options, name, d_blob, nbytes, shape, origins, tiles, want, nthreads=0, layouts=((0, False), (2, True))):
    """the boxes through the subset path and the whole path, sources dense, then pitched and 2 bytes off the grid"""
    for shift, pitch in layouts:
        S = Sources(tiles[0].dtype, tiles, shift=shift, pitch=pitch, salt=5 + shift)
        for subset in (1, 0):
            options("update_boxes_subset", subset)
            rc, n, b = _update(sqy, name, d_blob, nbytes, origins, S, nthreads=nthreads, shape=shape)
            assert rc == 0 and b == want, (name, shape, origins, subset, shift, pitch, n, len(want))
        _unchanged(S)
    options("update_boxes_subset", 1)


@pytest.mark.parametrize("pipeline, dtype", KINDS, ids=KIND_IDS)
@pytest.mark.parametrize("case", C.CASES, ids=[c.name for c in C.CASES])
def test_bytes(sqy, oracle, options, case, pipeline, dtype):
    if case.u16_only and dtype != np.uint16:
        return                                                          # (the shape is in the table for its 16-voxel words)
    blob, full = _old(sqy, oracle, case, pipeline, dtype)
    tiles = C.tiles(case, dtype, full)
    origins = [o for o, _ in case.boxes]
    name = pipeline + case.cfg
    want = _expect(sqy, oracle, name, full, case.boxes, tiles)
    d_blob = _to_device(blob)
    if case.kind == "unchanged":
        assert want == blob
    if case.kind == "one":                                              # .. is SQYAMD_Update_Box_*, byte for byte
        S = Sources(dtype, tiles, shift=2, pitch=True)
        import torch
        cap = sqy.max_compressed_length(name, case.shape, dtype)
        out = torch.full((cap,), CANARY, dtype=torch.uint8, device=_dev())
        rc, n = sqy.update_box_device(name, d_blob.data_ptr(), len(blob), origins[0], S.ptrs[0], S.extents[0], S.strides[0], dtype, out.data_ptr(), cap)
        assert rc == 0 and out[:n].cpu().numpy().tobytes() == want
    if case.reverse:                                                    # each order its own: the other order's blob is another one
        other = BY_NAME["overlap"]
        assert want != _expect(sqy, oracle, name, full, other.boxes, C.tiles(other, dtype, full))
    _both_paths(sqy, options, name, d_blob, len(blob), case.shape, origins, tiles, want)


def _counted(sqy, fn):
    """{profile name: launches} of fn"""
    return {k: v[1] for k, v in _profile(sqy, fn).items()}


@pytest.mark.parametrize("pipeline", [BSL, "lz4"])
def test_launches(sqy, oracle, options, pipeline):
    """K = 5 on the subset path: every stage ONCE; the option at 0: the whole path's names and none of the subset path's"""
    case = BY_NAME["same-frames-5"]
    blob, full = _old(sqy, oracle, case, pipeline, np.uint16)
    tiles = C.tiles(case, np.uint16, full)
    origins = [o for o, _ in case.boxes]
    want = _expect(sqy, oracle, pipeline, full, case.boxes, tiles)
    d_blob = _to_device(blob)
    S = Sources(np.uint16, tiles, shift=2, pitch=True)
    out = {}
    names = _counted(sqy, lambda: out.update(r=_update(sqy, pipeline, d_blob, len(blob), origins, S, shape=case.shape)))
    assert out["r"][0] == 0 and out["r"][2] == want
    for k in SUBSET_ONCE + (PATCH[pipeline],):
        assert names.get(k) == 1, (k, names)
    assert not any(k in names for k in ("lz4_frames_decode", "bitswap1_range_patch", "box_window_paste", "batch_window_paste", "bitswap1_decode", "lz4_chunks")), names
    options("update_boxes_subset", 0)
    names = _counted(sqy, lambda: out.update(r=_update(sqy, pipeline, d_blob, len(blob), origins, S, shape=case.shape)))
    assert out["r"][0] == 0 and out["r"][2] == want
    assert "lz4_frames_decode" in names and names.get("batch_window_paste") == 1, names
    assert not any(k in names for k in SUBSET_ONCE + tuple(PATCH.values()) + ("bitswap1_range_patch", "box_window_paste")), names
    options("update_boxes_subset", 1)


def test_overlap_launches(sqy, oracle, options):
    """overlapping boxes: the plain form pastes in two launches, one per layer; the planes form patches in ONE (a thread owns its words)"""
    case = BY_NAME["overlap"]
    for pipeline, launches in ((BSL, 1), ("lz4", 2)):
        blob, full = _old(sqy, oracle, case, pipeline, np.uint16)
        tiles = C.tiles(case, np.uint16, full)
        S = Sources(np.uint16, tiles)
        out = {}
        names = _counted(sqy, lambda: out.update(r=_update(sqy, pipeline + case.cfg, _to_device(blob), len(blob), [o for o, _ in case.boxes], S, shape=case.shape)))
        assert out["r"][0] == 0 and out["r"][2] == _expect(sqy, oracle, pipeline + case.cfg, full, case.boxes, tiles)
        assert names.get(PATCH[pipeline]) == launches, names
        for k in SUBSET_ONCE:
            assert names.get(k) == 1, (k, names)
        options("update_boxes_subset", 0)
        names = _counted(sqy, lambda: out.update(r=_update(sqy, pipeline + case.cfg, _to_device(blob), len(blob), [o for o, _ in case.boxes], S, shape=case.shape)))
        assert out["r"][0] == 0 and names.get("batch_window_paste") == 2, names
        options("update_boxes_subset", 1)


@pytest.mark.parametrize("pipeline, dtype", KINDS, ids=KIND_IDS)
def test_a_chain_of_update_box_calls_gives_the_same_bytes(sqy, oracle, pipeline, dtype):
    import torch
    for case in (BY_NAME["overlap"], BY_NAME["same-frames-5"], BY_NAME["shared-word-frames"]):
        blob, full = _old(sqy, oracle, case, pipeline, dtype)
        tiles = C.tiles(case, dtype, full)
        name = pipeline + case.cfg
        S = Sources(dtype, tiles, shift=2, pitch=True)
        cap = sqy.max_compressed_length(name, case.shape, dtype)
        ping = [torch.full((cap,), CANARY, dtype=torch.uint8, device=_dev()) for _ in range(2)]
        src, n = _to_device(blob), len(blob)
        for i, (o, _) in enumerate(case.boxes):
            rc, n = sqy.update_box_device(name, src.data_ptr(), n, o, S.ptrs[i], S.extents[i], S.strides[i], dtype, ping[i & 1].data_ptr(), cap)
            assert rc == 0
            src = ping[i & 1]
        chain = src[:n].cpu().numpy().tobytes()
        rc, m, b = _update(sqy, name, _to_device(blob), len(blob), [o for o, _ in case.boxes], S, shape=case.shape)
        assert rc == 0 and b == chain and chain == _expect(sqy, oracle, name, full, case.boxes, tiles), (case.name, m, n)


REST = [o for o in OTHERS if "rmestbkrd" not in o[0]]


@pytest.mark.parametrize("old, new, nthreads, shape", REST, ids=["%s|%s%s" % (o, n, "-serial" if t else "") for o, n, t, _ in REST])
def test_blobs_the_subset_path_does_not_take(sqy, oracle, options, old, new, nthreads, shape):
    """the whole path: the new blob equals the single call's blob of the pasted decode; no splice launch shows -- but for lz4(accel=2), which
    liblz4 compresses with acceleration 1 like accel=1: sqy::update_box_path takes it, the bytes decide"""
    made = _case_blob(sqy, oracle, old, shape, np.uint16, nthreads)
    assert made is not None
    blob, full = made
    boxes = [((3, 5, 16), (shape[0] - 5, shape[1] - 28, shape[2] - 40)), ((0, 0, 0), (4, 9, 17)), ((shape[0] - 1, 1, 1), (1, 3, 3))]
    case = C._case("rest", "overlap", shape, "", boxes)
    tiles = C.tiles(case, np.uint16, full)
    want = _expect(sqy, oracle, new, full, boxes, tiles, nthreads)
    d_blob = _to_device(blob)
    for subset in (1, 0):
        options("update_boxes_subset", subset)
        S = Sources(np.uint16, tiles, shift=2, pitch=True)
        out = {}
        names = _profile_names(sqy, lambda: out.update(r=_update(sqy, new, d_blob, len(blob), [o for o, _ in boxes], S, nthreads=nthreads, shape=shape)))
        assert out["r"][0] == 0 and out["r"][2] == want, (old, new, subset)
        if "accel=2" not in new:
            assert not any(k in names for k in SPLICE), names
        _unchanged(S)
    options("update_boxes_subset", 1)


@pytest.mark.parametrize("subset", [1, 0])
def test_capacity(sqy, oracle, options, subset):
    """a capacity equal to the blob's length succeeds; one byte less: 1, *dstlength = the bytes needed, every canary intact"""
    options("update_boxes_subset", subset)
    case = BY_NAME["overlap"]
    name = BSL + case.cfg
    blob, full = _old(sqy, oracle, case, BSL, np.uint16)
    tiles = C.tiles(case, np.uint16, full)
    origins = [o for o, _ in case.boxes]
    want = _expect(sqy, oracle, name, full, case.boxes, tiles)
    S = Sources(np.uint16, tiles)
    d_blob = _to_device(blob)
    rc, n, b = _update(sqy, name, d_blob, len(blob), origins, S, cap=len(want))
    assert rc == 0 and b == want
    rc, n, b = _update(sqy, name, d_blob, len(blob), origins, S, cap=len(want) - 1)
    assert rc == 1 and n == len(want) and b is None
    options("update_boxes_subset", 1)


def test_refusals(sqy, oracle):
    """each admission rule, a bad box in the LAST row and a NULL in the middle of d_views among them: (1, 0), the destination all canaries"""
    import torch
    shape = (3, 5, 7)
    blob, full = _blob(sqy, oracle, BSL, shape, np.uint16)
    u8 = _blob(sqy, oracle, BSL, shape, np.uint8)[0]
    d_blob, d_u8 = _to_device(blob), _to_device(u8)
    boxes = [((0, 0, 0), (1, 2, 3)), ((1, 1, 1), (2, 3, 4)), ((2, 4, 0), (1, 1, 7))]
    case = C._case("refusals", "disjoint_ranges", shape, "", boxes)
    tiles = C.tiles(case, np.uint16, full)
    S = Sources(np.uint16, tiles, pitch=True)
    cap = sqy.max_compressed_length(BSL, shape, np.uint16)
    buf = torch.full((cap,), CANARY, dtype=torch.uint8, device=_dev())
    O, E, ST = [o for o, _ in boxes], [e for _, e in boxes], list(S.strides)
    good = dict(pipeline=BSL, src=d_blob.data_ptr(), n=len(blob), origins=O, views=S.ptrs, shapes=E, strides=ST, dtype=np.uint16, dst=buf.data_ptr(), cap=cap, count=None)

    def call(**kw):
        a = dict(good, **kw)
        out = sqy.update_boxes_device(a["pipeline"], a["src"], a["n"], a["origins"], a["views"], a["shapes"], a["strides"], a["dtype"], a["dst"], a["cap"], count=a["count"])
        torch.cuda.synchronize()
        return out

    def refused(**kw):
        assert call(**kw) == (1, 0), kw
        assert (buf.cpu().numpy() == CANARY).all(), kw
    last = lambda rows, row: rows[:2] + [row]
    LONG_MAX = 2 ** 63 - 1
    for kw in (dict(pipeline=None), dict(src=None), dict(origins=None), dict(views=None), dict(shapes=None, strides=None), dict(dst=None), dict(n=0), dict(n=-1), dict(cap=0),
               dict(cap=-5), dict(count=0), dict(count=-1), dict(views=[S.ptrs[0], None, S.ptrs[2]]), dict(views=last(S.ptrs, None)), dict(views=last(S.ptrs, S.ptrs[2] + 1)),
               dict(origins=last(O, (2, -1, 0))), dict(origins=last(O, (3, 4, 0))), dict(origins=last(O, (2, 4, 1))), dict(origins=last(O, (LONG_MAX, 0, 0))),
               dict(shapes=last(E, (1, 0, 7)), strides=None), dict(shapes=last(E, (2, 1, 7)), strides=None), dict(strides=last(ST, (7, 7, 2))), dict(strides=last(ST, (7, 6, 1))),
               dict(pipeline="nonsense->lz4"), dict(pipeline="quantiser->bitswap1->lz4", dtype=np.uint8, src=d_u8.data_ptr(), n=len(u8)),
               dict(src=d_u8.data_ptr(), n=len(u8)), dict(dtype=np.uint8), dict(origins=[o[1:] for o in O], shapes=[e[1:] for e in E], strides=[s[1:] for s in ST])):
        refused(**kw)
    rc, n = call()
    assert rc == 0 and buf.cpu().numpy()[:n].tobytes() == _expect(sqy, oracle, BSL, full, boxes, tiles)
    _unchanged(S)


@pytest.mark.parametrize("pipeline", ["lz4", BSL])
def test_damage(sqy, oracle, pipeline):
    """a damaged frame that only box 2 of 3 needs: SQY_Decode's code, the destination all canaries; one that no box needs: rc 0, the frame
    is carried over -- every frame but that one is the expectation's, and the full decode of the new blob reports it"""
    shape = (16, 64, 64)
    name = pipeline + SMALL_CHUNKS
    vol = (np.arange(np.prod(shape)) % 300).astype(np.uint16).reshape(shape)      # every 4 KiB chunk compressible
    old = _want(sqy, oracle, name, vol, 0, _dev())
    frames = _lz4_frames(old, sqy)
    bad = _damaged(old, frames[-1])                                     # (the last LZ4 frame: voxels, or plane words, of frames 8 .. 15 only)
    rc_full, _ = sqy.decode(bad)
    assert rc_full not in (0, 1)
    d_bad = _to_device(bad)
    extents = [(1, 50, 40), (1, 30, 64), (2, 5, 5)]
    case = C._case("damage", "disjoint_ranges", shape, SMALL_CHUNKS, [((0, 5, 7), extents[0]), ((15, 1, 0), extents[1]), ((3, 0, 0), extents[2])])
    tiles = C.tiles(case, np.uint16, vol)
    S = Sources(np.uint16, tiles, shift=2, pitch=True)
    rc, n, b = _update(sqy, name, d_bad, len(bad), [(0, 5, 7), (15, 1, 0), (3, 0, 0)], S, shape=shape)
    assert rc == rc_full and b is None
    boxes = [((0, 5, 7), extents[0]), ((5, 1, 0), extents[1]), ((3, 0, 0), extents[2])]
    rc, n, b = _update(sqy, name, d_bad, len(bad), [o for o, _ in boxes], S, shape=shape)
    assert rc == 0
    want = _expect(sqy, oracle, name, vol, boxes, tiles)
    f_new, f_want = _lz4_frames(b, sqy), _lz4_frames(want, sqy)
    assert len(f_new) == len(f_want) == len(frames) and len(b) == len(want)
    for k, (g, w) in enumerate(zip(f_new, f_want)):
        same = b[g[0]:g[1] + g[2] + 4] == want[w[0]:w[1] + w[2] + 4]
        assert same == (k != len(frames) - 1), k
    assert b[f_new[-1][1]:f_new[-1][1] + f_new[-1][2]] == b"\xff" * f_new[-1][2]
    assert sqy.decode(b)[0] == rc_full
    _unchanged(S)


def test_host_variants(sqy, oracle, options):
    """update_boxes (host pointers, the views dense and back to back): the bytes of a three-box call on both paths; views_bytes off by one: 1"""
    for pipeline, dtype in ((BSL, np.uint16), ("lz4", np.uint8)):
        case = BY_NAME["same-frames-small"]
        blob, full = _old(sqy, oracle, case, pipeline, dtype)
        tiles = C.tiles(case, dtype, full)
        origins = [o for o, _ in case.boxes]
        name = pipeline + case.cfg
        want = _expect(sqy, oracle, name, full, case.boxes, tiles)
        for subset in (1, 0):
            options("update_boxes_subset", subset)
            rc, b = sqy.update_boxes(name, blob, origins, tiles)
            assert rc == 0 and b == want, (pipeline, subset)
        options("update_boxes_subset", 1)
        fn = getattr(sqy.lib(), "SQYAMD_Update_Boxes_" + ("UI16" if dtype == np.uint16 else "UI8"))
        dense = np.concatenate([t.reshape(-1) for t in tiles])
        src = np.frombuffer(blob, np.uint8)
        dst = np.full(sqy.max_compressed_length(name, case.shape, dtype), CANARY, np.uint8)
        longs = lambda rows: (ctypes.c_long * (3 * len(rows)))(*[v for r in rows for v in r])
        for nbytes, rc_want in ((dense.nbytes - 1, 1), (dense.nbytes + 1, 1), (dense.nbytes, 0)):
            n = ctypes.c_long(77)
            rc = fn(name.encode(), src.ctypes.data, len(blob), 3, longs(origins), longs([t.shape for t in tiles]), ctypes.c_uint(3), dense.ctypes.data, nbytes, dst.ctypes.data,
                    dst.nbytes, ctypes.byref(n), 0)
            assert rc == rc_want, nbytes
            if rc:
                assert n.value == 0 and (dst == CANARY).all()
            else:
                assert dst[:n.value].tobytes() == want and (dst[n.value:] == CANARY).all()


def test_two_host_threads_and_a_callers_stream(sqy, oracle):
    import torch
    case = BY_NAME["same-frames-5"]
    made = [_old(sqy, oracle, case, p, np.uint16) for p in (BSL, "lz4")]
    origins = [o for o, _ in case.boxes]
    tiles = [C.tiles(case, np.uint16, m[1]) for m in made]
    wants = [_expect(sqy, oracle, p, m[1], case.boxes, t) for p, m, t in zip((BSL, "lz4"), made, tiles)]
    d_blobs = [_to_device(m[0]) for m in made]
    S = [Sources(np.uint16, t, shift=2, pitch=True) for t in tiles]
    torch.cuda.synchronize()

    def one(k):
        s = torch.cuda.Stream(device=_dev())
        ok = True
        for _ in range(3):
            rc, n, b = _update(sqy, (BSL, "lz4")[k], d_blobs[k], len(made[k][0]), origins, S[k], shape=case.shape, stream=s.cuda_stream)
            ok = ok and rc == 0 and b == wants[k]
        return ok
    with ThreadPoolExecutor(2) as ex:
        assert all(ex.map(one, range(2)))
    # a call on a non-default stream behind the kernel that made the views (dense, back to back in one buffer)
    s = torch.cuda.Stream(device=_dev())
    dense = np.concatenate([t.reshape(-1) for t in tiles[0]])
    at = np.cumsum([0] + [t.size for t in tiles[0]]) * 2
    with torch.cuda.stream(s):
        views = torch.zeros(dense.size, dtype=torch.int16, device=_dev())
        src = torch.from_numpy(dense.view(np.int16).copy()).pin_memory()
        cap = sqy.max_compressed_length(BSL, case.shape, np.uint16)
        out = torch.full((cap,), CANARY, dtype=torch.uint8, device=_dev())
        views.copy_(src, non_blocking=True)
        views.add_(0)                                                   # (a kernel on the stream writes the views)
        rc, n = sqy.update_boxes_device(BSL, d_blobs[0].data_ptr(), len(made[0][0]), origins, [views.data_ptr() + int(a) for a in at[:-1]], [t.shape for t in tiles[0]], None,
                                        np.uint16, out.data_ptr(), cap, stream=s.cuda_stream)
    assert rc == 0 and out[:n].cpu().numpy().tobytes() == wants[0]
