"""GPU: SQYAMD_Decode_Boxes_* -- many boxes of ONE blob decoded with one call, each into a view of its shape (include/sqeazy_amd.h,
DESIGN.md 2).

Every box must equal the same box of what SQY_Decode gives for the blob (test_gpu_decode_box's `full`) at exactly its view's voxel places: ALL
boxes of a case go in ONE call, their views lie in one buffer of a position-dependent pattern that is compared, whole, with an image built on
the CPU.  The joint path (the boxes' LZ4 frames united and decoded once, ONE output launch), the box-by-box path ("decode_boxes_joint" = 0)
and the joint path off the subset ("decode_box_subset" = 0: the blob decoded whole once, one window copy) give the same bytes, and each
shows its launches in the profile -- so none can stand in for another."""
import ctypes
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from test_gpu_batch_window import Targets, _blob, _cut, _same
from test_gpu_decode_box import FALLBACK, LONG_MAX, SMALL_CHUNKS, SUBSET, _boxes, _case_blob, _launch_case, _made, _to_device
from test_gpu_decode_frames import _damaged, _lz4_frames, _profile_names

pytestmark = pytest.mark.gpu

MODES = ((1, 1), (0, 1), (1, 0))                                        # (decode_boxes_joint, decode_box_subset)
FINAL = {"bitswap1->lz4": "bitswap1_decode_boxes", "rmestbkrd->bitswap1->lz4": "bitswap1_decode_boxes", "quantiser->bitswap1->lz4": "bitswap1_quantiser_decode_boxes",
         "lz4": "boxes_window_copy", "frame_shuffle->lz4": "boxes_window_copy"}
NEW_NAMES = set(FINAL.values())
IDS = ["%s-%s" % (p, np.dtype(d).name) for p, d in SUBSET]


def _dev():
    import torch
    return torch.device("cuda", 0)


def _call(sqy, d_blob, nbytes, boxes, T, stream=None):
    return sqy.decode_boxes_device(d_blob.data_ptr(), nbytes, [o for o, _ in boxes], T.ptrs, [e for _, e in boxes], T.strides, T.dtype, stream=stream)


def _three_ways(sqy, options, d_blob, nbytes, full, boxes, dtype, shift, pitch):
    """the boxes in ONE call through every mode: each image is the CPU's, so the three are equal"""
    tiles = [_cut(full, o, e) for o, e in boxes]
    images = []
    for joint, subset in MODES:
        options("decode_boxes_joint", joint)
        options("decode_box_subset", subset)
        T = Targets(dtype, [e for _, e in boxes], shift=shift, pitch=pitch, salt=7 * shift + pitch)
        assert _call(sqy, d_blob, nbytes, boxes, T) == 0, (joint, subset)
        got = T.read()
        _same(got, T.expect(tiles)[0])
        images.append(got)
    options("decode_boxes_joint", 1)
    options("decode_box_subset", 1)
    assert np.array_equal(images[0], images[1]) and np.array_equal(images[0], images[2])


def _voxels(sqy, oracle, options, pipeline, dtype, nthreads=0):
    item = np.dtype(dtype).itemsize
    made = _made(sqy, oracle, pipeline, dtype, nthreads)
    assert made
    for shape, d_blob, nbytes, full in made:
        boxes = _boxes(shape, item)
        assert any(tuple(e) == tuple(shape) for _, e in boxes) and len(boxes) > shape[0]     # the whole blob, a box of every frame alone
        for shift in (0, item):
            for pitch in (False, True):
                _three_ways(sqy, options, d_blob, nbytes, full, boxes, dtype, shift, pitch)


@pytest.mark.parametrize("pipeline, dtype", SUBSET, ids=IDS)
def test_voxels(sqy, oracle, options, pipeline, dtype):
    """all boxes of every shape in one call, with the views' bases on and one voxel behind the 16-byte grid, dense and pitched, through the
    three modes: the whole target buffer byte for byte"""
    _voxels(sqy, oracle, options, pipeline, dtype)


@pytest.mark.parametrize("pipeline, dtype, nthreads", FALLBACK, ids=["%s%s" % (p, "-serial" if t else "") for p, _, t in FALLBACK])
def test_voxels_of_blobs_the_subset_path_does_not_take(sqy, oracle, options, pipeline, dtype, nthreads):
    _voxels(sqy, oracle, options, pipeline, dtype, nthreads)


@pytest.mark.parametrize("pipeline, dtype", SUBSET, ids=IDS)
def test_two_boxes_with_a_gap_of_unneeded_frames_between_them(sqy, oracle, options, pipeline, dtype):
    """frames {0} and {Z - 1}: the union's compaction has other frames' places missing between the two boxes' words; and the same two with
    a box that reaches over both and one nested in it"""
    item = np.dtype(dtype).itemsize
    seen = 0
    for shape, cfg in (((23, 131, 151), ""), ((16, 64, 64), SMALL_CHUNKS)):
        b = _case_blob(sqy, oracle, pipeline + cfg, shape, dtype)
        if b is None:                                                   # (a geometry the stage refuses at encode)
            continue
        seen += 1
        blob, full = b
        d_blob = _to_device(blob)
        Z, Y, X = shape
        ends = [((0, 1, 2), (1, Y - 2, X - 3)), ((Z - 1, 0, 0), (1, Y, X))]
        for boxes in (ends, ends[::-1], ends + [((0, 3, 1), (Z, 5, X - 1)), ((Z // 2, 0, 0), (2, Y, 9))]):
            for shift, pitch in ((0, False), (item, True)):
                _three_ways(sqy, options, d_blob, len(blob), full, boxes, dtype, shift, pitch)
    assert seen >= 1


@pytest.mark.parametrize("pipeline, dtype", SUBSET, ids=IDS)
def test_one_box_is_decode_box(sqy, oracle, pipeline, dtype):
    """count = 1 writes what SQYAMD_Decode_Box_*_Device writes: the two buffers, whole"""
    item = np.dtype(dtype).itemsize
    shape, d_blob, nbytes, full = _made(sqy, oracle, pipeline, dtype)[0]
    for o, e in _boxes(shape, item):
        images = []
        for many in (True, False):
            T = Targets(dtype, [e], shift=item, pitch=True, salt=3)
            if many:
                assert _call(sqy, d_blob, nbytes, [(o, e)], T) == 0
            else:
                assert sqy.decode_box_device(d_blob.data_ptr(), nbytes, o, T.ptrs[0], e, T.strides[0], dtype) == 0
            images.append(T.read())
        _same(images[0], T.expect([_cut(full, o, e)])[0])
        assert np.array_equal(images[0], images[1])


@pytest.mark.parametrize("pipeline, dtype", SUBSET, ids=IDS)
def test_launches(sqy, oracle, options, pipeline, dtype):
    """the joint subset path: ONE pruned LZ4 launch and ONE of the new final launches for K boxes, none of the single-box driver's; the
    subset off: the whole blob once and one boxes_window_copy; SQYAMD_Decode_Box_* and SQYAMD_Decode_Frames_* launch what they launched"""
    shape, blob, full = _launch_case(sqy, oracle, pipeline, dtype)
    d_blob = _to_device(blob)
    Z = shape[0]
    boxes = [((Z // 2, 1, 1), (1, shape[1] - 2, shape[2] - 2)), ((0, 0, 3), (Z, shape[1], 5)), ((0, 2, 0), (1, 7, shape[2])), ((Z - 1, 0, 0), (1, shape[1], shape[2]))]
    tiles = [_cut(full, o, e) for o, e in boxes]

    def single():
        T = Targets(dtype, [boxes[0][1]], pitch=True)
        assert sqy.decode_box_device(d_blob.data_ptr(), len(blob), boxes[0][0], T.ptrs[0], boxes[0][1], T.strides[0], dtype) == 0
        T.read()
    frames_before = _profile_names(sqy, lambda: sqy.decode_frames(blob, Z // 2, 1))
    box_before = _profile_names(sqy, single)
    for k in (3, 4):
        T = Targets(dtype, [e for _, e in boxes[:k]], shift=np.dtype(dtype).itemsize, pitch=True)
        names = _profile_names(sqy, lambda: (_call(sqy, d_blob, len(blob), boxes[:k], T), T.read()))
        _same(T.read(), T.expect(tiles[:k])[0])
        assert "lz4_frames_subset_decode" in names and FINAL[pipeline] in names, names
        assert sum(n in names for n in NEW_NAMES) == 1, names
        assert not any(n in names for n in ("bitswap1_decode_box", "bitswap1_quantiser_decode_box", "box_window_copy", "lz4_frames_decode", "batch_window_copy",
                                            "frames_range_copy", "frame_scatter")), names
    options("decode_box_subset", 0)
    T = Targets(dtype, [e for _, e in boxes], pitch=True)
    names = _profile_names(sqy, lambda: (_call(sqy, d_blob, len(blob), boxes, T), T.read()))
    _same(T.read(), T.expect(tiles)[0])
    assert "lz4_frames_decode" in names and "boxes_window_copy" in names, names
    assert not any(n in names for n in ("lz4_frames_subset_decode", "bitswap1_decode_boxes", "bitswap1_quantiser_decode_boxes", "box_window_copy")), names
    options("decode_box_subset", 1)
    options("decode_boxes_joint", 0)                                     # box by box: the single-box driver's launches, none of the new ones
    T = Targets(dtype, [e for _, e in boxes], pitch=True)
    names = _profile_names(sqy, lambda: (_call(sqy, d_blob, len(blob), boxes, T), T.read()))
    _same(T.read(), T.expect(tiles)[0])
    assert names == box_before, (names, box_before)
    options("decode_boxes_joint", 1)
    frames_after = _profile_names(sqy, lambda: sqy.decode_frames(blob, Z // 2, 1))
    box_after = _profile_names(sqy, single)
    assert frames_before == frames_after and box_before == box_after, (frames_before, frames_after, box_before, box_after)
    assert "lz4_frames_subset_decode" in frames_before and "lz4_frames_subset_decode" in box_before
    assert not any("boxes" in n for n in frames_before | box_before), (frames_before, box_before)


@pytest.mark.parametrize("pipeline", ["lz4", "bitswap1->lz4"])
def test_damaged_frame_that_no_box_needs_goes_unnoticed(sqy, options, pipeline):
    """pruning is real: the last compressed LZ4 frame damaged -- boxes in frames 0 and 3 do not need it (of every bit plane two chunks: their
    words lie in the first), a box in frame 15 among them does and the call gives the full decode's code; nothing outside the views is
    written either way"""
    shape = (16, 64, 64)
    vol = (np.arange(np.prod(shape)) % 300).astype(np.uint16).reshape(shape)      # every 4 KiB chunk compressible
    rc, blob = sqy.encode(pipeline + SMALL_CHUNKS, vol)
    assert rc == 0
    frames = _lz4_frames(blob, sqy)
    assert len(frames) == vol.nbytes // 4096
    bad = _damaged(blob, frames[-1])
    rc_full, _ = sqy.decode(bad)
    assert rc_full not in (0, 1)
    d_bad = _to_device(bad)
    boxes = [((0, 5, 7), (1, 50, 40)), ((3, 0, 0), (1, 64, 64)), ((0, 1, 1), (1, 3, 60))]
    tiles = [_cut(vol, o, e) for o, e in boxes]
    T = Targets(np.uint16, [e for _, e in boxes], shift=2, pitch=True)
    names = _profile_names(sqy, lambda: (_call(sqy, d_bad, len(bad), boxes, T), T.read()))
    assert "lz4_frames_subset_decode" in names and "lz4_frames_decode" not in names, names
    T = Targets(np.uint16, [e for _, e in boxes], shift=2, pitch=True)
    assert _call(sqy, d_bad, len(bad), boxes, T) == 0
    _same(T.read(), T.expect(tiles)[0])
    rc, got = sqy.decode_boxes(bad, [o for o, _ in boxes], [e for _, e in boxes])
    assert rc == 0 and all(np.array_equal(g, t) for g, t in zip(got, tiles))
    more = boxes[:2] + [((15, 2, 2), (1, 9, 9))] + boxes[2:]
    for joint in (1, 0):
        options("decode_boxes_joint", joint)
        T = Targets(np.uint16, [e for _, e in more], pitch=True)
        assert _call(sqy, d_bad, len(bad), more, T) == rc_full
        want, mask = T.expect([None] * len(more), skip=range(len(more)))
        _same(T.read(), want, mask)                                     # the views may hold anything, the bytes around and between them are intact
        assert sqy.decode_boxes(bad, [o for o, _ in more], [e for _, e in more]) == (rc_full, None)


def test_refusals(sqy, oracle):
    """test_gpu_decode_box.test_refusals' table applied to ONE box of three in turn; 1 and all three views' canaries intact"""
    shape = (3, 5, 7)
    blob, full = _blob(sqy, oracle, "bitswap1->lz4", shape, np.uint16)
    u8 = _blob(sqy, oracle, "bitswap1->lz4", shape, np.uint8)[0]
    d_blob, d_u8 = _to_device(blob), _to_device(u8)
    extents = [(2, 3, 4), (1, 5, 7), (2, 3, 4)]
    origins = [(1, 1, 1), (2, 0, 0), (0, 2, 3)]
    T = Targets(np.uint16, extents, pitch=True)
    assert T.strides[0] == (26, 7, 1)
    dense = lambda e: (e[1] * e[2], e[2], 1)

    def call(k=None, src=d_blob.data_ptr(), n=len(blob), dtype=np.uint16, count=None, origins_=origins, **box):
        """box k with the fields of `box` in place of its own"""
        o, p, e, s = [list(origins_) if origins_ is not None else None, list(T.ptrs), list(extents), list(T.strides)]
        if k is not None:
            if "origin" in box: o[k] = box["origin"]
            if "dst" in box: p[k] = box["dst"]
            if "shape" in box: e[k] = box["shape"]
            if "strides" in box: s[k] = box["strides"]
        return sqy.decode_boxes_device(src, n, o, p, e, s, dtype, count=count)

    def refused(**kw):
        for k in range(3):
            assert call(k, **kw) == 1, (k, kw)
            _same(T.read(), T.host)
    refused(origin=(0, -1, 0))                                          # a negative origin
    refused(shape=(2, 0, 4))                                            # an extent of 0
    for d in range(3):                                                  # origin + extent one voxel beyond the shape, each dimension in turn
        e = [2, 4, 6]
        e[d] += 1
        refused(origin=(1, 1, 1), shape=tuple(e), strides=dense(e))
        o = [0, 0, 0]
        o[d] = 1
        refused(origin=tuple(o), shape=shape, strides=dense(shape))
        o = [0, 0, 0]
        o[d] = LONG_MAX
        refused(origin=tuple(o), shape=(1, 1, 1))                       # no wrap to a small sum
    refused(shape=(2, 3, 4), strides=(40, 10, 2))                       # an innermost stride of 2
    refused(shape=(2, 3, 4), strides=(26, 3, 1))                        # a row stride smaller than the extent below it
    refused(shape=(2, 3, 4), strides=(20, 7, 1))                        # a frame stride smaller than the rows below it
    refused(dst=T.ptrs[0] + 1)                                          # a destination off the voxel grid
    refused(dst=None)                                                   # a NULL entry in d_dsts
    # what holds for the whole call: a rank other than the header's, a blob or an entry point of the other voxel type, NULL tables, no boxes
    assert sqy.decode_boxes_device(d_blob.data_ptr(), len(blob), [(1, 1)] * 3, T.ptrs, [(3, 4)] * 3, [(7, 1)] * 3, np.uint16) == 1
    assert sqy.decode_boxes_device(d_blob.data_ptr(), len(blob), [(1,)] * 3, T.ptrs, [(4,)] * 3, [(1,)] * 3, np.uint16) == 1
    assert call(src=d_u8.data_ptr(), n=len(u8)) == 1
    assert call(dtype=np.uint8) == 1
    assert call(src=None) == 1
    assert call(n=0) == 1
    assert call(origins_=None) == 1
    assert call(count=0) == 1 and call(count=-1) == 1 and call(count=-(2 ** 40)) == 1
    assert sqy.decode_boxes_device(d_blob.data_ptr(), len(blob), origins, None, extents, T.strides, np.uint16) == 1
    assert sqy.decode_boxes_device(d_blob.data_ptr(), len(blob), origins, T.ptrs, None, None, np.uint16, count=3) == 1
    _same(T.read(), T.host)
    # the good call: the table above refuses for its reasons
    assert call() == 0
    tiles = [_cut(full, o, e) for o, e in zip(origins, extents)]
    _same(T.read(), T.expect(tiles)[0])
    # the host variant: a capacity one byte short of the sum, the other type, a box outside, another rank
    L = sqy.lib()
    src = np.frombuffer(blob, np.uint8)
    total = sum(int(np.prod(e)) for e in extents) * 2
    host = np.full(total, 0x5A, np.uint8)
    rows = lambda v: (ctypes.c_long * sum(len(r) for r in v))(*[x for r in v for x in r])
    assert L.SQYAMD_Decode_Boxes_UI16(src.ctypes.data, len(blob), 3, rows(origins), rows(extents), 3, host.ctypes.data, total - 1) == 1
    assert L.SQYAMD_Decode_Boxes_UI8(src.ctypes.data, len(blob), 3, rows(origins), rows(extents), 3, host.ctypes.data, total) == 1
    assert L.SQYAMD_Decode_Boxes_UI16(src.ctypes.data, len(blob), 3, rows(origins), rows(extents[:2] + [(2, 3, 5)]), 3, host.ctypes.data, total) == 1
    assert L.SQYAMD_Decode_Boxes_UI16(src.ctypes.data, len(blob), 3, rows([(1, 1)] * 3), rows([(2, 3)] * 3), 2, host.ctypes.data, total) == 1
    assert L.SQYAMD_Decode_Boxes_UI16(src.ctypes.data, len(blob), 0, rows(origins), rows(extents), 3, host.ctypes.data, total) == 1
    assert (host == 0x5A).all()
    assert L.SQYAMD_Decode_Boxes_UI16(src.ctypes.data, len(blob), 3, rows(origins), rows(extents), 3, host.ctypes.data, total) == 0
    assert np.array_equal(host.view(np.uint16), np.concatenate([t.reshape(-1) for t in tiles]))       # dense, back to back in box order


def test_host_variant_and_lower_ranks(sqy, oracle, options):
    """decode_boxes (host pointers, the boxes dense and back to back) equals the device variant's voxels; blobs of rank 1 and 2: the frames
    are the first dimension"""
    for pipeline, dtype in (("bitswap1->lz4", np.uint16), ("lz4", np.uint8), ("quantiser->bitswap1->lz4", np.uint16), ("diff3x3x1->bitswap1->lz4", np.uint16)):
        blob, full = _blob(sqy, oracle, pipeline + (SMALL_CHUNKS if "diff" not in pipeline else ""), (7, 33, 31), dtype)
        boxes = _boxes((7, 33, 31), np.dtype(dtype).itemsize)
        for joint in (1, 0):
            options("decode_boxes_joint", joint)
            rc, got = sqy.decode_boxes(blob, [o for o, _ in boxes], [e for _, e in boxes])
            assert rc == 0 and len(got) == len(boxes)
            for g, (o, e) in zip(got, boxes):
                assert g.dtype == np.dtype(dtype) and np.array_equal(g, _cut(full, o, e)), (pipeline, o, e)
    options("decode_boxes_joint", 1)
    from sqeazy_amd import synth
    cases = (((40, 300), [((3, 17), (30, 200)), ((39, 0), (1, 300)), ((0, 299), (40, 1))]), ((9000,), [((4100,), (4000,)), ((0,), (9000,)), ((8999,), (1,))]))
    for shape, boxes in cases:
        vol = synth.stack((1, 1, int(np.prod(shape))), np.uint16, seed=731).reshape(shape)
        for pipeline in ("bitswap1->lz4" + SMALL_CHUNKS, "lz4" + SMALL_CHUNKS):
            rc, blob = sqy.encode(pipeline, vol)
            assert rc == 0
            d_blob = _to_device(blob)
            for pitch in (False, True):
                T = Targets(np.uint16, [e for _, e in boxes], shift=2, pitch=pitch)
                assert _call(sqy, d_blob, len(blob), boxes, T) == 0
                _same(T.read(), T.expect([_cut(vol, o, e) for o, e in boxes])[0])


def test_work_queued_on_the_callers_stream_is_respected(sqy):
    """the blob is written by a copy queued on the caller's stream just before the call, and the destinations are filled the same way"""
    import torch
    from sqeazy_amd import synth
    dev = _dev()
    vol = synth.stack((16, 128, 160), np.uint16)
    rc, blob = sqy.encode("bitswap1->lz4", vol, nthreads=2)
    assert rc == 0
    host_blob = torch.from_numpy(np.frombuffer(blob, np.uint8).copy()).pin_memory()
    boxes = [((5, 3, 17), (8, 100, 120)), ((0, 0, 0), (2, 100, 120)), ((14, 28, 40), (2, 100, 120))]
    sz, sy = 100 * 130 + 7, 130                                         # pitched views, one behind the other
    per = 8 * sz + 64
    s = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(s):
        d_blob = torch.empty(len(blob), dtype=torch.uint8, device=dev)
        out = torch.empty(3 * per, dtype=torch.int16, device=dev)
        for _ in range(2):
            d_blob.zero_()
            out.fill_(7)
            d_blob.copy_(host_blob, non_blocking=True)
            rc = sqy.decode_boxes_device(d_blob.data_ptr(), len(blob), [o for o, _ in boxes], [out.data_ptr() + 2 * per * i for i in range(3)], [e for _, e in boxes],
                                         [(sz, sy, 1)] * 3, np.uint16, stream=s.cuda_stream)
            assert rc == 0
            got = out.cpu().numpy().view(np.uint16)
            want = np.full(3 * per, 7, np.uint16)
            for i, (o, e) in enumerate(boxes):
                idx = (i * per + np.arange(e[0])[:, None, None] * sz + np.arange(e[1])[None, :, None] * sy + np.arange(e[2])[None, None, :]).reshape(-1)
                want[idx] = _cut(vol, o, e).reshape(-1)
            assert np.array_equal(got, want)


def test_four_host_threads(sqy):
    from sqeazy_amd import synth
    vols = [synth.stack((14 + i, 128, 160), np.uint16) for i in range(4)]
    blobs = []
    for v in vols:
        rc, b = sqy.encode("bitswap1->lz4", v, nthreads=2)
        assert rc == 0
        blobs.append(b)

    def one(i):
        origins = [(z0, 2 + i, 5) for z0 in range(0, vols[i].shape[0] - 1, 3)]
        extents = [(2, 100, 131)] * len(origins)
        ok = True
        for _ in range(3):
            rc, got = sqy.decode_boxes(blobs[i], origins, extents)
            ok = ok and rc == 0 and all(np.array_equal(g, _cut(vols[i], o, e)) for g, o, e in zip(got, origins, extents))
        return ok
    with ThreadPoolExecutor(4) as ex:
        assert all(ex.map(one, range(4)))
