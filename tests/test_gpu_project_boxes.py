"""GPU: SQYAMD_Project_Boxes_* -- many boxes of ONE blob projected along an axis in one call: max, min or sum as uint32 images
(include/sqeazy_amd.h).

Every image must be what numpy computes from SQY_Decode's volume of the blob (test_gpu_decode_box's `full`, the oracle's decode):
full[box].max(axis), .min(axis), .sum(axis, dtype=uint64) cast to uint32 after asserting the sum is below 2^32 -- the code under test is
never the source of an expectation, integers are exact, there is no tolerance.  ALL boxes of a case go in ONE call; their images lie in
one buffer of position-dependent pattern bytes (test_gpu_batch_window.Targets with 32-bit elements), and the whole buffer and the blob are
compared byte for byte after every call: an element missed, a gap between pitched rows touched, a missing neutral element all show.  The
subset paths (the projecting range transposer, the projection in the compaction) and the whole decode ("project_boxes_subset" = 0) give
the same images, and each shows its launches in the profile -- so none can stand in for another."""
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from test_gpu_batch_window import Targets, _blob, _cut, _dev, _same
from test_gpu_compare_boxes import NEW_NAMES as COMPARE_NAMES, OTHERS
from test_gpu_decode_box import FALLBACK, SHAPES, SMALL_CHUNKS, SUBSET, _boxes, _case_blob, _launch_case, _made, _to_device
from test_gpu_decode_frames import _damaged, _lz4_frames, _profile_names

pytestmark = pytest.mark.gpu

OPS = ("max", "min", "sum")
FINAL = {"bitswap1->lz4": "bitswap1_project_boxes", "rmestbkrd->bitswap1->lz4": "bitswap1_project_boxes", "quantiser->bitswap1->lz4": "bitswap1_quantiser_project_boxes",
         "lz4": "boxes_window_project", "frame_shuffle->lz4": "boxes_window_project"}
NEW_NAMES = set(FINAL.values())
IDS = ["%s-%s" % (p, np.dtype(d).name) for p, d in SUBSET]
LAYOUTS = ((0, False), (4, True), (4, False), (0, True))                  # (the image's base behind the 16-byte grid in bytes, pitched rows)


def _reduce(tile, axis, op):
    """numpy's projection of a box, as uint32"""
    if op == "max":
        r = tile.max(axis)
    elif op == "min":
        r = tile.min(axis)
    else:
        r = tile.sum(axis, dtype=np.uint64)
        assert (r < 2 ** 32).all()
    return np.asarray(r).astype(np.uint32)                              # (a rank-1 box: zero dimensions, ONE element)


def _image_extents(boxes, axis):
    """the boxes' extents with `axis` removed (a rank-1 box: ONE element)"""
    return [tuple(n for k, n in enumerate(e) if k != axis) or (1,) for _, e in boxes]


def _call(sqy, d_blob, nbytes, boxes, axis, op, T, dtype, stream=None):
    return sqy.project_boxes_device(d_blob.data_ptr(), nbytes, [o for o, _ in boxes], [e for _, e in boxes], axis, op, T.ptrs, T.strides, dtype, stream=stream)


def _all_boxes(shape, item):
    """test_gpu_decode_box._boxes and, for every z, the whole frame z"""
    return _boxes(shape, item) + [((z, 0, 0), (1,) + tuple(shape[1:])) for z in range(shape[0])]


def _values(sqy, oracle, options, pipeline, dtype, nthreads=0):
    item = np.dtype(dtype).itemsize
    made = _made(sqy, oracle, pipeline, dtype, nthreads)
    assert made
    for shape, d_blob, nbytes, full in made:
        blob_host = d_blob.cpu().numpy()
        boxes = _all_boxes(shape, item)
        assert any(tuple(e) == tuple(shape) for _, e in boxes) and len(boxes) > 2 * shape[0]
        tiles = [_cut(full, o, e) for o, e in boxes]
        for axis in range(3):
            extents = _image_extents(boxes, axis)
            want = {op: [_reduce(t, axis, op) for t in tiles] for op in OPS}      # (numpy's images: once per shape and axis)
            for k, op in enumerate(OPS):
                # every op dense and pitched, on and 4 bytes behind the 16-byte grid; over the ops and axes all four combinations
                for shift, pitch in (LAYOUTS[(k + axis) % 4], LAYOUTS[(k + axis + 1) % 4]):
                    images = []
                    # the subset path, along axis 0 in both of its forms (the z-walk where the frames allow it, and the atomics); the whole decode
                    for subset, walk in ((1, 1), (1, 0), (0, 1)) if axis == 0 else ((1, 1), (0, 1)):
                        options("project_boxes_subset", subset)
                        options("project_boxes_walk", walk)
                        T = Targets(np.uint32, extents, shift=shift, pitch=pitch, salt=7 * shift + pitch + 2 * axis)
                        rc = _call(sqy, d_blob, nbytes, boxes, axis, op, T, dtype)
                        assert rc == 0, (shape, axis, op, shift, pitch, subset, walk)
                        got = T.read()
                        _same(got, T.expect(want[op])[0])
                        images.append(got)
                    assert all(np.array_equal(images[0], g) for g in images[1:])
            # a box of extent 1 along the axis: Decode_Boxes' voxels, widened
            thin = [(o, e) for o, e in boxes if e[axis] == 1]
            assert thin
            rc, voxels = sqy.decode_boxes(blob_host.tobytes(), [o for o, _ in thin], [e for _, e in thin])
            assert rc == 0
            T = Targets(np.uint32, _image_extents(thin, axis), shift=4, pitch=True)
            for op in OPS:
                assert _call(sqy, d_blob, nbytes, thin, axis, op, T, dtype) == 0
                got = T.read()
                for i, v in enumerate(voxels):
                    assert np.array_equal(got[T.bytes_of(i)].view(np.uint32)[..., 0], np.squeeze(v, axis).astype(np.uint32)), (shape, axis, op, thin[i])
        assert np.array_equal(d_blob.cpu().numpy(), blob_host), shape


@pytest.mark.parametrize("pipeline, dtype", SUBSET, ids=IDS)
def test_values(sqy, oracle, options, pipeline, dtype):
    """all boxes of every shape plus every whole frame in one call; each axis x each op; the images dense and pitched, their bases on and
    4 bytes behind the 16-byte grid; through the subset path and the whole decode: the whole buffer byte for byte"""
    _values(sqy, oracle, options, pipeline, dtype)


@pytest.mark.parametrize("pipeline, dtype, nthreads", FALLBACK, ids=["%s%s" % (p, "-serial" if t else "") for p, _, t in FALLBACK])
def test_values_of_blobs_the_subset_path_does_not_take(sqy, oracle, options, pipeline, dtype, nthreads):
    _values(sqy, oracle, options, pipeline, dtype, nthreads)


@pytest.mark.parametrize("pipeline", ["bitswap1->lz4", "lz4"])
def test_neutral_elements_and_wrap(sqy, options, pipeline):
    """all 0xFFFF: min = 65535 and sum = 65535 n; all 0: max = 0 -- with the images pre-filled with all ones and with zeros, so an init that
    is missing shows either way"""
    import torch
    shape = (16, 128, 128)
    boxes = [((0, 0, 0), shape), ((3, 5, 7), (9, 100, 121)), ((15, 0, 0), (1, 128, 128))]
    for fill in (0xFFFF, 0):
        vol = np.full(shape, fill, np.uint16)
        rc, blob = sqy.encode(pipeline, vol)
        assert rc == 0
        full = vol                                                      # (lossless pipelines: the volume itself)
        d_blob = _to_device(blob)
        for axis in range(3):
            want = {op: [_reduce(_cut(full, o, e), axis, op) for o, e in boxes] for op in OPS}
            if fill:
                assert int(want["min"][0][0, 0]) == 65535 and int(want["sum"][0][0, 0]) == 65535 * shape[axis]
            for pre in (0xFFFFFFFF, 0):
                for subset, walk in ((1, 1), (1, 0), (0, 1)):
                    options("project_boxes_subset", subset)
                    options("project_boxes_walk", walk)
                    for op in OPS:
                        outs = [torch.full(tuple(w.shape), pre - 2 ** 32 if pre else 0, dtype=torch.int64, device=_dev()).to(torch.int32) for w in want[op]]
                        rc = sqy.project_boxes_device(d_blob.data_ptr(), len(blob), [o for o, _ in boxes], [e for _, e in boxes], axis, op, [t.data_ptr() for t in outs], None,
                                                      np.uint16)
                        assert rc == 0
                        torch.cuda.synchronize()
                        for t, w in zip(outs, want[op]):
                            assert np.array_equal(t.cpu().numpy().view(np.uint32), w), (fill, axis, pre, subset, walk, op)


def test_the_sum_bound_on_the_device(sqy, options):
    """(65537, 1, 2) maximal 16-bit voxels, 4 KiB chunks: an extent of 65536 along axis 0 sums to 65535 x 65536 exactly; 65537 returns 1 with
    the canaries intact.  262 KB: the smallest volume that reaches the bound"""
    vol = np.full((65537, 1, 2), 0xFFFF, np.uint16)
    rc, blob = sqy.encode("bitswap1->lz4" + SMALL_CHUNKS, vol)
    assert rc == 0
    d_blob = _to_device(blob)
    for subset in (1, 0):
        options("project_boxes_subset", subset)
        for o in ((0, 0, 0), (1, 0, 0)):
            T = Targets(np.uint32, [(1, 2)], shift=4)
            assert _call(sqy, d_blob, len(blob), [(o, (65536, 1, 2))], 0, "sum", T, np.uint16) == 0
            _same(T.read(), T.expect([np.full((1, 2), 65535 * 65536, np.uint32)])[0])
        T = Targets(np.uint32, [(1, 2)], shift=4)
        assert _call(sqy, d_blob, len(blob), [((0, 0, 0), (65537, 1, 2))], 0, "sum", T, np.uint16) == 1
        _same(T.read(), T.host)
        # max and min have no bound
        for op, v in (("max", 65535), ("min", 65535)):
            T = Targets(np.uint32, [(1, 2)])
            assert _call(sqy, d_blob, len(blob), [((0, 0, 0), (65537, 1, 2))], 0, op, T, np.uint16) == 0
            _same(T.read(), T.expect([np.full((1, 2), v, np.uint32)])[0])


@pytest.mark.parametrize("pipeline, dtype", SUBSET, ids=IDS)
def test_two_boxes_with_a_gap_of_unneeded_frames_between_them(sqy, oracle, options, pipeline, dtype):
    """frames {0} and {Z - 1}: the union's compaction has other frames' places missing between the two boxes' words; the same two the other
    way round; and with a box that reaches over both and one nested in it (overlapping boxes)"""
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
            tiles = [_cut(full, o, e) for o, e in boxes]
            for axis in range(3):
                for k, op in enumerate(OPS):
                    want = [_reduce(t, axis, op) for t in tiles]
                    for subset in (1, 0):
                        options("project_boxes_subset", subset)
                        T = Targets(np.uint32, _image_extents(boxes, axis), shift=4 * (k % 2), pitch=bool(axis % 2) ^ bool(subset), salt=axis + k)
                        assert _call(sqy, d_blob, len(blob), boxes, axis, op, T, dtype) == 0
                        _same(T.read(), T.expect(want)[0])
    assert seen >= 1


@pytest.mark.parametrize("pipeline, dtype", SUBSET, ids=IDS)
def test_launches(sqy, oracle, options, pipeline, dtype):
    """the subset path: ONE pruned LZ4 launch and ONE launch under the path's own name for K boxes -- the neutral elements in front of the
    transposer, none in front of the per-element projection --, none of the decode, compare or copy finals; the option off: the whole blob
    once and one boxes_window_project; SQYAMD_Decode_Boxes_* and SQYAMD_Compare_Boxes_* launch what they launched"""
    shape, blob, full = _launch_case(sqy, oracle, pipeline, dtype)
    d_blob = _to_device(blob)
    Z = shape[0]
    boxes = [((Z // 2, 1, 1), (1, shape[1] - 2, shape[2] - 2)), ((0, 0, 3), (Z, shape[1], 5)), ((0, 2, 0), (1, 7, shape[2])), ((Z - 1, 0, 0), (1, shape[1], shape[2]))]
    tiles = [_cut(full, o, e) for o, e in boxes]

    def decode_boxes():
        T = Targets(dtype, [e for _, e in boxes], pitch=True)
        assert sqy.decode_boxes_device(d_blob.data_ptr(), len(blob), [o for o, _ in boxes], T.ptrs, T.extents, T.strides, dtype) == 0
        T.read()

    def compare_boxes():
        T = Targets(dtype, [e for _, e in boxes], pitch=True)
        rc, _ = sqy.compare_boxes_device(d_blob.data_ptr(), len(blob), [o for o, _ in boxes], T.ptrs, T.extents, T.strides, dtype)
        assert rc == 0
    before = [_profile_names(sqy, f) for f in (decode_boxes, compare_boxes)]

    def profiled(bx, axis, op, pitch):
        T = Targets(np.uint32, _image_extents(bx, axis), shift=4, pitch=pitch)
        rcs = []
        sqy.profile_reset()
        sqy.profile_enable(True)
        try:
            rcs.append(_call(sqy, d_blob, len(blob), bx, axis, op, T, dtype))
        finally:
            sqy.profile_enable(False)
        prof = sqy.profile_get()
        sqy.profile_reset()
        assert rcs == [0]
        _same(T.read(), T.expect([_reduce(_cut(full, o, e), axis, op) for o, e in bx])[0])
        return prof
    transposer = FINAL[pipeline] != "boxes_window_project"
    for k, axis, op in ((3, 0, "max"), (4, 1, "min"), (4, 2, "sum")):
        prof = profiled(boxes[:k], axis, op, True)
        names = set(prof)
        assert "lz4_frames_subset_decode" in names and prof["lz4_frames_subset_decode"][1] == 1, prof
        assert prof[FINAL[pipeline]][1] == 1 and sum(n in names for n in NEW_NAMES) == 1, prof
        assert ("boxes_project_init" in names) == transposer and (not transposer or prof["boxes_project_init"][1] == 1), prof
        assert not any(n in names for n in ("lz4_frames_decode", "batch_compare_init") + OTHERS + tuple(COMPARE_NAMES)), names
    options("project_boxes_subset", 0)
    prof = profiled(boxes, 0, "max", True)
    names = set(prof)
    assert "lz4_frames_decode" in names and prof["boxes_window_project"][1] == 1, prof
    assert not any(n in names for n in ("lz4_frames_subset_decode", "bitswap1_project_boxes", "bitswap1_quantiser_project_boxes", "boxes_project_init", "boxes_window_copy",
                                        "boxes_window_compare", "batch_window_compare")), names
    options("project_boxes_subset", 1)
    after = [_profile_names(sqy, f) for f in (decode_boxes, compare_boxes)]
    assert before == after, (before, after)
    assert not any(n in s for s in before for n in NEW_NAMES | {"boxes_project_init"}), before
    assert len(tiles) == 4


@pytest.mark.parametrize("pipeline", ["lz4", "bitswap1->lz4"])
def test_damaged_frame(sqy, options, pipeline):
    """pruning is real: the last compressed LZ4 frame damaged -- boxes in frames 0 and 3 do not need it: rc 0 and right images on the subset
    path; with a box in frame 15 added the call gives the full decode's code; nothing outside the images is written and the blob keeps its
    bytes both times"""
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
    bad_host = d_bad.cpu().numpy()
    boxes = [((0, 5, 7), (1, 50, 40)), ((3, 0, 0), (1, 64, 64)), ((0, 1, 1), (1, 3, 60))]
    more = boxes[:2] + [((15, 2, 2), (1, 9, 9))] + boxes[2:]
    for axis in range(3):
        for op in OPS:
            want = [_reduce(_cut(vol, o, e), axis, op) for o, e in boxes]
            T = Targets(np.uint32, _image_extents(boxes, axis), shift=4, pitch=True)
            rcs = []
            names = _profile_names(sqy, lambda: rcs.append(_call(sqy, d_bad, len(bad), boxes, axis, op, T, np.uint16)))
            assert "lz4_frames_subset_decode" in names and "lz4_frames_decode" not in names, names
            assert rcs == [0]
            _same(T.read(), T.expect(want)[0])
    rc, images = sqy.project_boxes(bad, [o for o, _ in boxes], [e for _, e in boxes], 1, "sum")
    assert rc == 0 and all(np.array_equal(g, _reduce(_cut(vol, o, e), 1, "sum")) for g, (o, e) in zip(images, boxes))
    for subset in (1, 0):
        options("project_boxes_subset", subset)
        T = Targets(np.uint32, _image_extents(more, 0), pitch=True)
        assert _call(sqy, d_bad, len(bad), more, 0, "max", T, np.uint16) == rc_full, subset
        _, mask = T.expect([np.zeros(x, np.uint32) for x in _image_extents(more, 0)], skip=range(len(more)))
        _same(T.read(), T.host, mask)                                   # (the images may hold anything; nothing outside them is written)
        rc, images = sqy.project_boxes(bad, [o for o, _ in more], [e for _, e in more], 0, "max")
        assert rc == rc_full and images is None
    assert np.array_equal(d_bad.cpu().numpy(), bad_host)


def test_refusals(sqy, oracle):
    """each applied to ONE box of three in turn where it is a box's: 1 with all three images and the canaries around them intact; then the
    good call"""
    shape = (3, 5, 7)
    blob, full = _blob(sqy, oracle, "bitswap1->lz4", shape, np.uint16)
    u8 = _blob(sqy, oracle, "bitswap1->lz4", shape, np.uint8)[0]
    d_blob, d_u8 = _to_device(blob), _to_device(u8)
    extents = [(2, 3, 4), (1, 5, 7), (2, 3, 4)]
    origins = [(1, 1, 1), (2, 0, 0), (0, 2, 3)]
    boxes = list(zip(origins, extents))
    T = Targets(np.uint32, _image_extents(boxes, 0), pitch=True)
    assert T.strides[0] == (7, 1)

    def call(k=None, src=d_blob.data_ptr(), n=len(blob), dtype=np.uint16, count=None, axis=0, op="max", **box):
        """box k with the fields of `box` in place of its own"""
        o, p, e, s = list(origins), list(T.ptrs), list(extents), list(T.strides)
        if k is not None:
            if "origin" in box: o[k] = box["origin"]
            if "out" in box: p[k] = box["out"]
            if "shape" in box: e[k] = box["shape"]
            if "strides" in box: s[k] = box["strides"]
        return sqy.project_boxes_device(src, n, o, e, axis, op, p, s, dtype, count=count)

    def refused_call(rc):
        assert rc == 1, rc
        _same(T.read(), T.host)

    def refused(**kw):
        for k in range(3):
            refused_call(call(k, **kw))
    for axis in (3, -1, 2 ** 31 - 1):                                   # axis >= rank or < 0
        refused_call(call(axis=axis))
    for op in (3, -1, 77):                                              # op outside 0 .. 2
        refused_call(call(op=op))
    for count in (0, -1, -(2 ** 40)):
        refused_call(call(count=count))
    refused(out=None)                                                   # a NULL entry
    refused(out=T.ptrs[0] + 2)                                          # an image 2 bytes off
    refused(strides=(3, 1))                                             # a stride that overlaps: rows of 4 (or 7) elements, 3 apart
    refused(strides=(8, 2))                                             # an innermost stride of 2
    refused_call(call(src=d_u8.data_ptr(), n=len(u8)))                  # a blob of the other voxel type
    refused_call(call(dtype=np.uint8))                                  # .. an entry point of the other type
    refused(origin=(0, -1, 0))
    refused(shape=(2, 0, 4))
    for d in range(3):                                                  # origin + extent one voxel past the shape, each dimension in turn
        e = [2, 4, 6]
        e[d] += 1
        refused(origin=(1, 1, 1), shape=tuple(e), strides=(e[2] + 3, 1))
        o = [0, 0, 0]
        o[d] = 2 ** 63 - 1
        refused(origin=tuple(o), shape=(1, 1, 1), strides=(4, 1))       # no wrap to a small sum
    # a rank other than the header's
    refused_call(sqy.project_boxes_device(d_blob.data_ptr(), len(blob), [(1, 1)] * 3, [(3, 4)] * 3, 0, "max", T.ptrs, [(1,)] * 3, np.uint16))
    refused_call(call(src=None))
    refused_call(call(n=0))
    for axis in range(3):
        for op in OPS + (0, 1, 2):
            Tg = Targets(np.uint32, _image_extents(boxes, axis), pitch=True)
            assert sqy.project_boxes_device(d_blob.data_ptr(), len(blob), origins, extents, axis, op, Tg.ptrs, Tg.strides, np.uint16) == 0
            name = OPS[op] if isinstance(op, int) else op
            _same(Tg.read(), Tg.expect([_reduce(_cut(full, o, e), axis, name) for o, e in boxes])[0])
    # the host variant: a capacity one byte short, the other type, a box outside
    import ctypes
    L = sqy.lib()
    rows = lambda v: (ctypes.c_long * sum(len(r) for r in v))(*[x for r in v for x in r])
    src = np.frombuffer(blob, np.uint8)
    out = np.full(12 + 35 + 12, 0xA5A5A5A5, np.uint32)
    for fn, o, e, nbytes in ((L.SQYAMD_Project_Boxes_UI16, origins, extents, out.nbytes - 1), (L.SQYAMD_Project_Boxes_UI8, origins, extents, out.nbytes),
                             (L.SQYAMD_Project_Boxes_UI16, origins, extents[:2] + [(2, 3, 5)], out.nbytes + 64)):
        assert fn(src.ctypes.data, len(blob), 3, rows(o), rows(e), 3, 0, 0, out.ctypes.data, nbytes) == 1
        assert (out == 0xA5A5A5A5).all()
    assert L.SQYAMD_Project_Boxes_UI16(src.ctypes.data, len(blob), 3, rows(origins), rows(extents), 3, 0, 0, out.ctypes.data, out.nbytes) == 0
    assert np.array_equal(out, np.concatenate([_reduce(_cut(full, o, e), 0, "max").reshape(-1) for o, e in boxes]))


def test_host_variant_and_lower_ranks(sqy, oracle, options):
    """project_boxes (host pointers, the images dense and back to back) gives what the device variant gives and numpy's images; "mean" is
    numpy's float64 mean; blobs of rank 1 and 2: the frames are the first dimension, a rank-1 box gives ONE element"""
    for pipeline, dtype in (("bitswap1->lz4", np.uint16), ("lz4", np.uint8), ("quantiser->bitswap1->lz4", np.uint16), ("diff3x3x1->bitswap1->lz4", np.uint16)):
        blob, full = _blob(sqy, oracle, pipeline + (SMALL_CHUNKS if "diff" not in pipeline else ""), (7, 33, 31), dtype)
        d_blob = _to_device(blob)
        boxes = _boxes((7, 33, 31), np.dtype(dtype).itemsize)
        tiles = [_cut(full, o, e) for o, e in boxes]
        for subset in (1, 0):
            options("project_boxes_subset", subset)
            for axis in range(3):
                for op in OPS:
                    rc, images = sqy.project_boxes(blob, [o for o, _ in boxes], [e for _, e in boxes], axis, op)
                    assert rc == 0 and all(g.dtype == np.uint32 for g in images)
                    assert all(np.array_equal(g, _reduce(t, axis, op)) for g, t in zip(images, tiles)), (pipeline, subset, axis, op)
                    T = Targets(np.uint32, _image_extents(boxes, axis))
                    assert _call(sqy, d_blob, len(blob), boxes, axis, op, T, dtype) == 0
                    got = T.read()
                    assert all(np.array_equal(got[T.bytes_of(i)].view(np.uint32)[..., 0], g) for i, g in enumerate(images))
                rc, means = sqy.project_boxes(blob, [o for o, _ in boxes], [e for _, e in boxes], axis, "mean")
                assert rc == 0 and all(m.dtype == np.float64 for m in means)
                assert all(np.array_equal(m, t.mean(axis, dtype=np.float64)) for m, t in zip(means, tiles)), (pipeline, subset, axis)
    options("project_boxes_subset", 1)
    from sqeazy_amd import synth
    cases = (((40, 300), [((3, 17), (30, 200)), ((39, 0), (1, 300)), ((0, 299), (40, 1))]), ((9000,), [((4100,), (4000,)), ((0,), (9000,)), ((8999,), (1,))]))
    for shape, boxes in cases:
        vol = synth.stack((1, 1, int(np.prod(shape))), np.uint16, seed=731).reshape(shape)
        tiles = [_cut(vol, o, e) for o, e in boxes]
        for pipeline in ("bitswap1->lz4" + SMALL_CHUNKS, "lz4" + SMALL_CHUNKS):
            rc, blob = sqy.encode(pipeline, vol)
            assert rc == 0
            d_blob = _to_device(blob)
            for axis in range(len(shape)):
                for op in OPS:
                    want = [_reduce(t, axis, op) for t in tiles]
                    for pitch in (False, True):
                        T = Targets(np.uint32, _image_extents(boxes, axis), shift=4, pitch=pitch)
                        assert _call(sqy, d_blob, len(blob), boxes, axis, op, T, np.uint16) == 0, (shape, pipeline, axis, op, pitch)
                        _same(T.read(), T.expect(want)[0])
                    rc, images = sqy.project_boxes(blob, [o for o, _ in boxes], [e for _, e in boxes], axis, op)
                    assert rc == 0 and all(np.array_equal(g, w) and g.shape == w.shape for g, w in zip(images, want))


def test_work_queued_on_the_callers_stream_is_respected(sqy):
    """the blob and the images' fill are written by work queued on the caller's stream just before the call"""
    import torch
    from sqeazy_amd import synth
    dev = _dev()
    vol = synth.stack((16, 128, 160), np.uint16)
    rc, blob = sqy.encode("bitswap1->lz4", vol, nthreads=2)
    assert rc == 0
    host_blob = torch.from_numpy(np.frombuffer(blob, np.uint8).copy()).pin_memory()
    boxes = [((5, 3, 17), (8, 100, 120)), ((0, 0, 0), (2, 100, 120)), ((14, 28, 40), (2, 100, 120))]
    s = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(s):
        d_blob = torch.empty(len(blob), dtype=torch.uint8, device=dev)
        for k, (axis, op) in enumerate(((0, "max"), (2, "min"), (1, "sum"), (0, "min"))):
            want = [_reduce(_cut(vol, o, e), axis, op) for o, e in boxes]
            outs = [torch.empty(tuple(w.shape), dtype=torch.int32, device=dev) for w in want]
            d_blob.zero_()
            d_blob.copy_(host_blob, non_blocking=True)
            for t in outs:
                t.fill_(-1 if k % 2 else 0)
            rc = sqy.project_boxes_device(d_blob.data_ptr(), len(blob), [o for o, _ in boxes], [e for _, e in boxes], axis, op, [t.data_ptr() for t in outs], None, np.uint16,
                                          stream=s.cuda_stream)
            assert rc == 0
            s.synchronize()
            assert all(np.array_equal(t.cpu().numpy().view(np.uint32), w) for t, w in zip(outs, want)), (axis, op)


def test_four_host_threads(sqy):
    from sqeazy_amd import synth
    vols = [synth.stack((14 + i, 128, 160), np.uint16) for i in range(4)]
    blobs = []
    for v in vols:
        rc, b = sqy.encode("bitswap1->lz4", v, nthreads=2)
        assert rc == 0
        blobs.append(b)

    def one(i):
        import torch
        dev = _dev()
        origins = [(z0, 2 + i, 5) for z0 in range(0, vols[i].shape[0] - 1, 3)]
        extents = [(2, 100, 131)] * len(origins)
        axis, op = i % 3, OPS[i % 3]
        want = [_reduce(_cut(vols[i], o, e), axis, op) for o, e in zip(origins, extents)]
        s = torch.cuda.Stream(device=dev)
        ok = True
        with torch.cuda.stream(s):
            d_blob = torch.from_numpy(np.frombuffer(blobs[i], np.uint8).copy()).to(dev)
            for _ in range(3):
                outs = [torch.full(tuple(w.shape), 7, dtype=torch.int32, device=dev) for w in want]
                rc = sqy.project_boxes_device(d_blob.data_ptr(), len(blobs[i]), origins, extents, axis, op, [t.data_ptr() for t in outs], None, np.uint16, stream=s.cuda_stream)
                s.synchronize()
                ok = ok and rc == 0 and all(np.array_equal(t.cpu().numpy().view(np.uint32), w) for t, w in zip(outs, want))
            rc, images = sqy.project_boxes(blobs[i], origins, extents, axis, op)
            ok = ok and rc == 0 and all(np.array_equal(g, w) for g, w in zip(images, want))
        return ok
    with ThreadPoolExecutor(4) as ex:
        assert all(ex.map(one, range(4)))
