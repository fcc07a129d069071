"""GPU: SQYAMD_Pyramid_Boxes_* -- a whole resolution pyramid of many boxes of ONE blob in one call: level l of box i is the box binned under
row l of the bins' table, by max, min or sum, into a uint32 output of the box's rank (include/sqeazy_amd.h).

Every output must be what numpy computes from SQY_Decode's volume of the blob (test_gpu_decode_box's `full`, the oracle's decode):
test_gpu_bin_boxes._bin, ufunc.reduceat along every axis at the cells' first voxels, per level and from the VOXELS each time -- never from
a finer level, never from the library under test.  Integers are exact, there is no tolerance.  ALL boxes of a case go in ONE call; their
outputs, box by box and levels ascending within a box, lie in one buffer of position-dependent pattern bytes (test_gpu_batch_window.Targets
with 32-bit elements), and the whole buffer and the blob are compared byte for byte after every call: a cell missed, stored by two levels'
arithmetic at once, a gap between pitched rows touched, a cell left at its neutral element all show.  Every case runs with
"pyramid_boxes_subset" 1 and 0 and "pyramid_boxes_fused" 1 and 0: the fused kernel with its tail launch, the layered path (Bin_Boxes'
launch and a reduce per level) and the whole decode give the same outputs, and each shows its launches in the profile -- so none can stand
in for another."""
import numpy as np
import pytest

from test_gpu_batch_window import Targets, _blob, _cut, _dev, _same
from test_gpu_bin_boxes import NEW_NAMES as BIN_NAMES, _bin
from test_gpu_compare_boxes import NEW_NAMES as COMPARE_NAMES, OTHERS
from test_gpu_decode_box import FALLBACK, SHAPES, SMALL_CHUNKS, SUBSET, _boxes, _case_blob, _launch_case, _made, _to_device
from test_gpu_decode_frames import _damaged, _lz4_frames, _profile_names
from test_gpu_project_boxes import LAYOUTS, NEW_NAMES as PROJECT_NAMES, OPS

pytestmark = pytest.mark.gpu

FINAL = {"bitswap1->lz4": "bitswap1_pyramid_boxes", "rmestbkrd->bitswap1->lz4": "bitswap1_pyramid_boxes", "quantiser->bitswap1->lz4": "bitswap1_quantiser_pyramid_boxes",
         "lz4": "boxes_window_bin", "frame_shuffle->lz4": "boxes_window_bin"}
LAYERED = {"bitswap1->lz4": "bitswap1_bin_boxes", "rmestbkrd->bitswap1->lz4": "bitswap1_bin_boxes", "quantiser->bitswap1->lz4": "bitswap1_quantiser_bin_boxes",
           "lz4": "boxes_window_bin", "frame_shuffle->lz4": "boxes_window_bin"}
PYRAMID_NAMES = {"bitswap1_pyramid_boxes", "bitswap1_quantiser_pyramid_boxes", "pyramid_reduce"}
IDS = ["%s-%s" % (p, np.dtype(d).name) for p, d in SUBSET]
PYRAMIDS = (((1, 1, 1), (2, 2, 2), (4, 4, 4), (8, 8, 8)), ((1, 2, 2), (1, 4, 4), (1, 8, 8)), ((3, 5, 7), (6, 5, 21), (12, 10, 42)), ((2, 1, 1), (1000, 1, 1)),
            ((2, 2, 2), (2, 2, 2)), ((2, 2, 2),), ((1, 1, 1), (1, 128, 128)))
MODES = ((1, 1), (1, 0), (0, 1), (0, 0))                                 # (pyramid_boxes_subset, pyramid_boxes_fused)
assert [s for s, _ in SHAPES] == [(7, 33, 31), (2, 3, 300), (3, 128, 128), (23, 131, 151), (16, 128, 128)]


def _cells(boxes, pyramid):
    """the outputs' extents, box by box and levels ascending within a box: ceil(extent / bins)"""
    return [tuple(-(-n // b) for n, b in zip(e, bins)) for _, e in boxes for bins in pyramid]


def _want(tiles, pyramid, op):
    """numpy's outputs in the same order, every level from the voxels"""
    return [_bin(t, bins, op) for t in tiles for bins in pyramid]


def _mode(options, mode):
    options("pyramid_boxes_subset", mode[0])
    options("pyramid_boxes_fused", mode[1])


def _call(sqy, d_blob, nbytes, boxes, pyramid, op, T, dtype, stream=None):
    n = len(pyramid)
    return sqy.pyramid_boxes_device(d_blob.data_ptr(), nbytes, [o for o, _ in boxes], [e for _, e in boxes], pyramid, op, [T.ptrs[i * n:(i + 1) * n] for i in range(len(boxes))],
                                    [T.strides[i * n:(i + 1) * n] for i in range(len(boxes))], dtype, stream=stream)


def _values(sqy, oracle, options, pipeline, dtype, nthreads=0):
    item = np.dtype(dtype).itemsize
    made = _made(sqy, oracle, pipeline, dtype, nthreads)
    assert made
    for shape, d_blob, nbytes, full in made:
        blob_host = d_blob.cpu().numpy()
        boxes = _boxes(shape, item)
        assert any(tuple(e) == tuple(shape) for _, e in boxes) and len(boxes) > shape[0]
        tiles = [_cut(full, o, e) for o, e in boxes]
        for k, pyramid in enumerate(PYRAMIDS):
            extents = _cells(boxes, pyramid)
            for j, op in enumerate(OPS):
                want = _want(tiles, pyramid, op)                             # (numpy's outputs: once per shape, pyramid and op)
                assert [w.shape for w in want] == extents
                # dense and pitched, on and 4 bytes behind the 16-byte grid: over the pyramids and ops all four combinations
                shift, pitch = LAYOUTS[(k + j) % 4]
                images = []
                for mode in MODES:
                    _mode(options, mode)
                    T = Targets(np.uint32, extents, shift=shift, pitch=pitch, salt=7 * shift + pitch + 2 * k)
                    rc = _call(sqy, d_blob, nbytes, boxes, pyramid, op, T, dtype)
                    assert rc == 0, (shape, pyramid, op, shift, pitch, mode)
                    got = T.read()
                    _same(got, T.expect(want)[0])
                    assert np.array_equal(d_blob.cpu().numpy(), blob_host), (shape, pyramid, op, mode)
                    images.append(got)
                assert all(np.array_equal(images[0], im) for im in images[1:])


@pytest.mark.parametrize("pipeline, dtype", SUBSET, ids=IDS)
def test_values(sqy, oracle, options, pipeline, dtype):
    """all boxes of every shape in one call; each of the pyramids x each op; the outputs dense and pitched, their bases on and 4 bytes
    behind the 16-byte grid; through the fused path, the layered one and the whole decode: the whole buffer byte for byte.  In the last
    pyramid a level-1 cell of the 16 x 128 x 128 and 23 x 131 x 151 boxes holds 16384 level-0 cells per layer, above the 8192
    accumulators of level 0: it goes through the tail launch whatever the plan's cap is"""
    _values(sqy, oracle, options, pipeline, dtype)


@pytest.mark.parametrize("pipeline, dtype, nthreads", FALLBACK, ids=["%s%s" % (p, "-serial" if t else "") for p, _, t in FALLBACK])
def test_values_of_blobs_the_subset_path_does_not_take(sqy, oracle, options, pipeline, dtype, nthreads):
    _values(sqy, oracle, options, pipeline, dtype, nthreads)


@pytest.mark.parametrize("pipeline, dtype", [("bitswap1->lz4", np.uint16), ("quantiser->bitswap1->lz4", np.uint16), ("lz4", np.uint8), ("bitswap1->lz4", np.uint8)])
def test_the_two_identities(sqy, oracle, options, pipeline, dtype):
    """per level equal to sqy.bin_boxes of that level; a top level at or beyond the extent along one axis, ones elsewhere, equal to
    project_boxes' image with a kept dimension of 1 -- against the library's own two calls, which their own tests hold against numpy"""
    for shape, cfg in (((7, 33, 31), SMALL_CHUNKS), ((16, 128, 128), "")):
        blob, full = _blob(sqy, oracle, pipeline + cfg, shape, dtype)
        d_blob = _to_device(blob)
        boxes = _boxes(shape, np.dtype(dtype).itemsize)
        origins, extents = [o for o, _ in boxes], [e for _, e in boxes]
        for mode in MODES:
            _mode(options, mode)
            for pyramid in PYRAMIDS[:3] + PYRAMIDS[6:]:
                for op in OPS:
                    per_level = []
                    for bins in pyramid:
                        rc, cells = sqy.bin_boxes(blob, origins, extents, bins, op)
                        assert rc == 0
                        per_level.append(cells)
                    T = Targets(np.uint32, _cells(boxes, pyramid), shift=4, pitch=True)
                    assert _call(sqy, d_blob, len(blob), boxes, pyramid, op, T, dtype) == 0
                    _same(T.read(), T.expect([per_level[l][i] for i in range(len(boxes)) for l in range(len(pyramid))])[0])
            for axis in range(3):
                pyramid = (tuple(2 if k == axis else 1 for k in range(3)), tuple(1000 if k == axis else 1 for k in range(3)))
                for op in OPS:
                    rc, images = sqy.project_boxes(blob, origins, extents, axis, op)
                    assert rc == 0
                    rc, levels = sqy.pyramid_boxes(blob, origins, extents, pyramid, op)
                    assert rc == 0 and all(np.array_equal(lv[1], np.expand_dims(im, axis)) for lv, im in zip(levels, images)), (shape, mode, axis, op)


@pytest.mark.parametrize("pipeline", ["bitswap1->lz4", "lz4"])
def test_neutral_elements(sqy, options, pipeline):
    """all 0xFFFF: min = 65535 and sum = 65535 V; all 0: max = 0 -- with the outputs pre-filled with all ones and with zeros, so a cell of
    any level that is left at a neutral element, or never stored, shows either way"""
    import torch
    shape = (16, 128, 128)
    boxes = [((0, 0, 0), shape), ((3, 5, 7), (9, 100, 121)), ((15, 0, 0), (1, 128, 128))]
    for fill in (0xFFFF, 0):
        vol = np.full(shape, fill, np.uint16)
        rc, blob = sqy.encode(pipeline, vol)
        assert rc == 0
        d_blob = _to_device(blob)
        for pyramid in (((2, 2, 2), (4, 4, 4), (8, 8, 8)), ((3, 5, 7), (3, 5, 21)), ((16, 1, 1), (16, 1, 128)), ((1, 1, 1), (1, 128, 128))):
            want = {op: _want([_cut(vol, o, e) for o, e in boxes], pyramid, op) for op in OPS}
            if fill:
                assert int(want["min"][1].flat[0]) == 65535 and int(want["sum"][1].flat[0]) == 65535 * int(np.prod(pyramid[1]))
            for pre in (0xFFFFFFFF, 0):
                for mode in MODES:
                    _mode(options, mode)
                    for op in OPS:
                        outs = [torch.full(tuple(w.shape), pre - 2 ** 32 if pre else 0, dtype=torch.int64, device=_dev()).to(torch.int32) for w in want[op]]
                        n = len(pyramid)
                        rc = sqy.pyramid_boxes_device(d_blob.data_ptr(), len(blob), [o for o, _ in boxes], [e for _, e in boxes], pyramid, op,
                                                      [[t.data_ptr() for t in outs[i * n:(i + 1) * n]] for i in range(len(boxes))], None, np.uint16)
                        assert rc == 0
                        torch.cuda.synchronize()
                        for t, w in zip(outs, want[op]):
                            assert np.array_equal(t.cpu().numpy().view(np.uint32), w), (fill, pyramid, pre, mode, op)


def test_the_sum_bound_on_the_device(sqy, options):
    """(16, 64, 65) maximal 16-bit voxels: a top level of 16 x 64 x 64 = 65536 voxels sums to 65535 x 65536 exactly (the partial cell
    behind it to 65535 x 1024); a top level of 16 x 64 x 65 returns 1 with the canaries intact, though the level below it is far inside the
    bound; max and min have no bound"""
    shape = (16, 64, 65)
    vol = np.full(shape, 0xFFFF, np.uint16)
    rc, blob = sqy.encode("bitswap1->lz4", vol)
    assert rc == 0
    d_blob = _to_device(blob)
    box = [((0, 0, 0), shape)]
    fits, over = ((4, 16, 16), (16, 64, 64)), ((16, 64, 1), (16, 64, 65))
    for mode in MODES:
        _mode(options, mode)
        T = Targets(np.uint32, _cells(box, fits), shift=4)
        assert T.extents == [(4, 4, 5), (1, 1, 2)]
        assert _call(sqy, d_blob, len(blob), box, fits, "sum", T, np.uint16) == 0
        want = _want([vol], fits, "sum")
        assert want[1].tolist() == [[[65535 * 65536, 65535 * 16 * 64]]]
        _same(T.read(), T.expect(want)[0])
        T = Targets(np.uint32, _cells(box, over), shift=4)
        assert _call(sqy, d_blob, len(blob), box, over, "sum", T, np.uint16) == 1
        _same(T.read(), T.host)
        for op in ("max", "min"):
            T = Targets(np.uint32, _cells(box, over))
            assert _call(sqy, d_blob, len(blob), box, over, op, T, np.uint16) == 0
            _same(T.read(), T.expect([np.full(x, 65535, np.uint32) for x in T.extents])[0])


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
            for k, pyramid in enumerate((((2, 2, 2), (4, 4, 4)), ((1, 3, 5), (1, 3, 15), (2, 9, 15)), ((4, 1, 32), (4, 1, 1024)))):
                for j, op in enumerate(OPS):
                    want = _want(tiles, pyramid, op)
                    for mode in MODES:
                        _mode(options, mode)
                        T = Targets(np.uint32, _cells(boxes, pyramid), shift=4 * (j % 2), pitch=bool(k % 2) ^ bool(mode[0]), salt=k + j)
                        assert _call(sqy, d_blob, len(blob), boxes, pyramid, op, T, dtype) == 0
                        _same(T.read(), T.expect(want)[0])
    assert seen >= 1


def _profiled(sqy, call):
    rcs = []
    sqy.profile_reset()
    sqy.profile_enable(True)
    try:
        rcs.append(call())
    finally:
        sqy.profile_enable(False)
    prof = sqy.profile_get()
    sqy.profile_reset()
    assert rcs == [0]
    return prof


@pytest.mark.parametrize("pipeline, dtype", SUBSET, ids=IDS)
def test_launches(sqy, oracle, options, pipeline, dtype):
    """the subset path with every level fusable: ONE pruned LZ4 launch and ONE launch under the path's pyramid name for K boxes and all
    their levels -- no pyramid_reduce, none of the binning's names; the copy forms: one boxes_window_bin and one pyramid_reduce; with
    "pyramid_boxes_fused" off: the binning's launch and a pyramid_reduce per further level; the subset option off: the whole blob once;
    SQYAMD_Bin_Boxes_*, SQYAMD_Decode_Boxes_* and SQYAMD_Project_Boxes_* launch what they launched"""
    shape, blob, full = _launch_case(sqy, oracle, pipeline, dtype)
    d_blob = _to_device(blob)
    Z = shape[0]
    boxes = [((Z // 2, 1, 1), (1, shape[1] - 2, shape[2] - 2)), ((0, 0, 3), (Z, shape[1], 5)), ((0, 2, 0), (1, 7, shape[2])), ((Z - 1, 0, 0), (1, shape[1], shape[2]))]
    planes = "bitswap1" in pipeline

    def decode_boxes():
        T = Targets(dtype, [e for _, e in boxes], pitch=True)
        assert sqy.decode_boxes_device(d_blob.data_ptr(), len(blob), [o for o, _ in boxes], T.ptrs, T.extents, T.strides, dtype) == 0
        T.read()

    def project_boxes():
        T = Targets(np.uint32, [e[1:] for _, e in boxes], pitch=True)
        assert sqy.project_boxes_device(d_blob.data_ptr(), len(blob), [o for o, _ in boxes], [e for _, e in boxes], 0, "max", T.ptrs, T.strides, dtype) == 0
        T.read()

    def bin_boxes():
        T = Targets(np.uint32, _cells(boxes, ((2, 2, 2),)), pitch=True)
        assert sqy.bin_boxes_device(d_blob.data_ptr(), len(blob), [o for o, _ in boxes], [e for _, e in boxes], (2, 2, 2), "max", T.ptrs, T.strides, dtype) == 0
        T.read()
    before = [_profile_names(sqy, f) for f in (decode_boxes, project_boxes, bin_boxes)]

    def profiled(bx, pyramid, op, pitch):
        T = Targets(np.uint32, _cells(bx, pyramid), shift=4, pitch=pitch)
        prof = _profiled(sqy, lambda: _call(sqy, d_blob, len(blob), bx, pyramid, op, T, dtype))
        _same(T.read(), T.expect(_want([_cut(full, o, e) for o, e in bx], pyramid, op))[0])
        return prof
    foreign = ("lz4_frames_decode", "batch_compare_init", "boxes_project_init") + OTHERS + tuple(COMPARE_NAMES) + tuple(PROJECT_NAMES)
    for k, pyramid, op in ((3, ((2, 2, 2), (4, 4, 4), (8, 8, 8)), "max"), (4, ((1, 4, 4), (1, 8, 8)), "min"), (4, ((3, 1, 32), (3, 1, 32), (6, 2, 64), (12, 2, 64)), "sum")):
        prof = profiled(boxes[:k], pyramid, op, True)
        names = set(prof)
        assert "lz4_frames_subset_decode" in names and prof["lz4_frames_subset_decode"][1] == 1, prof
        assert prof[FINAL[pipeline]][1] == 1 and not any(n in names for n in foreign), prof
        if planes:
            assert "pyramid_reduce" not in names and not any(n in names for n in BIN_NAMES) and len(names & PYRAMID_NAMES) == 1, prof
        else:
            assert prof["pyramid_reduce"][1] == 1 and not any(n in names for n in PYRAMID_NAMES - {"pyramid_reduce"}), prof
    # the layered path: the binning's launch, a reduce per further level
    options("pyramid_boxes_fused", 0)
    prof = profiled(boxes, ((2, 2, 2), (4, 4, 4), (8, 8, 8)), "max", True)
    assert prof["lz4_frames_subset_decode"][1] == 1 and prof[LAYERED[pipeline]][1] == 1 and prof["pyramid_reduce"][1] == 2, prof
    assert not any(n in prof for n in PYRAMID_NAMES - {"pyramid_reduce"}) and not any(n in prof for n in foreign), prof
    prof = profiled(boxes, ((2, 2, 2),), "sum", False)
    assert prof[LAYERED[pipeline]][1] == 1 and "pyramid_reduce" not in prof, prof
    # the subset option off: the whole blob once, one per-cell launch, one reduce for all further levels (fused) or one per level
    options("pyramid_boxes_subset", 0)
    prof = profiled(boxes, ((2, 2, 2), (4, 4, 4), (8, 8, 8)), "max", True)
    assert "lz4_frames_decode" in prof and prof["boxes_window_bin"][1] == 1 and prof["pyramid_reduce"][1] == 2, prof
    options("pyramid_boxes_fused", 1)
    prof = profiled(boxes, ((2, 2, 2), (4, 4, 4), (8, 8, 8)), "max", True)
    assert "lz4_frames_decode" in prof and prof["boxes_window_bin"][1] == 1 and prof["pyramid_reduce"][1] == 1, prof
    assert not any(n in prof for n in ("lz4_frames_subset_decode", "boxes_project_init", "boxes_window_copy", "boxes_window_project") + tuple(PYRAMID_NAMES - {"pyramid_reduce"})), prof
    options("pyramid_boxes_subset", 1)
    after = [_profile_names(sqy, f) for f in (decode_boxes, project_boxes, bin_boxes)]
    assert before == after, (before, after)
    assert not any(n in s for s in before for n in PYRAMID_NAMES), before


@pytest.mark.parametrize("pipeline, dtype", [("bitswap1->lz4", np.uint16), ("quantiser->bitswap1->lz4", np.uint16), ("bitswap1->lz4", np.uint8)])
def test_a_top_level_above_the_fused_ones_takes_exactly_one_more_launch(sqy, oracle, pipeline, dtype):
    """16 x 128 x 128 under ((1, 1, 1), (1, 128, 128)): a level-1 cell holds 16384 level-0 cells per layer, above level 0's 8192
    accumulators -- the pyramid kernel once, pyramid_reduce once; under ((1, 1, 1), (1, 64, 64)) the level is fused: no pyramid_reduce; two
    levels above the fused ones share the one launch"""
    shape = (16, 128, 128)
    blob, full = _blob(sqy, oracle, pipeline + SMALL_CHUNKS, shape, dtype)      # (4 KiB chunks: several LZ4 frames at either voxel size)
    d_blob = _to_device(blob)
    boxes = [((0, 0, 0), shape), ((3, 0, 0), (2, 128, 128))]
    for pyramid, tail in ((((1, 1, 1), (1, 128, 128)), 1), (((1, 1, 1), (1, 64, 64)), 0), (((1, 1, 1), (1, 64, 64), (1, 128, 128), (16, 128, 128)), 1)):
        T = Targets(np.uint32, _cells(boxes, pyramid), pitch=True)
        prof = _profiled(sqy, lambda: _call(sqy, d_blob, len(blob), boxes, pyramid, "sum" if len(pyramid) < 4 else "max", T, dtype))
        _same(T.read(), T.expect(_want([_cut(full, o, e) for o, e in boxes], pyramid, "sum" if len(pyramid) < 4 else "max"))[0])
        assert prof["lz4_frames_subset_decode"][1] == 1 and prof[FINAL[pipeline]][1] == 1, prof
        assert ("pyramid_reduce" in prof and prof["pyramid_reduce"][1] == 1) if tail else "pyramid_reduce" not in prof, (pyramid, prof)
        assert not any(n in prof for n in BIN_NAMES), prof


@pytest.mark.parametrize("pipeline", ["lz4", "bitswap1->lz4"])
def test_damaged_frame(sqy, options, pipeline):
    """pruning is real: the last compressed LZ4 frame damaged -- boxes in frames 0 and 3 do not need it: rc 0 and right outputs on the subset
    path; with a box in frame 15 added the call gives the full decode's code; nothing outside the outputs is written and the blob keeps its
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
    pyramid = ((1, 2, 2), (1, 4, 6), (1, 64, 6))
    for fused in (1, 0):
        options("pyramid_boxes_fused", fused)
        for op in OPS:
            want = _want([_cut(vol, o, e) for o, e in boxes], pyramid, op)
            T = Targets(np.uint32, _cells(boxes, pyramid), shift=4, pitch=True)
            rcs = []
            names = _profile_names(sqy, lambda: rcs.append(_call(sqy, d_bad, len(bad), boxes, pyramid, op, T, np.uint16)))
            assert "lz4_frames_subset_decode" in names and "lz4_frames_decode" not in names, names
            assert rcs == [0]
            _same(T.read(), T.expect(want)[0])
        rc, levels = sqy.pyramid_boxes(bad, [o for o, _ in boxes], [e for _, e in boxes], pyramid, "sum")
        assert rc == 0 and all(np.array_equal(g, _bin(_cut(vol, o, e), bins, "sum")) for lv, (o, e) in zip(levels, boxes) for g, bins in zip(lv, pyramid))
    for mode in MODES:
        _mode(options, mode)
        T = Targets(np.uint32, _cells(more, pyramid), pitch=True)
        assert _call(sqy, d_bad, len(bad), more, pyramid, "max", T, np.uint16) == rc_full, mode
        _, mask = T.expect([np.zeros(x, np.uint32) for x in _cells(more, pyramid)], skip=range(len(more) * len(pyramid)))
        _same(T.read(), T.host, mask)                                   # (the outputs may hold anything; nothing outside them is written)
        rc, levels = sqy.pyramid_boxes(bad, [o for o, _ in more], [e for _, e in more], pyramid, "max")
        assert rc == rc_full and levels is None
    assert np.array_equal(d_bad.cpu().numpy(), bad_host)


def test_refusals_on_the_device(sqy, oracle):
    """each applied to ONE output of three boxes x two levels in turn where it is an output's: 1 with all outputs and the canaries around
    them intact; then the good call"""
    shape = (3, 5, 7)
    blob, full = _blob(sqy, oracle, "bitswap1->lz4", shape, np.uint16)
    d_blob = _to_device(blob)
    extents = [(2, 3, 4), (1, 5, 7), (2, 3, 4)]
    origins = [(1, 1, 1), (2, 0, 0), (0, 2, 3)]
    boxes = list(zip(origins, extents))
    pyramid = ((1, 1, 2), (2, 2, 2))
    T = Targets(np.uint32, _cells(boxes, pyramid), pitch=True)

    def call(ptrs=None, strides=None, pyramid=pyramid, op="max", levels=None, dtype=np.uint16):
        p = list(T.ptrs) if ptrs is None else ptrs
        s = list(T.strides) if strides is None else strides
        n = len(T.ptrs) // 3
        return sqy.pyramid_boxes_device(d_blob.data_ptr(), len(blob), origins, extents, pyramid, op, [p[i * n:(i + 1) * n] for i in range(3)],
                                        [s[i * n:(i + 1) * n] for i in range(3)], dtype, levels=levels)

    def refused(rc):
        assert rc == 1, rc
        _same(T.read(), T.host)
    for k in range(6):
        for bad in (None, T.ptrs[k] + 2):
            refused(call(ptrs=[bad if i == k else p for i, p in enumerate(T.ptrs)]))
        bads = [(T.strides[k][0], T.strides[k][1], 2), (T.strides[k][0], 1, 1)]      # an innermost stride of 2; a row pitch that overlaps
        if T.extents[k][0] > 1:
            bads.append((4, T.strides[k][1], 1))                                    # a layer pitch below the rows' reach
        for bad in bads:
            refused(call(strides=[bad if i == k else s for i, s in enumerate(T.strides)]))
    for levels in (0, 9, -1):
        refused(call(levels=levels))
    for bad in (((1, 1, 2), (2, 2, 3)), ((1, 2, 2), (2, 3, 2)), ((2, 1, 2), (3, 2, 2)), ((2, 2, 2), (1, 1, 1)), ((1, 1, 2), (0, 2, 2)), ((1, 1, 2), (2, 2, -4))):
        refused(call(pyramid=bad))
    for op in (3, -1, 77):
        refused(call(op=op))
    refused(call(dtype=np.uint8))                                       # an entry point of the other type
    for op in OPS:
        Tg = Targets(np.uint32, _cells(boxes, pyramid), pitch=True)
        n = len(pyramid)
        assert sqy.pyramid_boxes_device(d_blob.data_ptr(), len(blob), origins, extents, pyramid, op, [Tg.ptrs[i * n:(i + 1) * n] for i in range(3)],
                                        [Tg.strides[i * n:(i + 1) * n] for i in range(3)], np.uint16) == 0
        _same(Tg.read(), Tg.expect(_want([_cut(full, o, e) for o, e in boxes], pyramid, op))[0])


def test_host_variant_mean_and_lower_ranks(sqy, oracle, options):
    """pyramid_boxes (host pointers, the outputs dense and back to back, box by box and levels ascending) gives numpy's outputs; "mean" is
    the sum over each cell's ACTUAL voxel count in float64, partial cells included; blobs of rank 1 and 2: the frames are the first
    dimension"""
    pyramid = ((2, 2, 2), (4, 2, 6), (4, 6, 30))
    for pipeline, dtype in (("bitswap1->lz4", np.uint16), ("lz4", np.uint8), ("quantiser->bitswap1->lz4", np.uint16), ("diff3x3x1->bitswap1->lz4", np.uint16)):
        blob, full = _blob(sqy, oracle, pipeline + (SMALL_CHUNKS if "diff" not in pipeline else ""), (7, 33, 31), dtype)
        boxes = _boxes((7, 33, 31), np.dtype(dtype).itemsize)
        origins, extents = [o for o, _ in boxes], [e for _, e in boxes]
        tiles = [_cut(full, o, e) for o, e in boxes]
        for mode in MODES:
            _mode(options, mode)
            for op in OPS:
                rc, levels = sqy.pyramid_boxes(blob, origins, extents, pyramid, op)
                assert rc == 0 and all(g.dtype == np.uint32 for lv in levels for g in lv) and all(len(lv) == len(pyramid) for lv in levels)
                for lv, t in zip(levels, tiles):
                    for g, bins in zip(lv, pyramid):
                        w = _bin(t, bins, op)
                        assert g.shape == w.shape and np.array_equal(g, w), (pipeline, mode, op, bins)
            rc, means = sqy.pyramid_boxes(blob, origins, extents, pyramid, "mean")
            assert rc == 0 and all(m.dtype == np.float64 for lv in means for m in lv)
            for lv, t in zip(means, tiles):
                for m, bins in zip(lv, pyramid):
                    count = _bin(np.ones(t.shape, np.uint8), bins, "sum")
                    assert np.array_equal(m, _bin(t, bins, "sum").astype(np.float64) / count.astype(np.float64)), (pipeline, mode, bins)
    _mode(options, (1, 1))
    from sqeazy_amd import synth
    cases = (((40, 300), [((3, 17), (30, 200)), ((39, 0), (1, 300)), ((0, 299), (40, 1))], (((4, 7), (8, 7), (8, 63)), ((1, 64), (1000, 64)))),
             ((9000,), [((4100,), (4000,)), ((0,), (9000,)), ((8999,), (1,))], (((3,), (12,), (4092,)), ((4096,), (8192,), (8192,)))))
    for shape, boxes, pyramids in cases:
        vol = synth.stack((1, 1, int(np.prod(shape))), np.uint16, seed=731).reshape(shape)
        tiles = [_cut(vol, o, e) for o, e in boxes]
        for pipeline in ("bitswap1->lz4" + SMALL_CHUNKS, "lz4" + SMALL_CHUNKS):
            rc, blob = sqy.encode(pipeline, vol)
            assert rc == 0
            d_blob = _to_device(blob)
            for pyramid in pyramids:
                for op in OPS:
                    want = _want(tiles, pyramid, op)
                    for pitch in (False, True):
                        T = Targets(np.uint32, _cells(boxes, pyramid), shift=4, pitch=pitch)
                        assert _call(sqy, d_blob, len(blob), boxes, pyramid, op, T, np.uint16) == 0, (shape, pipeline, pyramid, op, pitch)
                        _same(T.read(), T.expect(want)[0])
                    rc, levels = sqy.pyramid_boxes(blob, [o for o, _ in boxes], [e for _, e in boxes], pyramid, op)
                    flat = [g for lv in levels for g in lv]
                    assert rc == 0 and all(np.array_equal(g, w) and g.shape == w.shape for g, w in zip(flat, want))
