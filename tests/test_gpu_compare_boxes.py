"""GPU: SQYAMD_Compare_Boxes_* -- many boxes of ONE blob compared with resident voxels in one call, nothing written (include/sqeazy_amd.h,
DESIGN.md 2).

Every row of statistics must be what the CPU computes with integers (test_gpu_batch_compare._stats) from SQY_Decode's volume of the blob
(test_gpu_decode_box's `full`, the oracle's decode) and the voxels the test put into the view -- the code under test is never the source of
an expectation, integers are exact, there is no tolerance.  ALL boxes of a case go in ONE call; their views lie in one buffer of
position-dependent pattern bytes (test_gpu_batch_window.Targets), so a reader that strays into the gaps between rows and frames, around the
views, or into the blob's voxels just outside a box counts them; and the whole view buffer and the blob buffer must be byte for byte what
they were after every call.  The subset paths (the comparing range transposer, the compare in the compaction) and the whole decode
("compare_boxes_subset" = 0) give the same rows, and each shows its launches in the profile -- so none can stand in for another."""
import ctypes
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from test_gpu_batch_compare import ONES, Views, _stats, _variants
from test_gpu_batch_window import Targets, _blob, _cut, _dev, _pack
from test_gpu_decode_box import FALLBACK, LONG_MAX, SMALL_CHUNKS, SUBSET, _boxes, _case_blob, _launch_case, _made, _to_device
from test_gpu_decode_frames import _damaged, _lz4_frames, _profile_names

pytestmark = pytest.mark.gpu

FINAL = {"bitswap1->lz4": "bitswap1_compare_boxes", "rmestbkrd->bitswap1->lz4": "bitswap1_compare_boxes", "quantiser->bitswap1->lz4": "bitswap1_quantiser_compare_boxes",
         "lz4": "boxes_window_compare", "frame_shuffle->lz4": "boxes_window_compare"}
NEW_NAMES = set(FINAL.values())
# the final launches of the decode drivers and of the tiled store's compare: none of them belongs to this call
OTHERS = ("bitswap1_decode", "bitswap1_quantiser_decode", "bitswap1_decode_range", "bitswap1_quantiser_decode_range", "bitswap1_decode_box", "bitswap1_quantiser_decode_box",
          "box_window_copy", "bitswap1_decode_boxes", "bitswap1_quantiser_decode_boxes", "boxes_window_copy", "frames_range_copy", "frame_scatter", "batch_window_copy",
          "batch_window_compare", "batch_bitswap1_decode_window_compare", "batch_compare_window")
IDS = ["%s-%s" % (p, np.dtype(d).name) for p, d in SUBSET]


def _call(sqy, d_blob, nbytes, boxes, V, stream=None):
    T = V.T
    rc, stats = sqy.compare_boxes_device(d_blob.data_ptr(), nbytes, [o for o, _ in boxes], T.ptrs, T.extents, T.strides, T.dtype, stream=stream)
    assert stats.dtype == np.uint64 and stats.shape == (len(boxes), 8)
    return rc, [[int(x) for x in row] for row in stats]


def _all_boxes(shape, item):
    """test_gpu_decode_box._boxes and, for every z, the whole frame z: the first and the last voxel of those lie in a range's first and last
    word"""
    return _boxes(shape, item) + [((z, 0, 0), (1,) + tuple(shape[1:])) for z in range(shape[0])]


def _planted(tiles, k0=0):
    """the tiles with one voxel changed in each"""
    views = []
    for k, t in enumerate(tiles):
        v = np.ascontiguousarray(t).copy()
        v.reshape(-1)[(7 * (k + k0) + 3) % v.size] ^= 0x55
        views.append(v)
    return views


def _statistics(sqy, oracle, options, pipeline, dtype, nthreads=0):
    item = np.dtype(dtype).itemsize
    made = _made(sqy, oracle, pipeline, dtype, nthreads)
    assert made
    for shape, d_blob, nbytes, full in made:
        blob_host = d_blob.cpu().numpy()
        boxes = _all_boxes(shape, item)
        assert any(tuple(e) == tuple(shape) for _, e in boxes) and len(boxes) > 2 * shape[0]
        tiles = [np.ascontiguousarray(_cut(full, o, e)) for o, e in boxes]
        variants = _variants([(shape, o, e) for o, e in boxes], tiles, dtype)      # (the CPU's rows: once per shape)
        assert len(variants) >= 7, [v[0] for v in variants]
        for shift in (0, item):
            for pitch in (False, True):
                V = Views(dtype, [e for _, e in boxes], shift=shift, pitch=pitch, salt=7 * shift + pitch)
                for subset in (1, 0):
                    options("compare_boxes_subset", subset)
                    for name, views, want in variants:
                        V.fill(views)
                        rc, got = _call(sqy, d_blob, nbytes, boxes, V)
                        assert rc == 0, (shape, subset, shift, pitch, name)
                        bad = [(i, boxes[i], g, w) for i, (g, w) in enumerate(zip(got, want)) if g != w]
                        assert not bad, (shape, subset, shift, pitch, name, len(bad), bad[:3])
                        assert V.unchanged(), (shape, subset, shift, pitch, name)
                assert np.array_equal(d_blob.cpu().numpy(), blob_host), (shape, shift, pitch)


@pytest.mark.parametrize("pipeline, dtype", SUBSET, ids=IDS)
def test_statistics(sqy, oracle, options, pipeline, dtype):
    """all boxes of every shape in one call, the views' bases on and one voxel behind the 16-byte grid, dense and pitched, through the subset
    path and the whole decode; view contents same, first, last, tail, run+0, run+127, run+128, all of _variants"""
    _statistics(sqy, oracle, options, pipeline, dtype)


@pytest.mark.parametrize("pipeline, dtype, nthreads", FALLBACK, ids=["%s%s" % (p, "-serial" if t else "") for p, _, t in FALLBACK])
def test_statistics_of_blobs_the_subset_path_does_not_take(sqy, oracle, options, pipeline, dtype, nthreads):
    _statistics(sqy, oracle, options, pipeline, dtype, nthreads)


@pytest.mark.parametrize("pipeline, dtype", SUBSET, ids=IDS)
def test_two_boxes_with_a_gap_of_unneeded_frames_between_them(sqy, oracle, options, pipeline, dtype):
    """frames {0} and {Z - 1}: the union's compaction has other frames' places missing between the two boxes' words; and the same two with
    a box that reaches over both and one nested in it; a planted difference in each box"""
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
            tiles = [_cut(full, o, e) for o, e in boxes]
            views = _planted(tiles)
            want = [_stats(t, v) for t, v in zip(tiles, views)]
            assert all(w[1] == 1 for w in want)
            for shift, pitch in ((0, False), (item, True)):
                V = Views(dtype, [e for _, e in boxes], shift=shift, pitch=pitch, salt=shift + pitch)
                V.fill(views)
                for subset in (1, 0):
                    options("compare_boxes_subset", subset)
                    rc, got = _call(sqy, d_blob, len(blob), boxes, V)
                    assert rc == 0 and got == want and V.unchanged(), (shape, boxes, shift, pitch, subset, got, want)
    assert seen >= 1


@pytest.mark.parametrize("pipeline", ["bitswap1->lz4", "lz4"])
def test_64_bits_where_they_are_needed(sqy, options, pipeline):
    """zeros against 65535 everywhere, 16 x 128 x 128, as one whole box plus sixteen one-frame boxes in the same call: above 2^32 in a
    thread's 128 voxels, 2^18 x 65535^2 in the whole box (a hair below 2^50), eight workgroups into one record"""
    import torch
    shape = (16, 128, 128)
    n = int(np.prod(shape))
    rc, blob = sqy.encode(pipeline, np.zeros(shape, np.uint16))
    assert rc == 0
    rc, full = sqy.decode(blob)
    assert rc == 0 and not full.any()
    d_blob = _to_device(blob)
    view = torch.full(shape, -1, dtype=torch.int16, device=_dev())      # (65535 as torch spells it)
    assert int(view.cpu().numpy().view(np.uint16).min()) == 65535
    row = lambda m: [m, m, m * 65535, m * 65535 ** 2, 65535, m * 65535, 65535, 65535]
    want = [row(n)] + [row(n // 16)] * 16
    assert 2 ** 49 < want[0][3] < 2 ** 50 and 128 * 65535 ** 2 > 2 ** 32
    origins = [(0, 0, 0)] + [(z, 0, 0) for z in range(16)]
    extents = [shape] + [(1, 128, 128)] * 16
    ptrs = [view.data_ptr()] + [view.data_ptr() + 2 * z * 128 * 128 for z in range(16)]
    for subset in (1, 0):
        options("compare_boxes_subset", subset)
        rc, stats = sqy.compare_boxes_device(d_blob.data_ptr(), len(blob), origins, ptrs, extents, None, np.uint16)
        assert rc == 0 and [[int(x) for x in r] for r in stats] == want, (subset, stats)
    torch.cuda.synchronize()
    assert int(view.cpu().numpy().view(np.uint16).min()) == 65535


@pytest.mark.parametrize("pipeline, dtype", SUBSET, ids=IDS)
def test_launches(sqy, oracle, options, pipeline, dtype):
    """the subset path: ONE pruned LZ4 launch and ONE of the new final launches for K boxes, none of the decode drivers' or of the tiled
    store's compare; the option off: the whole blob once and one boxes_window_compare; SQYAMD_Decode_Boxes_*, SQYAMD_Decode_Box_* and
    SQYAMD_Compare_BatchWindow_* launch what they launched"""
    shape, blob, full = _launch_case(sqy, oracle, pipeline, dtype)
    d_blob = _to_device(blob)
    Z = shape[0]
    boxes = [((Z // 2, 1, 1), (1, shape[1] - 2, shape[2] - 2)), ((0, 0, 3), (Z, shape[1], 5)), ((0, 2, 0), (1, 7, shape[2])), ((Z - 1, 0, 0), (1, shape[1], shape[2]))]
    tiles = [_cut(full, o, e) for o, e in boxes]
    views = _planted(tiles)
    want = [_stats(t, v) for t, v in zip(tiles, views)]

    def decode_boxes():
        T = Targets(dtype, [e for _, e in boxes], pitch=True)
        assert sqy.decode_boxes_device(d_blob.data_ptr(), len(blob), [o for o, _ in boxes], T.ptrs, T.extents, T.strides, dtype) == 0
        T.read()

    def decode_box():
        T = Targets(dtype, [boxes[0][1]], pitch=True)
        assert sqy.decode_box_device(d_blob.data_ptr(), len(blob), boxes[0][0], T.ptrs[0], boxes[0][1], T.strides[0], dtype) == 0
        T.read()

    def compare_tiles():
        V1 = Views(dtype, [boxes[0][1]], pitch=True)
        V1.fill(views[:1])
        rc, stats = sqy.compare_batch_window_device(d_blob.data_ptr(), [0], [len(blob)], [boxes[0][0]], V1.T.ptrs, V1.T.extents, V1.T.strides, dtype)
        assert rc == 0 and [int(x) for x in stats[0]] == want[0]
    before = [_profile_names(sqy, f) for f in (decode_boxes, decode_box, compare_tiles)]
    for k in (3, 4):
        V = Views(dtype, [e for _, e in boxes[:k]], shift=np.dtype(dtype).itemsize, pitch=True)
        V.fill(views[:k])
        got = []
        names = _profile_names(sqy, lambda: got.append(_call(sqy, d_blob, len(blob), boxes[:k], V)))
        assert got[0] == (0, want[:k]) and V.unchanged(), (got, want[:k])
        assert "lz4_frames_subset_decode" in names and FINAL[pipeline] in names and "batch_compare_init" in names, names
        assert sum(n in names for n in NEW_NAMES) == 1, names
        assert not any(n in names for n in ("lz4_frames_decode",) + OTHERS), names
    options("compare_boxes_subset", 0)
    V = Views(dtype, [e for _, e in boxes], pitch=True)
    V.fill(views)
    got = []
    names = _profile_names(sqy, lambda: got.append(_call(sqy, d_blob, len(blob), boxes, V)))
    assert got[0] == (0, want) and V.unchanged(), (got, want)
    assert "lz4_frames_decode" in names and "boxes_window_compare" in names, names
    assert not any(n in names for n in ("lz4_frames_subset_decode", "bitswap1_compare_boxes", "bitswap1_quantiser_compare_boxes", "boxes_window_copy", "batch_window_compare")), names
    options("compare_boxes_subset", 1)
    after = [_profile_names(sqy, f) for f in (decode_boxes, decode_box, compare_tiles)]
    assert before == after, (before, after)
    assert not any(n in s for s in before for n in NEW_NAMES), before


@pytest.mark.parametrize("pipeline", ["lz4", "bitswap1->lz4"])
def test_damaged_frame(sqy, options, pipeline):
    """pruning is real: the last compressed LZ4 frame damaged -- boxes in frames 0 and 3 do not need it (of every bit plane two chunks: their
    words lie in the first): rc 0 and right rows on the subset path; with a box in frame 15 added the call gives the full decode's code and
    every row all ones; the views and the blob keep their bytes both times"""
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
    tiles = [_cut(vol, o, e) for o, e in boxes]
    views = _planted(tiles)
    want = [_stats(t, v) for t, v in zip(tiles, views)]
    V = Views(np.uint16, [e for _, e in boxes], shift=2, pitch=True)
    V.fill(views)
    got = []
    names = _profile_names(sqy, lambda: got.append(_call(sqy, d_bad, len(bad), boxes, V)))
    assert "lz4_frames_subset_decode" in names and "lz4_frames_decode" not in names, names
    assert got[0] == (0, want) and V.unchanged(), (got, want)
    rc, stats = sqy.compare_boxes(bad, [o for o, _ in boxes], views)
    assert rc == 0 and [[int(x) for x in r] for r in stats] == want
    more = boxes[:2] + [((15, 2, 2), (1, 9, 9))] + boxes[2:]
    more_views = views[:2] + [_cut(vol, (15, 2, 2), (1, 9, 9)).copy()] + views[2:]
    for subset in (1, 0):
        options("compare_boxes_subset", subset)
        V = Views(np.uint16, [e for _, e in more], pitch=True)
        V.fill(more_views)
        rc, got = _call(sqy, d_bad, len(bad), more, V)
        assert rc == rc_full and got == [[ONES] * 8] * len(more), (subset, rc, got)
        assert V.unchanged()
        rc, stats = sqy.compare_boxes(bad, [o for o, _ in more], more_views)
        assert rc == rc_full and (stats == np.uint64(ONES)).all()
    assert np.array_equal(d_bad.cpu().numpy(), bad_host)


def test_shared_and_overlapping_views(sqy, oracle, options):
    """the same box twice onto one view gives equal rows; two boxes onto overlapping views (one view inside the other's buffer) each give the
    CPU's row; a box named twice against different views"""
    import torch
    from sqeazy_amd import synth
    shape = (7, 33, 31)
    for pipeline in ("bitswap1->lz4", "lz4", "quantiser->bitswap1->lz4"):
        blob, full = _blob(sqy, oracle, pipeline + SMALL_CHUNKS, shape, np.uint16)
        d_blob = _to_device(blob)
        buf = synth.stack((5, 31, 29), np.uint16, seed=955)             # the shared voxels: a dense view of (5, 31, 29)
        d_buf = torch.from_numpy(buf.copy()).to(_dev())
        p0 = d_buf.data_ptr()
        whole, st = (5, 31, 29), (31 * 29, 29, 1)
        # (origin, extent, view's first voxel in buf): the first two are the SAME box onto the SAME view, the third a box onto a view inside
        # it, the fourth another box onto the whole view again
        calls = [((1, 1, 1), whole, (0, 0, 0)), ((1, 1, 1), whole, (0, 0, 0)), ((0, 2, 2), (2, 3, 4), (1, 1, 1)), ((2, 2, 2), whole, (0, 0, 0))]
        ptrs = [p0 + 2 * sum(a * s for a, s in zip(at, st)) for _, _, at in calls]
        for subset in (1, 0):
            options("compare_boxes_subset", subset)
            rc, stats = sqy.compare_boxes_device(d_blob.data_ptr(), len(blob), [o for o, _, _ in calls], ptrs, [e for _, e, _ in calls], [st] * len(calls), np.uint16)
            assert rc == 0
            rows = [[int(x) for x in r] for r in stats]
            assert rows[0] == rows[1]
            for row, (o, e, at) in zip(rows, calls):
                assert row == _stats(_cut(full, o, e), _cut(buf, at, e)), (pipeline, subset, o, e)
        torch.cuda.synchronize()
        assert np.array_equal(d_buf.cpu().numpy(), buf)


@pytest.mark.parametrize("pipeline, dtype", SUBSET, ids=IDS)
def test_one_box_is_compare_batch_window(sqy, oracle, pipeline, dtype):
    """a cross-check beside the CPU's rows: row i of the one-blob call equals what SQYAMD_Compare_BatchWindow_* gives with the blob named
    once per box"""
    item = np.dtype(dtype).itemsize
    shape, d_blob, nbytes, full = _made(sqy, oracle, pipeline, dtype)[0]
    boxes = _all_boxes(shape, item)
    tiles = [_cut(full, o, e) for o, e in boxes]
    views = _planted(tiles)
    V = Views(dtype, [e for _, e in boxes], shift=item, pitch=True, salt=3)
    V.fill(views)
    rc, got = _call(sqy, d_blob, nbytes, boxes, V)
    rc2, tiled = sqy.compare_batch_window_device(d_blob.data_ptr(), [0] * len(boxes), [nbytes] * len(boxes), [o for o, _ in boxes], V.T.ptrs, V.T.extents, V.T.strides, dtype)
    assert rc == 0 and rc2 == 0
    assert got == [_stats(t, v) for t, v in zip(tiles, views)]
    assert got == [[int(x) for x in r] for r in tiled]
    for i in (0, len(boxes) // 2, len(boxes) - 1):                       # count = 1: the single box
        V1 = Views(dtype, [boxes[i][1]], shift=item, pitch=True)
        V1.fill(views[i:i + 1])
        assert _call(sqy, d_blob, nbytes, boxes[i:i + 1], V1) == (0, got[i:i + 1])


def test_after_update_box(sqy, options):
    """verify after write: SQYAMD_Update_Box_* of a box, then the box and two boxes around it against the pasted volume give NDIFF 0;
    against the old volume NDIFF is the CPU's count"""
    import torch
    from sqeazy_amd import synth
    shape = (16, 64, 64)
    name = "bitswap1->lz4" + SMALL_CHUNKS
    old = synth.stack(shape, np.uint16, seed=977)
    rc, blob = sqy.encode(name, old)
    assert rc == 0
    d_blob = _to_device(blob)
    o, e = (5, 7, 9), (3, 40, 33)
    box = (_cut(old, o, e) ^ np.uint16(0x0101)).copy()
    box[0, 0, :5] = _cut(old, o, e)[0, 0, :5]                            # (some voxels of the box keep their value)
    new = old.copy()
    new[tuple(slice(a, a + n) for a, n in zip(o, e))] = box
    d_box = torch.from_numpy(box.view(np.int16).copy()).to(_dev())
    cap = sqy.max_compressed_length(name, shape, np.uint16)
    out = torch.zeros(cap, dtype=torch.uint8, device=_dev())
    torch.cuda.synchronize()
    rc, n = sqy.update_box_device(name, d_blob.data_ptr(), len(blob), o, d_box.data_ptr(), e, None, np.uint16, out.data_ptr(), cap)
    assert rc == 0 and 0 < n <= cap
    boxes = [(o, e), ((4, 0, 0), (5, 64, 64)), ((0, 6, 8), (16, 42, 35))]
    for vol, changed in ((new, False), (old, True)):
        d_vol = torch.from_numpy(vol.view(np.int16).copy()).to(_dev())
        st = (64 * 64, 64, 1)
        ptrs = [d_vol.data_ptr() + 2 * sum(a * s for a, s in zip(bo, st)) for bo, _ in boxes]      # the boxes inside the resident volume itself
        for subset in (1, 0):
            options("compare_boxes_subset", subset)
            rc, stats = sqy.compare_boxes_device(out.data_ptr(), n, [bo for bo, _ in boxes], ptrs, [be for _, be in boxes], [st] * 3, np.uint16)
            assert rc == 0
            want = [_stats(_cut(new, bo, be), _cut(vol, bo, be)) for bo, be in boxes]
            assert [[int(x) for x in r] for r in stats] == want
            ndiff = [int(r[1]) for r in stats]
            assert ndiff == ([int(np.count_nonzero(box != _cut(old, o, e)))] * 3 if changed else [0, 0, 0]) and (ndiff[0] > 0) == changed


def test_refusals(sqy, oracle):
    """test_gpu_decode_boxes.test_refusals' table applied to ONE box of three in turn; 1, stats zeroed and all three views intact; then the
    good call"""
    shape = (3, 5, 7)
    blob, full = _blob(sqy, oracle, "bitswap1->lz4", shape, np.uint16)
    u8 = _blob(sqy, oracle, "bitswap1->lz4", shape, np.uint8)[0]
    d_blob, d_u8 = _to_device(blob), _to_device(u8)
    extents = [(2, 3, 4), (1, 5, 7), (2, 3, 4)]
    origins = [(1, 1, 1), (2, 0, 0), (0, 2, 3)]
    tiles = [_cut(full, o, e) for o, e in zip(origins, extents)]
    views = _planted(tiles)
    V = Views(np.uint16, extents, pitch=True)
    V.fill(views)
    T = V.T
    assert T.strides[0] == (26, 7, 1)
    dense = lambda e: (e[1] * e[2], e[2], 1)

    def call(k=None, src=d_blob.data_ptr(), n=len(blob), dtype=np.uint16, count=None, origins_=origins, **box):
        """box k with the fields of `box` in place of its own"""
        o, p, e, s = [list(origins_) if origins_ is not None else None, list(T.ptrs), list(extents), list(T.strides)]
        if k is not None:
            if "origin" in box: o[k] = box["origin"]
            if "view" in box: p[k] = box["view"]
            if "shape" in box: e[k] = box["shape"]
            if "strides" in box: s[k] = box["strides"]
        return sqy.compare_boxes_device(src, n, o, p, e, s, dtype, count=count)

    def refused_call(rc_stats):
        rc, stats = rc_stats
        assert rc == 1 and not stats.any(), (rc, stats)
        assert V.unchanged()

    def refused(**kw):
        for k in range(3):
            refused_call(call(k, **kw))
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
    refused(view=T.ptrs[0] + 1)                                         # a view off the voxel grid
    refused(view=None)                                                  # a NULL entry in d_views
    # what holds for the whole call: a rank other than the header's, a blob or an entry point of the other voxel type, NULL tables, no boxes
    refused_call(sqy.compare_boxes_device(d_blob.data_ptr(), len(blob), [(1, 1)] * 3, T.ptrs, [(3, 4)] * 3, [(7, 1)] * 3, np.uint16))
    refused_call(sqy.compare_boxes_device(d_blob.data_ptr(), len(blob), [(1,)] * 3, T.ptrs, [(4,)] * 3, [(1,)] * 3, np.uint16))
    refused_call(call(src=d_u8.data_ptr(), n=len(u8)))
    refused_call(call(dtype=np.uint8))
    refused_call(call(src=None))
    refused_call(call(n=0))
    refused_call(call(origins_=None))
    for count in (0, -1, -(2 ** 40)):
        refused_call(call(count=count))
    refused_call(sqy.compare_boxes_device(d_blob.data_ptr(), len(blob), origins, None, extents, T.strides, np.uint16))
    refused_call(sqy.compare_boxes_device(d_blob.data_ptr(), len(blob), origins, T.ptrs, None, None, np.uint16, count=3))
    L = sqy.lib()
    rows = lambda v: (ctypes.c_long * sum(len(r) for r in v))(*[x for r in v for x in r])
    ptrs = (ctypes.c_void_p * 3)(*T.ptrs)
    assert L.SQYAMD_Compare_Boxes_UI16_Device(d_blob.data_ptr(), len(blob), 3, rows(origins), ptrs, rows(extents), rows(T.strides), 3, None, None) == 1      # stats == NULL
    assert V.unchanged()
    # the good call: the table above refuses for its reasons
    want = [_stats(t, v) for t, v in zip(tiles, views)]
    rc, stats = call()
    assert rc == 0 and [[int(x) for x in r] for r in stats] == want and V.unchanged()
    # the host variant: views_bytes one byte off either way, the other type, a box outside, another rank, no boxes, stats == NULL
    src = np.frombuffer(blob, np.uint8)
    dense_views = np.concatenate([v.reshape(-1) for v in views])
    keep = dense_views.copy()
    total = dense_views.nbytes
    stats = np.zeros((3, 8), np.uint64)
    sp = stats.ctypes.data_as(ctypes.POINTER(ctypes.c_ulonglong))

    def host(fn, count, o, e, rank, nbytes, st=sp):
        stats[:] = 0xDEAD
        rc = fn(src.ctypes.data, len(blob), count, rows(o), rows(e), rank, dense_views.ctypes.data, nbytes, st)
        return rc, not stats[:max(count, 0)].any() if st else True
    assert host(L.SQYAMD_Compare_Boxes_UI16, 3, origins, extents, 3, total - 1) == (1, True)
    assert host(L.SQYAMD_Compare_Boxes_UI16, 3, origins, extents, 3, total + 1) == (1, True)
    assert host(L.SQYAMD_Compare_Boxes_UI8, 3, origins, extents, 3, total) == (1, True)
    assert host(L.SQYAMD_Compare_Boxes_UI16, 3, origins, extents[:2] + [(2, 3, 5)], 3, total + 12) == (1, True)
    assert host(L.SQYAMD_Compare_Boxes_UI16, 3, [(1, 1)] * 3, [(2, 3)] * 3, 2, 36) == (1, True)
    assert host(L.SQYAMD_Compare_Boxes_UI16, 0, origins, extents, 3, total) == (1, True)
    assert host(L.SQYAMD_Compare_Boxes_UI16, 3, origins, extents, 3, total, None) == (1, True)
    rc, ok = host(L.SQYAMD_Compare_Boxes_UI16, 3, origins, extents, 3, total)
    assert rc == 0 and [[int(x) for x in r] for r in stats] == want
    assert np.array_equal(dense_views, keep)


def test_host_variant_and_lower_ranks(sqy, oracle, options):
    """compare_boxes (host pointers, the views dense and back to back) gives the CPU's rows; blobs of rank 1 and 2: the frames are the first
    dimension"""
    for pipeline, dtype in (("bitswap1->lz4", np.uint16), ("lz4", np.uint8), ("quantiser->bitswap1->lz4", np.uint16), ("diff3x3x1->bitswap1->lz4", np.uint16)):
        blob, full = _blob(sqy, oracle, pipeline + (SMALL_CHUNKS if "diff" not in pipeline else ""), (7, 33, 31), dtype)
        boxes = _boxes((7, 33, 31), np.dtype(dtype).itemsize)
        tiles = [_cut(full, o, e) for o, e in boxes]
        views = _planted(tiles)
        want = [_stats(t, v) for t, v in zip(tiles, views)]
        for subset in (1, 0):
            options("compare_boxes_subset", subset)
            rc, stats = sqy.compare_boxes(blob, [o for o, _ in boxes], views)
            assert rc == 0 and [[int(x) for x in r] for r in stats] == want, (pipeline, subset)
    options("compare_boxes_subset", 1)
    from sqeazy_amd import synth
    cases = (((40, 300), [((3, 17), (30, 200)), ((39, 0), (1, 300)), ((0, 299), (40, 1))]), ((9000,), [((4100,), (4000,)), ((0,), (9000,)), ((8999,), (1,))]))
    for shape, boxes in cases:
        vol = synth.stack((1, 1, int(np.prod(shape))), np.uint16, seed=731).reshape(shape)
        tiles = [_cut(vol, o, e) for o, e in boxes]
        views = _planted(tiles)
        want = [_stats(t, v) for t, v in zip(tiles, views)]
        for pipeline in ("bitswap1->lz4" + SMALL_CHUNKS, "lz4" + SMALL_CHUNKS):
            rc, blob = sqy.encode(pipeline, vol)
            assert rc == 0
            d_blob = _to_device(blob)
            for pitch in (False, True):
                V = Views(np.uint16, [e for _, e in boxes], shift=2, pitch=pitch)
                V.fill(views)
                assert _call(sqy, d_blob, len(blob), boxes, V) == (0, want), (shape, pipeline, pitch)
                assert V.unchanged()


def test_work_queued_on_the_callers_stream_is_respected(sqy):
    """the blob and the views are written by copies queued on the caller's stream just before the call"""
    import torch
    from sqeazy_amd import synth
    dev = _dev()
    vol = synth.stack((16, 128, 160), np.uint16)
    rc, blob = sqy.encode("bitswap1->lz4", vol, nthreads=2)
    assert rc == 0
    host_blob = torch.from_numpy(np.frombuffer(blob, np.uint8).copy()).pin_memory()
    boxes = [((5, 3, 17), (8, 100, 120)), ((0, 0, 0), (2, 100, 120)), ((14, 28, 40), (2, 100, 120))]
    other = vol ^ np.uint16(1)
    other[6, 4, 18] = vol[6, 4, 18]
    host_vol = torch.from_numpy(other.view(np.int16).copy()).pin_memory()
    st = (128 * 160, 160, 1)
    want = [_stats(_cut(vol, o, e), _cut(other, o, e)) for o, e in boxes]
    s = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(s):
        d_blob = torch.empty(len(blob), dtype=torch.uint8, device=dev)
        d_vol = torch.empty(vol.shape, dtype=torch.int16, device=dev)
        for _ in range(2):
            d_blob.zero_()
            d_vol.fill_(7)
            d_blob.copy_(host_blob, non_blocking=True)
            d_vol.copy_(host_vol, non_blocking=True)
            ptrs = [d_vol.data_ptr() + 2 * sum(a * b for a, b in zip(o, st)) for o, _ in boxes]
            rc, stats = sqy.compare_boxes_device(d_blob.data_ptr(), len(blob), [o for o, _ in boxes], ptrs, [e for _, e in boxes], [st] * 3, np.uint16, stream=s.cuda_stream)
            assert rc == 0 and [[int(x) for x in r] for r in stats] == want


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
        tiles = [_cut(vols[i], o, (2, 100, 131)) for o in origins]
        views = _planted(tiles, k0=i)
        want = [_stats(t, v) for t, v in zip(tiles, views)]
        ok = True
        for _ in range(3):
            rc, stats = sqy.compare_boxes(blobs[i], origins, views)
            ok = ok and rc == 0 and [[int(x) for x in r] for r in stats] == want
        return ok
    with ThreadPoolExecutor(4) as ex:
        assert all(ex.map(one, range(4)))
