"""GPU: SQYAMD_Histogram_Boxes_* -- the intensity histograms of many boxes of ONE blob in one call: voxel v in bin v >> shift of
(65536 or 256) >> shift uint32 counters per box (include/sqeazy_amd.h).

Every histogram must be np.bincount((box >> shift).ravel(), minlength=nbins).astype(np.uint32) of SQY_Decode's volume of the blob
(test_gpu_decode_box's `full`, the oracle's decode; of the encoded volume where a test encodes a lossless one itself).  The code under
test is never the source of an expectation, integers are exact, there is no tolerance.  ALL boxes of a case go in ONE call; their
histograms lie in one buffer of position-dependent pattern bytes (test_gpu_batch_window.Targets with 32-bit elements and extents
(nbins,)), and the whole buffer and the blob are compared byte for byte after every call: a counter never zeroed, never stored or
counted twice, a byte around a histogram touched all show.  The subset paths (the counting range transposer, the window histogram in
the compaction) and the whole decode ("histogram_boxes_subset" = 0) give the same buffers, and each shows its launches in the profile
-- so none can stand in for another."""
import ctypes

import numpy as np
import pytest

from test_gpu_batch_window import Targets, _blob, _cut, _same
from test_gpu_bin_boxes import NEW_NAMES as BIN_NAMES
from test_gpu_compare_boxes import NEW_NAMES as COMPARE_NAMES, OTHERS
from test_gpu_decode_box import FALLBACK, SMALL_CHUNKS, SUBSET, _boxes, _case_blob, _launch_case, _made, _to_device
from test_gpu_decode_frames import _damaged, _lz4_frames, _profile_names
from test_gpu_project_boxes import NEW_NAMES as PROJECT_NAMES

pytestmark = pytest.mark.gpu

FINAL = {"bitswap1->lz4": "bitswap1_histogram_boxes", "rmestbkrd->bitswap1->lz4": "bitswap1_histogram_boxes",
         "quantiser->bitswap1->lz4": "bitswap1_quantiser_histogram_boxes", "lz4": "boxes_window_histogram", "frame_shuffle->lz4": "boxes_window_histogram"}
NEW_NAMES = set(FINAL.values())
INIT = "boxes_histogram_init"
IDS = ["%s-%s" % (p, np.dtype(d).name) for p, d in SUBSET]
SHIFTS = {2: (0, 1, 2, 6, 15), 1: (0, 3, 7)}
PLANTED = (0, 16383, 16384, 32767, 32768, 49151, 49152, 65535)


def _nbins(dtype, shift):
    return (65536 if np.dtype(dtype).itemsize == 2 else 256) >> shift


def _hist(tile, shift, dtype):
    """numpy's histogram of a box, as uint32"""
    h = np.bincount((tile.astype(np.int64) >> shift).ravel(), minlength=_nbins(dtype, shift))
    assert h.size == _nbins(dtype, shift) and int(h.sum()) == tile.size
    return h.astype(np.uint32)


def _call(sqy, d_blob, nbytes, boxes, shift, T, dtype, stream=None):
    return sqy.histogram_boxes_device(d_blob.data_ptr(), nbytes, [o for o, _ in boxes], [e for _, e in boxes], shift, T.ptrs, dtype, stream=stream)


def _targets(dtype, shift, n, off=0, salt=0):
    return Targets(np.uint32, [(_nbins(dtype, shift),)] * n, shift=off, salt=salt)


def _both(sqy, options, d_blob, nbytes, blob_host, boxes, shift, want, dtype, off=0, salt=0):
    """the call through the subset path and through the whole decode: the whole buffer byte for byte both times, and the two equal"""
    images = []
    for subset in (1, 0):
        options("histogram_boxes_subset", subset)
        T = _targets(dtype, shift, len(boxes), off, salt)
        rc = _call(sqy, d_blob, nbytes, boxes, shift, T, dtype)
        assert rc == 0, (boxes[0], shift, subset)
        got = T.read()
        _same(got, T.expect(want)[0])
        assert np.array_equal(d_blob.cpu().numpy(), blob_host), (shift, subset)
        images.append(got)
    assert np.array_equal(images[0], images[1])


def _values(sqy, oracle, options, pipeline, dtype, nthreads=0):
    item = np.dtype(dtype).itemsize
    made = _made(sqy, oracle, pipeline, dtype, nthreads)
    assert made
    for shape, d_blob, nbytes, full in made:
        blob_host = d_blob.cpu().numpy()
        boxes = _boxes(shape, item)
        assert any(tuple(e) == tuple(shape) for _, e in boxes) and len(boxes) > shape[0]
        tiles = [_cut(full, o, e) for o, e in boxes]
        for k, shift in enumerate(SHIFTS[item]):
            want = [_hist(t, shift, dtype) for t in tiles]                  # (numpy's histograms: once per shape and shift)
            _both(sqy, options, d_blob, nbytes, blob_host, boxes, shift, want, dtype, off=4 * (k % 2), salt=k)


@pytest.mark.parametrize("pipeline, dtype", SUBSET, ids=IDS)
def test_values(sqy, oracle, options, pipeline, dtype):
    """all boxes of every shape in one call, at every shift, the histograms' bases on and 4 bytes behind the 16-byte grid; through the
    subset path and the whole decode: the whole buffer byte for byte"""
    _values(sqy, oracle, options, pipeline, dtype)


@pytest.mark.parametrize("pipeline, dtype, nthreads", FALLBACK, ids=["%s%s" % (p, "-serial" if t else "") for p, _, t in FALLBACK])
def test_values_of_blobs_the_subset_path_does_not_take(sqy, oracle, options, pipeline, dtype, nthreads):
    _values(sqy, oracle, options, pipeline, dtype, nthreads)


@pytest.mark.parametrize("pipeline", ["bitswap1->lz4", "lz4"])
@pytest.mark.parametrize("halves", [False, True], ids=["uniform", "z-halves-in-two-quarters"])
def test_voxels_outside_the_lds_window(sqy, options, pipeline, halves):
    """(16, 128, 128) 16-bit voxels uniform over the whole range at shift 0 and 1: whatever window a workgroup votes for, most voxels miss
    it and go to the output one by one; `halves`: frames 0 .. 7 in the first quarter of the range and 8 .. 15 in the third, so the
    workgroups of one box vote differently; 0, 16383 | 16384, 32767 | 32768, 49151 | 49152 and 65535 planted in every frame"""
    shape = (16, 128, 128)
    rng = np.random.default_rng(41 + halves)
    vol = rng.integers(0, 65536, shape).astype(np.uint16)
    if halves:
        vol[:8] = rng.integers(0, 16384, (8, 128, 128)).astype(np.uint16)
        vol[8:] = rng.integers(32768, 49152, (8, 128, 128)).astype(np.uint16)
    for z in range(16):
        for k, v in enumerate(PLANTED):
            vol[z, 5 * k + z, 11 * k + 3] = v
            vol[z, 127 - k, z] = v
    rc, blob = sqy.encode(pipeline, vol)
    assert rc == 0
    rc, back = sqy.decode(blob)
    assert rc == 0 and np.array_equal(back, vol)
    d_blob = _to_device(blob)
    blob_host = d_blob.cpu().numpy()
    boxes = [((0, 0, 0), shape), ((3, 5, 7), (9, 100, 121)), ((7, 0, 0), (2, 128, 128)), ((0, 0, 0), (16, 128, 1)), ((15, 127, 0), (1, 1, 128))]
    tiles = [_cut(vol, o, e) for o, e in boxes]
    for shift in (0, 1):
        want = [_hist(t, shift, np.uint16) for t in tiles]
        assert all(int(want[0][v >> shift]) >= 1 for v in PLANTED)
        _both(sqy, options, d_blob, len(blob), blob_host, boxes, shift, want, np.uint16, salt=shift)


@pytest.mark.parametrize("pipeline", ["bitswap1->lz4", "lz4"])
def test_constant_volumes(sqy, options, pipeline):
    """all 0, all 0xFFFF and all 12345: one counter equals the box's voxel count -- for the whole (16, 128, 128) volume 8 workgroups add
    into it -- and every other counter is zero; with the histograms pre-filled with all ones and with zeros, so that a counter never
    stored, or never zeroed, shows either way"""
    import torch
    from test_gpu_batch_window import _dev
    shape = (16, 128, 128)
    boxes = [((0, 0, 0), shape), ((3, 5, 7), (9, 100, 121)), ((15, 0, 0), (1, 128, 128)), ((2, 2, 2), (1, 1, 1))]
    for fill in (0, 0xFFFF, 12345):
        vol = np.full(shape, fill, np.uint16)
        rc, blob = sqy.encode(pipeline, vol)
        assert rc == 0
        rc, back = sqy.decode(blob)
        assert rc == 0 and np.array_equal(back, vol)
        d_blob = _to_device(blob)
        for shift in (0, 1, 6, 15):
            nbins = _nbins(np.uint16, shift)
            want = [_hist(_cut(vol, o, e), shift, np.uint16) for o, e in boxes]
            assert int(want[0][fill >> shift]) == 16 * 128 * 128 and np.count_nonzero(want[0]) == 1
            for pre in (0xFFFFFFFF, 0):
                for subset in (1, 0):
                    options("histogram_boxes_subset", subset)
                    outs = [torch.full((nbins,), -1 if pre else 0, dtype=torch.int32, device=_dev()) for _ in boxes]
                    rc = sqy.histogram_boxes_device(d_blob.data_ptr(), len(blob), [o for o, _ in boxes], [e for _, e in boxes], shift, [t.data_ptr() for t in outs],
                                                    np.uint16)
                    assert rc == 0
                    torch.cuda.synchronize()
                    for t, w in zip(outs, want):
                        assert np.array_equal(t.cpu().numpy().view(np.uint32), w), (fill, shift, pre, subset)


@pytest.mark.parametrize("pipeline, dtype", [("bitswap1->lz4", np.uint16), ("bitswap1->lz4", np.uint8), ("quantiser->bitswap1->lz4", np.uint16), ("lz4", np.uint16)],
                         ids=["bitswap1->lz4-uint16", "bitswap1->lz4-uint8", "quantiser->bitswap1->lz4-uint16", "lz4-uint16"])
def test_the_three_merges_count_the_same(sqy, oracle, options, pipeline, dtype):
    """"histogram_boxes_merge" 0 (an add per voxel), 1 (equal neighbours of a thread's run in one add) and 2 (a piece of sixteen bytes whose
    bins are all equal in one add): numpy's histograms each time, on a stack with equal runs inside and across pieces and on a plain one"""
    item = np.dtype(dtype).itemsize
    shape = (16, 128, 128)
    blob, full = _blob(sqy, oracle, pipeline, shape, dtype)
    rng = np.random.default_rng(3)
    runs = np.repeat(rng.integers(0, 256 ** item, full.size // 8), 8)[rng.integers(0, 8):][:full.size - 8]      # runs of eight, off the pieces' grid
    runs = np.concatenate([runs, np.zeros(full.size - runs.size, np.int64)]).astype(dtype).reshape(shape)
    runs[4:8] = 777 % 256 ** item                                      # four constant frames
    cases = [(blob, full)]
    if "quantiser" not in pipeline:                                     # (lossless: the encoded volume is the expectation)
        rc, run_blob = sqy.encode(pipeline, runs)
        assert rc == 0
        rc, back = sqy.decode(run_blob)
        assert rc == 0 and np.array_equal(back, runs)
        cases.append((run_blob, runs))
    boxes = _boxes(shape, item)
    for b, vol in cases:
        d_blob = _to_device(b)
        tiles = [_cut(vol, o, e) for o, e in boxes]
        for shift in SHIFTS[item][:4:2] + SHIFTS[item][1:2]:
            want = [_hist(t, shift, dtype) for t in tiles]
            for merge in (0, 1, 2):
                options("histogram_boxes_merge", merge)
                for subset in (1, 0):
                    options("histogram_boxes_subset", subset)
                    T = _targets(dtype, shift, len(boxes), salt=merge)
                    assert _call(sqy, d_blob, len(b), boxes, shift, T, dtype) == 0
                    _same(T.read(), T.expect(want)[0])


@pytest.mark.parametrize("pipeline, dtype", SUBSET, ids=IDS)
def test_two_boxes_with_a_gap_of_unneeded_frames_between_them(sqy, oracle, options, pipeline, dtype):
    """frames {0} and {Z - 1}: the union's compaction has other frames' places missing between the two boxes' words; the same two the other
    way round; and with a box that reaches over both and one nested in it (overlapping boxes)"""
    seen = 0
    item = np.dtype(dtype).itemsize
    for shape, cfg in (((23, 131, 151), ""), ((16, 64, 64), SMALL_CHUNKS)):
        b = _case_blob(sqy, oracle, pipeline + cfg, shape, dtype)
        if b is None:                                                   # (a geometry the stage refuses at encode)
            continue
        seen += 1
        blob, full = b
        d_blob = _to_device(blob)
        blob_host = d_blob.cpu().numpy()
        Z, Y, X = shape
        ends = [((0, 1, 2), (1, Y - 2, X - 3)), ((Z - 1, 0, 0), (1, Y, X))]
        for boxes in (ends, ends[::-1], ends + [((0, 3, 1), (Z, 5, X - 1)), ((Z // 2, 0, 0), (2, Y, 9))]):
            tiles = [_cut(full, o, e) for o, e in boxes]
            for k, shift in enumerate(SHIFTS[item][:3]):
                _both(sqy, options, d_blob, len(blob), blob_host, boxes, shift, [_hist(t, shift, dtype) for t in tiles], dtype, off=4 * (k % 2), salt=k)
    assert seen >= 1


@pytest.mark.parametrize("pipeline, dtype", SUBSET, ids=IDS)
def test_launches(sqy, oracle, options, pipeline, dtype):
    """the subset path: ONE pruned LZ4 launch, ONE init and ONE launch under the path's own name for K boxes -- none of the decode, compare,
    project or bin finals; the option off: the whole blob once and one boxes_window_histogram; SQYAMD_Decode_Boxes_*,
    SQYAMD_Compare_Boxes_*, SQYAMD_Project_Boxes_* and SQYAMD_Bin_Boxes_* launch what they launched"""
    shape, blob, full = _launch_case(sqy, oracle, pipeline, dtype)
    d_blob = _to_device(blob)
    Z = shape[0]
    boxes = [((Z // 2, 1, 1), (1, shape[1] - 2, shape[2] - 2)), ((0, 0, 3), (Z, shape[1], 5)), ((0, 2, 0), (1, 7, shape[2])), ((Z - 1, 0, 0), (1, shape[1], shape[2]))]

    def decode_boxes():
        T = Targets(dtype, [e for _, e in boxes], pitch=True)
        assert sqy.decode_boxes_device(d_blob.data_ptr(), len(blob), [o for o, _ in boxes], T.ptrs, T.extents, T.strides, dtype) == 0
        T.read()

    def compare_boxes():
        T = Targets(dtype, [e for _, e in boxes], pitch=True)
        rc, _ = sqy.compare_boxes_device(d_blob.data_ptr(), len(blob), [o for o, _ in boxes], T.ptrs, T.extents, T.strides, dtype)
        assert rc == 0

    def project_boxes():
        T = Targets(np.uint32, [e[1:] for _, e in boxes], pitch=True)
        assert sqy.project_boxes_device(d_blob.data_ptr(), len(blob), [o for o, _ in boxes], [e for _, e in boxes], 0, "max", T.ptrs, T.strides, dtype) == 0
        T.read()

    def bin_boxes():
        T = Targets(np.uint32, [tuple(-(-n // 2) for n in e) for _, e in boxes], pitch=True)
        assert sqy.bin_boxes_device(d_blob.data_ptr(), len(blob), [o for o, _ in boxes], [e for _, e in boxes], (2, 2, 2), "max", T.ptrs, T.strides, dtype) == 0
        T.read()
    callers = (decode_boxes, compare_boxes, project_boxes, bin_boxes)
    before = [_profile_names(sqy, f) for f in callers]

    def profiled(bx, shift):
        T = _targets(dtype, shift, len(bx), off=4)
        rcs = []
        sqy.profile_reset()
        sqy.profile_enable(True)
        try:
            rcs.append(_call(sqy, d_blob, len(blob), bx, shift, T, dtype))
        finally:
            sqy.profile_enable(False)
        prof = sqy.profile_get()
        sqy.profile_reset()
        assert rcs == [0]
        _same(T.read(), T.expect([_hist(_cut(full, o, e), shift, dtype) for o, e in bx])[0])
        return prof
    others = ("batch_compare_init", "boxes_project_init") + OTHERS + tuple(COMPARE_NAMES) + tuple(PROJECT_NAMES) + tuple(BIN_NAMES)
    for k, shift in ((3, 0), (4, 2), (4, SHIFTS[np.dtype(dtype).itemsize][-1])):
        prof = profiled(boxes[:k], shift)
        names = set(prof)
        assert "lz4_frames_subset_decode" in names and prof["lz4_frames_subset_decode"][1] == 1, prof
        assert prof[INIT][1] == 1 and prof[FINAL[pipeline]][1] == 1 and sum(n in names for n in NEW_NAMES) == 1, prof
        assert not any(n in names for n in ("lz4_frames_decode",) + others), names
    options("histogram_boxes_subset", 0)
    prof = profiled(boxes, 2)
    names = set(prof)
    assert "lz4_frames_decode" in names and prof["lz4_frames_decode"][1] == 1 and prof["boxes_window_histogram"][1] == 1 and prof[INIT][1] == 1, prof
    assert not any(n in names for n in ("lz4_frames_subset_decode", "bitswap1_histogram_boxes", "bitswap1_quantiser_histogram_boxes", "batch_compare_init",
                                        "boxes_project_init", "boxes_window_copy", "boxes_window_compare", "batch_window_compare", "boxes_window_project",
                                        "boxes_window_bin")), names
    options("histogram_boxes_subset", 1)
    after = [_profile_names(sqy, f) for f in callers]
    assert before == after, (before, after)
    assert not any(n in s for s in before for n in NEW_NAMES | {INIT}), before


@pytest.mark.parametrize("pipeline", ["lz4", "bitswap1->lz4"])
def test_damaged_frame(sqy, options, pipeline):
    """pruning is real: the last compressed LZ4 frame damaged -- boxes in frames 0 and 3 do not need it: rc 0 and right histograms on the
    subset path; with a box in frame 15 added both option settings give the full decode's code; nothing outside the histograms is written
    and the blob keeps its bytes both times"""
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
    for shift in (0, 2, 6):
        want = [_hist(_cut(vol, o, e), shift, np.uint16) for o, e in boxes]
        T = _targets(np.uint16, shift, len(boxes), off=4)
        rcs = []
        names = _profile_names(sqy, lambda: rcs.append(_call(sqy, d_bad, len(bad), boxes, shift, T, np.uint16)))
        assert "lz4_frames_subset_decode" in names and "lz4_frames_decode" not in names, names
        assert rcs == [0]
        _same(T.read(), T.expect(want)[0])
    rc, hists = sqy.histogram_boxes(bad, [o for o, _ in boxes], [e for _, e in boxes], 2)
    assert rc == 0 and all(np.array_equal(g, _hist(_cut(vol, o, e), 2, np.uint16)) for g, (o, e) in zip(hists, boxes))
    for subset in (1, 0):
        options("histogram_boxes_subset", subset)
        T = _targets(np.uint16, 2, len(more))
        assert _call(sqy, d_bad, len(bad), more, 2, T, np.uint16) == rc_full, subset
        _, mask = T.expect([np.zeros(_nbins(np.uint16, 2), np.uint32)] * len(more), skip=range(len(more)))
        _same(T.read(), T.host, mask)                                   # (the histograms may hold anything; nothing outside them is written)
        rc, hists = sqy.histogram_boxes(bad, [o for o, _ in more], [e for _, e in more], 2)
        assert rc == rc_full and hists is None
    assert np.array_equal(d_bad.cpu().numpy(), bad_host)


def test_refusals(sqy, oracle):
    """each applied to ONE box of three in turn where it is a box's: 1 with all three histograms and the canaries around them intact; then
    the good call"""
    shape = (3, 5, 7)
    blob, full = _blob(sqy, oracle, "bitswap1->lz4", shape, np.uint16)
    u8, full8 = _blob(sqy, oracle, "bitswap1->lz4", shape, np.uint8)
    d_blob, d_u8 = _to_device(blob), _to_device(u8)
    extents = [(2, 3, 4), (1, 5, 7), (2, 3, 4)]
    origins = [(1, 1, 1), (2, 0, 0), (0, 2, 3)]
    boxes = list(zip(origins, extents))
    SHIFT = 6
    T = _targets(np.uint16, SHIFT, 3)

    def call(k=None, src=d_blob.data_ptr(), n=len(blob), dtype=np.uint16, count=None, shift=SHIFT, ptrs="T", **box):
        """box k with the fields of `box` in place of its own"""
        o, p, e = list(origins), (list(T.ptrs) if ptrs == "T" else ptrs), list(extents)
        if k is not None:
            if "origin" in box: o[k] = box["origin"]
            if "out" in box: p[k] = box["out"]
            if "shape" in box: e[k] = box["shape"]
        return sqy.histogram_boxes_device(src, n, o, e, shift, p, dtype, count=count)

    def refused_call(rc):
        assert rc == 1, rc
        _same(T.read(), T.host)

    def refused(**kw):
        for k in range(3):
            refused_call(call(k, **kw))
    for shift in (16, -1, 17, 2 ** 31 - 1, -(2 ** 31)):                 # shift outside [0, 16)
        refused_call(call(shift=shift))
    refused_call(call(src=d_u8.data_ptr(), n=len(u8), dtype=np.uint8, shift=8))      # .. outside [0, 8) at 8 bits
    refused_call(call(ptrs=None))                                       # d_hists NULL
    for count in (0, -1, -(2 ** 40)):
        refused_call(call(count=count))
    refused(out=None)                                                   # a NULL entry
    for off in (1, 2, 3):
        refused(out=T.ptrs[0] + off)                                    # a histogram off the 4-byte grid
    refused_call(call(src=d_u8.data_ptr(), n=len(u8)))                  # a blob of the other voxel type
    refused_call(call(dtype=np.uint8))                                  # .. an entry point of the other type
    refused(origin=(0, -1, 0))
    refused(shape=(2, 0, 4))
    for d in range(3):                                                  # origin + extent one voxel past the shape, each dimension in turn
        e = [2, 4, 6]
        e[d] += 1
        refused(origin=(1, 1, 1), shape=tuple(e))
        o = [0, 0, 0]
        o[d] = 2 ** 63 - 1
        refused(origin=tuple(o), shape=(1, 1, 1))                       # no wrap to a small sum
    # a rank other than the header's
    refused_call(sqy.histogram_boxes_device(d_blob.data_ptr(), len(blob), [(1, 1)] * 3, [(3, 4)] * 3, SHIFT, T.ptrs, np.uint16))
    refused_call(call(src=None))
    refused_call(call(n=0))
    for shift in (SHIFT, 0, 15):
        Tg = _targets(np.uint16, shift, 3, off=4)
        assert _call(sqy, d_blob, len(blob), boxes, shift, Tg, np.uint16) == 0
        _same(Tg.read(), Tg.expect([_hist(_cut(full, o, e), shift, np.uint16) for o, e in boxes])[0])
    for shift in (0, 7):
        Tg = _targets(np.uint8, shift, 3)
        assert _call(sqy, d_u8, len(u8), boxes, shift, Tg, np.uint8) == 0
        _same(Tg.read(), Tg.expect([_hist(_cut(full8, o, e), shift, np.uint8) for o, e in boxes])[0])
    # the host variant: a capacity one byte short, the other type, a box outside
    L = sqy.lib()
    rows = lambda v: (ctypes.c_long * sum(len(r) for r in v))(*[x for r in v for x in r])
    src = np.frombuffer(blob, np.uint8)
    out = np.full(3 * _nbins(np.uint16, SHIFT), 0xA5A5A5A5, np.uint32)
    for fn, o, e, nbytes in ((L.SQYAMD_Histogram_Boxes_UI16, origins, extents, out.nbytes - 1), (L.SQYAMD_Histogram_Boxes_UI8, origins, extents, out.nbytes),
                             (L.SQYAMD_Histogram_Boxes_UI16, origins, extents[:2] + [(2, 3, 5)], out.nbytes)):
        assert fn(src.ctypes.data, len(blob), 3, rows(o), rows(e), 3, SHIFT, out.ctypes.data, nbytes) == 1
        assert (out == 0xA5A5A5A5).all()
    assert L.SQYAMD_Histogram_Boxes_UI16(src.ctypes.data, len(blob), 3, rows(origins), rows(extents), 3, SHIFT, out.ctypes.data, out.nbytes) == 0
    assert np.array_equal(out, np.concatenate([_hist(_cut(full, o, e), SHIFT, np.uint16) for o, e in boxes]))


def test_host_variant_and_lower_ranks(sqy, oracle, options):
    """histogram_boxes (host pointers, the histograms dense and back to back) gives what the device variant gives and numpy's histograms;
    blobs of rank 1 and 2: the frames are the first dimension"""
    for pipeline, dtype in (("bitswap1->lz4", np.uint16), ("lz4", np.uint8), ("quantiser->bitswap1->lz4", np.uint16), ("diff3x3x1->bitswap1->lz4", np.uint16)):
        blob, full = _blob(sqy, oracle, pipeline + (SMALL_CHUNKS if "diff" not in pipeline else ""), (7, 33, 31), dtype)
        d_blob = _to_device(blob)
        item = np.dtype(dtype).itemsize
        boxes = _boxes((7, 33, 31), item)
        origins, extents = [o for o, _ in boxes], [e for _, e in boxes]
        tiles = [_cut(full, o, e) for o, e in boxes]
        for subset in (1, 0):
            options("histogram_boxes_subset", subset)
            for shift in SHIFTS[item]:
                rc, hists = sqy.histogram_boxes(blob, origins, extents, shift)
                assert rc == 0 and all(g.dtype == np.uint32 and g.shape == (_nbins(dtype, shift),) for g in hists)
                assert all(np.array_equal(g, _hist(t, shift, dtype)) for g, t in zip(hists, tiles)), (pipeline, subset, shift)
                T = _targets(dtype, shift, len(boxes))
                assert _call(sqy, d_blob, len(blob), boxes, shift, T, dtype) == 0
                got = T.read()
                assert all(np.array_equal(got[T.bytes_of(i)].view(np.uint32)[..., 0], g) for i, g in enumerate(hists))
    options("histogram_boxes_subset", 1)
    assert sqy.histogram_boxes(blob, origins, extents, 16) == (1, None) and sqy.histogram_boxes(blob, origins, extents, -1) == (1, None)
    from sqeazy_amd import synth
    cases = (((40, 300), [((3, 17), (30, 200)), ((39, 0), (1, 300)), ((0, 299), (40, 1))]), ((9000,), [((4100,), (4000,)), ((0,), (9000,)), ((8999,), (1,))]))
    for shape, boxes in cases:
        vol = synth.stack((1, 1, int(np.prod(shape))), np.uint16, seed=731).reshape(shape)
        tiles = [_cut(vol, o, e) for o, e in boxes]
        for pipeline in ("bitswap1->lz4" + SMALL_CHUNKS, "lz4" + SMALL_CHUNKS):
            rc, blob = sqy.encode(pipeline, vol)
            assert rc == 0
            d_blob = _to_device(blob)
            for shift in (0, 2, 15):
                want = [_hist(t, shift, np.uint16) for t in tiles]
                T = _targets(np.uint16, shift, len(boxes), off=4)
                assert _call(sqy, d_blob, len(blob), boxes, shift, T, np.uint16) == 0, (shape, pipeline, shift)
                _same(T.read(), T.expect(want)[0])
                rc, hists = sqy.histogram_boxes(blob, [o for o, _ in boxes], [e for _, e in boxes], shift)
                assert rc == 0 and all(np.array_equal(g, w) for g, w in zip(hists, want))


def test_quantiles_of_a_box(sqy, oracle):
    """the percentiles a display range is set from: histogram_quantile on the library's histogram against numpy's nearest rank on the box"""
    import math
    blob, full = _blob(sqy, oracle, "bitswap1->lz4" + SMALL_CHUNKS, (7, 33, 31), np.uint16)
    box = ((1, 2, 3), (5, 30, 20))
    tile = np.sort(_cut(full, *box).ravel())
    for shift in (0, 4):
        rc, (h,) = sqy.histogram_boxes(blob, [box[0]], [box[1]], shift)
        assert rc == 0
        for q in (0.0, 0.01, 0.5, 0.99, 1.0):
            assert sqy.histogram_quantile(h, q, shift) == int(tile[max(1, math.ceil(q * tile.size)) - 1]) >> shift << shift, (shift, q)
