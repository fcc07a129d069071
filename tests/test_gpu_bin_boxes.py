"""GPU: SQYAMD_Bin_Boxes_* -- many boxes of ONE blob read at a coarser resolution in one call: cells of `bins` voxels reduced by max, min or
sum into uint32 outputs of the boxes' rank (include/sqeazy_amd.h).

Every output must be what numpy computes from SQY_Decode's volume of the blob (test_gpu_decode_box's `full`, the oracle's decode):
ufunc.reduceat along every axis at the cells' first voxels -- np.maximum, np.minimum, np.add in 64 bits, cast to uint32 after asserting the
sum is below 2^32.  The code under test is never the source of an expectation, integers are exact, there is no tolerance.  ALL boxes of a
case go in ONE call; their outputs lie in one buffer of position-dependent pattern bytes (test_gpu_batch_window.Targets with 32-bit
elements), and the whole buffer and the blob are compared byte for byte after every call: a cell missed, a gap between pitched rows
touched, a cell left at its neutral element all show.  The subset paths (the binning kernel with its LDS accumulators, the per-cell launch
in the compaction) and the whole decode ("bin_boxes_subset" = 0) give the same outputs, and each shows its launches in the profile -- so
none can stand in for another."""
import numpy as np
import pytest

from test_gpu_batch_window import Targets, _blob, _cut, _dev, _same
from test_gpu_compare_boxes import NEW_NAMES as COMPARE_NAMES, OTHERS
from test_gpu_decode_box import FALLBACK, SMALL_CHUNKS, SUBSET, _boxes, _case_blob, _launch_case, _made, _to_device
from test_gpu_decode_frames import _damaged, _lz4_frames, _profile_names
from test_gpu_project_boxes import LAYOUTS, NEW_NAMES as PROJECT_NAMES, OPS, _reduce

pytestmark = pytest.mark.gpu

FINAL = {"bitswap1->lz4": "bitswap1_bin_boxes", "rmestbkrd->bitswap1->lz4": "bitswap1_bin_boxes", "quantiser->bitswap1->lz4": "bitswap1_quantiser_bin_boxes",
         "lz4": "boxes_window_bin", "frame_shuffle->lz4": "boxes_window_bin"}
NEW_NAMES = set(FINAL.values())
IDS = ["%s-%s" % (p, np.dtype(d).name) for p, d in SUBSET]
BINS = ((1, 1, 1), (2, 2, 2), (3, 5, 7), (1, 1, 32), (1, 1, 128), (2, 1, 1), (1000, 1, 1), (1, 1000, 1), (1, 1, 1000))
UFUNC = {"max": np.maximum, "min": np.minimum, "sum": np.add}


def _bin(tile, bins, op):
    """numpy's binning of a box, as uint32: reduceat along every axis at the cells' first voxels (the last cell takes what is left)"""
    r = tile.astype(np.uint64) if op == "sum" else tile
    for ax, b in enumerate(bins):
        r = UFUNC[op].reduceat(r, np.arange(0, r.shape[ax], b), axis=ax)
    assert (r < 2 ** 32).all()
    return r.astype(np.uint32)


def _cells(boxes, bins):
    """the outputs' extents: ceil(extent / bins)"""
    return [tuple(-(-n // b) for n, b in zip(e, bins)) for _, e in boxes]


def _call(sqy, d_blob, nbytes, boxes, bins, op, T, dtype, stream=None):
    return sqy.bin_boxes_device(d_blob.data_ptr(), nbytes, [o for o, _ in boxes], [e for _, e in boxes], bins, op, T.ptrs, T.strides, dtype, stream=stream)


def _values(sqy, oracle, options, pipeline, dtype, nthreads=0):
    item = np.dtype(dtype).itemsize
    made = _made(sqy, oracle, pipeline, dtype, nthreads)
    assert made
    for shape, d_blob, nbytes, full in made:
        blob_host = d_blob.cpu().numpy()
        boxes = _boxes(shape, item)
        assert any(tuple(e) == tuple(shape) for _, e in boxes) and len(boxes) > shape[0]
        tiles = [_cut(full, o, e) for o, e in boxes]
        for k, bins in enumerate(BINS):
            extents = _cells(boxes, bins)
            for j, op in enumerate(OPS):
                want = [_bin(t, bins, op) for t in tiles]                    # (numpy's outputs: once per shape, bins and op)
                assert [w.shape for w in want] == extents
                # every op dense and pitched, on and 4 bytes behind the 16-byte grid; over the bins and ops all four combinations
                for shift, pitch in (LAYOUTS[(k + j) % 4], LAYOUTS[(k + j + 1) % 4]):
                    images = []
                    for subset in (1, 0):
                        options("bin_boxes_subset", subset)
                        T = Targets(np.uint32, extents, shift=shift, pitch=pitch, salt=7 * shift + pitch + 2 * k)
                        rc = _call(sqy, d_blob, nbytes, boxes, bins, op, T, dtype)
                        assert rc == 0, (shape, bins, op, shift, pitch, subset)
                        got = T.read()
                        _same(got, T.expect(want)[0])
                        assert np.array_equal(d_blob.cpu().numpy(), blob_host), (shape, bins, op, subset)
                        images.append(got)
                    assert np.array_equal(images[0], images[1])


@pytest.mark.parametrize("pipeline, dtype", SUBSET, ids=IDS)
def test_values(sqy, oracle, options, pipeline, dtype):
    """all boxes of every shape in one call; each of the bins x each op; the outputs dense and pitched, their bases on and 4 bytes behind
    the 16-byte grid; through the subset path and the whole decode: the whole buffer byte for byte"""
    _values(sqy, oracle, options, pipeline, dtype)


@pytest.mark.parametrize("pipeline, dtype, nthreads", FALLBACK, ids=["%s%s" % (p, "-serial" if t else "") for p, _, t in FALLBACK])
def test_values_of_blobs_the_subset_path_does_not_take(sqy, oracle, options, pipeline, dtype, nthreads):
    _values(sqy, oracle, options, pipeline, dtype, nthreads)


@pytest.mark.parametrize("pipeline, dtype", [("bitswap1->lz4", np.uint16), ("quantiser->bitswap1->lz4", np.uint16), ("lz4", np.uint8), ("bitswap1->lz4", np.uint8)])
def test_the_two_identities(sqy, oracle, options, pipeline, dtype):
    """bins of all ones: Decode_Boxes' voxels, widened; bins[axis] = 1000 with ones elsewhere: Project_Boxes' image with a kept dimension of
    1 -- against the library's own two calls, which their own tests hold against numpy"""
    for shape, cfg in (((7, 33, 31), SMALL_CHUNKS), ((16, 128, 128), "")):
        blob, full = _blob(sqy, oracle, pipeline + cfg, shape, dtype)
        d_blob = _to_device(blob)
        boxes = _boxes(shape, np.dtype(dtype).itemsize)
        origins, extents = [o for o, _ in boxes], [e for _, e in boxes]
        rc, voxels = sqy.decode_boxes(blob, origins, extents)
        assert rc == 0
        for subset in (1, 0):
            options("bin_boxes_subset", subset)
            for op in OPS:
                T = Targets(np.uint32, extents, shift=4, pitch=True)
                assert _call(sqy, d_blob, len(blob), boxes, (1, 1, 1), op, T, dtype) == 0
                _same(T.read(), T.expect([v.astype(np.uint32) for v in voxels])[0])
            for axis in range(3):
                bins = tuple(1000 if k == axis else 1 for k in range(3))
                for op in OPS:
                    rc, images = sqy.project_boxes(blob, origins, extents, axis, op)
                    assert rc == 0
                    T = Targets(np.uint32, _cells(boxes, bins), pitch=bool(axis % 2))
                    assert _call(sqy, d_blob, len(blob), boxes, bins, op, T, dtype) == 0
                    _same(T.read(), T.expect([np.expand_dims(im, axis) for im in images])[0])


@pytest.mark.parametrize("pipeline", ["bitswap1->lz4", "lz4"])
def test_neutral_elements(sqy, options, pipeline):
    """all 0xFFFF: min = 65535 and sum = 65535 V; all 0: max = 0 -- with the outputs pre-filled with all ones and with zeros, so a cell that
    is left at a neutral element, or never stored, shows either way"""
    import torch
    shape = (16, 128, 128)
    boxes = [((0, 0, 0), shape), ((3, 5, 7), (9, 100, 121)), ((15, 0, 0), (1, 128, 128))]
    for fill in (0xFFFF, 0):
        vol = np.full(shape, fill, np.uint16)
        rc, blob = sqy.encode(pipeline, vol)
        assert rc == 0
        d_blob = _to_device(blob)
        for bins in ((2, 2, 2), (3, 5, 7), (16, 1, 128), (1, 128, 1)):
            want = {op: [_bin(_cut(vol, o, e), bins, op) for o, e in boxes] for op in OPS}
            if fill:
                assert int(want["min"][0][0, 0, 0]) == 65535 and int(want["sum"][0][0, 0, 0]) == 65535 * int(np.prod(bins))
            for pre in (0xFFFFFFFF, 0):
                for subset in (1, 0):
                    options("bin_boxes_subset", subset)
                    for op in OPS:
                        outs = [torch.full(tuple(w.shape), pre - 2 ** 32 if pre else 0, dtype=torch.int64, device=_dev()).to(torch.int32) for w in want[op]]
                        rc = sqy.bin_boxes_device(d_blob.data_ptr(), len(blob), [o for o, _ in boxes], [e for _, e in boxes], bins, op, [t.data_ptr() for t in outs], None,
                                                  np.uint16)
                        assert rc == 0
                        torch.cuda.synchronize()
                        for t, w in zip(outs, want[op]):
                            assert np.array_equal(t.cpu().numpy().view(np.uint32), w), (fill, bins, pre, subset, op)


def test_the_sum_bound_on_the_device(sqy, options):
    """(16, 64, 65) maximal 16-bit voxels, 133 KB: cells of 16 x 64 x 64 = 65536 voxels sum to 65535 x 65536 exactly (the partial cell behind
    them to 65535 x 1024); cells of 16 x 64 x 65 return 1 with the canaries intact; max and min have no bound"""
    shape = (16, 64, 65)
    vol = np.full(shape, 0xFFFF, np.uint16)
    rc, blob = sqy.encode("bitswap1->lz4", vol)
    assert rc == 0
    d_blob = _to_device(blob)
    box = [((0, 0, 0), shape)]
    for subset in (1, 0):
        options("bin_boxes_subset", subset)
        T = Targets(np.uint32, [(1, 1, 2)], shift=4)
        assert _call(sqy, d_blob, len(blob), box, (16, 64, 64), "sum", T, np.uint16) == 0
        _same(T.read(), T.expect([np.array([[[65535 * 65536, 65535 * 16 * 64]]], np.uint32)])[0])
        T = Targets(np.uint32, [(1, 1, 1)], shift=4)
        assert _call(sqy, d_blob, len(blob), box, (16, 64, 65), "sum", T, np.uint16) == 1
        _same(T.read(), T.host)
        for op in ("max", "min"):
            T = Targets(np.uint32, [(1, 1, 1)])
            assert _call(sqy, d_blob, len(blob), box, (16, 64, 65), op, T, np.uint16) == 0
            _same(T.read(), T.expect([np.full((1, 1, 1), 65535, np.uint32)])[0])


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
            for k, bins in enumerate(((2, 2, 2), (1, 3, 5), (4, 1, 32))):
                for j, op in enumerate(OPS):
                    want = [_bin(t, bins, op) for t in tiles]
                    for subset in (1, 0):
                        options("bin_boxes_subset", subset)
                        T = Targets(np.uint32, _cells(boxes, bins), shift=4 * (j % 2), pitch=bool(k % 2) ^ bool(subset), salt=k + j)
                        assert _call(sqy, d_blob, len(blob), boxes, bins, op, T, dtype) == 0
                        _same(T.read(), T.expect(want)[0])
    assert seen >= 1


@pytest.mark.parametrize("pipeline, dtype", SUBSET, ids=IDS)
def test_launches(sqy, oracle, options, pipeline, dtype):
    """the subset path: ONE pruned LZ4 launch and ONE launch under the path's own name for K boxes -- no projection init, none of the decode,
    compare, copy or project finals; the option off: the whole blob once and one boxes_window_bin; SQYAMD_Decode_Boxes_*,
    SQYAMD_Compare_Boxes_* and SQYAMD_Project_Boxes_* launch what they launched"""
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
    before = [_profile_names(sqy, f) for f in (decode_boxes, compare_boxes, project_boxes)]

    def profiled(bx, bins, op, pitch):
        T = Targets(np.uint32, _cells(bx, bins), shift=4, pitch=pitch)
        rcs = []
        sqy.profile_reset()
        sqy.profile_enable(True)
        try:
            rcs.append(_call(sqy, d_blob, len(blob), bx, bins, op, T, dtype))
        finally:
            sqy.profile_enable(False)
        prof = sqy.profile_get()
        sqy.profile_reset()
        assert rcs == [0]
        _same(T.read(), T.expect([_bin(_cut(full, o, e), bins, op) for o, e in bx])[0])
        return prof
    for k, bins, op in ((3, (2, 2, 2), "max"), (4, (1, 4, 4), "min"), (4, (3, 1, 32), "sum")):
        prof = profiled(boxes[:k], bins, op, True)
        names = set(prof)
        assert "lz4_frames_subset_decode" in names and prof["lz4_frames_subset_decode"][1] == 1, prof
        assert prof[FINAL[pipeline]][1] == 1 and sum(n in names for n in NEW_NAMES) == 1, prof
        assert not any(n in names for n in ("lz4_frames_decode", "batch_compare_init", "boxes_project_init") + OTHERS + tuple(COMPARE_NAMES) + tuple(PROJECT_NAMES)), names
    options("bin_boxes_subset", 0)
    prof = profiled(boxes, (2, 2, 2), "max", True)
    names = set(prof)
    assert "lz4_frames_decode" in names and prof["boxes_window_bin"][1] == 1, prof
    assert not any(n in names for n in ("lz4_frames_subset_decode", "bitswap1_bin_boxes", "bitswap1_quantiser_bin_boxes", "boxes_project_init", "boxes_window_copy",
                                        "boxes_window_compare", "batch_window_compare", "boxes_window_project")), names
    options("bin_boxes_subset", 1)
    after = [_profile_names(sqy, f) for f in (decode_boxes, compare_boxes, project_boxes)]
    assert before == after, (before, after)
    assert not any(n in s for s in before for n in NEW_NAMES), before


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
    for bins in ((1, 2, 2), (1, 3, 7)):
        for op in OPS:
            want = [_bin(_cut(vol, o, e), bins, op) for o, e in boxes]
            T = Targets(np.uint32, _cells(boxes, bins), shift=4, pitch=True)
            rcs = []
            names = _profile_names(sqy, lambda: rcs.append(_call(sqy, d_bad, len(bad), boxes, bins, op, T, np.uint16)))
            assert "lz4_frames_subset_decode" in names and "lz4_frames_decode" not in names, names
            assert rcs == [0]
            _same(T.read(), T.expect(want)[0])
    rc, cells = sqy.bin_boxes(bad, [o for o, _ in boxes], [e for _, e in boxes], (1, 2, 2), "sum")
    assert rc == 0 and all(np.array_equal(g, _bin(_cut(vol, o, e), (1, 2, 2), "sum")) for g, (o, e) in zip(cells, boxes))
    for subset in (1, 0):
        options("bin_boxes_subset", subset)
        T = Targets(np.uint32, _cells(more, (1, 2, 2)), pitch=True)
        assert _call(sqy, d_bad, len(bad), more, (1, 2, 2), "max", T, np.uint16) == rc_full, subset
        _, mask = T.expect([np.zeros(x, np.uint32) for x in _cells(more, (1, 2, 2))], skip=range(len(more)))
        _same(T.read(), T.host, mask)                                   # (the outputs may hold anything; nothing outside them is written)
        rc, cells = sqy.bin_boxes(bad, [o for o, _ in more], [e for _, e in more], (1, 2, 2), "max")
        assert rc == rc_full and cells is None
    assert np.array_equal(d_bad.cpu().numpy(), bad_host)


def test_refusals(sqy, oracle):
    """each applied to ONE box of three in turn where it is a box's: 1 with all three outputs and the canaries around them intact; then the
    good call"""
    shape = (3, 5, 7)
    blob, full = _blob(sqy, oracle, "bitswap1->lz4", shape, np.uint16)
    u8 = _blob(sqy, oracle, "bitswap1->lz4", shape, np.uint8)[0]
    d_blob, d_u8 = _to_device(blob), _to_device(u8)
    extents = [(2, 3, 4), (1, 5, 7), (2, 3, 4)]
    origins = [(1, 1, 1), (2, 0, 0), (0, 2, 3)]
    boxes = list(zip(origins, extents))
    BIN = (2, 2, 3)
    T = Targets(np.uint32, _cells(boxes, BIN), pitch=True)
    assert T.extents[0] == (1, 2, 2) and T.strides[0] == (15, 5, 1)

    def call(k=None, src=d_blob.data_ptr(), n=len(blob), dtype=np.uint16, count=None, bins=BIN, op="max", **box):
        """box k with the fields of `box` in place of its own"""
        o, p, e, s = list(origins), list(T.ptrs), list(extents), list(T.strides)
        if k is not None:
            if "origin" in box: o[k] = box["origin"]
            if "out" in box: p[k] = box["out"]
            if "shape" in box: e[k] = box["shape"]
            if "strides" in box: s[k] = box["strides"]
        return sqy.bin_boxes_device(src, n, o, e, bins, op, p, s, dtype, count=count)

    def refused_call(rc):
        assert rc == 1, rc
        _same(T.read(), T.host)

    def refused(**kw):
        for k in range(3):
            refused_call(call(k, **kw))
    refused_call(call(bins=None))                                       # bins NULL
    for bins in ((0, 2, 3), (2, -1, 3), (2, 2, -(2 ** 63))):            # an entry < 1
        refused_call(call(bins=bins))
    for op in (3, -1, 77):                                              # op outside 0 .. 2
        refused_call(call(op=op))
    for count in (0, -1, -(2 ** 40)):
        refused_call(call(count=count))
    refused(out=None)                                                   # a NULL entry
    refused(out=T.ptrs[0] + 2)                                          # an output 2 bytes off
    refused(strides=(15, 1, 1))                                         # a row pitch that overlaps: rows of 2 (or 3) cells, 1 apart
    refused(strides=(15, 5, 2))                                         # an innermost stride of 2
    refused(strides=(4, 5, 1))                                          # a layer pitch below the rows' reach
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
    refused_call(sqy.bin_boxes_device(d_blob.data_ptr(), len(blob), [(1, 1)] * 3, [(3, 4)] * 3, (2, 2), "max", T.ptrs, [(5, 1)] * 3, np.uint16))
    refused_call(call(src=None))
    refused_call(call(n=0))
    for bins in (BIN, (1, 1, 1), (9, 9, 9), (1, 2, 7)):
        for op in OPS + (0, 1, 2):
            Tg = Targets(np.uint32, _cells(boxes, bins), pitch=True)
            assert sqy.bin_boxes_device(d_blob.data_ptr(), len(blob), origins, extents, bins, op, Tg.ptrs, Tg.strides, np.uint16) == 0
            name = OPS[op] if isinstance(op, int) else op
            _same(Tg.read(), Tg.expect([_bin(_cut(full, o, e), bins, name) for o, e in boxes])[0])
    # the host variant: a capacity one byte short, the other type, a box outside
    import ctypes
    L = sqy.lib()
    rows = lambda v: (ctypes.c_long * sum(len(r) for r in v))(*[x for r in v for x in r])
    src = np.frombuffer(blob, np.uint8)
    out = np.full(4 + 9 + 4, 0xA5A5A5A5, np.uint32)
    for fn, o, e, nbytes in ((L.SQYAMD_Bin_Boxes_UI16, origins, extents, out.nbytes - 1), (L.SQYAMD_Bin_Boxes_UI8, origins, extents, out.nbytes),
                             (L.SQYAMD_Bin_Boxes_UI16, origins, extents[:2] + [(2, 3, 5)], out.nbytes + 64)):
        assert fn(src.ctypes.data, len(blob), 3, rows(o), rows(e), 3, rows([BIN]), 0, out.ctypes.data, nbytes) == 1
        assert (out == 0xA5A5A5A5).all()
    assert L.SQYAMD_Bin_Boxes_UI16(src.ctypes.data, len(blob), 3, rows(origins), rows(extents), 3, rows([BIN]), 0, out.ctypes.data, out.nbytes) == 0
    assert np.array_equal(out, np.concatenate([_bin(_cut(full, o, e), BIN, "max").reshape(-1) for o, e in boxes]))


def test_host_variant_mean_and_lower_ranks(sqy, oracle, options):
    """bin_boxes (host pointers, the outputs dense and back to back) gives what the device variant gives and numpy's outputs; "mean" is the
    sum over each cell's ACTUAL voxel count in float64, partial cells included; blobs of rank 1 and 2: the frames are the first dimension"""
    for pipeline, dtype in (("bitswap1->lz4", np.uint16), ("lz4", np.uint8), ("quantiser->bitswap1->lz4", np.uint16), ("diff3x3x1->bitswap1->lz4", np.uint16)):
        blob, full = _blob(sqy, oracle, pipeline + (SMALL_CHUNKS if "diff" not in pipeline else ""), (7, 33, 31), dtype)
        d_blob = _to_device(blob)
        boxes = _boxes((7, 33, 31), np.dtype(dtype).itemsize)
        origins, extents = [o for o, _ in boxes], [e for _, e in boxes]
        tiles = [_cut(full, o, e) for o, e in boxes]
        for subset in (1, 0):
            options("bin_boxes_subset", subset)
            for bins in ((2, 2, 2), (3, 5, 7), (1, 1, 32)):
                assert any(n % b for e in extents for n, b in zip(e, bins))      # partial cells are among them
                for op in OPS:
                    rc, cells = sqy.bin_boxes(blob, origins, extents, bins, op)
                    assert rc == 0 and all(g.dtype == np.uint32 for g in cells)
                    assert all(np.array_equal(g, _bin(t, bins, op)) and g.shape == _bin(t, bins, op).shape for g, t in zip(cells, tiles)), (pipeline, subset, bins, op)
                    T = Targets(np.uint32, _cells(boxes, bins))
                    assert _call(sqy, d_blob, len(blob), boxes, bins, op, T, dtype) == 0
                    got = T.read()
                    assert all(np.array_equal(got[T.bytes_of(i)].view(np.uint32)[..., 0], g) for i, g in enumerate(cells))
                rc, means = sqy.bin_boxes(blob, origins, extents, bins, "mean")
                assert rc == 0 and all(m.dtype == np.float64 for m in means)
                for m, t in zip(means, tiles):
                    count = _bin(np.ones(t.shape, np.uint8), bins, "sum")
                    assert np.array_equal(m, _bin(t, bins, "sum").astype(np.float64) / count.astype(np.float64)), (pipeline, subset, bins)
    options("bin_boxes_subset", 1)
    from sqeazy_amd import synth
    cases = (((40, 300), [((3, 17), (30, 200)), ((39, 0), (1, 300)), ((0, 299), (40, 1))], ((4, 7), (1, 64), (1000, 1))),
             ((9000,), [((4100,), (4000,)), ((0,), (9000,)), ((8999,), (1,))], ((3,), (4096,), (10000,))))
    for shape, boxes, binsets in cases:
        vol = synth.stack((1, 1, int(np.prod(shape))), np.uint16, seed=731).reshape(shape)
        tiles = [_cut(vol, o, e) for o, e in boxes]
        for pipeline in ("bitswap1->lz4" + SMALL_CHUNKS, "lz4" + SMALL_CHUNKS):
            rc, blob = sqy.encode(pipeline, vol)
            assert rc == 0
            d_blob = _to_device(blob)
            for bins in binsets:
                for op in OPS:
                    want = [_bin(t, bins, op) for t in tiles]
                    for pitch in (False, True):
                        T = Targets(np.uint32, _cells(boxes, bins), shift=4, pitch=pitch)
                        assert _call(sqy, d_blob, len(blob), boxes, bins, op, T, np.uint16) == 0, (shape, pipeline, bins, op, pitch)
                        _same(T.read(), T.expect(want)[0])
                    rc, cells = sqy.bin_boxes(blob, [o for o, _ in boxes], [e for _, e in boxes], bins, op)
                    assert rc == 0 and all(np.array_equal(g, w) and g.shape == w.shape for g, w in zip(cells, want))
