"""GPU: SQYAMD_Decode_Box_* -- a box of ONE blob decoded into a view of the box's shape (include/sqeazy_amd.h).

Every box must equal the same box of what SQY_Decode gives for the blob (test_gpu_batch_window._blob's `full`: the encoded volume where
the pipeline is lossless, the oracle's inverse for `quantiser`) at exactly the view's voxel places: all views of a run lie in one buffer of
a position-dependent pattern that is compared, whole, with an image built on the CPU.  The subset path (only the LZ4 frames the box's
z-range needs, then the windowed range transposer or one window copy) and the fallback ("decode_box_subset" = 0) give the same bytes,
and each shows its launches in the profile -- so the fallback cannot stand in for a broken subset path."""
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from test_gpu_batch_window import SERIAL_SHAPE, Targets, _blob, _cut, _same, _windows
from test_gpu_decode_frames import _damaged, _lz4_frames, _profile_names

pytestmark = pytest.mark.gpu

LONG_MAX = 2 ** 63 - 1
SMALL_CHUNKS = "(blocksize_kb=4,framestep_kb=4)"
# the shapes at the range transposer's seams and the chunk geometry each is encoded with: several 4 KiB chunks, plane segments that
# straddle chunks, word addresses off the 16-byte grid, tails | rows longer than a thread's run | 16-bit: 24 chunks, every plane on the
# grid | the default chunk: four of them, a segment size that is no multiple of 16 | everything wide
SHAPES = (((7, 33, 31), SMALL_CHUNKS), ((2, 3, 300), SMALL_CHUNKS), ((3, 128, 128), SMALL_CHUNKS), ((23, 131, 151), ""), ((16, 128, 128), ""))
# frame_shuffle->lz4 folds the map into the LZ4 decode where every place is a whole number of chunks: 8-bit frames of 256 KiB, the fewest
# with a frame between two others
SHUFFLE_SHAPE = (3, 512, 512)
SUBSET = [("bitswap1->lz4", np.uint16), ("bitswap1->lz4", np.uint8), ("lz4", np.uint16), ("lz4", np.uint8), ("quantiser->bitswap1->lz4", np.uint16),
          ("frame_shuffle->lz4", np.uint8), ("rmestbkrd->bitswap1->lz4", np.uint16)]
FALLBACK = [("diff3x3x1->bitswap1->lz4", np.uint16, 0), ("bitswap1", np.uint16, 0), ("bitswap1->lz4(blocksize_kb=64,framestep_kb=64)", np.uint16, 1)]
FINAL = {"bitswap1->lz4": "bitswap1_decode_box", "rmestbkrd->bitswap1->lz4": "bitswap1_decode_box", "quantiser->bitswap1->lz4": "bitswap1_quantiser_decode_box",
         "lz4": "box_window_copy", "frame_shuffle->lz4": "box_window_copy"}


def _dev():
    import torch
    return torch.device("cuda", 0)


def _to_device(blob):
    import torch
    return torch.from_numpy(np.frombuffer(blob, np.uint8).copy()).to(_dev())


def _boxes(shape, itemsize):
    """the windows of test_gpu_batch_window (the whole blob among them), and for EVERY frame an interior box of that frame alone: the ranges
    whose first or last word lies inside a thread's 128 voxels, or on a chunk boundary, are among them"""
    inner = [(1, d - 2) if d >= 3 else (0, d) for d in shape[1:]]
    frames = [((z,) + tuple(o for o, _ in inner), (1,) + tuple(e for _, e in inner)) for z in range(shape[0])]
    return _windows(shape, itemsize) + frames


_filtered = {}


def _case_blob(sqy, oracle, pipeline, shape, dtype, nthreads=0):
    """test_gpu_batch_window._blob; behind a background head (lossy, and the oracle has no inverse of it: it decodes as a copy) `full` is
    the filtered volume of the numpy restatement (tests/bkrd_restate.py), which SQY_Decode must give -- on a stack with signal above the
    background the filter estimates, so that voxels are left"""
    if "rmestbkrd" not in pipeline:
        return _blob(sqy, oracle, pipeline, shape, dtype, nthreads)
    import bkrd_restate as R
    from sqeazy_amd import synth
    key = (pipeline, tuple(shape), np.dtype(dtype).name)
    if key not in _filtered:
        vol = synth.stack(shape, dtype, seed=700 + len(shape) + shape[2] % 97)
        rng = np.random.default_rng(shape[2])
        vol[1:-1] += (rng.integers(500, 3000, vol[1:-1].shape) * (rng.random(vol[1:-1].shape) < 0.4)).astype(dtype)      # (not on the z faces)
        rc, blob = sqy.encode(pipeline, vol, nthreads=nthreads)
        if rc:
            _filtered[key] = None
            return None
        full = np.ascontiguousarray(R.filtered_volume(pipeline, vol, sqy.get_option("host_l2_bytes")))
        rc, back = sqy.decode(blob)
        assert rc == 0 and np.array_equal(back, full) and full.shape == tuple(shape) and full.dtype == np.dtype(dtype), (pipeline, shape)
        assert shape[0] < 3 or np.count_nonzero(full) > full.size // 8, (pipeline, shape)
        full.setflags(write=False)
        _filtered[key] = (blob, full)
    return _filtered[key]


def _made(sqy, oracle, pipeline, dtype, nthreads=0):
    """[(shape, blob on the device, its length, full)] of the case"""
    if nthreads:
        shapes = [(SERIAL_SHAPE, "")]
    elif "frame_shuffle" in pipeline:
        shapes = [(SHUFFLE_SHAPE, ""), ((7, 33, 31), SMALL_CHUNKS), ((3, 128, 128), SMALL_CHUNKS)]
    else:
        shapes = SHAPES
    out = []
    for shape, cfg in shapes:
        b = _case_blob(sqy, oracle, pipeline + (cfg if pipeline.endswith("lz4") else ""), shape, dtype, nthreads)
        if b is not None:                                               # (a geometry a stage refuses at encode)
            out.append((shape, _to_device(b[0]), len(b[0]), b[1]))
    return out


def _run_boxes(sqy, d_blob, nbytes, boxes, T, stream=None):
    for i, (o, e) in enumerate(boxes):
        rc = sqy.decode_box_device(d_blob.data_ptr(), nbytes, o, T.ptrs[i], e, T.strides[i], T.dtype, stream=stream)
        assert rc == 0, (o, e)
    return T.read()


def _voxels(sqy, oracle, options, pipeline, dtype, nthreads=0):
    item = np.dtype(dtype).itemsize
    made = _made(sqy, oracle, pipeline, dtype, nthreads)
    if "frame_shuffle" in pipeline:
        assert made and made[0][0] == SHUFFLE_SHAPE                     # (the folded shape; the others as far as the stage takes them)
    else:
        assert len(made) >= (1 if nthreads else 3), [s for s, _, _, _ in made]
    for shape, d_blob, nbytes, full in made:
        boxes = _boxes(shape, item)
        tiles = [_cut(full, o, e) for o, e in boxes]
        assert any(t.shape == tuple(shape) for t in tiles)               # the whole blob: it must equal the full decode
        for shift in (0, item):
            for pitch in (False, True):
                images = []
                for subset in (1, 0):
                    options("decode_box_subset", subset)
                    T = Targets(dtype, [e for _, e in boxes], shift=shift, pitch=pitch, salt=7 * shift + pitch)
                    got = _run_boxes(sqy, d_blob, nbytes, boxes, T)
                    _same(got, T.expect(tiles)[0])
                    images.append(got)
                assert np.array_equal(images[0], images[1])


@pytest.mark.parametrize("pipeline, dtype", SUBSET, ids=["%s-%s" % (p, np.dtype(d).name) for p, d in SUBSET])
def test_voxels(sqy, oracle, options, pipeline, dtype):
    """every box of every shape, with the views' bases on and one voxel behind the 16-byte grid, dense and pitched, through the subset path
    and through the fallback: the whole target buffer byte for byte"""
    _voxels(sqy, oracle, options, pipeline, dtype)


@pytest.mark.parametrize("pipeline, dtype, nthreads", FALLBACK, ids=["%s%s" % (p, "-serial" if t else "") for p, _, t in FALLBACK])
def test_voxels_of_blobs_the_subset_path_does_not_take(sqy, oracle, options, pipeline, dtype, nthreads):
    _voxels(sqy, oracle, options, pipeline, dtype, nthreads)


def test_host_variant_and_lower_ranks(sqy, oracle):
    """decode_box (host pointers, dense) equals the device variant's voxels; blobs of rank 1 and 2: the frames are the first dimension"""
    for pipeline, dtype in (("bitswap1->lz4", np.uint16), ("lz4", np.uint8), ("quantiser->bitswap1->lz4", np.uint16)):
        blob, full = _blob(sqy, oracle, pipeline + SMALL_CHUNKS, (7, 33, 31), dtype)
        for o, e in _boxes((7, 33, 31), np.dtype(dtype).itemsize):
            rc, box = sqy.decode_box(blob, o, e)
            assert rc == 0 and box.dtype == np.dtype(dtype) and np.array_equal(box, _cut(full, o, e)), (pipeline, o, e)
    from sqeazy_amd import synth
    for shape, origin, extent in (((40, 300), (3, 17), (30, 200)), ((40, 300), (39, 0), (1, 300)), ((9000,), (4100,), (4000,)), ((9000,), (0,), (9000,))):
        vol = synth.stack((1, 1, int(np.prod(shape))), np.uint16, seed=731).reshape(shape)
        for pipeline in ("bitswap1->lz4" + SMALL_CHUNKS, "lz4" + SMALL_CHUNKS):
            rc, blob = sqy.encode(pipeline, vol)
            assert rc == 0
            d_blob = _to_device(blob)
            for pitch in (False, True):
                T = Targets(np.uint16, [extent], shift=2, pitch=pitch)
                got = _run_boxes(sqy, d_blob, len(blob), [(origin, extent)], T)
                _same(got, T.expect([_cut(vol, origin, extent)])[0])


def _launch_case(sqy, oracle, pipeline, dtype):
    """a blob of several LZ4 frames: four (two at 8 bit) default chunks, or the shuffle's three"""
    shape = SHUFFLE_SHAPE if "frame_shuffle" in pipeline else (23, 131, 151)
    blob, full = _case_blob(sqy, oracle, pipeline, shape, dtype)
    return shape, blob, full


@pytest.mark.parametrize("pipeline, dtype", SUBSET, ids=["%s-%s" % (p, np.dtype(d).name) for p, d in SUBSET])
def test_launches(sqy, oracle, options, pipeline, dtype):
    """the subset path decodes a subset and ends in the case's own launch; the option off: the whole blob and one window copy; and
    SQYAMD_Decode_Frames_* launches what it launched before"""
    shape, blob, full = _launch_case(sqy, oracle, pipeline, dtype)
    d_blob = _to_device(blob)
    Z = shape[0]
    frames_before = _profile_names(sqy, lambda: sqy.decode_frames(blob, Z // 2, 1))
    boxes = [((Z // 2, 1, 1), (1, shape[1] - 2, shape[2] - 2)), ((0, 0, 3), (Z, shape[1], 5)), ((0, 0, 0), shape)]
    for o, e in boxes:
        T = Targets(dtype, [e], shift=np.dtype(dtype).itemsize, pitch=True)
        names = _profile_names(sqy, lambda: _run_boxes(sqy, d_blob, len(blob), [(o, e)], T))
        _same(T.read(), T.expect([_cut(full, o, e)])[0])
        assert "lz4_frames_subset_decode" in names and FINAL[pipeline] in names, names
        assert not any(k in names for k in ("lz4_frames_decode", "bitswap1_decode", "bitswap1_quantiser_decode", "bitswap1_decode_range", "bitswap1_quantiser_decode_range", "batch_window_copy",
                                            "frames_range_copy", "frame_scatter")), names
        assert sum(k in names for k in set(FINAL.values())) == 1, names
    options("decode_box_subset", 0)
    o, e = boxes[0]
    T = Targets(dtype, [e], pitch=True)
    names = _profile_names(sqy, lambda: _run_boxes(sqy, d_blob, len(blob), [(o, e)], T))
    _same(T.read(), T.expect([_cut(full, o, e)])[0])
    assert "lz4_frames_decode" in names and "box_window_copy" in names, names
    assert not any(k in names for k in ("lz4_frames_subset_decode", "bitswap1_decode_box", "bitswap1_quantiser_decode_box", "batch_window_copy")), names
    options("decode_box_subset", 1)
    frames_after = _profile_names(sqy, lambda: sqy.decode_frames(blob, Z // 2, 1))
    assert frames_before == frames_after and "lz4_frames_subset_decode" in frames_before, (frames_before, frames_after)
    assert not any("box" in k for k in frames_before), frames_before
    range_kernel = {"bitswap1_decode_box": "bitswap1_decode_range", "bitswap1_quantiser_decode_box": "bitswap1_quantiser_decode_range"}.get(FINAL[pipeline])
    if range_kernel:
        assert range_kernel in frames_before, frames_before


@pytest.mark.parametrize("pipeline", ["lz4", "bitswap1->lz4"])
def test_damaged_frame_outside_the_boxs_frames_goes_unnoticed(sqy, pipeline):
    """pruning is real: the last compressed LZ4 frame damaged -- a box in frame 0 does not need it (of every bit plane two chunks: frame 0's
    words lie in the first), a box in the last frame does and gives the full decode's code"""
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
    o, e = (0, 5, 7), (1, 50, 40)
    T = Targets(np.uint16, [e], shift=2, pitch=True)
    names = _profile_names(sqy, lambda: _run_boxes(sqy, d_bad, len(bad), [(o, e)], T))
    assert "lz4_frames_subset_decode" in names
    _same(T.read(), T.expect([_cut(vol, o, e)])[0])
    rc, box = sqy.decode_box(bad, o, e)
    assert rc == 0 and np.array_equal(box, _cut(vol, o, e))
    for o in ((15, 5, 7), (0, 5, 7)):                                   # the last frame alone; all frames
        T = Targets(np.uint16, [(16 - o[0], 50, 40)], pitch=True)
        assert sqy.decode_box_device(d_bad.data_ptr(), len(bad), o, T.ptrs[0], T.extents[0], T.strides[0], np.uint16) == rc_full
        assert sqy.decode_box(bad, o, T.extents[0]) == (rc_full, None)


def test_refusals(sqy, oracle):
    """1 and the destination's canaries intact"""
    import ctypes
    shape = (3, 5, 7)
    blob, full = _blob(sqy, oracle, "bitswap1->lz4", shape, np.uint16)
    u8 = _blob(sqy, oracle, "bitswap1->lz4", shape, np.uint8)[0]
    d_blob, d_u8 = _to_device(blob), _to_device(u8)
    T = Targets(np.uint16, [(2, 3, 4)], pitch=True)
    assert T.strides[0] == (26, 7, 1)
    good = dict(src=d_blob.data_ptr(), n=len(blob), origin=(1, 1, 1), dst=T.ptrs[0], shape=(2, 3, 4), strides=T.strides[0], dtype=np.uint16)

    def refused(**kw):
        a = dict(good, **kw)
        assert sqy.decode_box_device(a["src"], a["n"], a["origin"], a["dst"], a["shape"], a["strides"], a["dtype"]) == 1, kw
        _same(T.read(), T.host)
    refused(origin=(0, -1, 0))                                          # a negative origin
    refused(shape=(2, 0, 4))                                            # an extent of 0
    for k in range(3):                                                  # origin + extent one voxel beyond the shape, each dimension in turn
        e = [2, 4, 6]
        e[k] += 1
        refused(shape=tuple(e), strides=None)
        o = [0, 0, 0]
        o[k] = 1
        refused(origin=tuple(o), shape=shape, strides=None)
        o = [0, 0, 0]
        o[k] = LONG_MAX
        refused(origin=tuple(o), shape=(1, 1, 1))                       # no wrap to a small sum
    refused(origin=(1, 1), shape=(3, 4), strides=(7, 1))                # a rank other than the header's
    refused(origin=(1,), shape=(4,), strides=(1,))
    refused(src=d_u8.data_ptr(), n=len(u8))                             # a blob of the other voxel type
    refused(dtype=np.uint8)                                             # .. the entry point of the other type
    refused(strides=(40, 10, 2))                                        # an innermost stride of 2
    refused(strides=(26, 3, 1))                                         # a row stride smaller than the extent below it
    refused(strides=(20, 7, 1))                                         # a frame stride smaller than the rows below it
    refused(dst=T.ptrs[0] + 1)                                          # a destination off the voxel grid
    refused(src=None)
    refused(dst=None)
    refused(origin=None)
    refused(shape=None, strides=None)
    refused(n=0)
    # the good call: the table above refuses for its reasons
    assert sqy.decode_box_device(good["src"], good["n"], good["origin"], good["dst"], good["shape"], good["strides"], np.uint16) == 0
    _same(T.read(), T.expect([_cut(full, (1, 1, 1), (2, 3, 4))])[0])
    # the host variant: a capacity one byte short, the other type, a box outside, another rank
    L = sqy.lib()
    src = np.frombuffer(blob, np.uint8)
    host = np.full(2 * 3 * 4 * 2, 0x5A, np.uint8)
    longs = lambda v: (ctypes.c_long * len(v))(*v)
    assert L.SQYAMD_Decode_Box_UI16(src.ctypes.data, len(blob), longs((1, 1, 1)), longs((2, 3, 4)), 3, host.ctypes.data, host.nbytes - 1) == 1
    assert L.SQYAMD_Decode_Box_UI8(src.ctypes.data, len(blob), longs((1, 1, 1)), longs((2, 3, 4)), 3, host.ctypes.data, host.nbytes) == 1
    assert L.SQYAMD_Decode_Box_UI16(src.ctypes.data, len(blob), longs((1, 1, 1)), longs((2, 3, 7)), 3, host.ctypes.data, host.nbytes) == 1
    assert L.SQYAMD_Decode_Box_UI16(src.ctypes.data, len(blob), longs((1, 1)), longs((2, 3)), 2, host.ctypes.data, host.nbytes) == 1
    assert (host == 0x5A).all()
    assert L.SQYAMD_Decode_Box_UI16(src.ctypes.data, len(blob), longs((1, 1, 1)), longs((2, 3, 4)), 3, host.ctypes.data, host.nbytes) == 0
    assert np.array_equal(host.view(np.uint16).reshape(2, 3, 4), _cut(full, (1, 1, 1), (2, 3, 4)))


def test_work_queued_on_the_callers_stream_is_respected(sqy):
    """the blob is written by a copy queued on the caller's stream just before the call, and the destination is filled the same way"""
    import torch
    from sqeazy_amd import synth
    dev = _dev()
    vol = synth.stack((16, 128, 160), np.uint16)
    rc, blob = sqy.encode("bitswap1->lz4", vol, nthreads=2)
    assert rc == 0
    host_blob = torch.from_numpy(np.frombuffer(blob, np.uint8).copy()).pin_memory()
    o, e = (5, 3, 17), (8, 100, 120)
    sz, sy = 100 * 130 + 7, 130                                         # a pitched view
    s = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(s):
        d_blob = torch.empty(len(blob), dtype=torch.uint8, device=dev)
        out = torch.empty(8 * sz, dtype=torch.int16, device=dev)
        for _ in range(2):
            d_blob.zero_()
            out.fill_(7)
            d_blob.copy_(host_blob, non_blocking=True)
            rc = sqy.decode_box_device(d_blob.data_ptr(), len(blob), o, out.data_ptr(), e, (sz, sy, 1), np.uint16, stream=s.cuda_stream)
            assert rc == 0
            got = out.cpu().numpy().view(np.uint16)
            want = np.full(8 * sz, 7, np.uint16)
            idx = (np.arange(8)[:, None, None] * sz + np.arange(100)[None, :, None] * sy + np.arange(120)[None, None, :]).reshape(-1)
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
        ok = True
        for z0 in range(0, vols[i].shape[0] - 1, 3):
            o, e = (z0, 2 + i, 5), (2, 100, 131)
            rc, box = sqy.decode_box(blobs[i], o, e)
            ok = ok and rc == 0 and np.array_equal(box, _cut(vols[i], o, e))
        return ok
    with ThreadPoolExecutor(4) as ex:
        assert all(ex.map(one, range(4)))
