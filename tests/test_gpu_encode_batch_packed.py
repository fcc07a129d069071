"""SQYAMD_PipelineEncode_BatchPacked_*: the batch encode with the blobs back to back in ONE buffer.  Blob i must be byte for byte the oracle's
and SQYAMD_PipelineEncode_*_Device's for volume i; offsets, lengths and total must be the placement rule applied to the blobs' lengths
(offsets[0] = 0, offsets[i + 1] = offsets[i] + lengths[i] rounded up to align, total = offsets[-1] + lengths[-1]); and the call writes the
blobs' bytes and nothing else -- the destination is filled with canaries, in front of it, behind its capacity and in it, and every byte
outside the blobs must still be one, the gap bytes between blobs included.  Whichever way the volumes are grouped, on the joint path, beside
it or without it, dense or as views, whatever the capacity."""
import threading

import numpy as np
import pytest

from sqeazy_amd import synth
from test_gpu_encode_batch import CANARY, GAP, MIXED_SHAPES, SINGLE_KERNELS, _profile, _want

pytestmark = pytest.mark.gpu

SHIFT = 3                     # d_dst lies this far behind an aligned address: no alignment of d_dst is required
BSW, LZ4, QUANT, DIFF = "bitswap1->lz4", "lz4", "quantiser->bitswap1->lz4", "diff3x3x1->bitswap1->lz4"
CASES = [(BSW, np.uint16), (BSW, np.uint8), (LZ4, np.uint16), (QUANT, np.uint16)]


def _dev():
    import torch
    return torch.device("cuda", 0)


def restate(lens, align):
    """the placement rule: (offsets, total)"""
    offs, at = [], 0
    for n in lens:
        offs.append(at)
        at = -(-(at + n) // align) * align
    return offs, offs[-1] + lens[-1]


def _extra(pipeline, dtype):
    """a small volume whose blob length is a multiple of 16 (found with the oracle; the fixture below asserts it)"""
    if pipeline == LZ4:                                                 # (synth's noise is stored by a plain lz4: odd lengths only)
        v = np.zeros((3, 5, 24), np.uint16)
        v[1, 2, :12] = np.arange(12) * 9 + 1
        return v
    shape, seed = {(BSW, np.uint16): ((4, 6, 10), 432), (BSW, np.uint8): ((2, 9, 11), 408), (QUANT, np.uint16): ((3, 5, 7), 409)}[(pipeline, dtype)]
    return synth.stack(shape, dtype, seed=seed)


_sets = {}


def _set(sqy, oracle, pipeline, dtype):
    """MIXED_SHAPES with the extra volume in the middle: (volumes, the blobs both references give)"""
    k = (pipeline, np.dtype(dtype).name)
    if k not in _sets:
        vols = [synth.stack(s, dtype, seed=300 + i) for i, s in enumerate(MIXED_SHAPES)]
        vols.insert(2, _extra(pipeline, dtype))
        want = [_want(sqy, oracle, pipeline, v, 0, _dev(), "packed-%s-%d" % (k[1], i)) for i, v in enumerate(vols)]
        assert any(len(w) % 16 == 0 for w in want) and any(len(w) % 16 for w in want), [len(w) for w in want]
        _sets[k] = (vols, want)
    return _sets[k]


def _upload(vols):
    import torch
    return [torch.from_numpy(np.ascontiguousarray(v)).to(_dev()) for v in vols]


def _call(sqy, pipeline, ptrs, shapes, dtype, capacity, align=1, strides=None, nthreads=0, stream=None):
    """the call into `capacity` bytes SHIFT behind an aligned address, canaries everywhere: (rc, offsets, lengths, total, the destination's
    capacity bytes as the call left them).  The canaries in front of d_dst and behind its capacity must hold whatever rc is."""
    import torch
    buf = torch.full((GAP + SHIFT + capacity + GAP,), CANARY, dtype=torch.uint8, device=_dev())
    lo = GAP + SHIFT
    rc, offs, lens, total = sqy.encode_batch_packed_device(pipeline, ptrs, shapes, strides, dtype, buf.data_ptr() + lo, capacity, align=align, nthreads=nthreads,
                                                           stream=stream)
    torch.cuda.synchronize()
    h = buf.cpu().numpy()
    assert (h[:lo] == CANARY).all() and (h[lo + capacity:] == CANARY).all(), "written outside the destination"
    if rc:
        assert offs == [0] * len(ptrs) and lens == [0] * len(ptrs)
    return rc, offs, lens, total, h[lo:lo + capacity]


def _image(capacity, offs, blobs):
    """what the destination must hold: canaries, and the blobs at their places"""
    img = np.full(capacity, CANARY, np.uint8)
    for o, b in zip(offs, blobs):
        img[o:o + len(b)] = np.frombuffer(b, np.uint8)
    return img


def _check(sqy, pipeline, srcs, shapes, dtype, want, align, slack=37, **kw):
    """a call that must succeed: the rule's offsets, lengths and total, the blobs in place and not a byte else"""
    woffs, wtotal = restate([len(w) for w in want], align)
    capacity = wtotal + slack
    rc, offs, lens, total, got = _call(sqy, pipeline, [s if isinstance(s, int) else s.data_ptr() for s in srcs], shapes, dtype, capacity, align=align, **kw)
    assert rc == 0
    assert (offs, lens, total) == (woffs, [len(w) for w in want], wtotal)
    assert np.array_equal(got, _image(capacity, woffs, want)), "a blob differs, or a byte outside the blobs was written"
    return offs, lens, total


@pytest.mark.parametrize("align", [1, 16, 4096])
@pytest.mark.parametrize("pipeline, dtype", CASES)
def test_bytes_and_placement(sqy, oracle, pipeline, dtype, align):
    vols, want = _set(sqy, oracle, pipeline, dtype)
    _check(sqy, pipeline, _upload(vols), [v.shape for v in vols], dtype, want, align)


def test_launch_counts_and_the_base_across_groups(sqy, oracle, options):
    import torch
    vols, want = _set(sqy, oracle, BSW, np.uint16)
    srcs, shapes = _upload(vols), [v.shape for v in vols]
    once = ("batch_lz4_place", "batch_lz4_frame_scan", "batch_lz4_frame_gather", "batch_lz4_chunks")
    for align in (1, 16):
        (one, p) = _profile(sqy, lambda: _check(sqy, BSW, srcs, shapes, np.uint16, want, align))
        assert all(p[k][1] == 1 for k in once), p
        assert not any(k in p for k in SINGLE_KERNELS), p
        # LZ4 input: 256 KiB, 320 KiB, 480 B, 210 B, 10 B, 512 KiB -- at 400000 bytes a group: {0} | {1, 2, 3, 4} | {5}
        options("encode_batch_group_bytes", 400000)
        (three, p) = _profile(sqy, lambda: _check(sqy, BSW, srcs, shapes, np.uint16, want, align))
        assert all(p[k][1] == 3 for k in once), p
        assert not any(k in p for k in SINGLE_KERNELS), p
        assert three == one
        options("encode_batch_group_bytes", 1 << 30)
    # the slot call knows nothing of the placement scan
    cap = max(sqy.max_compressed_length(BSW, s, np.uint16) for s in shapes)
    out = torch.empty(cap * len(vols), dtype=torch.uint8, device=_dev())
    ((rc, offs, lens), p) = _profile(sqy, lambda: sqy.encode_batch_device(BSW, [s.data_ptr() for s in srcs], shapes, np.uint16, out.data_ptr(), cap))
    assert rc == 0 and lens == [len(w) for w in want] and "batch_lz4_place" not in p and p["batch_lz4_frame_gather"][1] == 1, p


@pytest.mark.parametrize("align", [1, 16])
@pytest.mark.parametrize("n", [257, 300])
def test_place_scan_boundaries(sqy, oracle, n, align):
    """blobs of a few hundred bytes, more volumes than the scan has threads: the offsets cross the 64-lane and the 256-thread carry"""
    kinds = [synth.stack(s, np.uint16, seed=500 + i) for i, s in enumerate(((1, 1, 5), (3, 5, 7)) * 3)]
    blobs = [_want(sqy, oracle, BSW, v, 0, _dev(), "scan%d" % i) for i, v in enumerate(kinds)]
    d = _upload(kinds)
    pick = [i % len(kinds) for i in range(n)]
    (_, p) = _profile(sqy, lambda: _check(sqy, BSW, [d[i] for i in pick], [kinds[i].shape for i in pick], np.uint16, [blobs[i] for i in pick], align))
    assert p["batch_lz4_place"][1] == 1 and p["batch_lz4_frame_gather"][1] == 1, p


@pytest.mark.parametrize("align", [1, 16])
def test_capacity(sqy, oracle, align):
    vols, want = _set(sqy, oracle, BSW, np.uint16)
    srcs = _upload(vols)
    ptrs, shapes = [s.data_ptr() for s in srcs], [v.shape for v in vols]
    n = len(vols)
    woffs, wtotal = restate([len(w) for w in want], align)
    rc, offs, lens, total, got = _call(sqy, BSW, ptrs, shapes, np.uint16, wtotal, align=align)
    assert rc == 0 and (offs, total) == (woffs, wtotal) and np.array_equal(got, _image(wtotal, woffs, want))
    # one byte short: refused, the exact figure for the retry, and the retry
    rc, offs, lens, total, got = _call(sqy, BSW, ptrs, shapes, np.uint16, wtotal - 1, align=align)
    assert rc == 1 and total == wtotal
    img = _image(wtotal - 1, woffs[:n - 1], want[:n - 1])              # (the blobs that fit may have been written, the last one not)
    assert ((got == img) | (got == CANARY)).all()
    rc, offs, lens, again, got = _call(sqy, BSW, ptrs, shapes, np.uint16, total, align=align)
    assert rc == 0 and again == wtotal and offs == woffs
    # a capacity that cuts in mid-batch, one byte into the third blob's room: every byte in front of it is a canary or the right blob byte
    cut = woffs[1] + len(want[1]) + 1
    rc, offs, lens, total, got = _call(sqy, BSW, ptrs, shapes, np.uint16, cut, align=align)
    assert rc == 1 and total == wtotal
    fits = [i for i in range(n) if woffs[i] + len(want[i]) <= cut]
    assert fits == [0, 1]
    img = _image(cut, [woffs[i] for i in fits], [want[i] for i in fits])
    assert ((got == img) | (got == CANARY)).all(), "a byte that is neither a canary nor the blob's"
    # a capacity of one byte
    rc, offs, lens, total, got = _call(sqy, BSW, ptrs, shapes, np.uint16, 1, align=align)
    assert rc == 1 and total == wtotal and (got == CANARY).all()


def test_every_path_same_layout(sqy, oracle, options):
    vols, want = _set(sqy, oracle, BSW, np.uint16)
    srcs, shapes = _upload(vols), [v.shape for v in vols]
    for align in (1, 16):
        joint = _check(sqy, BSW, srcs, shapes, np.uint16, want, align)
        options("encode_batch_joint", 0)
        (alone, p) = _profile(sqy, lambda: _check(sqy, BSW, srcs, shapes, np.uint16, want, align))
        options("encode_batch_joint", 1)
        assert alone == joint and not any(k.startswith("batch_") for k in p), p
        assert p["lz4_chunks"][1] == len(vols), p
    # a pipeline outside the joint forms
    three = [vols[0], vols[1], vols[5]]
    dwant = [_want(sqy, oracle, DIFF, v, 0, _dev(), "packed-diff%d" % i) for i, v in enumerate(three)]
    (_, p) = _profile(sqy, lambda: _check(sqy, DIFF, _upload(three), [v.shape for v in three], np.uint16, dwant, 16))
    assert not any(k.startswith("batch_") for k in p), p
    # a mixed call: nthreads = 1 sends the two-chunk volume (20, 64, 128) to the serial layout, outside the joint forms -- first, in the
    # middle and last among single-chunk volumes, which share ONE group
    two = vols[1]
    assert two.shape == (20, 64, 128)
    order = [two, vols[0], vols[3], two, vols[4], two]
    mwant = [_want(sqy, oracle, BSW, v, 1, _dev(), "packed-serial%d" % i) for i, v in enumerate(order)]
    for align in (1, 4096):
        (_, p) = _profile(sqy, lambda: _check(sqy, BSW, _upload(order), [v.shape for v in order], np.uint16, mwant, align, nthreads=1))
        assert p["batch_lz4_place"][1] == 1 and p["batch_lz4_chunks"][1] == 1, p
    # .. and one that can be cut short: the exact figure comes out of a mixed call too
    woffs, wtotal = restate([len(w) for w in mwant], 16)
    srcs = _upload(order)
    rc, _, _, total, got = _call(sqy, BSW, [s.data_ptr() for s in srcs], [v.shape for v in order], np.uint16, woffs[2] + 5, align=16, nthreads=1)
    assert rc == 1 and total == wtotal
    img = _image(woffs[2] + 5, woffs[:2], mwant[:2])
    assert ((got == img) | (got == CANARY)).all()


@pytest.mark.parametrize("pipeline", [BSW, LZ4, QUANT])
def test_views(sqy, oracle, options, pipeline):
    """a 32 x 128 x 256 parent cut by tile_views into 16 x 64 x 128 tiles: the blobs of the dense copies, packed"""
    import torch
    parent = synth.stack((32, 128, 256), np.uint16, seed=610)
    d_parent = torch.from_numpy(parent).to(_dev())
    ptrs, shapes, strides = sqy.tile_views(d_parent.data_ptr(), parent.shape, (16, 64, 128), 2)
    assert len(ptrs) == 8
    tiles = [np.ascontiguousarray(parent[z:z + 16, y:y + 64, x:x + 128]) for z in (0, 16) for y in (0, 64) for x in (0, 128)]
    want = [_want(sqy, oracle, pipeline, t, 0, _dev(), "packed-tile%d" % i) for i, t in enumerate(tiles)]
    got = []
    for fused in (1, 0):
        options("batch_strided_fused", fused)
        (r, p) = _profile(sqy, lambda: _check(sqy, pipeline, ptrs, shapes, np.uint16, want, 16, strides=strides))
        assert p["batch_lz4_place"][1] == 1 and not any(k in p for k in SINGLE_KERNELS), p
        got.append(r)
    assert got[0] == got[1]
    assert torch.equal(d_parent.cpu(), torch.from_numpy(parent)), "the parent was written"


@pytest.mark.parametrize("why, strides", [("innermost stride 2", (32768, 256, 2)), ("a stride of 0", (32768, 0, 1)), ("rows that overlap", (32768, 100, 1)),
                                          ("frames that overlap", (4096, 256, 1))])
def test_refused_views(sqy, why, strides):
    import torch
    d_parent = torch.zeros(32 * 128 * 256, dtype=torch.int16, device=_dev())
    rc, offs, lens, total, got = _call(sqy, BSW, [d_parent.data_ptr()] * 2, [(16, 64, 128)] * 2, np.uint16, 4096, align=16, strides=[strides] * 2)
    assert rc == 1 and total == 0 and (got == CANARY).all(), why
    # a source that is not aligned to its voxels
    rc, offs, lens, total, got = _call(sqy, BSW, [d_parent.data_ptr() + 1] * 2, [(16, 64, 128)] * 2, np.uint16, 4096, strides=[(32768, 256, 1)] * 2)
    assert rc == 1 and total == 0 and (got == CANARY).all()


@pytest.mark.parametrize("pipeline, dtype", CASES)
def test_way_back(sqy, oracle, pipeline, dtype):
    """the call's offsets and lengths straight into SQYAMD_Decode_Batch_*_Device"""
    import torch
    vols, want = _set(sqy, oracle, pipeline, dtype)
    srcs = _upload(vols)
    total = restate([len(w) for w in want], 16)[1]
    buf = torch.full((total,), CANARY, dtype=torch.uint8, device=_dev())
    rc, offs, lens, got_total = sqy.encode_batch_packed_device(pipeline, [s.data_ptr() for s in srcs], [v.shape for v in vols], None, dtype, buf.data_ptr(), total, align=16)
    assert rc == 0 and got_total == total
    outs = [torch.zeros_like(s) for s in srcs]
    rc, decoded = sqy.decode_batch_device(buf.data_ptr(), offs, lens, [o.data_ptr() for o in outs], [v.nbytes for v in vols], dtype)
    torch.cuda.synchronize()
    assert rc == 0 and decoded == [v.nbytes for v in vols]
    for v, w, o in zip(vols, want, outs):
        back = v if pipeline != QUANT else oracle.pipeline_decode(w)
        assert np.array_equal(o.cpu().numpy(), np.asarray(back).reshape(v.shape)), (pipeline, v.shape)


def test_callers_stream_and_two_host_threads(sqy, oracle):
    import torch
    dev = _dev()
    vols, want = _set(sqy, oracle, BSW, np.uint16)
    qvols, qwant = _set(sqy, oracle, QUANT, np.uint16)
    # (the helper fills sources and canaries on torch's current stream: made the caller's stream here, so the fills are ordered in front of
    # the call whatever else is queued)
    s = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(s):
        _check(sqy, BSW, _upload(vols), [v.shape for v in vols], np.uint16, want, 16, stream=s.cuda_stream)
    sets = [(BSW, [vols[0], vols[2], vols[4]], [want[0], want[2], want[4]]), (QUANT, [qvols[1], qvols[3], qvols[5]], [qwant[1], qwant[3], qwant[5]])]
    streams = [torch.cuda.Stream(device=dev) for _ in sets]
    ok = [False, False]

    def one(t):
        pipeline, vs, ws = sets[t]
        good = True
        with torch.cuda.stream(streams[t]):
            for r in range(3):
                try:
                    _check(sqy, pipeline, _upload(vs), [v.shape for v in vs], np.uint16, ws, (1, 16, 4096)[r], stream=streams[t].cuda_stream)
                except AssertionError:
                    good = False
        ok[t] = good
    th = [threading.Thread(target=one, args=(t,)) for t in range(2)]
    for x in th:
        x.start()
    for x in th:
        x.join()
    assert all(ok)


@pytest.mark.parametrize("align", [1, 16])
def test_host_entry(sqy, oracle, align):
    vols, want = _set(sqy, oracle, BSW, np.uint16)
    buf, offs, lens = sqy.encode_batch_packed(BSW, vols, align=align)
    woffs, wtotal = restate([len(w) for w in want], align)
    assert len(buf) == wtotal and offs == woffs and lens == [len(w) for w in want]
    blobs = [buf[o:o + n] for o, n in zip(offs, lens)]
    assert blobs == want
    gaps = np.ones(wtotal, bool)                                        # (between the blobs: zeros)
    for o, n in zip(offs, lens):
        gaps[o:o + n] = False
    assert (np.frombuffer(buf, np.uint8)[gaps] == 0).all()
    back = sqy.decode_batch(blobs)
    assert all(np.array_equal(b, v) for b, v in zip(back, vols))
    u8, w8 = _set(sqy, oracle, BSW, np.uint8)
    buf, offs, lens = sqy.encode_batch_packed(BSW, u8, align=align)
    assert [buf[o:o + n] for o, n in zip(offs, lens)] == w8
    with pytest.raises(ValueError):
        sqy.encode_batch_packed(BSW, vols, align=3)
