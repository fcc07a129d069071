"""GPU: SQYAMD_Update_Box_* -- a box written into ONE large blob (include/sqeazy_amd.h).

The expectation is never the code under test: the old blob comes from the single call (test_gpu_batch_window._blob), the box is pasted
into its decode with numpy, and the new blob must be, byte for byte, the single call's blob of the pasted volume
(test_gpu_encode_batch._want, which holds that blob to the oracle).  Every destination lies between canaries; the view sources are
test_gpu_batch_update.Sources (dense, then pitched and 2 bytes off the 16-byte grid) and must be unchanged afterwards.  The subset path
(only the LZ4 frames the box's z-range needs: decoded, patched, parsed again, spliced between the old ones) and the whole path
("update_box_subset" = 0) must give the same bytes, and each shows its launches in the profile -- so the fallback cannot stand in for a
broken subset path."""
import hashlib
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from sqeazy_amd import synth
from test_gpu_batch_update import Sources, _paste
from test_gpu_batch_window import SERIAL_SHAPE, _blob, _cut
from test_gpu_decode_box import SHAPES, SMALL_CHUNKS, _case_blob, _to_device
from test_gpu_decode_frames import _damaged, _lz4_frames, _profile_names
from test_gpu_encode_batch import CANARY, GAP, _want

pytestmark = pytest.mark.gpu

BSL = "bitswap1->lz4"
SPLICE = ("lz4_splice_scan", "lz4_splice_gather")
PATCH = {BSL: "bitswap1_range_patch", "lz4": "box_window_paste"}
CASES = [(BSL, np.uint16), (BSL, np.uint8), ("lz4", np.uint16), ("lz4", np.uint8)]
IDS = ["%s-%s" % (p, np.dtype(d).name) for p, d in CASES]


def _dev():
    import torch
    return torch.device("cuda", 0)


def _boxes(shape):
    """the whole blob | one voxel | an interior box of the first, a middle and the last frame alone (ranges that begin or end inside a
    thread's run or on a chunk boundary) | rows of the first frame (`lz4`: inside the first chunk only) | the last row (inside the last,
    short chunk only) | one column through every frame"""
    Z, Y, X = shape
    inner = [(1, d - 2) if d >= 3 else (0, d) for d in shape[1:]]
    frame = lambda z: ((z,) + tuple(o for o, _ in inner), (1,) + tuple(e for _, e in inner))
    b = [((0, 0, 0), shape), ((Z // 2, Y // 2, X // 2), (1, 1, 1))]
    b += [frame(z) for z in sorted({0, Z // 2, Z - 1})]
    b += [((0, 0, 0), (1, min(2, Y), X)), ((Z - 1, Y - 1, 0), (1, 1, X)), ((0, 0, min(15, X - 1)), (Z, Y, 1))]
    return b


_tiles = {}


def _tile(extent, dtype, k):
    key = (tuple(extent), np.dtype(dtype).name, k)
    if key not in _tiles:
        _tiles[key] = synth.stack(tuple(extent), dtype, seed=1200 + k)
    return _tiles[key]


def _expect(sqy, oracle, pipeline, full, origin, tile, nthreads=0):
    """the single call's blob for the pasted volume, held to the oracle"""
    pasted = _paste(full, origin, tile)
    return _want(sqy, oracle, pipeline, pasted, nthreads, _dev(), key=("update_box", pasted.shape, pasted.dtype.name, hashlib.sha1(pasted.tobytes()).hexdigest()))


def _update(sqy, pipeline, d_blob, nbytes, origin, S, i=0, cap=None, nthreads=0, stream=None, shape=None):
    """the call into cap bytes between canaries: (rc, dstlength, blob or None).  The canaries hold whatever rc is, the bytes behind the blob
    too, and every byte when rc is not 0"""
    import torch
    if cap is None:
        cap = sqy.max_compressed_length(pipeline, shape, S.dtype)
    buf = torch.full((2 * GAP + cap,), CANARY, dtype=torch.uint8, device=_dev())
    torch.cuda.synchronize()                                            # (the fill is torch's stream's: the caller's to complete)
    rc, n = sqy.update_box_device(pipeline, d_blob.data_ptr(), nbytes, origin, S.ptrs[i], S.extents[i], S.strides[i], S.dtype, buf.data_ptr() + GAP, cap, nthreads=nthreads,
                                  stream=stream)
    torch.cuda.synchronize()
    h = buf.cpu().numpy()
    if rc:
        assert (h == CANARY).all(), "rc %d and the destination was written" % rc
        return rc, n, None
    assert 0 < n <= cap and (h[:GAP] == CANARY).all() and (h[GAP + n:] == CANARY).all(), "written outside the blob"
    return rc, n, h[GAP:GAP + n].tobytes()


def _unchanged(S):
    assert np.array_equal(S.buf.cpu().numpy(), S.host), "a view was written"


def _both_paths(sqy, options, pipeline, d_blob, nbytes, shape, origins, tiles, wants, nthreads=0):
    """every box through the subset path and the whole path, sources dense, then pitched and 2 bytes off the grid"""
    for shift, pitch in ((0, False), (2, True)):
        S = Sources(tiles[0].dtype, tiles, shift=shift, pitch=pitch, salt=5 + shift)
        for subset in (1, 0):
            options("update_box_subset", subset)
            for i, (o, w) in enumerate(zip(origins, wants)):
                rc, n, b = _update(sqy, pipeline, d_blob, nbytes, o, S, i, nthreads=nthreads, shape=shape)
                assert rc == 0 and b == w, (pipeline, shape, o, tiles[i].shape, subset, shift, pitch, n, len(w))
        _unchanged(S)
    options("update_box_subset", 1)


@pytest.mark.parametrize("pipeline, dtype", CASES, ids=IDS)
def test_bytes_both_paths(sqy, oracle, options, pipeline, dtype):
    for shape, cfg in SHAPES:
        blob, full = _blob(sqy, oracle, pipeline + cfg, shape, dtype)
        boxes = _boxes(shape)
        tiles = [_tile(e, dtype, k) for k, (_, e) in enumerate(boxes)]
        wants = [_expect(sqy, oracle, pipeline + cfg, full, o, t) for (o, _), t in zip(boxes, tiles)]
        assert wants[0] == _want(sqy, oracle, pipeline + cfg, tiles[0], 0, _dev())          # the whole blob: the single call's blob of the view
        _both_paths(sqy, options, pipeline + cfg, _to_device(blob), len(blob), shape, [o for o, _ in boxes], tiles, wants)


@pytest.mark.parametrize("pipeline, dtype", CASES, ids=IDS)
def test_the_old_voxels_give_the_old_blob(sqy, oracle, options, pipeline, dtype):
    for shape, cfg in SHAPES[:1] + SHAPES[3:4]:
        blob, full = _blob(sqy, oracle, pipeline + cfg, shape, dtype)
        boxes = _boxes(shape)[:4]
        _both_paths(sqy, options, pipeline + cfg, _to_device(blob), len(blob), shape, [o for o, _ in boxes], [np.ascontiguousarray(_cut(full, o, e)) for o, e in boxes],
                    [blob] * len(boxes))


def _payload(sqy, blob):
    return len(blob) - sqy.header_size(blob)


@pytest.mark.parametrize("pipeline, dtype", CASES, ids=IDS)
def test_frame_sizes_move_both_ways(sqy, oracle, options, pipeline, dtype):
    """4 KiB chunks.  Full-range noise over compressible data: replaced frames become stored and the payload length gains a decimal digit,
    so the header changes length; zeros over noise: they shrink.  That the volumes do this is checked on the single call's blobs, which are held to the
    oracle, before the call under test is run on them"""
    shape = (16, 64, 64)
    item = np.dtype(dtype).itemsize
    rng = np.random.default_rng(11)
    smooth = (np.arange(np.prod(shape)) // 4096 % 200).astype(dtype).reshape(shape)          # long runs: a few dozen bytes per chunk
    noise = rng.integers(0, 256 ** item, shape, dtype=np.uint32).astype(dtype)
    name = pipeline + SMALL_CHUNKS
    moved = 0
    # (frames 0..7 are the first 4 KiB chunk of every bit plane whole, and whole chunks of the voxels)
    for old_vol, tile, origin in ((smooth, noise[:8], (0, 0, 0)), (noise, np.zeros((15, 64, 64), dtype), (0, 0, 0)), (smooth, noise[5:6, 3:40, 1:60], (5, 3, 1))):
        old = _want(sqy, oracle, name, old_vol, 0, _dev())
        want = _expect(sqy, oracle, name, old_vol, origin, np.ascontiguousarray(tile))
        f_old, f_new = _lz4_frames(old, sqy), _lz4_frames(want, sqy)
        assert len(f_old) == len(f_new) == old_vol.nbytes // 4096
        if tile.shape[1:] == shape[1:]:
            stored = lambda fr: sum(1 for f in fr if f[3])
            if old_vol is smooth:
                assert stored(f_new) > stored(f_old), (stored(f_old), stored(f_new))
                assert len(str(_payload(sqy, want))) > len(str(_payload(sqy, old)))              # the payload length gains a digit ..
                if item == 1:                                           # .. and the header a byte (16-bit headers are padded to a multiple of 2)
                    assert (sqy.header_size(want) - sqy.header_size(old)) % 16 != 0
            else:
                assert stored(f_new) < stored(f_old) and _payload(sqy, want) < _payload(sqy, old) * 3 // 4
            moved += 1
        _both_paths(sqy, options, name, _to_device(old), len(old), shape, [origin], [np.ascontiguousarray(tile)], [want])
    assert moved == 2


@pytest.mark.parametrize("pipeline", [BSL, "lz4"])
def test_launches(sqy, oracle, options, pipeline):
    shape = (23, 131, 151)
    blob, full = _blob(sqy, oracle, pipeline, shape, np.uint16)
    d_blob = _to_device(blob)
    o, e = (11, 1, 1), (2, 129, 149)
    tile = _tile(e, np.uint16, 77)
    want = _expect(sqy, oracle, pipeline, full, o, tile)
    S = Sources(np.uint16, [tile], shift=2, pitch=True)
    out = {}
    names = _profile_names(sqy, lambda: out.update(r=_update(sqy, pipeline, d_blob, len(blob), o, S, shape=shape)))
    assert out["r"][0] == 0 and out["r"][2] == want
    for k in ("lz4_frames_subset_decode", PATCH[pipeline], "lz4_chunks_table") + SPLICE:
        assert k in names, (k, names)
    assert not any(k in names for k in ("lz4_frames_decode", "batch_window_paste", "bitswap1_decode", "lz4_chunks", "lz4_frame_gather", "lz4_inplace_tail")), names
    options("update_box_subset", 0)
    names = _profile_names(sqy, lambda: out.update(r=_update(sqy, pipeline, d_blob, len(blob), o, S, shape=shape)))
    assert out["r"][0] == 0 and out["r"][2] == want
    assert "lz4_frames_decode" in names and "batch_window_paste" in names, names
    assert not any(k in names for k in SPLICE + ("lz4_frames_subset_decode", "lz4_chunks_table", "bitswap1_range_patch", "box_window_paste")), names
    options("update_box_subset", 1)


OTHERS = [("diff3x3x1->bitswap1->lz4", "diff3x3x1->bitswap1->lz4", 0, (16, 128, 128)), ("quantiser->bitswap1->lz4", "quantiser->bitswap1->lz4", 0, (16, 128, 128)),
          ("rmestbkrd->bitswap1->lz4", "rmestbkrd->bitswap1->lz4", 0, (16, 128, 128)),
          ("bitswap1->lz4(blocksize_kb=64,framestep_kb=64)", "bitswap1->lz4(blocksize_kb=64,framestep_kb=64)", 1, SERIAL_SHAPE),
          ("lz4(accel=2)", "lz4(accel=2)", 0, (16, 128, 128)), ("lz4(accel=-2)", "lz4(accel=-2)", 0, (16, 128, 128)), ("lz4", BSL, 0, (16, 128, 128))]


@pytest.mark.parametrize("old, new, nthreads, shape", OTHERS, ids=["%s|%s%s" % (o, n, "-serial" if t else "") for o, n, t, _ in OTHERS])
def test_blobs_the_subset_path_does_not_take(sqy, oracle, options, old, new, nthreads, shape):
    """the new blob equals the single call's blob of the pasted decode (quantiser: the paste goes into the oracle's decode, which _blob
    holds SQY_Decode to; rmestbkrd: the oracle has no such stage, the single call itself is the reference); no splice launch shows --
    but for lz4(accel=2), which liblz4 compresses with acceleration 1 like accel=1: sqy::update_box_path takes it, the bytes decide"""
    made = _case_blob(sqy, oracle, old, shape, np.uint16, nthreads)
    assert made is not None
    blob, full = made
    o, e = (3, 5, 16), (shape[0] - 5, shape[1] - 28, shape[2] - 40)
    tile = _tile(e, np.uint16, 78)
    if "rmestbkrd" in new:
        rc, want = sqy.encode(new, _paste(full, o, tile), nthreads=nthreads)
        assert rc == 0
        want = bytes(want)
    else:
        want = _expect(sqy, oracle, new, full, o, tile, nthreads)
    d_blob = _to_device(blob)
    for subset in (1, 0):
        options("update_box_subset", subset)
        S = Sources(np.uint16, [tile], shift=2, pitch=True)
        out = {}
        names = _profile_names(sqy, lambda: out.update(r=_update(sqy, new, d_blob, len(blob), o, S, nthreads=nthreads, shape=shape)))
        assert out["r"][0] == 0 and out["r"][2] == want, (old, new, subset)
        if "accel=2" not in new:
            assert not any(k in names for k in SPLICE), names
        _unchanged(S)
    options("update_box_subset", 1)


@pytest.mark.parametrize("subset", [1, 0])
def test_capacity(sqy, oracle, options, subset):
    """a capacity equal to the blob's length succeeds; one byte less: 1, *dstlength = the bytes needed, every canary intact"""
    options("update_box_subset", subset)
    shape = (7, 33, 31)
    name = BSL + SMALL_CHUNKS
    blob, full = _blob(sqy, oracle, name, shape, np.uint16)
    o, e = (2, 3, 4), (3, 20, 20)
    tile = _tile(e, np.uint16, 79)
    want = _expect(sqy, oracle, name, full, o, tile)
    S = Sources(np.uint16, [tile])
    d_blob = _to_device(blob)
    rc, n, b = _update(sqy, name, d_blob, len(blob), o, S, cap=len(want))
    assert rc == 0 and b == want
    rc, n, b = _update(sqy, name, d_blob, len(blob), o, S, cap=len(want) - 1)
    assert rc == 1 and n == len(want) and b is None
    rc, n, b = _update(sqy, name, d_blob, len(blob), o, S, cap=sqy.max_compressed_length(name, shape, np.uint16))
    assert rc == 0 and b == want
    options("update_box_subset", 1)


def test_refusals(sqy, oracle):
    """each admission rule: 1, *dstlength = 0, the destination all canaries"""
    shape = (3, 5, 7)
    blob, full = _blob(sqy, oracle, BSL, shape, np.uint16)
    u8 = _blob(sqy, oracle, BSL, shape, np.uint8)[0]
    d_blob, d_u8 = _to_device(blob), _to_device(u8)
    tile = _tile((2, 3, 4), np.uint16, 80)
    S = Sources(np.uint16, [tile], pitch=True)
    assert S.strides[0] == (26, 7, 1)
    import torch
    cap = sqy.max_compressed_length(BSL, shape, np.uint16)
    buf = torch.full((cap,), CANARY, dtype=torch.uint8, device=_dev())
    good = dict(pipeline=BSL, src=d_blob.data_ptr(), n=len(blob), origin=(1, 1, 1), view=S.ptrs[0], shape=(2, 3, 4), strides=S.strides[0], dtype=np.uint16, dst=buf.data_ptr(),
                cap=cap)

    def call(**kw):
        a = dict(good, **kw)
        out = sqy.update_box_device(a["pipeline"], a["src"], a["n"], a["origin"], a["view"], a["shape"], a["strides"], a["dtype"], a["dst"], a["cap"])
        torch.cuda.synchronize()
        return out

    def refused(**kw):
        assert call(**kw) == (1, 0), kw
        assert (buf.cpu().numpy() == CANARY).all(), kw
    LONG_MAX = 2 ** 63 - 1
    for kw in (dict(pipeline=None), dict(src=None), dict(origin=None), dict(view=None), dict(shape=None, strides=None), dict(dst=None), dict(n=0), dict(n=-1), dict(cap=0),
               dict(cap=-5), dict(origin=(0, -1, 0)), dict(pipeline="nonsense->lz4"), dict(pipeline="quantiser->bitswap1->lz4", dtype=np.uint8, src=d_u8.data_ptr(), n=len(u8)),
               dict(strides=(40, 10, 2)), dict(strides=(26, 3, 1)), dict(strides=(20, 7, 1)), dict(view=S.ptrs[0] + 1), dict(shape=(2, 0, 4)),
               dict(src=d_u8.data_ptr(), n=len(u8)), dict(dtype=np.uint8), dict(origin=(1, 1), shape=(3, 4), strides=(7, 1)), dict(origin=(1,), shape=(4,), strides=(1,)),
               dict(origin=(2, 1, 1)), dict(origin=(1, 3, 1)), dict(origin=(1, 1, 4)), dict(origin=(LONG_MAX, 0, 0), shape=(1, 1, 1), strides=None),
               dict(pipeline="rmestbkrd->bitswap1->lz4", origin=(0, 0, 0), shape=(1, 1, 1), strides=None, src=_to_device(_blob(sqy, oracle, BSL, (1, 1, 5), np.uint16)[0]).data_ptr(),
                    n=len(_blob(sqy, oracle, BSL, (1, 1, 5), np.uint16)[0]))):
        refused(**kw)
    rc, n = call()
    assert rc == 0 and buf.cpu().numpy()[:n].tobytes() == _expect(sqy, oracle, BSL, full, (1, 1, 1), tile)
    _unchanged(S)


@pytest.mark.parametrize("pipeline", ["lz4", BSL])
def test_damage(sqy, oracle, pipeline):
    """a damaged frame inside the box's z-range: SQY_Decode's code, the destination all canaries; outside it: rc 0, the frame is carried
    over -- every frame but that one is the expectation's, and the full decode of the new blob reports it"""
    shape = (16, 64, 64)
    name = pipeline + SMALL_CHUNKS
    vol = (np.arange(np.prod(shape)) % 300).astype(np.uint16).reshape(shape)      # every 4 KiB chunk compressible
    old = _want(sqy, oracle, name, vol, 0, _dev())
    frames = _lz4_frames(old, sqy)
    bad = _damaged(old, frames[-1])
    rc_full, _ = sqy.decode(bad)
    assert rc_full not in (0, 1)
    d_bad = _to_device(bad)
    tile = _tile((1, 50, 40), np.uint16, 81)
    S = Sources(np.uint16, [tile], shift=2, pitch=True)
    rc, n, b = _update(sqy, name, d_bad, len(bad), (15, 5, 7), S, shape=shape)    # the last frame: needs the damaged LZ4 frame
    assert rc == rc_full and b is None
    rc, n, b = _update(sqy, name, d_bad, len(bad), (0, 5, 7), S, shape=shape)     # frame 0: its words lie in each plane's first chunk
    assert rc == 0
    want = _expect(sqy, oracle, name, vol, (0, 5, 7), tile)
    f_new, f_want = _lz4_frames(b, sqy), _lz4_frames(want, sqy)
    assert len(f_new) == len(f_want) == len(frames) and len(b) == len(want)
    for k, (g, w) in enumerate(zip(f_new, f_want)):
        same = b[g[0]:g[1] + g[2] + 4] == want[w[0]:w[1] + w[2] + 4]
        assert same == (k != len(frames) - 1), k
    assert b[f_new[-1][1]:f_new[-1][1] + f_new[-1][2]] == b"\xff" * f_new[-1][2]
    assert sqy.decode(b)[0] == rc_full
    _unchanged(S)


def test_two_host_threads_and_a_callers_stream(sqy, oracle):
    import torch
    shape = (23, 131, 151)
    made = [_blob(sqy, oracle, p, shape, np.uint16) for p in (BSL, "lz4")]
    tiles = [_tile((3, 100, 120), np.uint16, 82 + k) for k in range(2)]
    wants = [_expect(sqy, oracle, p, m[1], (9 + k, 2, 3), t) for k, (p, m, t) in enumerate(zip((BSL, "lz4"), made, tiles))]
    d_blobs = [_to_device(m[0]) for m in made]
    S = [Sources(np.uint16, [t], shift=2, pitch=True) for t in tiles]
    torch.cuda.synchronize()

    def one(k):
        s = torch.cuda.Stream(device=_dev())
        ok = True
        for _ in range(3):
            rc, n, b = _update(sqy, (BSL, "lz4")[k], d_blobs[k], len(made[k][0]), (9 + k, 2, 3), S[k], shape=shape, stream=s.cuda_stream)
            ok = ok and rc == 0 and b == wants[k]
        return ok
    with ThreadPoolExecutor(2) as ex:
        assert all(ex.map(one, range(2)))
    # a call on a non-default stream behind the kernel that made the view
    s = torch.cuda.Stream(device=_dev())
    e = (3, 100, 120)
    with torch.cuda.stream(s):
        view = torch.zeros(int(np.prod(e)), dtype=torch.int16, device=_dev())
        src = torch.from_numpy(tiles[0].view(np.int16).reshape(-1).copy()).pin_memory()
        cap = sqy.max_compressed_length(BSL, shape, np.uint16)
        out = torch.full((cap,), CANARY, dtype=torch.uint8, device=_dev())
        view.copy_(src, non_blocking=True)
        view.add_(0)                                                    # (a kernel on the stream writes the view)
        rc, n = sqy.update_box_device(BSL, d_blobs[0].data_ptr(), len(made[0][0]), (9, 2, 3), view.data_ptr(), e, None, np.uint16, out.data_ptr(), cap, stream=s.cuda_stream)
    assert rc == 0 and out[:n].cpu().numpy().tobytes() == wants[0]
