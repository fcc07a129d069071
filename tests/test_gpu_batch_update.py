"""SQYAMD_Update_BatchWindow_*: old blob + a window's new voxels -> new blob, many with one call.  The expectation is always built on the
CPU side: SQY_Decode of the old blob, a numpy paste, and the SINGLE call's blob for the pasted volume (test_gpu_encode_batch._want, which
holds that blob against the oracle) -- the call under test never supplies its own expectation.  The fused way (`bitswap1->lz4` blobs keep
their bit planes, the window is patched into them) and layer one ("batch_update_fused" = 0: decode dense, one paste, encode) must give the
same bytes, and each shows its launches in the profile.  Canary bytes in front of the destination, behind it and behind every blob hold."""
import hashlib
import threading

import numpy as np
import pytest

from sqeazy_amd import synth
from test_gpu_batch_window import SERIAL_SHAPE, SHAPES, Targets, _blob, _pack, _windows
from test_gpu_encode_batch import CANARY, GAP, _profile, _want

pytestmark = pytest.mark.gpu

BSL = "bitswap1->lz4"


def _dev():
    import torch
    return torch.device("cuda", 0)


class Sources(Targets):
    """Targets as window sources: view i holds the voxels tiles[i], pattern bytes lie between its rows and frames and around it"""

    def __init__(self, dtype, tiles, shift=0, pitch=False, salt=0):
        import torch
        super().__init__(dtype, [t.shape for t in tiles], shift=shift, pitch=pitch, salt=salt)
        for i, t in enumerate(tiles):
            self.host[self.bytes_of(i).reshape(-1)] = np.ascontiguousarray(t).view(np.uint8).reshape(-1)
        self.buf = torch.from_numpy(self.host.copy()).to(_dev())
        assert self.buf.data_ptr() % 16 == 0
        self.ptrs = [self.buf.data_ptr() + b for b in self.base]


def _update(sqy, pipeline, src, offs, lens, origins, S, nthreads=0, cap=None, stream=None, joint=None, shapes=None):
    """the call into slots of cap bytes filled with canaries, canaries in front of the first and behind the last: (rc, blobs or None).  The
    canaries around the slots must hold whatever rc is, the tables are zero when it is not 0, and the rest of the slot behind the blob
    holds for every blob in `joint` (None: all; a volume on the single-call path may use its whole slot)"""
    import torch
    n = len(offs)
    if cap is None:
        cap = max(sqy.max_compressed_length(pipeline, s, S.dtype) for s in shapes) + 13           # (no multiple of 16)
    buf = torch.full((2 * GAP + cap * n,), CANARY, dtype=torch.uint8, device=_dev())
    rc, o, l = sqy.update_batch_window_device(pipeline, src.data_ptr(), offs, lens, origins, S.ptrs, S.extents, S.strides, S.dtype, buf.data_ptr() + GAP, cap,
                                              nthreads=nthreads, stream=stream)
    torch.cuda.synchronize()
    h = buf.cpu().numpy()
    assert (h[:GAP] == CANARY).all() and (h[GAP + cap * n:] == CANARY).all(), "written outside the slots"
    assert np.array_equal(S.buf.cpu().numpy(), S.host), "a window's source was written"
    if rc:
        assert o == [0] * n and l == [0] * n
        return rc, None, h
    blobs = []
    for i in range(n):
        assert i * cap <= o[i] and l[i] > 0 and o[i] + l[i] <= (i + 1) * cap, (i, o[i], l[i])
        if joint is None or i in joint:
            assert o[i] == i * cap and (h[GAP + o[i] + l[i]:GAP + (i + 1) * cap] == CANARY).all(), "slot %d: written outside the blob" % i
        blobs.append(h[GAP + o[i]:GAP + o[i] + l[i]].tobytes())
    return rc, blobs, h


def _paste(full, origin, tile):
    v = np.array(full, copy=True)
    v[tuple(slice(o, o + n) for o, n in zip(origin, tile.shape))] = tile
    return v


_tiles = {}


def _tile(extent, dtype, k):
    """the new voxels of a window: made once per (extent, dtype, k)"""
    key = (tuple(extent), np.dtype(dtype).name, k)
    if key not in _tiles:
        _tiles[key] = synth.stack(tuple(extent), dtype, seed=900 + k)
    return _tiles[key]


def _expect(sqy, oracle, pipeline, full, origin, tile, nthreads=0):
    """the single call's blob for the pasted volume, made once per volume"""
    pasted = _paste(full, origin, tile)
    return _want(sqy, oracle, pipeline, pasted, nthreads, _dev(), key=("update", pasted.shape, pasted.dtype.name, hashlib.sha1(pasted.tobytes()).hexdigest()))


@pytest.mark.parametrize("dtype", [np.uint16, np.uint8], ids=["uint16", "uint8"])
def test_bytes_both_layers(sqy, oracle, options, dtype):
    """every window of every blob shape in one call (a blob is named once per window); sources dense, then pitched and 2 bytes off the
    16-byte grid; fused and layer one"""
    item = np.dtype(dtype).itemsize
    made = [(s, _blob(sqy, oracle, BSL, s, dtype)) for s in SHAPES]
    src, boffs, blens = _pack([b[0] for _, b in made], gaps=[3 + 2 * k for k in range(len(made))])
    offs, lens, origins, tiles, want, shapes = [], [], [], [], [], []
    for k, (s, (_, full)) in enumerate(made):
        for j, (o, e) in enumerate(_windows(s, item)):
            offs.append(boffs[k]); lens.append(blens[k]); origins.append(o); shapes.append(s)
            tiles.append(_tile(e, dtype, j))
            want.append(_expect(sqy, oracle, BSL, full, o, tiles[-1]))
    for fused in (1, 0):
        options("batch_update_fused", fused)
        for shift, pitch in ((0, False), (2, True)):
            S = Sources(dtype, tiles, shift=shift, pitch=pitch, salt=3 + shift)
            rc, blobs, _ = _update(sqy, BSL, src, offs, lens, origins, S, shapes=shapes)
            assert rc == 0
            for i, (b, w) in enumerate(zip(blobs, want)):
                assert b == w, (fused, shift, pitch, shapes[i], origins[i], tiles[i].shape)


def _some(sqy, oracle, old_pipeline, dtype=np.uint16, new_pipeline=BSL, nthreads=0):
    """several windowed blobs for one call: (src, offs, lens, origins, tiles, want, shapes)"""
    picks = [((7, 33, 31), (1, 1, 1), (5, 31, 29)), ((3, 128, 128), (2, 0, 0), (1, 128, 128)), ((2, 3, 300), (0, 0, 127), (2, 3, 2)), ((16, 128, 128), (3, 5, 16), (9, 100, 64))]
    blobs = [_blob(sqy, oracle, old_pipeline, s, dtype) for s, _, _ in picks]
    picks = [p for p, b in zip(picks, blobs) if b is not None]          # (diff3x3x1 refuses some geometries at encode)
    blobs = [b for b in blobs if b is not None]
    assert len(blobs) >= 3
    src, offs, lens = _pack([b[0] for b in blobs])
    tiles = [_tile(e, dtype, 40 + k) for k, (_, _, e) in enumerate(picks)]
    want = [_expect(sqy, oracle, new_pipeline, b[1], o, t, nthreads) for b, (_, o, _), t in zip(blobs, picks, tiles)]
    return src, offs, lens, [o for _, o, _ in picks], tiles, want, [s for s, _, _ in picks]


def test_launch_counts(sqy, oracle, options):
    src, offs, lens, origins, tiles, want, shapes = _some(sqy, oracle, BSL)
    S = Sources(np.uint16, tiles, shift=2, pitch=True)
    run = lambda: _update(sqy, BSL, src, offs, lens, origins, S, shapes=shapes)
    # fused: one patch launch for the one encode group, no transposer either way, no paste, no copy of the planes to their places
    ((rc, blobs, _), p) = _profile(sqy, run)
    assert rc == 0 and blobs == want
    assert p["batch_bitswap1_patch"][1] == 1 and p["batch_lz4_decode"][1] == 1 and p["batch_lz4_frame_gather"][1] == 1, p
    assert not any(k.startswith("batch_bitswap1_decode") for k in p) and "batch_bitswap1" not in p and "batch_window_paste" not in p and "batch_copy" not in p, p
    # a group bound of one byte: every volume an encode group of its own, a patch launch each
    bound = sqy.get_option("encode_batch_group_bytes")
    options("encode_batch_group_bytes", 1)
    ((rc, blobs, _), p) = _profile(sqy, run)
    assert rc == 0 and blobs == want
    assert p["batch_bitswap1_patch"][1] == len(tiles) and p["batch_lz4_frame_gather"][1] == len(tiles) and "batch_bitswap1" not in p and "batch_window_paste" not in p, p
    options("encode_batch_group_bytes", bound)
    # layer one: exactly one paste launch per call, the dense transposers on both sides
    options("batch_update_fused", 0)
    ((rc, blobs, _), p) = _profile(sqy, run)
    assert rc == 0 and blobs == want
    assert p["batch_window_paste"][1] == 1 and p["batch_bitswap1_decode"][1] == 1 and p["batch_bitswap1"][1] == 1 and "batch_bitswap1_patch" not in p, p


def test_the_old_voxels_give_the_old_blob(sqy, oracle, options):
    """a window filled with the old voxels: the old blob byte for byte, both layers"""
    picks = [((7, 33, 31), (1, 1, 1), (5, 31, 29)), ((3, 5, 7), (0, 0, 0), (3, 5, 7)), ((16, 128, 128), (3, 5, 16), (9, 100, 64))]
    made = [_blob(sqy, oracle, BSL, s, np.uint16) for s, _, _ in picks]
    src, offs, lens = _pack([b[0] for b in made])
    tiles = [np.ascontiguousarray(b[1][tuple(slice(a, a + n) for a, n in zip(o, e))]) for b, (_, o, e) in zip(made, picks)]
    S = Sources(np.uint16, tiles, shift=2, pitch=True)
    for fused in (1, 0):
        options("batch_update_fused", fused)
        rc, blobs, _ = _update(sqy, BSL, src, offs, lens, [o for _, o, _ in picks], S, shapes=[s for s, _, _ in picks])
        assert rc == 0 and blobs == [b[0] for b in made], fused


@pytest.mark.parametrize("old, new", [("lz4", BSL), ("quantiser->bitswap1->lz4", BSL), ("diff3x3x1->bitswap1->lz4", BSL), ("lz4", "lz4"), (BSL, "lz4"),
                                      (BSL, "quantiser->bitswap1->lz4"), (BSL, "diff3x3x1->bitswap1->lz4")])
def test_other_old_blobs_and_pipelines(sqy, oracle, options, old, new):
    """the old blobs of other pipelines, and other new pipelines: one paste launch, no patch launch -- and for an old `lz4` blob, whose LZ4
    output is the volume, no dense decode copy in front of the paste; with the option off the copy is there and the bytes are the same"""
    src, offs, lens, origins, tiles, want, shapes = _some(sqy, oracle, old, new_pipeline=new)
    S = Sources(np.uint16, tiles, shift=2, pitch=True)
    for fused in (1, 0):
        options("batch_update_fused", fused)
        ((rc, blobs, _), p) = _profile(sqy, lambda: _update(sqy, new, src, offs, lens, origins, S, shapes=shapes, joint=() if new.startswith("diff") else None))
        assert rc == 0 and blobs == want
        assert p["batch_window_paste"][1] == 1 and "batch_bitswap1_patch" not in p, p
        if old == "lz4":
            assert ("batch_copy" not in p) if fused else p["batch_copy"][1] == 1, p


def test_the_serial_layout(sqy, oracle):
    """`bitswap1->lz4` encoded with nthreads = 1 over two chunks: no joint decode, so no planes to keep -- decoded on its own, pasted"""
    blob, full = _blob(sqy, oracle, "bitswap1->lz4(blocksize_kb=64,framestep_kb=64)", SERIAL_SHAPE, np.uint16, 1)
    src, offs, lens = _pack([blob, blob])
    origins, tiles = [(3, 5, 7), (0, 0, 0)], [_tile((6, 50, 40), np.uint16, 50), _tile((1, 64, 64), np.uint16, 51)]
    want = [_expect(sqy, oracle, BSL, full, o, t) for o, t in zip(origins, tiles)]
    S = Sources(np.uint16, tiles, shift=2, pitch=True)
    ((rc, blobs, _), p) = _profile(sqy, lambda: _update(sqy, BSL, src, offs, lens, origins, S, shapes=[SERIAL_SHAPE] * 2))
    assert rc == 0 and blobs == want
    assert p["batch_window_paste"][1] == 1 and "batch_bitswap1_patch" not in p, p


def test_a_mixed_call(sqy, oracle):
    """fused and unfused blobs in one call: one patch launch for the one encode group, one paste launch for the others (the decode group
    is mixed as well: its `lz4` and kept-planes members reach their places by the batched copy)"""
    shape, origin = (7, 33, 31), (1, 1, 1)
    tile = _tile((5, 31, 29), np.uint16, 60)
    olds = [BSL, "lz4", "quantiser->bitswap1->lz4", BSL]
    made = [_blob(sqy, oracle, p, shape, np.uint16) for p in olds]
    src, offs, lens = _pack([b[0] for b in made])
    want = [_expect(sqy, oracle, BSL, b[1], origin, tile) for b in made]
    S = Sources(np.uint16, [tile] * 4, shift=2, pitch=True)
    ((rc, blobs, _), p) = _profile(sqy, lambda: _update(sqy, BSL, src, offs, lens, [origin] * 4, S, shapes=[shape] * 4))
    assert rc == 0 and blobs == want
    assert p["batch_bitswap1_patch"][1] == 1 and p["batch_window_paste"][1] == 1 and p["batch_bitswap1"][1] == 1 and p["batch_copy"][1] == 1, p


def test_nthreads_and_lower_ranks(sqy, oracle):
    """the new blobs in the layout nthreads asks for; NULL origins; blobs of ranks 1 and 2"""
    src, offs, lens, origins, tiles, want, shapes = _some(sqy, oracle, BSL, nthreads=1)
    S = Sources(np.uint16, tiles)
    rc, blobs, _ = _update(sqy, BSL, src, offs, lens, origins, S, nthreads=1, shapes=shapes, joint=())
    assert rc == 0 and blobs == want
    for shape, origin, extent in (((5, 7), (1, 2), (3, 4)), ((37,), (16,), (20,)), ((5, 7), None, (2, 6))):
        vol = synth.stack((1, 1, int(np.prod(shape))), np.uint16, seed=930).reshape(shape)
        rc, blob = sqy.encode(BSL, vol)
        assert rc == 0
        tile = synth.stack((1, 1, int(np.prod(extent))), np.uint16, seed=931).reshape(extent)
        src, offs, lens = _pack([blob, blob])
        S = Sources(np.uint16, [tile, tile], shift=2, pitch=True)
        rc, blobs, _ = _update(sqy, BSL, src, offs, lens, None if origin is None else [origin, origin], S, shapes=[shape] * 2)
        w = _want(sqy, oracle, BSL, _paste(vol, origin or (0,) * len(shape), tile), 0, _dev())
        assert rc == 0 and blobs == [w, w], shape


def test_a_box_into_a_tiled_store(sqy, oracle):
    """tile_views grid -> Batch encode -> update with box_windows of a box that cuts tiles in all three dimensions -> Decode_Batch of the
    tiles = the parent with the box pasted"""
    import torch
    shape, tile, origin, extent = (4, 40, 48), (2, 16, 16), (1, 9, 5), (2, 25, 30)
    parent = synth.stack(shape, np.uint16, seed=940)
    box = synth.stack(extent, np.uint16, seed=941)
    d_parent = torch.from_numpy(parent.copy()).to(_dev())
    ptrs, shapes, strides = sqy.tile_views(d_parent.data_ptr(), shape, tile, 2)
    slot = sqy.max_compressed_length(BSL, tile, np.uint16) + 13
    store = torch.zeros(slot * len(ptrs), dtype=torch.uint8, device=_dev())
    rc, offs, lens = sqy.encode_batch_strided_device(BSL, ptrs, shapes, strides, np.uint16, store.data_ptr(), slot)
    assert rc == 0 and len(offs) == 2 * 3 * 3
    d_box = torch.from_numpy(box.copy()).to(_dev())
    idx, origins, vptrs, vshapes, vstrides = sqy.box_windows(shape, tile, origin, extent, d_box.data_ptr(), None, 2)
    assert len(idx) == 2 * 3 * 3 and any(s != tuple(tile) for s in vshapes)
    fresh = torch.zeros(slot * len(idx), dtype=torch.uint8, device=_dev())
    rc, noffs, nlens = sqy.update_batch_window_device(BSL, store.data_ptr(), [offs[i] for i in idx], [lens[i] for i in idx], origins, vptrs, vshapes, vstrides, np.uint16,
                                                      fresh.data_ptr(), slot)
    assert rc == 0
    back = torch.zeros(parent.shape, dtype=torch.int16, device=_dev())
    bptrs, bshapes, bstrides = sqy.tile_views(back.data_ptr(), shape, tile, 2)
    rc, _ = sqy.decode_batch_strided_device(fresh.data_ptr(), noffs, nlens, [bptrs[i] for i in idx], [bshapes[i] for i in idx], [bstrides[i] for i in idx], np.uint16)
    assert rc == 0
    torch.cuda.synchronize()
    assert np.array_equal(back.cpu().numpy().view(np.uint16), _paste(parent, origin, box))


def test_capacity(sqy, oracle):
    """one byte short of the largest blob: 1 with zeroed tables; exactly its size: 0"""
    src, offs, lens, origins, tiles, want, shapes = _some(sqy, oracle, BSL)
    S = Sources(np.uint16, tiles, shift=2, pitch=True)
    most = max(len(w) for w in want)
    rc, blobs, _ = _update(sqy, BSL, src, offs, lens, origins, S, cap=most - 1)
    assert rc == 1 and blobs is None
    rc, blobs, _ = _update(sqy, BSL, src, offs, lens, origins, S, cap=most)
    assert rc == 0 and blobs == want


def test_refusals_on_the_device_side(sqy, oracle):
    """what only the header can tell: 1, the tables zeroed, every byte of the destination as it was"""
    shape = (3, 5, 7)
    a = _blob(sqy, oracle, BSL, shape, np.uint16)[0]
    u8 = _blob(sqy, oracle, BSL, shape, np.uint8)[0]
    src, offs, lens = _pack([a, a, u8])
    good = ((1, 1, 1), (2, 3, 4))

    def refused(origin, extent, blob=1):
        if len(extent) == 3:
            org, ext = [good[0], origin], [good[1], extent]
        else:                                                           # (one rank per call)
            org, ext = [origin, origin], [extent, extent]
        S = Sources(np.uint16, [np.zeros(e, np.uint16) for e in ext], pitch=True)
        rc, blobs, h = _update(sqy, BSL, src, [offs[0], offs[blob]], [lens[0], lens[blob]], org, S, cap=4096)
        assert rc == 1 and blobs is None and (h == CANARY).all(), (origin, extent)
    for k in range(3):                                                  # origin + extent one voxel beyond the shape, each dimension in turn
        o, e = [1, 1, 1], [2, 4, 6]
        e[k] += 1
        refused(tuple(o), tuple(e))
    refused((0, 0), (5, 7))                                             # a rank other than the header's
    refused((0,), (7,))
    refused(good[0], good[1], blob=2)                                   # a blob of the other voxel type


def test_a_damaged_old_blob(sqy, oracle):
    """a damaged blob between two good ones: the code SQY_Decode gives it, the tables zeroed, nothing written outside the slots"""
    shape, origin = (12, 64, 64), (3, 5, 7)
    blob, full = _blob(sqy, oracle, BSL, shape, np.uint16)
    off = sqy.header_size(blob)
    body, size = None, 0
    while off < len(blob):                                              # the first compressed frame: its block becomes bytes the decoder refuses
        assert blob[off:off + 4] == bytes([0x04, 0x22, 0x4D, 0x18])
        word = int.from_bytes(blob[off + 7:off + 11], "little")
        if not word >> 31:
            body, size = off + 11, word
            break
        off += 11 + (word & 0x7fffffff) + 4
    assert body is not None
    bad = bytearray(blob)
    bad[body:body + size] = b"\xff" * size
    rc_alone, _ = sqy.decode(bytes(bad))
    assert rc_alone not in (0, 1)
    src, offs, lens = _pack([blob, bytes(bad), blob], gaps=(0, 5, 3))
    S = Sources(np.uint16, [_tile((6, 50, 40), np.uint16, 70)] * 3, shift=2, pitch=True)
    rc, blobs, _ = _update(sqy, BSL, src, offs, lens, [origin] * 3, S, shapes=[shape] * 3)
    assert rc == rc_alone and blobs is None


def test_callers_stream_and_two_host_threads(sqy, oracle):
    import torch
    sets = [_some(sqy, oracle, p) + (torch.cuda.Stream(device=_dev()),) for p in (BSL, "lz4")]
    src, offs, lens, origins, tiles, want, shapes, s = sets[0]
    S = Sources(np.uint16, tiles, shift=2, pitch=True)
    rc, blobs, _ = _update(sqy, BSL, src, offs, lens, origins, S, shapes=shapes, stream=s.cuda_stream)
    assert rc == 0 and blobs == want
    torch.cuda.synchronize()
    ok = [False, False]

    def one(t):
        src, offs, lens, origins, tiles, want, shapes, s = sets[t]
        good = True
        cap = max(sqy.max_compressed_length(BSL, sh, np.uint16) for sh in shapes) + 13
        for r in range(3):
            S = Sources(np.uint16, tiles, shift=2 * (r & 1), pitch=True, salt=r)
            buf = torch.full((cap * len(tiles),), CANARY, dtype=torch.uint8, device=_dev())
            rc, o, l = sqy.update_batch_window_device(BSL, src.data_ptr(), offs, lens, origins, S.ptrs, S.extents, S.strides, np.uint16, buf.data_ptr(), cap,
                                                      stream=s.cuda_stream)
            s.synchronize()
            h = buf.cpu().numpy()
            good = good and rc == 0 and [h[a:a + n].tobytes() for a, n in zip(o, l)] == want
        ok[t] = good
    th = [threading.Thread(target=one, args=(t,)) for t in range(2)]
    for x in th:
        x.start()
    for x in th:
        x.join()
    assert all(ok)
