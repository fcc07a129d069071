"""SQYAMD_Decode_BatchWindow_*: a box of every blob decoded into a view of the box's shape.  Every window must equal the same box of what
SQY_Decode gives for its blob (itself held to the oracle's inverse where it has one, and to the encoded volume where the pipeline is
lossless), at exactly the view's voxel places: all views of a call lie in one buffer filled with a position-dependent pattern, and the
whole buffer is compared with an image built on the CPU -- the gaps between a view's rows and frames and around the views included.
The fused paths (the windowed transposer, the copy out of the LZ4 output) and layer one ("batch_window_fused" = 0) must give the same
bytes, and each shows its launches in the profile."""
import threading

import numpy as np
import pytest

from batch_window_cases import BOX_CASES, pitched
from sqeazy_amd import synth
from test_gpu_batch_strided import _pattern
from test_gpu_encode_batch import _profile

pytestmark = pytest.mark.gpu

GAP = 64
# blob shapes: no planes | tail of 9 voxels at 16 bit, of 1 at 8 bit | odd | runs of 128 voxels straddle rows | one run = one row, one whole
# chunk | two transposer tiles, frame 2 begins exactly at tile 1
SHAPES = ((1, 1, 5), (3, 5, 7), (7, 33, 31), (2, 3, 300), (16, 128, 128), (3, 128, 128))
SERIAL_SHAPE = (12, 64, 64)       # two 64 KiB chunks of 16-bit voxels


def _dev():
    import torch
    return torch.device("cuda", 0)


def _windows(shape, itemsize):
    """the windows (origin, extent) of a blob of `shape`"""
    bZ, bY, bX = shape
    n = bZ * bY * bX
    L = n // (8 * itemsize) * (8 * itemsize)                    # where the tail begins
    coords = lambda i: (i // (bY * bX), i // bX % bY, i % bX)
    w = [((0, 0, 0), shape), ((0, 0, 0), (1, 1, 1)), ((bZ - 1, bY - 1, bX - 1), (1, 1, 1))]
    if L < n:
        w.append((coords(L), (1, 1, 1)))                        # a voxel of the tail
        x0 = max(L - (n - bX), 0)                               # the tail's part of the last row: tail voxels only
        w.append(((bZ - 1, bY - 1, x0), (1, 1, bX - x0)))
    w.append(((bZ // 2, bY // 2, 0), (1, 1, bX)))               # one row
    w += [((0, 0, ox), (bZ, bY, 1)) for ox in (0, 15, 16, 127, 128) if ox < bX]      # one column
    inner = [(1, d - 2) if d >= 3 else (0, d) for d in shape]   # an interior box at (1, 1, 1) where the blob has an interior
    w.append((tuple(o for o, _ in inner), tuple(e for _, e in inner)))
    if shape == (3, 128, 128):
        w += [((1, 0, 0), (1, 128, 128)), ((2, 0, 0), (1, 128, 128))]
    for o, e in w:
        assert all(0 <= a and n_ >= 1 and a + n_ <= d for a, n_, d in zip(o, e, shape))
    return w


class Targets:
    """the views of one call in ONE device buffer of pattern bytes: view i has the extent extents[i], dense strides or pitched ones (rows
    X + 3, frames Y (X + 3) + 5 voxels apart), its base on the 16-byte grid or `shift` bytes behind it, GAP pattern bytes around it"""

    def __init__(self, dtype, extents, shift=0, pitch=False, salt=0):
        import torch
        self.dtype, self.extents = np.dtype(dtype), [tuple(e) for e in extents]
        item = self.dtype.itemsize
        self.base, self.strides = [], []
        at = GAP
        for e in self.extents:
            lead = (1,) * (3 - len(e))
            Z, Y, X = lead + e
            st = (Y * (X + 3) + 5, X + 3, 1) if pitch else (Y * X, X, 1)
            at = (at + 15) & ~15
            self.base.append(at + shift)
            self.strides.append(st[3 - len(e):])
            at += shift + ((Z - 1) * st[0] + (Y - 1) * st[1] + X) * item + GAP
        self.host = _pattern(at, salt)
        self.buf = torch.from_numpy(self.host.copy()).to(_dev())
        assert self.buf.data_ptr() % 16 == 0
        self.ptrs = [self.buf.data_ptr() + b for b in self.base]

    def bytes_of(self, i):
        """the byte offsets of view i's voxels in the buffer, shape extent + (itemsize,)"""
        e, st, item = self.extents[i], self.strides[i], self.dtype.itemsize
        vox = sum(np.arange(n).reshape([-1 if k == j else 1 for k in range(len(e))]) * st[j] for j, n in enumerate(e))
        return self.base[i] + vox[..., None] * item + np.arange(item)

    def expect(self, tiles, skip=()):
        """(image, mask): the buffer with tiles[i] in view i and everything else as it was; mask is False on the views in `skip`"""
        want, mask = self.host.copy(), np.ones(self.host.size, dtype=bool)
        for i, t in enumerate(tiles):
            idx = self.bytes_of(i)
            if i in skip:
                mask[idx.reshape(-1)] = False
            else:
                want[idx.reshape(-1)] = np.ascontiguousarray(t).view(np.uint8).reshape(-1)
        return want, mask

    def read(self):
        import torch
        torch.cuda.synchronize()
        return self.buf.cpu().numpy()


def _same(got, want, mask=None):
    bad = np.flatnonzero((got != want) if mask is None else ((got != want) & mask))
    assert bad.size == 0, "%d bytes differ, the first at %d" % (bad.size, bad[0])


def _pack(blobs, gaps=None):
    """blobs (bytes) in one device buffer, gaps[i] bytes in front of blob i: (buffer, offsets, lengths)"""
    import torch
    gaps = gaps or [3] * len(blobs)
    offs, parts, at = [], [], 0
    for b, g in zip(blobs, gaps):
        parts.append(b"\x00" * g)
        at += g
        offs.append(at)
        parts.append(b)
        at += len(b)
    host = np.frombuffer(b"".join(parts), dtype=np.uint8).copy()
    return torch.from_numpy(host).to(_dev()), offs, [len(b) for b in blobs]


_blobs = {}


def _blob(sqy, oracle, pipeline, shape, dtype, nthreads=0):
    """(blob, full) for the synthetic stack of `shape`: full is SQY_Decode's volume -- the encoded one where the pipeline is lossless, the
    oracle's inverse where it has one.  None: the pipeline does not take the shape.  Made once and never changed."""
    key = (pipeline, tuple(shape), np.dtype(dtype).name, nthreads)
    if key not in _blobs:
        vol = synth.stack(shape, dtype, seed=700 + len(shape) + shape[2] % 97)
        rc, blob = sqy.encode(pipeline, vol, nthreads=nthreads)
        if rc:
            _blobs[key] = None
            return None
        rc, full = sqy.decode(blob)
        assert rc == 0 and full.shape == tuple(shape) and full.dtype == np.dtype(dtype)
        if "quantiser" not in pipeline:
            assert np.array_equal(full, vol), (pipeline, shape)
        try:
            ref = oracle.pipeline_decode(blob)
        except (ValueError, KeyError, NotImplementedError):
            ref = None
        if ref is not None:
            assert np.array_equal(np.ascontiguousarray(ref).reshape(-1).view(dtype), full.reshape(-1)), (pipeline, shape)
        full.setflags(write=False)
        _blobs[key] = (blob, full)
    return _blobs[key]


def _cut(full, origin, extent):
    return full[tuple(slice(o, o + n) for o, n in zip(origin, extent))]


def _decode_windows(sqy, src, offs, lens, origins, T, stream=None):
    rc, decoded = sqy.decode_batch_window_device(src.data_ptr(), offs, lens, origins, T.ptrs, T.extents, T.strides, T.dtype, stream=stream)
    return rc, decoded, T.read()


CASES = [("bitswap1->lz4", np.uint16, 0), ("bitswap1->lz4", np.uint8, 0), ("lz4", np.uint16, 0), ("lz4", np.uint8, 0), ("quantiser->bitswap1->lz4", np.uint16, 0),
         ("diff3x3x1->bitswap1->lz4", np.uint16, 0), ("frame_shuffle->lz4", np.uint8, 0), ("bitswap1", np.uint16, 0),
         ("bitswap1->lz4(blocksize_kb=4,framestep_kb=4)", np.uint16, 0), ("bitswap1->lz4(blocksize_kb=64,framestep_kb=64)", np.uint16, 1)]


@pytest.mark.parametrize("pipeline, dtype, nthreads", CASES, ids=["%s-%s%s" % (p, np.dtype(d).name, "-serial" if t else "") for p, d, t in CASES])
def test_voxels(sqy, oracle, options, pipeline, dtype, nthreads):
    """every window of every blob shape in one call (a blob is named once per window), with the views' bases on and one voxel behind the
    16-byte grid, dense and pitched; then all of it again through layer one"""
    item = np.dtype(dtype).itemsize
    shapes = (SERIAL_SHAPE,) if nthreads else SHAPES
    made = [(s, _blob(sqy, oracle, pipeline, s, dtype, nthreads)) for s in shapes]
    made = [(s, b) for s, b in made if b is not None]                   # (diff3x3x1 and frame_shuffle refuse some geometries at encode)
    assert len(made) >= (1 if nthreads else 3), [s for s, _ in made]
    src, boffs, blens = _pack([b[0] for _, b in made], gaps=[3 + 2 * k for k in range(len(made))])
    offs, lens, origins, extents, tiles = [], [], [], [], []
    for k, (s, (_, full)) in enumerate(made):
        for o, e in _windows(s, item):
            offs.append(boffs[k]); lens.append(blens[k]); origins.append(o); extents.append(e)
            tiles.append(_cut(full, o, e))
    images = {}
    for fused in (1, 0):
        options("batch_window_fused", fused)
        for shift in (0, item):
            for pitch in (False, True):
                T = Targets(dtype, extents, shift=shift, pitch=pitch, salt=7 * shift + pitch)
                rc, decoded, got = _decode_windows(sqy, src, offs, lens, origins, T)
                assert rc == 0 and decoded == [t.size * item for t in tiles], (fused, shift, pitch)
                want, _ = T.expect(tiles)
                _same(got, want)
                if fused:
                    images[(shift, pitch)] = got
                else:
                    assert np.array_equal(got, images[(shift, pitch)])


def test_origins_null_and_lower_ranks(sqy, oracle):
    """NULL origins: every window at its blob's first voxel; blobs of ranks 1 and 2"""
    for shape, origin, extent in (((5, 7), (1, 2), (3, 4)), ((37,), (16,), (20,)), ((5, 7), None, (2, 6))):
        vol = synth.stack((1, 1, int(np.prod(shape))), np.uint16, seed=730).reshape(shape)
        rc, blob = sqy.encode("bitswap1->lz4", vol)
        assert rc == 0
        src, offs, lens = _pack([blob, blob])
        for pitch in (False, True):
            T = Targets(np.uint16, [extent, extent], shift=2, pitch=pitch)
            rc, decoded, got = _decode_windows(sqy, src, offs, lens, None if origin is None else [origin, origin], T)
            assert rc == 0 and decoded == [int(np.prod(extent)) * 2] * 2
            _same(got, T.expect([_cut(vol, origin or (0,) * len(shape), extent)] * 2)[0])


def _batch_of(sqy, oracle, pipeline, dtype=np.uint16):
    """several windowed blobs for one group: (src, offs, lens, origins, extents, tiles)"""
    picks = [((7, 33, 31), (1, 1, 1), (5, 31, 29)), ((3, 128, 128), (2, 0, 0), (1, 128, 128)), ((2, 3, 300), (0, 0, 127), (2, 3, 2)), ((16, 128, 128), (3, 5, 16), (9, 100, 64))]
    blobs = [_blob(sqy, oracle, pipeline, s, dtype) for s, _, _ in picks]
    src, offs, lens = _pack([b[0] for b in blobs])
    return src, offs, lens, [o for _, o, _ in picks], [e for _, _, e in picks], [_cut(b[1], o, e) for b, (_, o, e) in zip(blobs, picks)]


def test_launches(sqy, oracle, options):
    def run(pipeline):
        src, offs, lens, origins, extents, tiles = _batch_of(sqy, oracle, pipeline)      # (the blobs are made outside the profile)
        T = Targets(np.uint16, extents, shift=2, pitch=True)
        ((rc, _, got), p) = _profile(sqy, lambda: _decode_windows(sqy, src, offs, lens, origins, T))
        assert rc == 0
        _same(got, T.expect(tiles)[0])
        return p
    p = run("bitswap1->lz4")
    assert p["batch_bitswap1_decode_window"][1] == 1 and p["batch_lz4_decode"][1] == 1, p
    assert not any(k in p for k in ("batch_bitswap1_decode_strided", "batch_bitswap1_decode", "batch_unpack", "batch_window_copy")), p
    p = run("lz4")
    assert p["batch_copy_window"][1] == 1 and not any(k in p for k in ("batch_copy_strided", "batch_copy", "batch_unpack", "batch_window_copy")), p
    p = run("quantiser->bitswap1->lz4")
    assert p["batch_window_copy"][1] == 1 and p["batch_quantiser_decode"][1] == 1 and "batch_unpack" not in p, p
    options("batch_window_fused", 0)
    for pipeline in ("bitswap1->lz4", "lz4"):
        p = run(pipeline)
        assert p["batch_window_copy"][1] == 1 and "batch_bitswap1_decode_window" not in p and "batch_copy_window" not in p, p


def test_one_group_per_blob(sqy, oracle, options):
    """a group bound of one byte: every blob a group of its own, the window launches' tables made again group after group"""
    options("decode_batch_group_bytes", 1)
    for pipeline, name in (("bitswap1->lz4", "batch_bitswap1_decode_window"), ("lz4", "batch_copy_window")):
        src, offs, lens, origins, extents, tiles = _batch_of(sqy, oracle, pipeline)
        T = Targets(np.uint16, extents, shift=2, pitch=True)
        ((rc, _, got), p) = _profile(sqy, lambda: _decode_windows(sqy, src, offs, lens, origins, T))
        assert rc == 0 and p[name][1] == len(extents) and p["batch_lz4_decode"][1] == len(extents), p
        _same(got, T.expect(tiles)[0])


@pytest.mark.parametrize("pipeline", ["bitswap1->lz4", "lz4", "quantiser->bitswap1->lz4"])
def test_whole_blob_windows_are_the_strided_call(sqy, oracle, pipeline):
    """every window its whole blob: the launches of decode_batch_strided_device, name by name and count by count -- and its bytes"""
    shapes = [(7, 33, 31), (3, 5, 7), (3, 128, 128)]
    blobs = [_blob(sqy, oracle, pipeline, s, np.uint16) for s in shapes]
    src, offs, lens = _pack([b[0] for b in blobs])
    tiles = [b[1] for b in blobs]
    for pitch in (True, False):
        T = Targets(np.uint16, shapes, shift=2, pitch=pitch)
        ((rc, decoded), p_strided) = _profile(sqy, lambda: sqy.decode_batch_strided_device(src.data_ptr(), offs, lens, T.ptrs, T.extents, T.strides, np.uint16))
        assert rc == 0
        want = T.read()
        _same(want, T.expect(tiles)[0])
        for origins in (None, [(0, 0, 0)] * 3):
            W = Targets(np.uint16, shapes, shift=2, pitch=pitch)
            ((rc, decoded_w, got), p) = _profile(sqy, lambda: _decode_windows(sqy, src, offs, lens, origins, W))
            assert rc == 0 and decoded_w == decoded and np.array_equal(got, want)
            assert sorted(p) == sorted(p_strided) and all(p[k][1] == n for k, (_, n) in p_strided.items()), (p, p_strided)
            assert not any("window" in k for k in p), p


@pytest.mark.parametrize("pitch", [False, True], ids=["dense", "pitched"])
def test_a_box_from_a_tiled_store(sqy, pitch):
    import torch
    (shape, tile), boxes = next((k, v) for k, v in BOX_CASES.items() if k[0] == (9, 40, 72))
    parent = synth.stack(shape, np.uint16, seed=760)
    d_parent = torch.from_numpy(parent.copy()).to(_dev())
    ptrs, shapes, strides = sqy.tile_views(d_parent.data_ptr(), shape, tile, 2)
    slot = sqy.max_compressed_length("bitswap1->lz4", tile, np.uint16) + 13
    store = torch.zeros(slot * len(ptrs), dtype=torch.uint8, device=_dev())
    rc, offs, lens = sqy.encode_batch_strided_device("bitswap1->lz4", ptrs, shapes, strides, np.uint16, store.data_ptr(), slot)
    assert rc == 0 and len(offs) == 27
    for origin, extent in boxes:
        T = Targets(np.uint16, [extent], shift=2, pitch=pitch)
        idx, origins, vptrs, vshapes, vstrides = sqy.box_windows(shape, tile, origin, extent, T.ptrs[0], T.strides[0] if pitch else None, 2)
        assert len(idx) == {(9, 40, 72): 27, (2, 2, 2): 8}.get(tuple(extent), 1 if extent != (9, 1, 72) else 9)
        rc, decoded = sqy.decode_batch_window_device(store.data_ptr(), [offs[i] for i in idx], [lens[i] for i in idx], origins, vptrs, vshapes, vstrides, np.uint16)
        assert rc == 0 and decoded == [int(np.prod(s)) * 2 for s in vshapes] and sum(decoded) == int(np.prod(extent)) * 2
        _same(T.read(), T.expect([_cut(parent, origin, extent)])[0])


def test_refusals(sqy, oracle):
    """1, decoded_bytes zeroed, nothing written -- the good window in front of the bad one included"""
    shape = (3, 5, 7)
    a = _blob(sqy, oracle, "bitswap1->lz4", shape, np.uint16)[0]
    u8 = _blob(sqy, oracle, "bitswap1->lz4", shape, np.uint8)[0]
    src, offs, lens = _pack([a, a, u8])
    good = ((1, 1, 1), (2, 3, 4))

    def refused(origin, extent, blob=1, shift=0, null=False, n=2):
        ext = [good[1], extent][:n]
        T = Targets(np.uint16, [good[1], tuple(max(x, 1) for x in extent)], pitch=True)
        ptrs = [T.ptrs[0], None if null else T.ptrs[1] + shift][:n]
        st = [T.strides[0], T.strides[1]][:n]
        if len(extent) != 3:                                            # (one rank per call: both rows in the other rank, into the second view)
            ext, st, org, ptrs = [extent, extent], [st[1], st[1]], [origin, origin], [T.ptrs[1], T.ptrs[1]]
        else:
            org = [good[0], origin][:n]
        rc, decoded = sqy.decode_batch_window_device(src.data_ptr(), [offs[0], offs[blob]][:n], [lens[0], lens[blob]][:n], org, ptrs, ext, st, np.uint16)
        assert rc == 1 and decoded == [0] * n, (origin, extent)
        _same(T.read(), T.host)
    for k in range(3):                                                  # origin + extent one voxel beyond the shape, each dimension in turn
        o, e = [1, 1, 1], [2, 4, 6]
        e[k] += 1
        refused(tuple(o), tuple(e))
        o, e = [0, 0, 0], list(shape)
        o[k] = 1
        refused(tuple(o), tuple(e))
    refused((0, -1, 0), (1, 1, 1))                                      # a negative origin
    refused((0, 0, 0), (3, 0, 7))                                       # an extent of 0
    refused((0, 0), (5, 7))                                             # a rank other than the header's
    refused((0,), (7,))
    refused(good[0], good[1], blob=2)                                   # a blob of the other voxel type
    refused(good[0], good[1], shift=1)                                  # a destination off the voxel grid
    refused(good[0], good[1], null=True)                                # NULL inside d_dsts
    refused(good[0], good[1], n=0)                                      # nblobs = 0


def test_a_damaged_blob(sqy, oracle):
    """a damaged blob between two good ones: the code SQY_Decode gives it, both good windows in place, nothing written outside the views"""
    shape, origin, extent = (12, 64, 64), (3, 5, 7), (6, 50, 40)
    for pipeline, fused in (("bitswap1->lz4", 1), ("lz4", 1), ("bitswap1->lz4", 0)):
        blob, full = _blob(sqy, oracle, pipeline, shape, np.uint16)
        off = sqy.header_size(blob)
        body, size = None, 0
        while off < len(blob):                                          # the first compressed frame: its block becomes bytes the decoder refuses
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
        sqy.set_option("batch_window_fused", fused)
        try:
            T = Targets(np.uint16, [extent] * 3, shift=2, pitch=True)
            rc, decoded, got = _decode_windows(sqy, src, offs, lens, [origin] * 3, T)
        finally:
            sqy.set_option("batch_window_fused", 1)
        assert rc == rc_alone and decoded == [int(np.prod(extent)) * 2] * 3, (pipeline, fused)
        want, mask = T.expect([_cut(full, origin, extent)] * 3, skip=(1,))
        _same(got, want, mask)


def test_callers_stream_and_two_host_threads(sqy, oracle):
    import torch
    sets = []
    for t, pipeline in enumerate(("bitswap1->lz4", "lz4")):
        sets.append(_batch_of(sqy, oracle, pipeline) + (torch.cuda.Stream(device=_dev()),))
    # the call on a caller's stream
    src, offs, lens, origins, extents, tiles, s = sets[0]
    T = Targets(np.uint16, extents, shift=2, pitch=True)
    rc, _, got = _decode_windows(sqy, src, offs, lens, origins, T, stream=s.cuda_stream)
    assert rc == 0
    _same(got, T.expect(tiles)[0])
    torch.cuda.synchronize()
    ok = [False, False]

    def one(t):
        src, offs, lens, origins, extents, tiles, s = sets[t]
        good = True
        for r in range(3):
            T = Targets(np.uint16, extents, shift=2 * (r & 1), pitch=True, salt=r)
            rc, decoded = sqy.decode_batch_window_device(src.data_ptr(), offs, lens, origins, T.ptrs, T.extents, T.strides, np.uint16, stream=s.cuda_stream)
            s.synchronize()
            good = good and rc == 0 and np.array_equal(T.buf.cpu().numpy(), T.expect(tiles)[0])
        ok[t] = good
    th = [threading.Thread(target=one, args=(t,)) for t in range(2)]
    for x in th:
        x.start()
    for x in th:
        x.join()
    assert all(ok)
