"""SQYAMD_Compare_BatchWindow_*: a box of every blob compared with a view of the box's shape, nothing written.  Every row of statistics
must be what the CPU computes with integers from SQY_Decode's volume of the blob (test_gpu_batch_window._blob's `full`) and the voxels
the test put into the view -- the code under test is never the source of an expectation.  All views of a call lie in one buffer of
position-dependent pattern bytes (test_gpu_batch_window.Targets): a reader that strays into the gaps between rows and frames, around
the views, or into the blob's voxels just outside the window counts them; and the whole view buffer and the blob buffer must be byte
for byte what they were after every call.  The fused paths (the comparing transposer, the compare in the LZ4 output) and layer one
("batch_compare_fused" = 0) must give the same statistics, and each shows its launches in the profile."""
import threading

import numpy as np
import pytest

from batch_window_cases import BOX_CASES, pitched
from sqeazy_amd import synth
from test_gpu_batch_window import CASES, SERIAL_SHAPE, SHAPES, Targets, _batch_of, _blob, _cut, _dev, _pack, _windows
from test_gpu_encode_batch import _profile

pytestmark = pytest.mark.gpu

ONES = 2 ** 64 - 1


def _stats(a, b):
    """the eight fields for decoded voxels a against view voxels b, as Python integers (int64 holds 2^18 x 65535^2 exactly)"""
    a64, b64 = np.asarray(a).astype(np.int64).reshape(-1), np.asarray(b).astype(np.int64).reshape(-1)
    d = np.abs(a64 - b64)
    return [int(a64.size), int(np.count_nonzero(d)), int(d.sum()), int((d * d).sum()), int(d.max()), int(b64.sum()), int(b64.min()), int(b64.max())]


class Views:
    """Targets whose views can be filled again and again: the image of the buffer with views[i] in view i, the gaps as they were"""

    def __init__(self, dtype, extents, shift=0, pitch=False, salt=0):
        self.T = Targets(dtype, extents, shift=shift, pitch=pitch, salt=salt)
        self.idx = [self.T.bytes_of(i).reshape(-1) for i in range(len(extents))]
        self.image = None

    def fill(self, views):
        import torch
        image = self.T.host.copy()
        for i, v in enumerate(views):
            image[self.idx[i]] = np.ascontiguousarray(v).view(np.uint8).reshape(-1)
        self.T.buf.copy_(torch.from_numpy(image))
        self.image = image

    def unchanged(self):
        return np.array_equal(self.T.read(), self.image)


def _compare(sqy, src, offs, lens, origins, V, stream=None):
    T = V.T
    rc, stats = sqy.compare_batch_window_device(src.data_ptr(), offs, lens, origins, T.ptrs, T.extents, T.strides, T.dtype, stream=stream)
    assert stats.dtype == np.uint64 and stats.shape == (len(offs), 8)
    return rc, [[int(x) for x in row] for row in stats]


def _blob_index(shape, origin, extent):
    """the index in the BLOB's dense order of every voxel of the window, in the window's shape"""
    (bZ, bY, bX), (oz, oy, ox), (Z, Y, X) = shape, origin, extent
    z, y, x = np.ogrid[oz:oz + Z, oy:oy + Y, ox:ox + X]
    return (z * bY + y) * bX + x


def _variants(shapes_windows, tiles, dtype):
    """[(name, views, expected rows)]: (a) the decoded window itself; (b) one planted difference at a time -- the window's first voxel, its
    last one, a voxel of the blob's tail, voxels whose index in the blob's dense order is 0, 127 and 128 mod 128 (the last: the first
    voxel of a later run of 128) -- each with a delta of its own; (c) every voxel different"""
    item = np.dtype(dtype).itemsize
    top = np.iinfo(dtype).max
    out = [("same", tiles, [_stats(t, t) for t in tiles])]
    kinds = (("first", 1), ("last", 2), ("tail", 3), ("run+0", 5), ("run+127", 7), ("run+128", 11))
    for kind, delta in kinds:
        views, hit = [], 0
        for (shape, origin, extent), t in zip(shapes_windows, tiles):
            bi = _blob_index(shape, origin, extent).reshape(-1)
            n = int(np.prod(shape))
            L = n // (8 * item) * (8 * item)
            at = {"first": [0], "last": [bi.size - 1], "tail": np.flatnonzero(bi >= L)[:1], "run+0": np.flatnonzero(bi % 128 == 0)[:1],
                  "run+127": np.flatnonzero(bi % 128 == 127)[:1], "run+128": np.flatnonzero((bi % 128 == 0) & (bi >= 128))[-1:]}[kind]
            v = t.copy()
            for k in at:
                flat = v.reshape(-1)
                flat[k] = (int(flat[k]) + delta) & top
                hit += 1
            views.append(v)
        if kind == "tail" and hit == 0:                                  # (a call of blobs without a tail: the serial layout's shape)
            continue
        assert hit >= 1, kind
        want = [_stats(t, v) for t, v in zip(tiles, views)]
        assert all(w[1] <= 1 for w in want) and sum(w[1] for w in want) == hit
        out.append((kind, views, want))
    views = [t ^ np.dtype(dtype).type(top) for t in tiles]
    want = [_stats(t, v) for t, v in zip(tiles, views)]
    assert all(w[1] == w[0] for w in want)
    out.append(("all", views, want))
    return out


@pytest.mark.parametrize("pipeline, dtype, nthreads", CASES, ids=["%s-%s%s" % (p, np.dtype(d).name, "-serial" if t else "") for p, d, t in CASES])
def test_statistics(sqy, oracle, options, pipeline, dtype, nthreads):
    """every window of every blob shape in one call (a blob is named once per window), the views' bases on and one voxel behind the 16-byte
    grid, dense and pitched, fused and through layer one; view contents (a), (b), (c) of _variants"""
    item = np.dtype(dtype).itemsize
    shapes = (SERIAL_SHAPE,) if nthreads else SHAPES
    made = [(s, _blob(sqy, oracle, pipeline, s, dtype, nthreads)) for s in shapes]
    made = [(s, b) for s, b in made if b is not None]                   # (diff3x3x1 and frame_shuffle refuse some geometries at encode)
    assert len(made) >= (1 if nthreads else 3), [s for s, _ in made]
    src, boffs, blens = _pack([b[0] for _, b in made], gaps=[3 + 2 * k for k in range(len(made))])
    src_host = src.cpu().numpy()
    offs, lens, origins, extents, tiles, sw = [], [], [], [], [], []
    for k, (s, (_, full)) in enumerate(made):
        for o, e in _windows(s, item):
            offs.append(boffs[k]); lens.append(blens[k]); origins.append(o); extents.append(e)
            tiles.append(np.ascontiguousarray(_cut(full, o, e)))
            sw.append((s, o, e))
    variants = _variants(sw, tiles, dtype)
    assert len(variants) == (7 if nthreads else 8), [v[0] for v in variants]
    for fused in (1, 0):
        options("batch_compare_fused", fused)
        for shift in (0, item):
            for pitch in (False, True):
                V = Views(dtype, extents, shift=shift, pitch=pitch, salt=7 * shift + pitch)
                for name, views, want in variants:
                    V.fill(views)
                    rc, got = _compare(sqy, src, offs, lens, origins, V)
                    assert rc == 0, (fused, shift, pitch, name)
                    bad = [(i, sw[i], g, w) for i, (g, w) in enumerate(zip(got, want)) if g != w]
                    assert not bad, (fused, shift, pitch, name, len(bad), bad[:3])
                    assert V.unchanged(), (fused, shift, pitch, name)
                assert np.array_equal(src.cpu().numpy(), src_host), (fused, shift, pitch)


@pytest.mark.parametrize("pipeline", ["bitswap1->lz4", "lz4"])
def test_64_bits_where_they_are_needed(sqy, options, pipeline):
    """zeros against 65535 everywhere, 16 x 128 x 128: above 2^32 in a thread's 128 voxels, 2^18 x 65535^2 in the blob (a hair below 2^50),
    eight workgroups into one record"""
    import torch
    shape = (16, 128, 128)
    n = int(np.prod(shape))
    rc, blob = sqy.encode(pipeline, np.zeros(shape, np.uint16))
    assert rc == 0
    rc, full = sqy.decode(blob)
    assert rc == 0 and not full.any()
    src, offs, lens = _pack([blob])
    view = torch.full(shape, -1, dtype=torch.int16, device=_dev())      # (65535 as torch spells it)
    assert int(view.cpu().numpy().view(np.uint16).min()) == 65535
    want = [n, n, n * 65535, n * 65535 ** 2, 65535, n * 65535, 65535, 65535]
    assert 2 ** 49 < want[3] < 2 ** 50 and 128 * 65535 ** 2 > 2 ** 32
    for fused in (1, 0):
        options("batch_compare_fused", fused)
        rc, stats = sqy.compare_batch_window_device(src.data_ptr(), offs, lens, None, [view.data_ptr()], [shape], None, np.uint16)
        assert rc == 0 and [int(x) for x in stats[0]] == want, (fused, stats)
    torch.cuda.synchronize()
    assert int(view.cpu().numpy().view(np.uint16).min()) == 65535


def _views_of(tiles, extents, salt=0):
    """a filled Views of the tiles with one voxel changed in each (pitched, off the grid), and the expected rows"""
    views = []
    for k, t in enumerate(tiles):
        v = np.ascontiguousarray(t).copy()
        v.reshape(-1)[(7 * k + 3) % v.size] ^= 0x55
        views.append(v)
    V = Views(np.uint16, extents, shift=2, pitch=True, salt=salt)
    V.fill(views)
    return V, [_stats(t, v) for t, v in zip(tiles, views)]


def test_launches(sqy, oracle, options):
    def run(pipeline):
        src, offs, lens, origins, extents, tiles = _batch_of(sqy, oracle, pipeline)      # (the blobs are made outside the profile)
        V, want = _views_of(tiles, extents)
        ((rc, got), p) = _profile(sqy, lambda: _compare(sqy, src, offs, lens, origins, V))
        assert rc == 0 and got == want and V.unchanged(), (pipeline, got, want)
        return p, len(extents)
    p, _ = run("bitswap1->lz4")
    assert p["batch_bitswap1_decode_window_compare"][1] == 1 and p["batch_lz4_decode"][1] == 1, p
    assert not any(k in p for k in ("batch_window_compare", "batch_bitswap1_decode_window", "batch_window_copy", "batch_unpack")), p
    p, _ = run("lz4")
    assert p["batch_compare_window"][1] == 1 and not any(k in p for k in ("batch_window_compare", "batch_copy_window", "batch_window_copy", "batch_unpack")), p
    p, _ = run("quantiser->bitswap1->lz4")
    assert p["batch_quantiser_decode"][1] == 1 and p["batch_window_compare"][1] == 1 and "batch_window_copy" not in p, p
    options("batch_compare_fused", 0)
    for pipeline in ("bitswap1->lz4", "lz4"):
        p, _ = run(pipeline)
        assert p["batch_window_compare"][1] == 1 and "batch_bitswap1_decode_window_compare" not in p and "batch_compare_window" not in p, p
    options("batch_compare_fused", 1)
    options("decode_batch_group_bytes", 1)                              # every blob a group of its own: one fused launch per blob
    for pipeline, name in (("bitswap1->lz4", "batch_bitswap1_decode_window_compare"), ("lz4", "batch_compare_window")):
        p, n = run(pipeline)
        assert p[name][1] == n and p["batch_lz4_decode"][1] == n, p


def test_overlapping_and_shared_views(sqy, oracle):
    """one blob named three times with different windows; one view shared by two blobs (and a second window read through a view that lies
    inside the first one's buffer): every row is right"""
    import torch
    shape = (7, 33, 31)
    blob_a, full_a = _blob(sqy, oracle, "bitswap1->lz4", shape, np.uint16)
    blob_b, full_b = _blob(sqy, oracle, "lz4", shape, np.uint16)
    src, boffs, blens = _pack([blob_a, blob_b])
    buf = synth.stack((5, 31, 29), np.uint16, seed=955)                 # the shared voxels: a dense view of (5, 31, 29)
    d_buf = torch.from_numpy(buf.copy()).to(_dev())
    p0 = d_buf.data_ptr()
    whole, st = (5, 31, 29), (31 * 29, 29, 1)
    # (blob, origin, extent, view's first voxel in buf): three windows of blob a -- the first and the third read the SAME view, the second a
    # box inside it --, then blob b against the same view again
    calls = [(0, (1, 1, 1), whole, (0, 0, 0)), (0, (0, 2, 2), (2, 3, 4), (1, 1, 1)), (0, (2, 2, 2), whole, (0, 0, 0)), (1, (1, 1, 1), whole, (0, 0, 0))]
    offs = [boffs[b] for b, _, _, _ in calls]
    lens = [blens[b] for b, _, _, _ in calls]
    ptrs = [p0 + 2 * sum(a * s for a, s in zip(at, st)) for _, _, _, at in calls]
    rc, stats = sqy.compare_batch_window_device(src.data_ptr(), offs, lens, [o for _, o, _, _ in calls], ptrs, [e for _, _, e, _ in calls], [st] * len(calls), np.uint16)
    assert rc == 0
    for row, (b, o, e, at) in zip(stats, calls):
        assert [int(x) for x in row] == _stats(_cut((full_a, full_b)[b], o, e), _cut(buf, at, e)), (b, o, e)
    torch.cuda.synchronize()
    assert np.array_equal(d_buf.cpu().numpy(), buf)


def test_a_damaged_blob(sqy, oracle, options):
    """a damaged blob between two good ones: the code SQY_Decode gives it, its row all ones, both good rows right, the views unchanged"""
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
        src_host = src.cpu().numpy()
        tile = _cut(full, origin, extent)
        V, want = _views_of([tile] * 3, [extent] * 3, salt=fused)
        options("batch_compare_fused", fused)
        rc, got = _compare(sqy, src, offs, lens, [origin] * 3, V)
        assert rc == rc_alone, (pipeline, fused)
        assert got[1] == [ONES] * 8 and got[0] == want[0] and got[2] == want[2], (pipeline, fused, got)
        assert V.unchanged() and np.array_equal(src.cpu().numpy(), src_host)


@pytest.mark.parametrize("pitch", [False, True], ids=["dense", "pitched"])
def test_a_tiled_store(sqy, pitch):
    """verify after write, find the changed tiles, verify after an update: the boxes of BOX_CASES of a parent stored as tiles, compared
    with the parent's own voxels (the box buffer is the parent, or a pitched copy of the box)"""
    import torch
    (shape, tile), boxes = next((k, v) for k, v in BOX_CASES.items() if k[0] == (9, 40, 72))
    parent = synth.stack(shape, np.uint16, seed=960)
    d_parent = torch.from_numpy(parent.copy()).to(_dev())
    ptrs, shapes, strides = sqy.tile_views(d_parent.data_ptr(), shape, tile, 2)
    slot = sqy.max_compressed_length("bitswap1->lz4", tile, np.uint16) + 13
    store = torch.zeros(slot * len(ptrs), dtype=torch.uint8, device=_dev())
    rc, offs, lens = sqy.encode_batch_strided_device("bitswap1->lz4", ptrs, shapes, strides, np.uint16, store.data_ptr(), slot)
    assert rc == 0 and len(offs) == 27
    # the voxels that will change: corners and faces of tiles, inside and outside the boxes
    changed = [(0, 0, 0), (3, 15, 31), (4, 16, 32), (4, 15, 32), (3, 16, 33), (8, 39, 71), (5, 20, 40), (7, 31, 63), (0, 0, 71), (8, 0, 0), (2, 2, 2), (4, 17, 33)]
    newer = parent.copy()
    for k, c in enumerate(changed):
        newer[c] ^= 1 + k
    grid = [(shape[k] + tile[k] - 1) // tile[k] for k in range(3)]
    for origin, extent in boxes:
        st = pitched(extent) if pitch else tuple(int(s) // 2 for s in parent.strides)

        def box_buffer(vol):
            """(device tensor kept alive, pointer of the box's first voxel): the box of vol inside vol itself, or in a pitched buffer"""
            if not pitch:
                d = torch.from_numpy(vol.copy()).to(_dev())
                return d, d.data_ptr() + 2 * sum(o * s for o, s in zip(origin, st))
            host = np.full((extent[0] - 1) * st[0] + (extent[1] - 1) * st[1] + extent[2], 0xABCD, np.uint16)
            z, y, x = np.ogrid[0:extent[0], 0:extent[1], 0:extent[2]]
            host[z * st[0] + y * st[1] + x] = _cut(vol, origin, extent)
            d = torch.from_numpy(host).to(_dev())
            return d, d.data_ptr()
        keep, p0 = box_buffer(parent)
        idx, origins, vptrs, vshapes, vstrides = sqy.box_windows(shape, tile, origin, extent, p0, st, 2)
        pick = lambda table: [table[i] for i in idx]
        rc, stats = sqy.compare_batch_window_device(store.data_ptr(), pick(offs), pick(lens), origins, vptrs, vshapes, vstrides, np.uint16)
        assert rc == 0 and [int(r[1]) for r in stats] == [0] * len(idx)                       # the store holds what the parent holds
        assert sum(int(r[0]) for r in stats) == int(np.prod(extent)) and [int(r[0]) for r in stats] == [int(np.prod(s)) for s in vshapes]
        # the newer frame: which tiles under the box differ, and by how many voxels
        keep2, p1 = box_buffer(newer)
        idx, origins, vptrs, vshapes, vstrides = sqy.box_windows(shape, tile, origin, extent, p1, st, 2)
        rc, stats = sqy.compare_batch_window_device(store.data_ptr(), pick(offs), pick(lens), origins, vptrs, vshapes, vstrides, np.uint16)
        want = [0] * len(idx)
        for c in changed:
            if all(o <= a < o + e for a, o, e in zip(c, origin, extent)):
                t = 0
                for k in range(3):
                    t = t * grid[k] + c[k] // tile[k]
                want[idx.index(t)] += 1
        assert rc == 0 and [int(r[1]) for r in stats] == want, (origin, extent)
        # the box written: the NEW blobs hold the newer frame's box
        fresh = torch.zeros(slot * len(idx), dtype=torch.uint8, device=_dev())
        rc, noffs, nlens = sqy.update_batch_window_device("bitswap1->lz4", store.data_ptr(), pick(offs), pick(lens), origins, vptrs, vshapes, vstrides, np.uint16,
                                                          fresh.data_ptr(), slot)
        assert rc == 0
        rc, stats = sqy.compare_batch_window_device(fresh.data_ptr(), noffs, nlens, origins, vptrs, vshapes, vstrides, np.uint16)
        assert rc == 0 and [int(r[1]) for r in stats] == [0] * len(idx), (origin, extent)
        del keep, keep2


def test_origins_null_and_lower_ranks(sqy):
    """NULL origins: every window at its blob's first voxel; blobs of ranks 1 and 2"""
    for shape, origin, extent in (((5, 7), (1, 2), (3, 4)), ((37,), (16,), (20,)), ((5, 7), None, (2, 6))):
        vol = synth.stack((1, 1, int(np.prod(shape))), np.uint16, seed=730).reshape(shape)
        rc, blob = sqy.encode("bitswap1->lz4", vol)
        assert rc == 0
        src, offs, lens = _pack([blob, blob])
        tile = _cut(vol, origin or (0,) * len(shape), extent)
        for pitch in (False, True):
            other = np.ascontiguousarray(tile).copy()
            other.reshape(-1)[-1] ^= 0x101
            V = Views(np.uint16, [extent, extent], shift=2, pitch=pitch)
            V.fill([tile, other])
            rc, got = _compare(sqy, src, offs, lens, None if origin is None else [origin, origin], V)
            assert rc == 0 and got == [_stats(tile, tile), _stats(tile, other)] and V.unchanged(), (shape, pitch, got)


def test_callers_stream_and_two_host_threads(sqy, oracle):
    import torch
    sets = []
    for t, pipeline in enumerate(("bitswap1->lz4", "lz4")):
        src, offs, lens, origins, extents, tiles = _batch_of(sqy, oracle, pipeline)
        V, want = _views_of(tiles, extents, salt=t)
        sets.append((src, offs, lens, origins, V, want, torch.cuda.Stream(device=_dev())))
    torch.cuda.synchronize()
    # the call on a caller's stream
    src, offs, lens, origins, V, want, s = sets[0]
    rc, got = _compare(sqy, src, offs, lens, origins, V, stream=s.cuda_stream)
    assert rc == 0 and got == want and V.unchanged()
    ok = [False, False]

    def one(t):
        src, offs, lens, origins, V, want, s = sets[t]
        good = True
        for r in range(3):
            rc, got = _compare(sqy, src, offs, lens, origins, V, stream=s.cuda_stream)
            good = good and rc == 0 and got == want
        ok[t] = good
    th = [threading.Thread(target=one, args=(t,)) for t in range(2)]
    for x in th:
        x.start()
    for x in th:
        x.join()
    assert all(ok) and all(S[4].unchanged() for S in sets)


def test_compare_metrics(sqy, oracle):
    """the reference's help-text definitions in float64, from rows of the statistics test's kind against numpy on the two arrays: each
    metric is at most four correctly rounded double operations on exact integers, 1e-12 is thousands of ulps"""
    for dtype, shape in ((np.uint16, (7, 33, 31)), (np.uint8, (3, 5, 7))):
        blob, full = _blob(sqy, oracle, "bitswap1->lz4", shape, dtype)
        src, offs, lens = _pack([blob] * 3)
        const = np.full(shape, 9, dtype)
        views = [full ^ np.dtype(dtype).type(3), full.copy(), const]
        V = Views(dtype, [shape] * 3, shift=0, pitch=True)
        V.fill(views)
        rc, stats = sqy.compare_batch_window_device(src.data_ptr(), offs, lens, None, V.T.ptrs, V.T.extents, V.T.strides, dtype)
        assert rc == 0
        for row, b in zip(stats, views):
            a64, b64 = full.astype(np.float64).reshape(-1), b.astype(np.float64).reshape(-1)
            with np.errstate(divide="ignore", invalid="ignore"):
                mse = np.sum((a64 - b64) ** 2) / np.float64(a64.size)
                rms = np.sqrt(mse)
                want = dict(mse=mse, rms=rms, nrmse=rms / (b64.max() - b64.min()), mnmse=rms / (np.sum(b64) / np.float64(b64.size)), l1norm=np.sum(np.abs(a64 - b64)),
                            l2norm=np.sum((a64 - b64) ** 2), psnr=np.float64(20) * np.log10(np.float64(np.iinfo(dtype).max)) - np.float64(10) * np.log10(mse),
                            drange=b64.max() - b64.min())
            got = sqy.compare_metrics(row, dtype)
            assert sorted(got) == sorted(want)
            for k, w in want.items():
                if np.isfinite(w):
                    assert abs(got[k] - w) <= 1e-12 * abs(w), (k, got[k], w)
                else:
                    assert (np.isnan(w) and np.isnan(got[k])) or got[k] == w, (k, got[k], w)
        equal, constant = sqy.compare_metrics(stats[1], dtype), sqy.compare_metrics(stats[2], dtype)
        assert equal["mse"] == 0 and equal["psnr"] == np.inf and equal["nrmse"] == 0 and equal["l1norm"] == 0
        assert constant["drange"] == 0 and constant["nrmse"] == np.inf and np.isfinite(constant["mnmse"])
