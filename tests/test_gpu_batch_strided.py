"""SQYAMD_PipelineEncode_BatchStrided_* and SQYAMD_Decode_BatchStrided_*: tiles cut in place.  Views of larger resident parents -- tiles
at odd offsets, rows shorter than a 16-byte word, a padded pitch -- are encoded without a dense copy of the caller's and decoded back into
their parents.  Every blob must be byte for byte the oracle's and SQYAMD_PipelineEncode_*_Device's for np.ascontiguousarray(view); a decode
must write the view's voxels and nothing else: the whole parent is compared with an image built on the CPU, the gaps between the rows
and frames of a view included.  The fused path (the transposers gather from and scatter into the views) and the packed path
("batch_strided_fused" = 0) must give the same bytes, and each shows its launches in the profile."""
import threading

import numpy as np
import pytest

from sqeazy_amd import synth
from test_gpu_encode_batch import SINGLE_KERNELS, _profile, _want

pytestmark = pytest.mark.gpu

CANARY = 0xA5
GAP = 64                      # canary bytes around every parent and around the slots

# parents: A and B dense stacks; C a pitched volume that is cut from no dense parent (rows 27, frames 10 * 27 + 5 voxels apart), its last
# voxel the allocation's last
PARENT_SHAPES = {"A": (9, 40, 72), "B": (20, 64, 96)}
C_SHAPE, C_STRIDES = (6, 10, 24), (10 * 27 + 5, 27, 1)
C_VOXELS = 5 * C_STRIDES[0] + 9 * C_STRIDES[1] + 24
# name, parent, shape, origin
VIEWS = (("A_whole", "A", (9, 40, 72), (0, 0, 0)),          # dense: the Batch call's kernels
         ("A_wide", "A", (4, 16, 32), (0, 0, 0)),           # every row on the 16-byte grid
         ("A_short", "A", (3, 5, 7), (5, 3, 5)),            # rows shorter than a 16-voxel word; the 9-voxel tail spans rows
         ("A_last", "A", (1, 1, 5), (8, 39, 67)),           # no planes at all; the parent's last voxels
         ("A_odd", "A", (5, 33, 33), (0, 1, 35)),           # odd X, odd offset: the 16-byte phase changes every row; tail 5
         ("B_big", "B", (18, 60, 67), (1, 2, 3)),           # 72360 voxels: three transposer tiles, boundaries inside rows
         ("C", "C", C_SHAPE, (0, 0, 0)))                    # padded pitch
NON_DENSE = tuple(v[0] for v in VIEWS if v[0] != "A_whole")
LZ4_BATCH = ("batch_lz4_chunks", "batch_lz4_frame_scan", "batch_lz4_frame_gather")


def _dev():
    import torch
    return torch.device("cuda", 0)


def _strides_of(parent):
    if parent == "C":
        return C_STRIDES
    _, Y, X = PARENT_SHAPES[parent]
    return (Y * X, X, 1)


class View:
    def __init__(self, name, parent, shape, origin):
        self.name, self.parent, self.shape, self.strides = name, parent, tuple(shape), _strides_of(parent)
        self.offset = sum(o * s for o, s in zip(origin, self.strides))          # voxels

    def index(self):
        """the flat parent indices of the view's voxels, in the view's shape"""
        z, y, x = np.ix_(*[np.arange(n) for n in self.shape])
        return self.offset + z * self.strides[0] + y * self.strides[1] + x

    def cut(self, flat):
        return np.ascontiguousarray(flat[self.index()])


def _views(names):
    by_name = {v[0]: View(*v) for v in VIEWS}
    return [by_name[n] for n in names]


_parents = {}


def _parent_data(dtype):
    """the parents' voxels as flat arrays, made once per voxel type and never changed"""
    key = np.dtype(dtype).name
    if key not in _parents:
        p = {k: synth.stack(s, dtype, seed=500 + i).reshape(-1) for i, (k, s) in enumerate(sorted(PARENT_SHAPES.items()))}
        p["C"] = synth.stack((1, 1, C_VOXELS), dtype, seed=509).reshape(-1)
        for a in p.values():
            a.setflags(write=False)
        _parents[key] = p
    return _parents[key]


def _pattern(nbytes, salt):
    """canary bytes that depend on their position"""
    i = np.arange(nbytes, dtype=np.uint64)
    return ((i * 31 + i // 251 + salt) & 0xff).astype(np.uint8)


class Parents:
    """the parents on the device, GAP guard bytes around each: filled with their data (encode) or with a position-dependent pattern (decode)"""

    def __init__(self, dtype, data=True, keys=("A", "B", "C")):
        import torch
        self.dtype = np.dtype(dtype)
        src = _parent_data(dtype)
        self.host = {}
        for i, k in enumerate(keys):
            body = np.frombuffer(src[k].tobytes(), dtype=np.uint8) if data else _pattern(src[k].nbytes, 17 * i)
            self.host[k] = np.concatenate([_pattern(GAP, 101 + i), body, _pattern(GAP, 202 + i)])
        self.bufs = {k: torch.from_numpy(h.copy()).to(_dev()) for k, h in self.host.items()}
        assert all(b.data_ptr() % 16 == 0 for b in self.bufs.values())

    def ptr(self, view):
        return self.bufs[view.parent].data_ptr() + GAP + view.offset * self.dtype.itemsize

    def read(self):
        import torch
        torch.cuda.synchronize()
        return {k: b.cpu().numpy() for k, b in self.bufs.items()}

    def expect(self, views, tiles):
        """the image a decode of tiles[i] into views[i] must leave: everything else as it was"""
        want = {k: h.copy() for k, h in self.host.items()}
        for v, t in zip(views, tiles):
            body = want[v.parent][GAP:len(want[v.parent]) - GAP].view(self.dtype)
            body[v.index()] = t
        return want


def _disjoint(views):
    """on the CPU: the views of one decode call are pairwise disjoint"""
    seen = {}
    for v in views:
        idx = v.index().reshape(-1)
        s = seen.setdefault(v.parent, set())
        assert s.isdisjoint(idx.tolist()), "view %s overlaps another view of the call" % v.name
        s.update(idx.tolist())


def _admitted(sqy, pipeline, views, dtype):
    """the views whose dense copy SQYAMD_PipelineEncode_*_Device takes with this pipeline (diff3x3x1 refuses some geometries)"""
    import torch
    out = []
    for v in views:
        vol = v.cut(_parent_data(dtype)[v.parent])
        d_vol = torch.from_numpy(vol.copy()).to(_dev())
        cap = sqy.max_compressed_length(pipeline, vol.shape, vol.dtype) + 64
        dst = torch.empty(cap, dtype=torch.uint8, device=_dev())
        rc, _ = sqy.encode_device(pipeline, d_vol.data_ptr(), vol.shape, vol.dtype, dst.data_ptr(), cap)
        if rc == 0:
            out.append(v)
    return out


def _settle():
    """what torch queued on its own stream for the buffers of a call -- the parents' copies, the canary fill -- is complete before the call
    is made: the library orders a call behind hip_stream only, "work on OTHER streams that touches d_src or d_dst is the caller's to
    synchronise" (include/sqeazy_amd.h).  Without this a fill that waits in a hardware queue behind another thread's kernels can land on
    top of the blobs a call on a stream of its own has just written"""
    import torch
    torch.cuda.current_stream(_dev()).synchronize()


def _encode(sqy, pipeline, views, dtype, strided=True, joint=True, stream=None, keep=False):
    """the strided call on the views of fresh device parents, slots of canaries: (rc, blobs) -- or, keep = True, (rc, (buffer, offsets,
    lengths)) to pass straight through.  The canaries around the slots hold, the parents are unchanged; on the joint path a slot holds its
    blob at its start and nothing else"""
    import torch
    P = Parents(dtype)
    n = len(views)
    slot = max(sqy.max_compressed_length(pipeline, v.shape, dtype) for v in views) + 13          # (no multiple of 16)
    buf = torch.full((2 * GAP + slot * n,), CANARY, dtype=torch.uint8, device=_dev())
    _settle()
    rc, offs, lens = sqy.encode_batch_strided_device(pipeline, [P.ptr(v) for v in views], [v.shape for v in views],
                                                     [v.strides for v in views] if strided else None, dtype, buf.data_ptr() + GAP, slot, stream=stream)
    got = P.read()
    for k, h in got.items():
        assert np.array_equal(h, P.host[k]), "parent %s changed by an encode" % k
    h = buf.cpu().numpy()
    assert (h[:GAP] == CANARY).all() and (h[GAP + slot * n:] == CANARY).all(), "written outside the slots"
    if rc:
        assert offs == [0] * n and lens == [0] * n
        assert (h == CANARY).all(), "a refused call wrote"
        return rc, None
    blobs = []
    for i in range(n):
        assert i * slot <= offs[i] and lens[i] > 0 and offs[i] + lens[i] <= (i + 1) * slot, (i, offs[i], lens[i])
        lo, hi = GAP + offs[i], GAP + offs[i] + lens[i]
        if joint:
            assert offs[i] == i * slot and (h[hi:GAP + (i + 1) * slot] == CANARY).all(), "slot %d: written outside the blob" % i
        blobs.append(h[lo:hi].tobytes())
    if keep:
        return rc, (buf, [GAP + o for o in offs], lens, blobs)
    return rc, blobs


def _references(sqy, oracle, pipeline, views, dtype):
    """what both references give for a dense copy of every view (made once per pipeline, view and voxel type; the single call runs here,
    so a test that reads the profile of the strided call asks for them first)"""
    data = _parent_data(dtype)
    return [_want(sqy, oracle, pipeline, v.cut(data[v.parent]), 0, _dev(), ("strided", v.name, np.dtype(dtype).name)) for v in views]


def _check_encode(sqy, oracle, pipeline, views, dtype, **kw):
    want = _references(sqy, oracle, pipeline, views, dtype)
    rc, blobs = _encode(sqy, pipeline, views, dtype, **kw)
    assert rc == 0
    for v, b, w in zip(views, blobs, want):
        assert b == w, (pipeline, v.name)
    return blobs


PIPELINES = ("bitswap1->lz4", "bitswap1->lz4(blocksize_kb=4,framestep_kb=4)", "lz4", "quantiser->bitswap1->lz4", "diff3x3x1->bitswap1->lz4")
JOINT = PIPELINES[:4]


def _cases():
    for p in PIPELINES:
        for dt in (np.uint16, np.uint8):
            if p.startswith("quantiser") and dt == np.uint8:
                continue
            yield pytest.param(p, dt, id="%s-%s" % (p, np.dtype(dt).name))


@pytest.mark.parametrize("pipeline, dtype", list(_cases()))
def test_encode(sqy, oracle, pipeline, dtype):
    assert sqy.pipeline_possible(pipeline, dtype)
    views = _views([v[0] for v in VIEWS])
    if pipeline.startswith("diff3x3x1"):
        views = _admitted(sqy, pipeline, views, dtype)
        assert len(views) >= 3
    _check_encode(sqy, oracle, pipeline, views, dtype, joint=pipeline in JOINT)


def test_encode_launch_counts(sqy, oracle, options):
    views = _views(NON_DENSE)
    for pipeline, dt in (("bitswap1->lz4", np.uint16), ("lz4", np.uint16), ("lz4", np.uint8), ("bitswap1->lz4", np.uint8)):
        _references(sqy, oracle, pipeline, views, dt)                   # (the single call's kernels stay out of the profiles below)
    (blobs, p) = _profile(sqy, lambda: _check_encode(sqy, oracle, "bitswap1->lz4", views, np.uint16))
    assert p["batch_bitswap1_strided"][1] == 1 and all(p[k][1] == 1 for k in LZ4_BATCH), p
    assert "batch_pack" not in p and not any(k in p for k in SINGLE_KERNELS), p
    (_, p) = _profile(sqy, lambda: _check_encode(sqy, oracle, "lz4", views, np.uint16))
    assert p["batch_pack"][1] == 1 and all(p[k][1] == 1 for k in LZ4_BATCH) and not any(k in p for k in SINGLE_KERNELS), p
    options("batch_strided_fused", 0)
    (packed, p) = _profile(sqy, lambda: _check_encode(sqy, oracle, "bitswap1->lz4", views, np.uint16))
    assert p["batch_pack"][1] == 1 and p["batch_bitswap1"][1] == 1 and "batch_bitswap1_strided" not in p, p
    assert not any(k in p for k in SINGLE_KERNELS), p
    assert packed == blobs
    for pipeline, dt in (("lz4", np.uint16), ("lz4", np.uint8), ("bitswap1->lz4", np.uint8)):
        (_, p) = _profile(sqy, lambda: _check_encode(sqy, oracle, pipeline, views, dt))
        assert p["batch_pack"][1] == 1 and not any("strided" in k for k in p) and not any(k in p for k in SINGLE_KERNELS), p


def test_dense_views_are_the_batch_call(sqy, oracle):
    """a view with the dense strides, and strides = NULL: the Batch call's kernels -- no _strided, no batch_pack -- and its blobs"""
    import torch
    whole = _views(["A_whole", "A_last"])
    vols = [v.cut(_parent_data(np.uint16)[v.parent]) for v in whole]
    srcs = [torch.from_numpy(v.copy()).to(_dev()) for v in vols]
    slot = max(sqy.max_compressed_length("bitswap1->lz4", v.shape, np.uint16) for v in vols) + 13
    buf = torch.zeros(slot * len(vols), dtype=torch.uint8, device=_dev())

    def batch():
        rc, offs, lens = sqy.encode_batch_device("bitswap1->lz4", [s.data_ptr() for s in srcs], [v.shape for v in vols], np.uint16, buf.data_ptr(), slot)
        torch.cuda.synchronize()
        assert rc == 0
        h = buf.cpu().numpy()
        return [h[o:o + n].tobytes() for o, n in zip(offs, lens)]
    (want, p_batch) = _profile(sqy, batch)
    _references(sqy, oracle, "bitswap1->lz4", whole, np.uint16)
    for strided in (True, False):
        (blobs, p) = _profile(sqy, lambda: _check_encode(sqy, oracle, "bitswap1->lz4", whole, np.uint16, strided=strided))
        assert blobs == want
        assert sorted(p) == sorted(p_batch) and all(p[k][1] == n for k, (_, n) in p_batch.items()), (p, p_batch)


DECODE_CASES = [("bitswap1->lz4", np.uint16), ("bitswap1->lz4", np.uint8), ("bitswap1->lz4(blocksize_kb=4,framestep_kb=4)", np.uint16), ("lz4", np.uint16),
                ("lz4", np.uint8), ("quantiser->bitswap1->lz4", np.uint16), ("diff3x3x1->bitswap1->lz4", np.uint16)]


def _decode(sqy, buf, offs, lens, views, dtype, stream=None):
    """the strided decode into pattern-filled parents: (rc, decoded, the parents' bytes, the Parents)"""
    P = Parents(dtype, data=False)
    _settle()
    rc, decoded = sqy.decode_batch_strided_device(buf.data_ptr(), offs, lens, [P.ptr(v) for v in views], [v.shape for v in views], [v.strides for v in views],
                                                  dtype, stream=stream)
    return rc, decoded, P.read(), P


def _same(got, want):
    for k in want:
        bad = np.flatnonzero(got[k] != want[k])
        assert bad.size == 0, "parent %s: %d bytes differ, the first at %d (body from %d)" % (k, bad.size, bad[0], GAP)


@pytest.mark.parametrize("pipeline, dtype", DECODE_CASES, ids=["%s-%s" % (p, np.dtype(d).name) for p, d in DECODE_CASES])
def test_decode(sqy, oracle, options, pipeline, dtype):
    views = _views(NON_DENSE)
    if pipeline.startswith("diff3x3x1"):
        views = _admitted(sqy, pipeline, views, dtype)
        assert len(views) >= 3
    _disjoint(views)
    rc, (buf, offs, lens, blobs) = _encode(sqy, pipeline, views, dtype, joint=pipeline in JOINT, keep=True)
    assert rc == 0
    data = _parent_data(dtype)
    tiles = []
    for v, b in zip(views, blobs):
        rc, back = sqy.decode(b)
        assert rc == 0 and back.shape == v.shape
        if not pipeline.startswith("quantiser"):
            assert np.array_equal(back, v.cut(data[v.parent])), v.name
        tiles.append(back)
    ((rc, decoded, got, P), p) = _profile(sqy, lambda: _decode(sqy, buf, offs, lens, views, dtype))
    assert rc == 0 and decoded == [t.nbytes for t in tiles]
    _same(got, P.expect(views, tiles))
    if pipeline == "bitswap1->lz4":
        assert p["batch_bitswap1_decode_strided"][1] == 1 and "batch_unpack" not in p and p["batch_lz4_decode"][1] == 1, p
    elif pipeline == "lz4":
        assert p["batch_copy_strided"][1] == 1 and "batch_unpack" not in p, p
    elif pipeline.startswith("quantiser") or pipeline.startswith("diff3x3x1"):
        assert p["batch_unpack"][1] == 1 and not any("strided" in k for k in p), p
    options("batch_strided_fused", 0)
    ((rc, decoded, packed, P), p) = _profile(sqy, lambda: _decode(sqy, buf, offs, lens, views, dtype))
    assert rc == 0 and p["batch_unpack"][1] == 1 and not any("strided" in k for k in p), p
    _same(packed, got)


def test_decode_mixes_dense_and_strided(sqy):
    """a dense view (its own allocation) next to tiles of a parent: the dense launch and the strided one side by side"""
    import torch
    views = _views(["A_whole", "B_big", "C"])
    rc, (buf, offs, lens, blobs) = _encode(sqy, "bitswap1->lz4", views, np.uint16, keep=True)
    assert rc == 0
    data = _parent_data(np.uint16)
    P = Parents(np.uint16, data=False)
    ((rc, _), p) = _profile(sqy, lambda: sqy.decode_batch_strided_device(buf.data_ptr(), offs, lens, [P.ptr(v) for v in views], [v.shape for v in views],
                                                                        [v.strides for v in views], np.uint16))
    assert rc == 0 and p["batch_bitswap1_decode"][1] == 1 and p["batch_bitswap1_decode_strided"][1] == 1, p
    _same(P.read(), P.expect(views, [v.cut(data[v.parent]) for v in views]))


@pytest.mark.parametrize("pipeline, dtype", [("bitswap1->lz4", np.uint16), ("lz4", np.uint8), ("quantiser->bitswap1->lz4", np.uint16)])
def test_way_back_over_a_tile_grid(sqy, pipeline, dtype):
    """tile_views' grid of parent A, edge tiles included: the encode's offsets and lengths straight into the decode; the result is the parent"""
    import torch
    shape, tile = PARENT_SHAPES["A"], (4, 16, 32)
    src = Parents(dtype, keys=("A",))
    ptrs, shapes, strides = sqy.tile_views(src.bufs["A"].data_ptr() + GAP, shape, tile, np.dtype(dtype).itemsize)
    assert len(ptrs) == 27 and (1, 8, 8) in shapes
    slot = sqy.max_compressed_length(pipeline, tile, dtype) + 13
    buf = torch.zeros(slot * len(ptrs), dtype=torch.uint8, device=_dev())
    rc, offs, lens = sqy.encode_batch_strided_device(pipeline, ptrs, shapes, strides, dtype, buf.data_ptr(), slot)
    assert rc == 0
    dst = Parents(dtype, data=False, keys=("A",))
    back, _, _ = sqy.tile_views(dst.bufs["A"].data_ptr() + GAP, shape, tile, np.dtype(dtype).itemsize)
    rc, decoded = sqy.decode_batch_strided_device(buf.data_ptr(), offs, lens, back, shapes, strides, dtype)
    assert rc == 0 and decoded == [int(np.prod(s)) * np.dtype(dtype).itemsize for s in shapes]
    got = dst.read()["A"]
    if pipeline.startswith("quantiser"):
        # lossy: every tile is what the single decode gives for its blob
        h = buf.cpu().numpy()
        want = dst.host["A"].copy()
        body = want[GAP:len(want) - GAP].view(dtype).reshape(shape)
        at = [(z, y, x) for z in range(0, shape[0], tile[0]) for y in range(0, shape[1], tile[1]) for x in range(0, shape[2], tile[2])]
        for (z, y, x), s, o, n in zip(at, shapes, offs, lens):
            rc, t = sqy.decode(h[o:o + n].tobytes())
            assert rc == 0
            body[z:z + s[0], y:y + s[1], x:x + s[2]] = t
        assert np.array_equal(got, want)
    else:
        assert np.array_equal(got[GAP:len(got) - GAP], src.host["A"][GAP:len(got) - GAP])
        assert np.array_equal(got[:GAP], dst.host["A"][:GAP]) and np.array_equal(got[len(got) - GAP:], dst.host["A"][len(got) - GAP:])


BAD_STRIDES = [("innermost stride 2", (3, 5, 7), (2880, 72, 2)), ("a stride of 0", (3, 5, 7), (2880, 0, 1)),
               ("frames overlap", (3, 5, 7), (5 * 72 - 1, 72, 1)), ("rank 4", (1, 3, 5, 7), (8640, 2880, 72, 1))]


@pytest.mark.parametrize("why, shape, strides", BAD_STRIDES, ids=[b[0] for b in BAD_STRIDES])
def test_refused_views(sqy, why, shape, strides):
    """1 with the tables zeroed before anything is written -- the good view in front of the bad one included"""
    import torch
    dtype = np.uint16
    good = _views(["A_short"])[0]
    # encode
    P = Parents(dtype)
    slot = 4096
    buf = torch.full((slot * 2,), CANARY, dtype=torch.uint8, device=_dev())
    pad = (1,) * (len(shape) - 3)
    rc, offs, lens = sqy.encode_batch_strided_device("bitswap1->lz4", [P.ptr(good), P.ptr(good)], [pad + good.shape, shape], [pad + good.strides, strides], dtype,
                                                     buf.data_ptr(), slot)
    torch.cuda.synchronize()
    assert rc == 1 and offs == [0, 0] and lens == [0, 0] and (buf.cpu().numpy() == CANARY).all(), why
    # decode: blobs of the right shapes, so that only the strides are wrong
    rc, blob = sqy.encode("bitswap1->lz4", good.cut(_parent_data(dtype)[good.parent]))
    rc2, blob2 = sqy.encode("bitswap1->lz4", synth.stack((3, 5, 7), dtype, seed=3))
    assert rc == 0 and rc2 == 0
    src = torch.from_numpy(np.frombuffer(blob + blob2, dtype=np.uint8).copy()).to(_dev())
    D = Parents(dtype, data=False)
    rc, decoded = sqy.decode_batch_strided_device(src.data_ptr(), [0, len(blob)], [len(blob), len(blob2)], [D.ptr(good), D.ptr(good)], [pad + good.shape, shape],
                                                  [pad + good.strides, strides], dtype)
    assert rc == 1 and decoded == [0, 0], why
    _same(D.read(), D.host)


def test_refused_pointer_and_shape(sqy):
    import torch
    dtype = np.uint16
    a, b = _views(["A_short", "A_wide"])
    P = Parents(dtype)
    buf = torch.full((2 * 8192,), CANARY, dtype=torch.uint8, device=_dev())
    rc, offs, lens = sqy.encode_batch_strided_device("lz4", [P.ptr(a), P.ptr(b) + 1], [a.shape, b.shape], [a.strides, b.strides], dtype, buf.data_ptr(), 8192)
    torch.cuda.synchronize()
    assert rc == 1 and offs == [0, 0] and lens == [0, 0] and (buf.cpu().numpy() == CANARY).all()
    rc, (src, offs, lens, _) = _encode(sqy, "bitswap1->lz4", [a, b], dtype, keep=True)
    assert rc == 0
    D = Parents(dtype, data=False)
    # a misaligned destination
    rc, decoded = sqy.decode_batch_strided_device(src.data_ptr(), offs, lens, [D.ptr(a), D.ptr(b) + 1], [a.shape, b.shape], [a.strides, b.strides], dtype)
    assert rc == 1 and decoded == [0, 0]
    _same(D.read(), D.host)
    # the header's shape is not the view's: another extent, the same voxels in another shape, another rank
    for shapes, strides in (([a.shape, (4, 16, 31)], [a.strides, b.strides]), ([a.shape, (4, 32, 16)], [a.strides, b.strides]),
                            ([(15, 7), (64, 32)], [(72, 1), (72, 1)])):
        rc, decoded = sqy.decode_batch_strided_device(src.data_ptr(), offs, lens, [D.ptr(a), D.ptr(b)], shapes, strides, dtype)
        assert rc == 1 and decoded == [0, 0], shapes
        _same(D.read(), D.host)


def test_callers_stream(sqy, oracle):
    import torch
    views = _views(NON_DENSE)
    s = torch.cuda.Stream(device=_dev())
    blobs = _check_encode(sqy, oracle, "bitswap1->lz4", views, np.uint16, stream=s.cuda_stream)
    rc, (buf, offs, lens, _) = _encode(sqy, "bitswap1->lz4", views, np.uint16, stream=s.cuda_stream, keep=True)
    assert rc == 0
    rc, _, got, P = _decode(sqy, buf, offs, lens, views, np.uint16, stream=s.cuda_stream)
    data = _parent_data(np.uint16)
    assert rc == 0 and len(blobs) == len(views)
    _same(got, P.expect(views, [v.cut(data[v.parent]) for v in views]))


def test_two_host_threads(sqy, oracle):
    import torch
    sets = [_views(["A_wide", "A_short", "B_big"]), _views(["A_odd", "C", "A_last"])]
    data = _parent_data(np.uint16)
    want = [[_want(sqy, oracle, "bitswap1->lz4", v.cut(data[v.parent]), 0, _dev(), ("strided", v.name, "uint16")) for v in s] for s in sets]
    streams = [torch.cuda.Stream(device=_dev()) for _ in sets]
    ok = [False, False]

    def one(t):
        good = True
        for _ in range(3):
            rc, (buf, offs, lens, blobs) = _encode(sqy, "bitswap1->lz4", sets[t], np.uint16, stream=streams[t].cuda_stream, keep=True)
            good = good and rc == 0 and blobs == want[t]
            rc, _, got, P = _decode(sqy, buf, offs, lens, sets[t], np.uint16, stream=streams[t].cuda_stream)
            image = P.expect(sets[t], [v.cut(data[v.parent]) for v in sets[t]])
            good = good and rc == 0 and all(np.array_equal(got[k], image[k]) for k in image)
        ok[t] = good
    th = [threading.Thread(target=one, args=(t,)) for t in range(2)]
    for x in th:
        x.start()
    for x in th:
        x.join()
    assert all(ok)
