"""SQYAMD_Decode_Slabs_*: a set of z-slab blobs decoded with one call -- the inverse of SQYAMD_PipelineEncode_Slabs_*_Device and the reader
of the multi-GPU container.  The volume must be the concatenation of what SQYAMD_Decode_*_Device gives for every blob (and the source for
lossless pipelines), whichever way the blobs are grouped, with the joint path or without it."""
import ctypes
import threading

import numpy as np
import pytest

from sqeazy_amd import synth, multi

pytestmark = pytest.mark.gpu

CANARY = 0xA5


def _encode_slabs(sqy, pipeline, vol, nslabs, dev):
    """(device buffer, offsets, lengths) of SQYAMD_PipelineEncode_Slabs_*_Device on vol"""
    import torch
    shape, dtype = vol.shape, vol.dtype
    d_vol = torch.from_numpy(vol.copy()).to(dev)
    biggest = (-(-shape[0] // nslabs),) + tuple(shape[1:])
    cap = (sqy.max_compressed_length(pipeline, biggest, dtype) + 255) & ~255
    out = torch.zeros(cap * nslabs, dtype=torch.uint8, device=dev)
    rc, offs, lens = sqy.encode_slabs_device(pipeline, d_vol.data_ptr(), shape, dtype, nslabs, out.data_ptr(), cap, inflight=3)
    assert rc == 0
    return out, offs, lens


def _decode_one_device(sqy, d_src, length, d_dst, capacity, dtype):
    fn = getattr(sqy.lib(), "SQYAMD_Decode_%s_Device" % ("UI16" if np.dtype(dtype) == np.uint16 else "UI8"))
    return fn(ctypes.c_void_p(int(d_src)), ctypes.c_long(int(length)), ctypes.c_void_p(int(d_dst)), ctypes.c_long(int(capacity)), None)


def _per_blob(sqy, buf, offs, lens, dtype, dev):
    """the concatenation of SQYAMD_Decode_*_Device of every blob (bytes, on the host) and the frames of every blob"""
    import torch
    parts, frames = [], []
    for o, n in zip(offs, lens):
        blob = bytes(buf[o:o + n].cpu().numpy().tobytes())
        shape = sqy.decompressed_shape(blob)
        nb = int(np.prod(shape)) * np.dtype(dtype).itemsize
        dst = torch.empty(nb, dtype=torch.uint8, device=dev)
        assert _decode_one_device(sqy, buf.data_ptr() + o, n, dst.data_ptr(), nb, dtype) == 0
        parts.append(dst.cpu().numpy().tobytes())
        frames.append(shape[0])
    return b"".join(parts), frames


def _decode_slabs(sqy, buf, offs, lens, total, dtype, dev, inflight=0, canary=256):
    """Decode_Slabs into a buffer with canaries on both sides; returns (rc, frames, volume bytes); the canaries must hold"""
    import torch
    d = torch.full((total + 2 * canary,), CANARY, dtype=torch.uint8, device=dev)
    rc, frames = sqy.decode_slabs_device(buf.data_ptr(), offs, lens, d.data_ptr() + canary, total, dtype, inflight=inflight)
    torch.cuda.synchronize()
    h = d.cpu().numpy()
    assert (h[:canary] == CANARY).all() and (h[canary + total:] == CANARY).all(), "written outside the volume"
    return rc, frames, h[canary:canary + total].tobytes()


def _profile_names(sqy, fn):
    sqy.profile_reset()
    sqy.profile_enable(True)
    try:
        fn()
    finally:
        sqy.profile_enable(False)
    got = sqy.profile_get()
    sqy.profile_reset()
    return got


LOSSLESS = ("bitswap1->lz4", "diff3x3x1->bitswap1->lz4", "frame_shuffle->lz4", "lz4")


@pytest.mark.parametrize("pipeline,shape,dtype,nslabs", [
    ("bitswap1->lz4", (64, 256, 256), np.uint16, 4),
    ("bitswap1->lz4", (37, 128, 256), np.uint16, 5),            # uneven split: 8, 8, 7, 7, 7 frames
    ("diff3x3x1->bitswap1->lz4", (48, 128, 128), np.uint16, 3),
    ("quantiser->bitswap1->lz4", (32, 128, 128), np.uint16, 4),
    ("frame_shuffle->lz4", (64, 64, 128), np.uint8, 4),
    ("bitswap1->lz4", (16, 64, 64), np.uint16, 16),
    ("bitswap1->lz4", (48, 256, 512), np.uint16, 3),             # 16 and more chunks per blob: the joint path
    ("diff3x3x1->bitswap1->lz4", (48, 256, 512), np.uint16, 3),
    ("quantiser->bitswap1->lz4", (48, 512, 512), np.uint16, 3),
    ("frame_shuffle->lz4", (48, 512, 512), np.uint8, 3),
])
def test_round_trip_with_encode_slabs(sqy, options, pipeline, shape, dtype, nslabs):
    import torch
    dev = torch.device("cuda", 0)
    vol = synth.stack(shape, dtype)
    buf, offs, lens = _encode_slabs(sqy, pipeline, vol, nslabs, dev)
    want, want_frames = _per_blob(sqy, buf, offs, lens, dtype, dev)
    assert want_frames == [multi.slab_range(shape[0], i, nslabs)[1] for i in range(nslabs)]
    if pipeline in LOSSLESS:
        assert want == vol.tobytes()
    for inflight in (1, 3, nslabs, 0):
        rc, frames, got = _decode_slabs(sqy, buf, offs, lens, len(want), dtype, dev, inflight=inflight)
        assert rc == 0 and frames == want_frames and got == want, (pipeline, inflight)
    options("decode_slabs_joint", 0)
    rc, frames, got = _decode_slabs(sqy, buf, offs, lens, len(want), dtype, dev)
    assert rc == 0 and frames == want_frames and got == want


@pytest.mark.parametrize("pipeline,dtype", [("bitswap1->lz4", np.uint16), ("quantiser->bitswap1->lz4", np.uint16),
                                            ("frame_shuffle->lz4", np.uint8), ("lz4", np.uint16)])
def test_the_joint_path_is_taken(sqy, options, pipeline, dtype):
    import torch
    dev = torch.device("cuda", 0)
    k = 5
    shape = (8 * k, 256, 512) if dtype == np.uint16 else (8 * k, 512, 512)
    vol = synth.stack(shape, dtype)
    buf, offs, lens = _encode_slabs(sqy, pipeline, vol, k, dev)
    want, _ = _per_blob(sqy, buf, offs, lens, dtype, dev)
    out = torch.empty(len(want), dtype=torch.uint8, device=dev)

    def run(inflight):
        return _profile_names(sqy, lambda: sqy.decode_slabs_device(buf.data_ptr(), offs, lens, out.data_ptr(), len(want), dtype,
                                                                   inflight=inflight))
    for inflight, groups in ((0, 1), (2, (k + 1) // 2)):
        p = run(inflight)
        assert p["slabs_frame_index"][1] == groups and p["slabs_lz4_decode"][1] == groups, p
        assert "lz4_frame_rank" not in p and "lz4_frames_decode" not in p and "lz4_frame_index" not in p, p
        assert bytes(out.cpu().numpy().tobytes()) == want
    options("decode_slabs_joint", 0)
    out.zero_()
    p = run(0)
    assert "slabs_frame_index" not in p and "slabs_lz4_decode" not in p, p
    assert p["lz4_frame_rank"][1] >= k and p["lz4_frames_decode"][1] == k, p
    assert bytes(out.cpu().numpy().tobytes()) == want


def _blob(sqy, pipeline, vol, nthreads=2):
    rc, b = sqy.encode(pipeline, vol, nthreads=nthreads, extra_capacity=4096)
    assert rc == 0
    return b


def _to_device(blobs, dev, gaps):
    """the blobs back to back in one device buffer, gaps[i] bytes in front of blob i (unaligned offsets)"""
    import torch
    offs, parts, at = [], [], 0
    for b, g in zip(blobs, gaps):
        parts.append(b"\x00" * g)
        at += g
        offs.append(at)
        parts.append(b)
        at += len(b)
    host = np.frombuffer(b"".join(parts), dtype=np.uint8).copy()
    return torch.from_numpy(host).to(dev), offs, [len(b) for b in blobs]


def test_mixed_sets_u16(sqy, options):
    """blobs of different pipelines -- chunked, the serial layout (nthreads = 1), plain lz4, a single chunk -- in one set"""
    import torch
    dev = torch.device("cuda", 0)
    Y, X = 256, 512
    vols = [synth.stack((z, Y, X), np.uint16, seed=100 + i) for i, z in enumerate((9, 16, 5, 12, 1, 7))]
    blobs = [_blob(sqy, "bitswap1->lz4", vols[0]), _blob(sqy, "bitswap1->lz4", vols[1], nthreads=1), _blob(sqy, "lz4", vols[2]),
             _blob(sqy, "diff3x3x1->bitswap1->lz4", vols[3]), _blob(sqy, "bitswap1->lz4", vols[4]), _blob(sqy, "quantiser->bitswap1->lz4", vols[5])]
    buf, offs, lens = _to_device(blobs, dev, (3, 1, 7, 0, 5, 2))
    want, frames_want = _per_blob(sqy, buf, offs, lens, np.uint16, dev)
    assert want[:vols[0].nbytes + vols[1].nbytes + vols[2].nbytes] == b"".join(v.tobytes() for v in vols[:3])
    for joint in (1, 0):
        options("decode_slabs_joint", joint)
        for inflight in (0, 2):
            rc, frames, got = _decode_slabs(sqy, buf, offs, lens, len(want), np.uint16, dev, inflight=inflight)
            assert rc == 0 and frames == frames_want and got == want, (joint, inflight)


def test_mixed_sets_u8_unaligned_places(sqy):
    """u8 slabs of 5, 33 and 37 frames of odd frame bytes: the slabs' places in d_dst are not aligned"""
    import torch
    dev = torch.device("cuda", 0)
    Y, X = 331, 799
    vols = [synth.stack((z, Y, X), np.uint8, seed=7 + z) for z in (5, 33, 37)]
    for pipeline in ("lz4", "bitswap1->lz4", "frame_shuffle->lz4"):
        blobs = [_blob(sqy, pipeline, v) for v in vols]
        buf, offs, lens = _to_device(blobs, dev, (1, 3, 2))
        want, frames_want = _per_blob(sqy, buf, offs, lens, np.uint8, dev)
        assert want == b"".join(v.tobytes() for v in vols)
        rc, frames, got = _decode_slabs(sqy, buf, offs, lens, len(want), np.uint8, dev)
        assert rc == 0 and frames == [5, 33, 37] and got == want, pipeline


def test_container(sqy):
    """the container of the multi-GPU path (u64 count | u64 sizes | blobs, back to back at unaligned offsets) through decode_container and
    the host-pointer entry point"""
    import torch
    vol = synth.stack((40, 256, 384), np.uint16)
    blobs = []
    for i in range(4):
        z0, nz = multi.slab_range(40, i, 4)
        blobs.append(_blob(sqy, "bitswap1->lz4" if i != 2 else "diff3x3x1->bitswap1->lz4", vol[z0:z0 + nz]))
    flat = torch.from_numpy(np.frombuffer(b"".join(blobs), dtype=np.uint8).copy())
    buf = multi.pack_container([len(b) for b in blobs], flat)
    assert any((8 + 8 * 4 + sum(len(b) for b in blobs[:i])) % 16 for i in range(1, 4))
    rc, got = multi.decode_container(buf, np.uint16)
    assert rc == 0 and np.array_equal(got, vol)
    assert multi.decode_container(buf, np.uint8)[0] == 1
    rc, got = sqy.decode_slabs(blobs)
    assert rc == 0 and np.array_equal(got, vol)


def test_errors_write_nothing(sqy):
    import torch
    dev = torch.device("cuda", 0)
    a = _blob(sqy, "bitswap1->lz4", synth.stack((6, 128, 256), np.uint16))
    b = _blob(sqy, "bitswap1->lz4", synth.stack((5, 128, 256), np.uint16, seed=3))
    other = _blob(sqy, "bitswap1->lz4", synth.stack((5, 128, 128), np.uint16))          # another shape[1..]
    u8 = _blob(sqy, "bitswap1->lz4", synth.stack((5, 128, 256), np.uint8))               # another voxel type
    total = (6 + 5) * 128 * 256 * 2

    def check(blobs, capacity=total, cut=None, nslabs=None):
        buf, offs, lens = _to_device(blobs, dev, [1] * len(blobs))
        if cut is not None:
            lens[cut] = 40                                                                # a length that cuts the header
        d = torch.full((total + 512,), CANARY, dtype=torch.uint8, device=dev)
        n = len(blobs) if nslabs is None else nslabs
        rc, _ = sqy.decode_slabs_device(buf.data_ptr(), offs[:max(n, 0)], lens[:max(n, 0)], d.data_ptr() + 256, capacity, np.uint16)
        torch.cuda.synchronize()
        assert (d.cpu().numpy() == CANARY).all(), "written although the call was refused"
        return rc
    assert check([a, other]) == 1
    assert check([a, u8]) == 1
    assert check([a, b], capacity=total - 1) == 1
    assert check([a, b], cut=1) == 1
    assert check([a, b], nslabs=0) == 1
    assert sqy.decode_slabs([])[0] == 1


@pytest.mark.parametrize("joint", [1, 0])
def test_damaged_frame(sqy, options, joint):
    """a damaged LZ4 frame in slab k: SQY_Decode's code for that blob alone, nothing written outside the volume"""
    import torch
    dev = torch.device("cuda", 0)
    options("decode_slabs_joint", joint)
    vols = [synth.stack((16, 256, 256), np.uint16, seed=40 + i) for i in range(4)]
    blobs = [_blob(sqy, "bitswap1->lz4", v) for v in vols]
    comp = [f for f in _lz4_frames(blobs[2], sqy) if not f[3]]
    bad = _damaged(blobs[2], comp[0])
    rc_alone, _ = sqy.decode(bad)
    assert rc_alone == 11
    buf, offs, lens = _to_device(blobs[:2] + [bad] + blobs[3:], dev, (0, 5, 3, 1))
    total = sum(v.nbytes for v in vols)
    rc, frames, got = _decode_slabs(sqy, buf, offs, lens, total, np.uint16, dev)
    assert rc == rc_alone
    fb = vols[0].nbytes
    assert got[:2 * fb] == b"".join(v.tobytes() for v in vols[:2]) and got[3 * fb:] == vols[3].tobytes()


def _lz4_frames(blob, sqy):
    """(start, body start, body size, stored) of every LZ4 frame of a single-block-frame payload"""
    out, off = [], sqy.header_size(blob)
    while off < len(blob):
        assert blob[off:off + 4] == bytes([0x04, 0x22, 0x4D, 0x18])
        word = int.from_bytes(blob[off + 7:off + 11], "little")
        out.append((off, off + 11, word & 0x7fffffff, bool(word >> 31)))
        off += 11 + (word & 0x7fffffff) + 4
    return out


def _damaged(blob, frame):
    _, body, size, stored = frame
    assert not stored
    b = bytearray(blob)
    b[body:body + size] = b"\xff" * size                  # a literal length that runs past the block's end
    return bytes(b)


def test_work_queued_on_the_callers_stream_is_respected(sqy):
    """the blobs are written by a copy queued on the caller's stream just before the call, and a fill of the destination as well"""
    import torch
    dev = torch.device("cuda", 0)
    vols = [synth.stack((16, 256, 512), np.uint16, seed=60 + i) for i in range(3)]
    blobs = [_blob(sqy, "bitswap1->lz4", v) for v in vols]
    host = torch.from_numpy(np.frombuffer(b"".join(blobs), dtype=np.uint8).copy()).pin_memory()
    offs = [0, len(blobs[0]), len(blobs[0]) + len(blobs[1])]
    lens = [len(b) for b in blobs]
    total = sum(v.nbytes for v in vols)
    s = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(s):
        d_blobs = torch.empty(len(host), dtype=torch.uint8, device=dev)
        out = torch.empty(total, dtype=torch.uint8, device=dev)
        for _ in range(2):
            d_blobs.zero_()
            out.fill_(7)
            d_blobs.copy_(host, non_blocking=True)
            rc, frames = sqy.decode_slabs_device(d_blobs.data_ptr(), offs, lens, out.data_ptr(), total, np.uint16, stream=s.cuda_stream)
            assert rc == 0 and frames == [16, 16, 16]
            assert bytes(out.cpu().numpy().tobytes()) == b"".join(v.tobytes() for v in vols)


def test_several_host_threads(sqy):
    sets = []
    for t in range(4):
        vols = [synth.stack((8 + t, 256, 256), np.uint16, seed=80 + 4 * t + i) for i in range(3)]
        sets.append((vols, [_blob(sqy, "bitswap1->lz4", v) for v in vols]))
    ok = [False] * 4

    def one(t):
        vols, blobs = sets[t]
        good = True
        for _ in range(3):
            rc, got = sqy.decode_slabs(blobs)
            good = good and rc == 0 and np.array_equal(got, np.concatenate(vols))
        ok[t] = good
    th = [threading.Thread(target=one, args=(t,)) for t in range(4)]
    for x in th:
        x.start()
    for x in th:
        x.join()
    assert all(ok)


def test_full_size(sqy):
    """four 2048 x 2048 x 256 u16 bitswap1->lz4 slabs of one volume, Encode_Slabs -> Decode_Slabs, equal the source"""
    import torch
    dev = torch.device("cuda", 0)
    Z, Y, X, n = 1024, 2048, 2048, 4
    pipeline = "bitswap1->lz4"
    cap = (sqy.max_compressed_length(pipeline, (Z // n, Y, X), np.uint16) + 255) & ~255
    enc = torch.empty(cap * n, dtype=torch.uint8, device=dev)
    vol = torch.empty((Z, Y, X), dtype=torch.uint16, device=dev)
    for i in range(n):
        vol[i * (Z // n):(i + 1) * (Z // n)] = synth.stack_torch((Z // n, Y, X), np.uint16, dev, z_offset=i * (Z // n), z_total=Z)
    rc, offs, lens = sqy.encode_slabs_device(pipeline, vol.data_ptr(), (Z, Y, X), np.uint16, n, enc.data_ptr(), cap, inflight=3)
    assert rc == 0
    out = torch.empty((Z, Y, X), dtype=torch.uint16, device=dev)
    rc, frames = sqy.decode_slabs_device(enc.data_ptr(), offs, lens, out.data_ptr(), out.numel() * 2, np.uint16)
    torch.cuda.synchronize()
    assert rc == 0 and frames == [Z // n] * n
    assert torch.equal(out, vol)
    del enc, vol, out
    torch.cuda.empty_cache()
