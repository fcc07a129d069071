"""SQYAMD_Decode_Batch_*: many independent blobs -- shapes and pipelines may differ -- decoded with one call, each into an allocation of its
own: the way back from SQYAMD_PipelineEncode_Batch_*.  Every destination must hold the source volume (lossless pipelines) and exactly what
SQYAMD_Decode_*_Device writes for that blob alone, and nothing outside it may be touched (64 canary bytes in front of and behind every
destination are checked after every call, whatever it returns) -- whichever way the blobs are grouped, on the joint path or without it."""
import ctypes
import threading

import numpy as np
import pytest

from sqeazy_amd import synth

pytestmark = pytest.mark.gpu

CANARY = 0xA5
GAP = 64

SHAPES = ((16, 64, 128),          # one chunk
          (20, 64, 128),          # two chunks with a short last one, exactly 5 transposer tiles
          (9, 61, 67),            # 36 783 voxels: a partial last tile, plane bytes no multiple of 16, 15 tail voxels
          (3, 5, 7),              # 105 voxels, 9 tail voxels
          (1, 1, 5),              # no whole plane word, a stored frame below LZ4's minimum
          (32, 64, 128))          # two whole chunks
SINGLE_KERNELS = ("bitswap1_decode", "bitswap1_quantiser_decode", "lz4_frame_index", "lz4_frame_rank", "lz4_frames_decode")


def _dev():
    import torch
    return torch.device("cuda", 0)


def _profiled(sqy, fn):
    sqy.profile_reset()
    sqy.profile_enable(True)
    try:
        out = fn()
    finally:
        sqy.profile_enable(False)
    got = sqy.profile_get()
    sqy.profile_reset()
    return out, got


def _encode_batch(sqy, pipeline, vols, nthreads=0):
    """SQYAMD_PipelineEncode_Batch_*_Device on device copies of vols; the blobs stay in the call's own buffer (slots no multiple of 16:
    the blobs are misaligned) -- (buffer, offsets, lengths), to be passed straight through"""
    import torch
    dev = _dev()
    dtype = vols[0].dtype
    srcs = [torch.from_numpy(v.copy()).to(dev) for v in vols]
    slot = ((max(max(sqy.max_compressed_length(pipeline, v.shape, dtype), 64) for v in vols) + 15) & ~15) + 13      # 13 modulo 16, whatever the set
    buf = torch.zeros(slot * len(vols), dtype=torch.uint8, device=dev)
    rc, offs, lens = sqy.encode_batch_device(pipeline, [s.data_ptr() for s in srcs], [v.shape for v in vols], dtype, buf.data_ptr(), slot, nthreads=nthreads)
    torch.cuda.synchronize()
    assert rc == 0
    assert any(o % 16 for o in offs)
    return buf, offs, lens


def _pack(blobs, gaps=None):
    """blobs (bytes) in one device buffer, gaps[i] bytes in front of blob i"""
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


def _alone(sqy, buf, off, length, nbytes, dtype):
    """(rc, bytes) of SQYAMD_Decode_*_Device for one blob of the buffer"""
    import torch
    fn = getattr(sqy.lib(), "SQYAMD_Decode_%s_Device" % ("UI16" if np.dtype(dtype) == np.uint16 else "UI8"))
    dst = torch.zeros(max(nbytes, 1), dtype=torch.uint8, device=_dev())
    rc = fn(ctypes.c_void_p(buf.data_ptr() + off), ctypes.c_long(length), ctypes.c_void_p(dst.data_ptr()), ctypes.c_long(nbytes), None)
    torch.cuda.synchronize()
    return rc, dst[:nbytes].cpu().numpy().tobytes()


class Dsts:
    """one allocation per destination: 64 canary bytes, `shift` more to leave the 16-byte grid, the volume's place, 64 canary bytes"""

    def __init__(self, nbytes, shift=0):
        import torch
        self.nbytes, self.shift = list(nbytes), shift
        self.bufs = [torch.full((GAP + shift + nb + GAP,), CANARY, dtype=torch.uint8, device=_dev()) for nb in self.nbytes]
        assert all(b.data_ptr() % 16 == 0 for b in self.bufs)
        self.ptrs = [b.data_ptr() + GAP + shift for b in self.bufs]

    def read(self, written=True):
        """the destinations' bytes; the canaries must hold (written = False: the places themselves as well)"""
        import torch
        torch.cuda.synchronize()
        out = []
        for i, (b, nb) in enumerate(zip(self.bufs, self.nbytes)):
            h = b.cpu().numpy()
            lo = GAP + self.shift
            assert (h[:lo] == CANARY).all() and (h[lo + nb:] == CANARY).all(), "written outside destination %d" % i
            if not written:
                assert (h == CANARY).all(), "destination %d written although the call was refused" % i
            out.append(h[lo:lo + nb].tobytes())
        return out


def _decode_batch(sqy, buf, offs, lens, nbytes, dtype, shift=0, stream=None):
    d = Dsts(nbytes, shift)
    rc, decoded = sqy.decode_batch_device(buf.data_ptr(), offs, lens, d.ptrs, nbytes, dtype, stream=stream)
    return rc, decoded, d.read()


def _expected(sqy, buf, offs, lens, vols, got, lossless=True):
    """`expected` of every test: the source volume, and what the single call writes for that blob alone"""
    for i, v in enumerate(vols):
        if lossless is True or i in lossless:
            assert got[i] == v.tobytes(), "blob %d differs from its source" % i
        rc, alone = _alone(sqy, buf, offs[i], lens[i], v.nbytes, v.dtype)
        assert rc == 0 and got[i] == alone, "blob %d differs from the single call" % i


def _vols(dtype, shapes=SHAPES, seed=500):
    return [synth.stack(s, dtype, seed=seed + i) for i, s in enumerate(shapes)]


@pytest.mark.parametrize("shift_words", [0, 1])
@pytest.mark.parametrize("dtype", [np.uint16, np.uint8])
@pytest.mark.parametrize("pipeline", ["bitswap1->lz4", "lz4"])
def test_round_trip_of_a_batch_encode(sqy, pipeline, dtype, shift_words):
    """the six shapes through PipelineEncode_Batch and back, offsets and lengths passed straight through; shift_words = 1: every destination
    one voxel behind a 16-byte boundary (the word-by-word stores)"""
    vols = _vols(dtype)
    buf, offs, lens = _encode_batch(sqy, pipeline, vols)
    nbytes = [v.nbytes for v in vols]
    shift = shift_words * np.dtype(dtype).itemsize
    (rc, decoded, got), prof = _profiled(sqy, lambda: _decode_batch(sqy, buf, offs, lens, nbytes, dtype, shift=shift))
    assert rc == 0 and decoded == nbytes
    _expected(sqy, buf, offs, lens, vols, got)
    assert prof["batch_frame_index"][1] == 1 and prof["batch_lz4_decode"][1] == 1, prof
    if pipeline == "bitswap1->lz4":
        assert prof["batch_bitswap1_decode"][1] == 1 and "batch_copy" not in prof, prof
    else:
        assert "batch_bitswap1_decode" not in prof and prof["batch_copy"][1] == 1, prof
    assert not any(k.startswith(SINGLE_KERNELS) for k in prof), prof


@pytest.mark.parametrize("dtype", [np.uint16, np.uint8])
@pytest.mark.parametrize("pipeline", ["bitswap1->lz4(blocksize_kb=4,framestep_kb=4)", "lz4(n_chunks_of_input=7)"])
def test_small_chunks(sqy, pipeline, dtype):
    """many frames per blob in one joint launch"""
    vols = _vols(dtype, ((8, 32, 32), (7, 33, 31)), seed=520)
    buf, offs, lens = _encode_batch(sqy, pipeline, vols)
    nbytes = [v.nbytes for v in vols]
    (rc, decoded, got), prof = _profiled(sqy, lambda: _decode_batch(sqy, buf, offs, lens, nbytes, dtype))
    assert rc == 0 and decoded == nbytes
    _expected(sqy, buf, offs, lens, vols, got)
    assert prof["batch_lz4_decode"][1] == 1 and not any(k.startswith(SINGLE_KERNELS) for k in prof), prof


def test_mixed_pipelines_and_layouts_u16(sqy, oracle):
    """oracle-made blobs (independent of the product's encoder): three lz4-terminated pipelines, pass_through, and a two-chunk blob in the
    serial layout (nthreads = 1), which must take the single path"""
    shape = (12, 64, 64)
    pipes = [("bitswap1->lz4", 2), ("quantiser->bitswap1->lz4", 2), ("diff3x3x1->bitswap1->lz4", 2), ("pass_through", 2),
             ("bitswap1->lz4(blocksize_kb=64,framestep_kb=64)", 1)]
    vols = _vols(np.uint16, [shape] * len(pipes), seed=540)
    buf, offs, lens = _pack([oracle.pipeline_encode(p, v, nthreads=t) for (p, t), v in zip(pipes, vols)], gaps=(3, 1, 7, 0, 5))
    nbytes = [v.nbytes for v in vols]
    (rc, decoded, got), prof = _profiled(sqy, lambda: _decode_batch(sqy, buf, offs, lens, nbytes, np.uint16))
    assert rc == 0 and decoded == nbytes
    _expected(sqy, buf, offs, lens, vols, got, lossless=(0, 2, 3, 4))
    assert prof["batch_lz4_decode"][1] == 1, prof
    assert prof["batch_bitswap1_decode"][1] == 1, prof                      # blob 0; the other two run their inverses blob by blob
    assert "lz4_frame_index" in prof or "lz4_linked_decode" in prof, prof  # the serial layout went through the single path


def test_mixed_pipelines_u8(sqy, oracle):
    shape = (12, 64, 64)
    pipes = ["frame_shuffle->lz4", "bitswap1->lz4", "pass_through", "lz4"]
    vols = _vols(np.uint8, [shape] * len(pipes), seed=560)
    buf, offs, lens = _pack([oracle.pipeline_encode(p, v, nthreads=2) for p, v in zip(pipes, vols)], gaps=(1, 2, 3, 5))
    nbytes = [v.nbytes for v in vols]
    (rc, decoded, got), prof = _profiled(sqy, lambda: _decode_batch(sqy, buf, offs, lens, nbytes, np.uint8))
    assert rc == 0 and decoded == nbytes
    _expected(sqy, buf, offs, lens, vols, got)
    assert prof["batch_lz4_decode"][1] == 1, prof


def test_grouping_and_the_switch(sqy, options):
    vols = _vols(np.uint16)
    buf, offs, lens = _encode_batch(sqy, "bitswap1->lz4", vols)
    nbytes = [v.nbytes for v in vols]
    want = [v.tobytes() for v in vols]
    options("decode_batch_group_bytes", 300000)
    (rc, _, got), prof = _profiled(sqy, lambda: _decode_batch(sqy, buf, offs, lens, nbytes, np.uint16))
    assert rc == 0 and got == want
    assert prof["batch_lz4_decode"][1] > 1 and prof["batch_lz4_decode"][1] == prof["batch_frame_index"][1], prof
    options("decode_batch_joint", 0)
    (rc, _, got), prof = _profiled(sqy, lambda: _decode_batch(sqy, buf, offs, lens, nbytes, np.uint16))
    assert rc == 0 and got == want
    assert not any(k.startswith("batch_") for k in prof), prof


@pytest.mark.parametrize("pipeline", ["bitswap1->lz4", "lz4"])
def test_stored_and_compressed_side_by_side(sqy, pipeline):
    rng = np.random.default_rng(7)
    vols = [rng.integers(0, 65536, (9, 64, 64), dtype=np.uint16), np.zeros((10, 64, 64), np.uint16), synth.stack((12, 64, 64), np.uint16, seed=580)]
    buf, offs, lens = _encode_batch(sqy, pipeline, vols)
    nbytes = [v.nbytes for v in vols]
    rc, decoded, got = _decode_batch(sqy, buf, offs, lens, nbytes, np.uint16)
    assert rc == 0 and decoded == nbytes
    _expected(sqy, buf, offs, lens, vols, got)


def _first_compressed_frame(sqy, blob):
    off = sqy.header_size(blob)
    while off < len(blob):
        assert blob[off:off + 4] == bytes([0x04, 0x22, 0x4D, 0x18])
        word = int.from_bytes(blob[off + 7:off + 11], "little")
        if not word >> 31:
            return off + 11, word
        off += 11 + (word & 0x7fffffff) + 4
    raise AssertionError("no compressed frame")


def test_a_damaged_blob_in_mid_batch(sqy):
    """blob 2 of 5 holds a compressed block whose bytes are all 0xff -- a literal length that runs past the block's end, the damage the
    decoder's tests use: input the decoder refuses.  The call returns the code the single call gives that blob, the other four are in place."""
    vols = _vols(np.uint16, [(12, 64, 64)] * 5, seed=600)
    blobs = []
    for v in vols:
        rc, b = sqy.encode("bitswap1->lz4", v, nthreads=2)
        assert rc == 0
        blobs.append(b)
    body, size = _first_compressed_frame(sqy, blobs[2])
    bad = bytearray(blobs[2])
    bad[body:body + size] = b"\xff" * size
    blobs[2] = bytes(bad)
    buf, offs, lens = _pack(blobs, gaps=(0, 5, 3, 1, 2))
    nbytes = [v.nbytes for v in vols]
    rc_alone, _ = _alone(sqy, buf, offs[2], lens[2], nbytes[2], np.uint16)
    assert rc_alone not in (0, 1)
    rc, decoded, got = _decode_batch(sqy, buf, offs, lens, nbytes, np.uint16)
    assert rc == rc_alone and decoded == nbytes
    for i in (0, 1, 3, 4):
        assert got[i] == vols[i].tobytes(), i


def test_checks_before_anything_is_written(sqy):
    vols = _vols(np.uint16, [(6, 32, 64), (5, 32, 64)], seed=620)
    a, b = [sqy.encode("bitswap1->lz4", v, nthreads=2)[1] for v in vols]
    u8 = sqy.encode("bitswap1->lz4", synth.stack((5, 32, 64), np.uint8), nthreads=2)[1]
    nbytes = [v.nbytes for v in vols]

    def refused(blobs, caps=nbytes, cut=None):
        buf, offs, lens = _pack(blobs)
        if cut is not None:
            lens[cut] = 40                                                  # a length that cuts the header
        d = Dsts(nbytes)
        rc, decoded = sqy.decode_batch_device(buf.data_ptr(), offs, lens, d.ptrs, caps, np.uint16)
        d.read(written=False)
        assert decoded == [0, 0]
        return rc
    assert refused([a, b], caps=[nbytes[0], nbytes[1] - 1]) == 1
    assert refused([a, u8]) == 1
    assert refused([a, b], cut=1) == 1
    # a destination off the voxel grid
    buf, offs, lens = _pack([a, b])
    d = Dsts(nbytes)
    rc, decoded = sqy.decode_batch_device(buf.data_ptr(), offs, lens, [d.ptrs[0], d.ptrs[1] + 1], nbytes, np.uint16)
    d.read(written=False)
    assert rc == 1 and decoded == [0, 0]


def test_two_host_threads(sqy):
    import torch
    sets = []
    for t in range(2):
        vols = _vols(np.uint16, [(8 + t, 64, 64), (3, 5, 7), (20, 64, 128), (9, 61, 67)], seed=640 + 10 * t)
        sets.append((vols, _encode_batch(sqy, "bitswap1->lz4", vols), torch.cuda.Stream(device=_dev())))
    torch.cuda.synchronize()
    out = [None, None]

    def one(t):
        vols, (buf, offs, lens), s = sets[t]
        out[t] = _decode_batch(sqy, buf, offs, lens, [v.nbytes for v in vols], np.uint16, stream=s.cuda_stream)
    th = [threading.Thread(target=one, args=(t,)) for t in range(2)]
    for x in th:
        x.start()
    for x in th:
        x.join()
    for t in range(2):
        vols, (buf, offs, lens), _ = sets[t]
        rc, decoded, got = out[t]
        assert rc == 0 and decoded == [v.nbytes for v in vols]
        _expected(sqy, buf, offs, lens, vols, got)


def test_work_queued_on_the_callers_stream_is_seen(sqy):
    """the source buffer is filled -- the blobs copied in from a staging tensor -- on the caller's stream just before the call"""
    import torch
    vols = _vols(np.uint16, [(16, 64, 128), (3, 5, 7), (12, 64, 64)], seed=660)
    buf, offs, lens = _encode_batch(sqy, "bitswap1->lz4", vols)
    staging = buf.cpu().pin_memory()
    nbytes = [v.nbytes for v in vols]
    s = torch.cuda.Stream(device=_dev())
    d = Dsts(nbytes)
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        d_blobs = torch.zeros(len(staging), dtype=torch.uint8, device=_dev())
        d_blobs.copy_(staging, non_blocking=True)
        rc, decoded = sqy.decode_batch_device(d_blobs.data_ptr(), offs, lens, d.ptrs, nbytes, np.uint16, stream=s.cuda_stream)
    assert rc == 0 and decoded == nbytes
    assert d.read() == [v.tobytes() for v in vols]


@pytest.mark.parametrize("dtype", [np.uint16, np.uint8])
@pytest.mark.parametrize("pipeline", ["bitswap1->lz4", "lz4"])
def test_host_variants(sqy, pipeline, dtype):
    vols = _vols(dtype)
    back = sqy.decode_batch(sqy.encode_batch(pipeline, vols))
    assert len(back) == len(vols)
    for v, b in zip(vols, back):
        assert b.dtype == v.dtype and b.shape == v.shape and np.array_equal(v, b)
