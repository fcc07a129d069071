"""GPU: SQYAMD_Decode_Frames_* -- frames [z0, z0 + nz) of a blob without decoding the whole of it (include/sqeazy_amd.h).

Every range equals the same slice of the full decode (and of the oracle's decode), through the subset path and through the fallback
(option decode_frames_subset = 0); the subset path decodes only the LZ4 frames the range needs (profile names, damaged frames outside
the range); arguments are checked before anything is written."""
import base64

import numpy as np
import pytest

from sqeazy_amd import synth

pytestmark = pytest.mark.gpu

PIPES_U16 = ["bitswap1->lz4", "lz4", "bitswap1", "diff3x3x1->bitswap1->lz4", "diff3x3x1->lz4", "frame_shuffle->lz4",
             "frame_shuffle->bitswap1->lz4", "quantiser->bitswap1->lz4", "quantiser->lz4", "quantiser",
             "rmestbkrd->bitswap1->lz4", "rmbkrd_neighbor5x5x5(threshold=40,fraction=0.5)->lz4",
             "rmestbkrd->rmbkrd_neighbor5x5x5->quantiser->bitswap1->lz4"]
PIPES_U8 = ["bitswap1->lz4", "lz4", "frame_shuffle->lz4", "diff3x3x1->lz4", "rmestbkrd->bitswap1->lz4",
            "rmbkrd_neighbor5x5x5(threshold=40,fraction=0.5)->frame_shuffle->lz4"]
GEOMETRIES = ["", "(blocksize_kb=64)", "(n_chunks_of_input=7)"]
# pipelines of the subset path and the range kernel each runs behind lz4_frames_subset_decode
FAST = [("lz4", np.uint16, None), ("lz4", np.uint8, None), ("bitswap1->lz4", np.uint16, "bitswap1_decode_range"),
        ("bitswap1->lz4", np.uint8, "bitswap1_decode_range"), ("quantiser->bitswap1->lz4", np.uint16, "bitswap1_quantiser_decode_range"),
        ("frame_shuffle->lz4", np.uint8, None), ("frame_shuffle->lz4", np.uint16, None),
        ("rmestbkrd->bitswap1->lz4", np.uint16, "bitswap1_decode_range")]


def _volumes(dtype):
    """Y*X not a multiple of 16 and a non-zero len % 16 (len % 8) tail, several LZ4 chunks; Z = 1"""
    rng = np.random.default_rng(5)
    hi = 65536 if dtype == np.uint16 else 256
    a = synth.stack((23, 131, 151), dtype)
    b = rng.integers(0, hi, (7, 97, 203), dtype=dtype)
    b[2:4] = (np.arange(2 * 97 * 203) % 3000).reshape(2, 97, 203).astype(dtype)
    c = synth.stack((1, 700, 777), dtype)
    d = synth.stack((11, 97, 121), dtype)                  # (8-bit diff3x3x1 takes extents up to 127)
    return [a, b, c, d]


def _ranges(Z):
    r = {(0, 1), (Z - 1, 1), (0, Z), (Z // 3, min(5, Z - Z // 3))}
    r.update((z, 1) for z in range(Z))                # every frame: the ones whose plane words straddle a chunk boundary among them
    if Z > 2:
        r.add((1, Z - 2))
    return sorted(r)


def _check_blob(sqy, blob, want_full, ranges):
    for z0, nz in ranges:
        rc, part = sqy.decode_frames(blob, z0, nz)
        assert rc == 0, (z0, nz)
        assert np.array_equal(part, want_full[z0:z0 + nz]), (z0, nz)


def _parity(sqy, oracle, options, pipeline, dtype, nthreads):
    for vol in _volumes(dtype):
        rc, blob = sqy.encode(pipeline, vol, nthreads=nthreads, extra_capacity=16 * vol.shape[0] + 4096)
        if rc:                                            # (a geometry a stage refuses: rmestbkrd on Z = 1, 8-bit diff3x3x1 beyond 127)
            assert "rmestbkrd" in pipeline or "rmbkrd" in pipeline or ("diff3x3x1" in pipeline and max(vol.shape) > 127), (pipeline, vol.shape)
            continue
        rc, full = sqy.decode(blob)
        assert rc == 0
        want = full if "rmestbkrd" in pipeline or "rmbkrd" in pipeline else oracle.pipeline_decode(blob)   # (the oracle has no inverse of the
        if "frame_shuffle" in pipeline:                                                                    #  background heads: a copy)
            _, dmap = oracle.frame_shuffle_encode(vol)
            keep = np.unique(dmap.astype(np.int64))
            assert np.array_equal(full[keep], want[keep])
        else:
            assert np.array_equal(full, want), pipeline
        for subset in (1, 0):
            options("decode_frames_subset", subset)
            _check_blob(sqy, blob, full, _ranges(vol.shape[0]))


@pytest.mark.parametrize("nthreads", [2, 1])
@pytest.mark.parametrize("pipeline", PIPES_U16)
def test_parity_u16(sqy, oracle, options, pipeline, nthreads):
    _parity(sqy, oracle, options, pipeline, np.uint16, nthreads)


@pytest.mark.parametrize("nthreads", [2, 1])
@pytest.mark.parametrize("pipeline", PIPES_U8)
def test_parity_u8(sqy, oracle, options, pipeline, nthreads):
    _parity(sqy, oracle, options, pipeline, np.uint8, nthreads)


@pytest.mark.parametrize("cfg", GEOMETRIES[1:])
@pytest.mark.parametrize("pipeline,dtype", [("bitswap1->lz4", np.uint16), ("bitswap1->lz4", np.uint8), ("lz4", np.uint16),
                                            ("quantiser->bitswap1->lz4", np.uint16), ("frame_shuffle->lz4", np.uint8)])
def test_parity_chunk_geometries(sqy, oracle, options, pipeline, dtype, cfg):
    _parity(sqy, oracle, options, pipeline + cfg, dtype, 2)


def _profile_names(sqy, fn):
    sqy.profile_reset()
    sqy.profile_enable(True)
    try:
        fn()
    finally:
        sqy.profile_enable(False)
    names = set(sqy.profile_get())
    sqy.profile_reset()
    return names


@pytest.mark.parametrize("pipeline,dtype,range_kernel", FAST)
def test_subset_path_decodes_only_a_subset(sqy, options, pipeline, dtype, range_kernel):
    shape = (23, 131, 151)
    if "frame_shuffle" in pipeline:                       # (frames of whole 256 KiB chunks: the map folded into the LZ4 decode)
        shape = (16, 256, 512) if dtype == np.uint16 else (16, 512, 512)
    vol = synth.stack(shape, dtype)
    rc, blob = sqy.encode(pipeline, vol, nthreads=2, extra_capacity=4096)
    assert rc == 0
    rc, full = sqy.decode(blob)
    assert rc == 0
    Z = shape[0]
    for z0, nz in ((0, 1), (Z // 2, 1), (Z - 1, 1), (Z // 2 - 1, 3)):
        out = {}
        names = _profile_names(sqy, lambda: out.update(r=sqy.decode_frames(blob, z0, nz)))
        rc, part = out["r"]
        assert rc == 0 and np.array_equal(part, full[z0:z0 + nz])
        assert "lz4_frames_subset_decode" in names, names
        assert "lz4_frames_decode" not in names and "bitswap1_decode" not in names and "bitswap1_quantiser_decode" not in names, names
        assert "frame_scatter" not in names
        if range_kernel:
            assert range_kernel in names, names
    options("decode_frames_subset", 0)
    names = _profile_names(sqy, lambda: sqy.decode_frames(blob, 0, 1))
    assert "lz4_frames_subset_decode" not in names and "lz4_frames_decode" in names


def _lz4_frames(blob, sqy):
    """(start, body start, body size, stored) of every LZ4 frame of a single-block-frame payload"""
    hs = sqy.header_size(blob)
    out, off = [], hs
    while off < len(blob):
        assert blob[off:off + 4] == bytes([0x04, 0x22, 0x4D, 0x18])
        word = int.from_bytes(blob[off + 7:off + 11], "little")
        size = word & 0x7fffffff
        out.append((off, off + 11, size, bool(word >> 31)))
        off += 11 + size + 4
    return out


def _damaged(blob, frame):
    _, body, size, stored = frame
    assert not stored
    b = bytearray(blob)
    b[body:body + size] = b"\xff" * size                  # a literal length that runs past the block's end
    return bytes(b)


@pytest.mark.parametrize("dtype", [np.uint16, np.uint8])
def test_damaged_frame_outside_the_range_goes_unnoticed(sqy, dtype):
    shape = (8, 512, 512)
    vol = (np.arange(np.prod(shape)) % 3000).astype(dtype).reshape(shape)     # every chunk compressible
    rc, blob = sqy.encode("lz4", vol, nthreads=2)
    assert rc == 0
    frames = _lz4_frames(blob, sqy)
    fb = 512 * 512 * np.dtype(dtype).itemsize
    chunk = 256 << 10
    assert len(frames) == vol.nbytes // chunk
    last = frames[-1]
    bad = _damaged(blob, last)
    rc_full, _ = sqy.decode(bad)
    assert rc_full != 0
    # frame 0 of the volume: its bytes lie in the first chunk(s) only
    nz = 1
    rc, part = sqy.decode_frames(bad, 0, nz)
    assert rc == 0 and np.array_equal(part, vol[:nz])
    # a range that needs the damaged frame: the full decode's code
    zl = (len(frames) - 1) * chunk // fb
    rc, part = sqy.decode_frames(bad, zl, shape[0] - zl)
    assert rc == rc_full and part is None
    rc, part = sqy.decode_frames(bad, 0, shape[0])
    assert rc == rc_full


def test_damaged_frame_inside_the_range_bitswap1(sqy):
    """bitswap1->lz4: a damaged compressed plane frame that the range needs gives SQY_Decode's code (the sink's: 11)"""
    vol = synth.stack((16, 256, 256), np.uint16)
    rc, blob = sqy.encode("bitswap1->lz4", vol, nthreads=2)
    assert rc == 0
    frames = _lz4_frames(blob, sqy)
    comp = [f for f in frames if not f[3]]
    assert comp
    bad = _damaged(blob, comp[0])
    rc_full, _ = sqy.decode(bad)
    assert rc_full == 11
    rc, _ = sqy.decode_frames(bad, 0, 16)
    assert rc == rc_full


def _set_map(blob, fn):
    """the blob with the frame_shuffle reorder_map in its header replaced by fn(map)"""
    from oracle import sqy_oracle as oracle
    blob = bytearray(blob)
    hs = oracle.header_unpack(bytes(blob))["size"]
    head = bytes(blob[:hs])
    a = head.index(b"<verbatim>") + len(b"<verbatim>")
    b = head.index(b"<\\/verbatim>")
    m = np.frombuffer(base64.b64decode(head[a:b]), dtype=np.uint64).copy()
    m = fn(m)
    enc = base64.b64encode(m.astype(np.uint64).tobytes())
    assert len(enc) == b - a
    blob[a:b] = enc
    return bytes(blob)


@pytest.mark.parametrize("dtype,shape", [(np.uint8, (12, 512, 512)), (np.uint16, (9, 256, 512))])
def test_frame_shuffle_maps_that_are_no_permutation(sqy, oracle, options, dtype, shape):
    rng = np.random.default_rng(17)
    hi = 256 if dtype == np.uint8 else 4096
    vol = (rng.integers(0, hi, shape) * (rng.random(shape) < 0.3)).astype(dtype)
    vol[2] = vol[0]                                       # equal frame metrics: the encoder's map names one place for all of them
    vol[3:5] = 0
    vol[-1] = 0
    blob = oracle.pipeline_encode("frame_shuffle->lz4", vol, nthreads=2)
    crafted = _set_map(blob, lambda m: np.concatenate([m[:1], m[:1], m[2:3], m[:1], m[4:]]))    # a place named three times
    for b in (blob, crafted):
        rc, full = sqy.decode(b)
        assert rc == 0
        assert np.array_equal(full, oracle.pipeline_decode(b))
        for subset in (1, 0):
            options("decode_frames_subset", subset)
            _check_blob(sqy, b, full, _ranges(shape[0]))


def test_bounds_arguments_and_canaries(sqy):
    import torch
    dev = torch.device("cuda", 0)
    for dtype in (np.uint16, np.uint8):
        vol = synth.stack((23, 131, 151), dtype)
        rc, blob = sqy.encode("bitswap1->lz4", vol, nthreads=2)
        assert rc == 0
        d_blob = torch.from_numpy(np.frombuffer(blob, np.uint8).copy()).to(dev)
        fb = vol[0].nbytes
        other = np.uint8 if dtype == np.uint16 else np.uint16
        pad = 4096
        for z0, nz in ((0, 1), (22, 1), (5, 7), (0, 23)):
            buf = torch.full((pad + nz * fb + pad,), 0xA5, dtype=torch.uint8, device=dev)
            rc = sqy.decode_frames_device(d_blob.data_ptr(), len(blob), z0, nz, buf.data_ptr() + pad, nz * fb, dtype)
            torch.cuda.synchronize()
            assert rc == 0
            host = buf.cpu().numpy()
            assert (host[:pad] == 0xA5).all() and (host[pad + nz * fb:] == 0xA5).all()
            assert np.array_equal(host[pad:pad + nz * fb].view(dtype).reshape((nz,) + vol.shape[1:]), vol[z0:z0 + nz])
            rc, part = sqy.decode_frames(blob, z0, nz)                # the host variant agrees
            assert rc == 0 and np.array_equal(part, vol[z0:z0 + nz])
        # refused, nothing written
        buf = torch.full((pad + 24 * fb + pad,), 0x5A, dtype=torch.uint8, device=dev)
        for z0, nz, cap, dt in ((0, 0, fb, dtype), (0, -1, fb, dtype), (-1, 1, fb, dtype), (22, 2, 2 * fb, dtype), (23, 1, fb, dtype),
                                (3, 2, 2 * fb - 1, dtype), (0, 1, fb, other)):
            rc = sqy.decode_frames_device(d_blob.data_ptr(), len(blob), z0, nz, buf.data_ptr() + pad, cap, dt)
            torch.cuda.synchronize()
            assert rc == 1, (z0, nz, cap, dt)
        assert (buf.cpu().numpy() == 0x5A).all()
        L = sqy.lib()
        sfx = "UI16" if dtype == np.uint16 else "UI8"
        osfx = "UI8" if dtype == np.uint16 else "UI16"
        host = np.full(2 * fb, 0x5A, np.uint8)
        src = np.frombuffer(blob, np.uint8)
        assert getattr(L, "SQYAMD_Decode_Frames_" + sfx)(src.ctypes.data, len(blob), 22, 2, host.ctypes.data, 2 * fb) == 1
        assert getattr(L, "SQYAMD_Decode_Frames_" + sfx)(src.ctypes.data, len(blob), 0, 2, host.ctypes.data, 2 * fb - 1) == 1
        assert getattr(L, "SQYAMD_Decode_Frames_" + osfx)(src.ctypes.data, len(blob), 0, 1, host.ctypes.data, 2 * fb) == 1
        assert (host == 0x5A).all()


def test_work_queued_on_the_callers_stream_is_respected(sqy):
    """the blob is written by a copy queued on the caller's stream just before the call, and a fill of the destination as well"""
    import torch
    dev = torch.device("cuda", 0)
    vol = synth.stack((64, 256, 512), np.uint16)
    rc, blob = sqy.encode("bitswap1->lz4", vol, nthreads=2)
    assert rc == 0
    fb = vol[0].nbytes
    host_blob = torch.from_numpy(np.frombuffer(blob, np.uint8).copy()).pin_memory()
    s = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(s):
        d_blob = torch.empty(len(blob), dtype=torch.uint8, device=dev)
        out = torch.empty(8 * fb, dtype=torch.uint8, device=dev)
        for _ in range(2):
            d_blob.zero_()
            out.fill_(7)
            d_blob.copy_(host_blob, non_blocking=True)
            rc = sqy.decode_frames_device(d_blob.data_ptr(), len(blob), 30, 8, out.data_ptr(), 8 * fb, np.uint16, stream=s.cuda_stream)
            assert rc == 0
            got = out.cpu().numpy().view(np.uint16).reshape((8,) + vol.shape[1:])
            assert np.array_equal(got, vol[30:38])


def test_several_host_threads(sqy):
    from concurrent.futures import ThreadPoolExecutor
    vols = [synth.stack((20 + i, 128, 160), np.uint16) for i in range(4)]
    blobs = []
    for v in vols:
        rc, b = sqy.encode("bitswap1->lz4", v, nthreads=2)
        assert rc == 0
        blobs.append(b)

    def one(i):
        ok = True
        for z0 in range(0, vols[i].shape[0], 3):
            nz = min(2, vols[i].shape[0] - z0)
            rc, part = sqy.decode_frames(blobs[i], z0, nz)
            ok = ok and rc == 0 and np.array_equal(part, vols[i][z0:z0 + nz])
        return ok
    with ThreadPoolExecutor(4) as ex:
        assert all(ex.map(one, range(4)))


def _fullsize(sqy, pipeline, shape, dtype, nthreads=0):
    import torch
    dev = torch.device("cuda", 0)
    vol = synth.stack_torch(shape, dtype, dev)
    cap = sqy.max_compressed_length(pipeline, shape, dtype)
    enc = torch.empty(cap, dtype=torch.uint8, device=dev)
    rc, n = sqy.encode_device(pipeline, vol.data_ptr(), shape, dtype, enc.data_ptr(), cap, nthreads=nthreads)
    assert rc == 0
    del vol
    full = torch.empty(int(np.prod(shape)) * np.dtype(dtype).itemsize, dtype=torch.uint8, device=dev)
    sfx = "UI16" if dtype == np.uint16 else "UI8"
    import ctypes
    rc = getattr(sqy.lib(), "SQYAMD_Decode_%s_Device" % sfx)(ctypes.c_void_p(enc.data_ptr()), n, ctypes.c_void_p(full.data_ptr()),
                                                             full.numel(), None)
    assert rc == 0
    fb = full.numel() // shape[0]
    Z = shape[0]
    for z0, nz in ((0, 1), (Z // 2, 1), (Z - 1, 1), (Z // 2 - 8, 16), (100, 128), (0, Z)):
        part = torch.empty(nz * fb, dtype=torch.uint8, device=dev)
        rc = sqy.decode_frames_device(enc.data_ptr(), n, z0, nz, part.data_ptr(), nz * fb, dtype)
        torch.cuda.synchronize()
        assert rc == 0, (z0, nz)
        assert torch.equal(part, full[z0 * fb:(z0 + nz) * fb]), (pipeline, z0, nz)
    del enc, full
    torch.cuda.empty_cache()


@pytest.mark.parametrize("pipeline,shape,dtype", [("bitswap1->lz4", (512, 1024, 1024), np.uint16),
                                                  ("frame_shuffle->lz4", (1024, 1024, 1024), np.uint8),
                                                  ("quantiser->bitswap1->lz4", (256, 2048, 2048), np.uint16)],
                         ids=["bench_stack", "C4", "C5_slab"])
def test_full_size(sqy, pipeline, shape, dtype):
    _fullsize(sqy, pipeline, shape, dtype)
