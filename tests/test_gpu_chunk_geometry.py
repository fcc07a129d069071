"""LZ4 chunk geometries against liblz4 (the oracle), blob bytes and round trips.  Most tests run 64 KiB .. 4 MiB chunks; the encoder and
decoder change behaviour with the chunk size in many places below that: table entries (position << tsh | tag, the tag 21 bits wide for
a 1 KiB chunk), piece hashes and the holes map of frames in place (1 KiB pieces), frames of linked blocks (100 KiB frames of 64 + 36 KiB
blocks), literal-only chunks shorter than LZ4_MINLENGTH (n_chunks_of_input=100000 on 1 MiB) and chunks that start at addresses that are
not 16-byte aligned (n_chunks_of_input=7).  Entry points: the host API with nthreads 2 and 1, the in-place device entry point inside a
guarded destination, and the slab call."""
import numpy as np
import pytest

from sqeazy_amd import multi, synth

pytestmark = pytest.mark.gpu

SHAPE = (32, 128, 128)                                                 # 1 MiB of 16-bit voxels
BLOCKS = [1, 2, 4, 8, 16, 32, 48, 100, 128, 512]                        # blocksize_kb = framestep_kb
CONFIGS = ["(blocksize_kb=%d,framestep_kb=%d)" % (k, k) for k in BLOCKS] + ["(n_chunks_of_input=1000)", "(n_chunks_of_input=100000)"]
IDS = ["bs%dk" % k for k in BLOCKS] + ["n1000", "n100000"]


def _volumes():
    rng = np.random.default_rng(71)
    yield "stack", synth.stack(SHAPE, np.uint16)
    yield "noise", rng.integers(0, 65536, SHAPE, dtype=np.uint16)
    yield "zeros", np.zeros(SHAPE, np.uint16)
    # duplicate chunks and all-zero 1 KiB pieces of the plane stream (as test_gpu_inplace.py's holes cases)
    dup = rng.integers(0, 256, SHAPE).astype(np.uint16)
    dup.reshape(-1, 2048)[1::3] = 0
    dup[16:] = dup[:16]
    yield "dup_holes", dup


VOLUMES = dict(_volumes())


def _guarded(n, fill=0x5A, pad=4096):
    import torch
    return torch.full((pad + n + pad,), fill, dtype=torch.uint8, device=torch.device("cuda", 0)), pad


def _check_host(sqy, oracle, pipe, vol):
    for nthreads in (2, 1):
        want = oracle.pipeline_encode(pipe, vol, nthreads=nthreads)
        rc, blob = sqy.encode(pipe, vol, nthreads=nthreads)
        assert rc == 0 and blob == want, (pipe, nthreads, "host API blob differs from the oracle's")
        rc, back = sqy.decode(blob)
        assert rc == 0 and back.dtype == vol.dtype and np.array_equal(back.reshape(vol.shape), vol), (pipe, nthreads, "round trip")


def _check_device_at(sqy, oracle, pipe, vol):
    """the in-place entry point inside a 0x5A-filled destination: the blob equals the oracle's, nothing outside [d_dst, d_dst + cap)
    is written"""
    import torch
    want = oracle.pipeline_encode(pipe, vol, nthreads=2)
    cap = sqy.max_compressed_length(pipe, vol.shape, vol.dtype)
    buf, pad = _guarded(cap)
    d_vol = torch.from_numpy(vol.copy()).to(buf.device)
    rc, off, n = sqy.encode_device_at(pipe, d_vol.data_ptr(), vol.shape, vol.dtype, buf.data_ptr() + pad, cap, nthreads=2)
    assert rc == 0 and 0 <= off and off + n <= cap
    h = buf.cpu().numpy()
    assert (h[:pad] == 0x5A).all() and (h[pad + cap:] == 0x5A).all(), (pipe, "bytes outside the destination were written")
    assert h[pad + off:pad + off + n].tobytes() == want, (pipe, off, "in-place blob differs from the oracle's")
    return off


@pytest.mark.parametrize("cfg", CONFIGS, ids=IDS)
@pytest.mark.parametrize("data", list(VOLUMES), ids=list(VOLUMES))
def test_u16_bitswap1_lz4(sqy, oracle, cfg, data):
    vol = VOLUMES[data]
    pipe = "bitswap1->lz4" + cfg
    _check_host(sqy, oracle, pipe, vol)
    off = _check_device_at(sqy, oracle, pipe, vol)
    chunk = oracle.Lz4Config(cfg[1:-1]).bytes_per_chunk(vol.nbytes)
    if chunk >= 1024 and chunk & (chunk - 1) == 0 and chunk <= (64 << 10) and data != "zeros":
        assert off > 0, (pipe, "frames in place were not taken")             # (power-of-two chunks of 1 KiB and up, one block each)


@pytest.mark.parametrize("cfg", ["(blocksize_kb=1,framestep_kb=1)", "(blocksize_kb=48,framestep_kb=48)", "(n_chunks_of_input=100000)"],
                         ids=["bs1k", "bs48k", "n100000"])
@pytest.mark.parametrize("pipe", ["lz4", "bitswap1->lz4"])
def test_u8(sqy, oracle, cfg, pipe):
    rng = np.random.default_rng(72)
    vols = [synth.stack(SHAPE, np.uint8), rng.integers(0, 256, SHAPE, dtype=np.uint8), np.zeros(SHAPE, np.uint8)]
    for vol in vols:
        _check_host(sqy, oracle, pipe + cfg, vol)


@pytest.mark.parametrize("shape", [(3, 7, 333), (5, 97, 211)], ids=["small", "larger"])
@pytest.mark.parametrize("pipe", ["lz4", "bitswap1->lz4"])
def test_seven_chunks_not_aligned(sqy, oracle, shape, pipe):
    """n_chunks_of_input=7 on lengths whose chunks are not a multiple of 16 bytes: chunks start at misaligned addresses"""
    cfg = "(n_chunks_of_input=7)"
    rng = np.random.default_rng(73)
    vol = synth.stack(shape, np.uint16)
    vol.reshape(-1)[: vol.size // 3] = rng.integers(0, 65536, vol.size // 3, dtype=np.uint16)
    assert oracle.Lz4Config(cfg[1:-1]).bytes_per_chunk(vol.nbytes) % 16 != 0
    _check_host(sqy, oracle, pipe + cfg, vol)
    _check_device_at(sqy, oracle, pipe + cfg, vol)


@pytest.mark.parametrize("cfg", ["(blocksize_kb=4,framestep_kb=4)", "(blocksize_kb=100,framestep_kb=100)"], ids=["bs4k", "bs100k"])
def test_slabs(sqy, oracle, cfg):
    import torch
    dev = torch.device("cuda", 0)
    pipe = "bitswap1->lz4" + cfg
    vol = VOLUMES["dup_holes"].copy()
    vol[::3] = VOLUMES["stack"][::3]
    nslabs = 4
    biggest = (-(-SHAPE[0] // nslabs),) + SHAPE[1:]
    cap = (sqy.max_compressed_length(pipe, biggest, np.uint16) + 255) & ~255
    out = torch.full((cap * nslabs,), 0x5A, dtype=torch.uint8, device=dev)
    d_vol = torch.from_numpy(vol).to(dev)
    rc, offs, lens = sqy.encode_slabs_device(pipe, d_vol.data_ptr(), SHAPE, np.uint16, nslabs, out.data_ptr(), cap)
    assert rc == 0
    for i in range(nslabs):
        z0, nz = multi.slab_range(SHAPE[0], i, nslabs)
        assert i * cap <= offs[i] and offs[i] + lens[i] <= (i + 1) * cap
        blob = bytes(out[offs[i]:offs[i] + lens[i]].cpu().numpy().tobytes())
        assert blob == oracle.pipeline_encode(pipe, vol[z0:z0 + nz], nthreads=2), (pipe, i)
        rc, back = sqy.decode(blob)
        assert rc == 0 and np.array_equal(back, vol[z0:z0 + nz])
