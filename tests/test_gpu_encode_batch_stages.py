"""SQYAMD_PipelineEncode_Batch_*: the joint path of `quantiser->bitswap1->lz4` volumes (16-bit, default weighting, the decode LUT in the
header) -- histograms, LUTs, look-up + transpose and the LZ4 kernels with one launch each per group, the LUTs built on the GPU.  The
quantiser is lossy, so nothing here asks for a round trip to the source: every blob must be byte for byte the oracle's and
SQYAMD_PipelineEncode_UI16_Device's, and decode to what the oracle's blob decodes to.  The helpers are tests/test_gpu_encode_batch.py's."""
import threading

import numpy as np
import pytest

from sqeazy_amd import synth
from test_gpu_encode_batch import CANARY, GAP, _batch, _profile, _want

pytestmark = pytest.mark.gpu

QUANT = "quantiser->bitswap1->lz4"
QUANT_KERNELS = ("batch_quantiser_histogram", "batch_quantiser_lut", "batch_quantiser_bitswap1")
ONCE = QUANT_KERNELS + ("batch_lz4_chunks", "batch_lz4_frame_scan", "batch_lz4_frame_gather")
SINGLE = ("histogram_u16", "quantiser_bitswap1_u8", "quantiser_apply", "lz4_chunks")
TABLE_BYTES = 65536 * 4 + 65536 + 512           # what a quantised volume counts against encode_batch_group_bytes besides its stream


def _volumes():
    """the batch of the byte and launch-count tests; what the level counts must be is asserted in the module fixture"""
    rng = np.random.default_rng
    return [synth.stack((3, 5, 7), np.uint16, seed=300),                            # 105 voxels, a tail of 1
            synth.stack((1, 1, 5), np.uint16, seed=301),                            # no planes at all
            synth.stack((7, 33, 31), np.uint16, seed=302),                          # 7161 voxels, at most 256 levels: linear mapping
            synth.stack((12, 64, 64), np.uint16, seed=303),                         # more than 256 levels: the Lloyd walk
            synth.stack((16, 128, 128), np.uint16, seed=304),                       # one whole 256 KiB chunk
            rng(6).integers(0, 65536, (8, 32, 32), dtype=np.uint16),                # thousands of levels
            (rng(7).integers(0, 256, (4, 32, 32)) * 257).astype(np.uint16),         # exactly 256 levels: the linear mapping's last case
            (rng(8).integers(0, 257, (4, 32, 32)) * 255).astype(np.uint16),         # exactly 257 levels: the Lloyd walk's first
            np.zeros((4, 16, 16), np.uint16),                                       # one level
            np.full((2, 8, 8), 65535, np.uint16)]                                   # the top bin occupied


@pytest.fixture(scope="module")
def vols():
    v = _volumes()
    levels = [len(np.unique(x)) for x in v]
    assert levels[2] <= 256 < levels[3] and levels[6] == 256 and levels[7] == 257 and levels[8] == 1 and levels[5] > 4000, levels
    return v


def _dev():
    import torch
    return torch.device("cuda", 0)


def _keys(n):
    return ["quant%d" % i for i in range(n)]


def _check(sqy, oracle, pipeline, vols, nthreads=0, keys=None, **kw):
    """the batch call's blobs against the oracle's and the single call's (test_gpu_encode_batch._want holds those two against each other);
    -> (blobs, the profile of the batch call alone)"""
    want = [_want(sqy, oracle, pipeline, v, nthreads, _dev(), None if keys is None else keys[i]) for i, v in enumerate(vols)]
    (rc, blobs), prof = _profile(sqy, lambda: _batch(sqy, pipeline, vols, _dev(), nthreads=nthreads, **kw))
    assert rc == 0
    for i, (v, b) in enumerate(zip(vols, blobs)):
        assert b == want[i], (pipeline, i, v.shape)
    return blobs, prof


def _launches(p, names):
    return {k: p[k][1] if k in p else 0 for k in names}


def test_bytes_and_launch_counts(sqy, oracle, vols):
    keys = _keys(len(vols))
    blobs, p = _check(sqy, oracle, QUANT, vols, keys=keys)
    assert _launches(p, ONCE) == {k: 1 for k in ONCE}, p
    assert not any(k in p for k in SINGLE), p
    # what the oracle's blob decodes to (the blobs are the oracle's, byte for byte: this holds the decoder to the same tables)
    for i, b in enumerate(blobs):
        rc, back = sqy.decode(b)
        rc2, ref = sqy.decode(_want(sqy, oracle, QUANT, vols[i], 0, _dev(), keys[i]))
        assert rc == 0 and rc2 == 0 and np.array_equal(back, ref), i


def test_unaligned_sources_and_slots(sqy, oracle, vols):
    cap = max(sqy.max_compressed_length(QUANT, v.shape, np.uint16) for v in vols) + 7
    assert cap % 16 != 0
    _, p = _check(sqy, oracle, QUANT, vols, keys=_keys(len(vols)), src_shift=2, cap=cap)
    assert _launches(p, ONCE) == {k: 1 for k in ONCE}, p


def test_several_chunks_per_volume(sqy, oracle):
    pipeline = "quantiser->bitswap1->lz4(blocksize_kb=4,framestep_kb=4)"
    small = [synth.stack((8, 32, 32), np.uint16, seed=11), synth.stack((7, 33, 31), np.uint16, seed=12)]     # 2 chunks; 1 and a short one, in mid-table
    small.append(synth.stack((5, 40, 41), np.uint16, seed=13))
    _, p = _check(sqy, oracle, pipeline, small)
    assert _launches(p, ONCE) == {k: 1 for k in ONCE}, p


def test_groups_and_the_joint_switch(sqy, oracle, options, vols):
    keys = _keys(len(vols))
    # every volume counts its stream (a byte per voxel) and TABLE_BYTES: 328297, 328197, 335353, 377344 | 590336, 336384, 332288 | 332288, ..
    cost = [v.size + TABLE_BYTES for v in vols]
    bound = 1400000
    assert sum(cost[:4]) <= bound < sum(cost[:5]) and sum(cost[4:7]) <= bound < sum(cost[4:8]) and sum(cost[7:]) <= bound
    assert sum(v.size for v in vols) < bound // 3                 # (the streams alone would make one group: the tables cut)
    options("encode_batch_group_bytes", bound)
    _, p = _check(sqy, oracle, QUANT, vols, keys=keys)
    assert _launches(p, ONCE) == {k: 3 for k in ONCE}, p
    assert not any(k in p for k in SINGLE), p
    options("encode_batch_joint", 0)
    _, p = _check(sqy, oracle, QUANT, vols, keys=keys, joint=())
    assert not any(k.startswith("batch_") for k in p), p
    assert p["histogram_u16"][1] == len(vols), p


def test_eligibility(sqy, oracle, vols, tmp_path):
    some, keys = vols[2:5], _keys(5)[2:5]
    lut = str(tmp_path / "decode.lut")
    for pipeline in ("quantiser(decode_lut_path=%s)->bitswap1->lz4" % lut, "quantiser(weighting_function=power_of_1_2)->bitswap1->lz4"):
        _, p = _check(sqy, oracle, pipeline, some, joint=())
        assert not any(k.startswith("batch_") for k in p), (pipeline, p)
        assert p["histogram_u16"][1] == len(some), p
    # nthreads = 1 and two chunks: the serial layout, one block-linked frame
    two = [synth.stack((20, 128, 128), np.uint16, seed=21)]
    _, p = _check(sqy, oracle, QUANT, two, nthreads=1, joint=())
    assert not any(k.startswith("batch_") for k in p), p
    # .. next to single-chunk volumes, which stay eligible
    _, p = _check(sqy, oracle, QUANT, two + some, nthreads=1, joint=(1, 2, 3))
    assert _launches(p, ONCE) == {k: 1 for k in ONCE} and p["histogram_u16"][1] == 1, p
    # 8-bit voxels have no quantiser: 1, zeroed tables, nothing written
    import torch
    u8 = [np.zeros((2, 3, 4), np.uint8), np.ones((1, 2, 3), np.uint8)]
    srcs = [torch.from_numpy(v).to(_dev()) for v in u8]
    buf = torch.full((2 * 4096,), CANARY, dtype=torch.uint8, device=_dev())
    rc, offs, lens = sqy.encode_batch_device(QUANT, [s.data_ptr() for s in srcs], [v.shape for v in u8], np.uint8, buf.data_ptr(), 4096)
    torch.cuda.synchronize()
    assert rc == 1 and offs == [0, 0] and lens == [0, 0] and bool((buf == CANARY).all())


def test_capacity(sqy, oracle, vols):
    """slot_capacity itself: one byte short of the largest blob the call returns 1 and every canary holds, at exactly its size 0"""
    import torch
    dev = _dev()
    want = [_want(sqy, oracle, QUANT, v, 0, dev, k) for v, k in zip(vols, _keys(len(vols)))]
    largest = max(len(w) for w in want)
    srcs = [torch.from_numpy(v.copy()).to(dev) for v in vols]
    for cap, rc_want in ((largest - 1, 1), (largest, 0)):
        buf = torch.full((2 * GAP + cap * len(vols),), CANARY, dtype=torch.uint8, device=dev)
        rc, offs, lens = sqy.encode_batch_device(QUANT, [s.data_ptr() for s in srcs], [v.shape for v in vols], np.uint16, buf.data_ptr() + GAP, cap)
        torch.cuda.synchronize()
        h = buf.cpu().numpy()
        assert rc == rc_want
        assert (h[:GAP] == CANARY).all() and (h[GAP + cap * len(vols):] == CANARY).all()
        for i, w in enumerate(want):
            slot = h[GAP + i * cap:GAP + (i + 1) * cap]
            if rc == 0:
                assert offs[i] == i * cap and lens[i] == len(w) and slot[:len(w)].tobytes() == w and (slot[len(w):] == CANARY).all(), i
            else:
                assert offs[i] == 0 and lens[i] == 0
                # a volume that fits may have been written -- inside its own slot; the one that does not fit wrote nothing
                assert (slot == CANARY).all() if len(w) > cap else (slot[len(w):] == CANARY).all(), i


def test_way_back(sqy, oracle, vols):
    """offsets and lengths of the batch encode passed straight to the batch decode: the voxels the oracle's blob decodes to"""
    import torch
    dev = _dev()
    srcs = [torch.from_numpy(v.copy()).to(dev) for v in vols]
    cap = max(sqy.max_compressed_length(QUANT, v.shape, np.uint16) for v in vols) + 13
    buf = torch.full((cap * len(vols),), CANARY, dtype=torch.uint8, device=dev)
    rc, offs, lens = sqy.encode_batch_device(QUANT, [s.data_ptr() for s in srcs], [v.shape for v in vols], np.uint16, buf.data_ptr(), cap)
    assert rc == 0
    outs = [torch.full((GAP + v.nbytes + GAP,), CANARY, dtype=torch.uint8, device=dev) for v in vols]
    rc, decoded = sqy.decode_batch_device(buf.data_ptr(), offs, lens, [o.data_ptr() + GAP for o in outs], [v.nbytes for v in vols], np.uint16)
    torch.cuda.synchronize()
    assert rc == 0 and decoded == [v.nbytes for v in vols]
    for i, (v, o) in enumerate(zip(vols, outs)):
        h = o.cpu().numpy()
        assert (h[:GAP] == CANARY).all() and (h[GAP + v.nbytes:] == CANARY).all(), i
        rc, ref = sqy.decode(_want(sqy, oracle, QUANT, v, 0, dev, "quant%d" % i))
        assert rc == 0 and h[GAP:GAP + v.nbytes].tobytes() == ref.tobytes(), i


def test_callers_stream_and_two_host_threads(sqy, oracle, vols):
    import torch
    dev = _dev()
    keys = _keys(len(vols))
    # (the helper fills sources and canaries on torch's current stream: made the caller's stream here, so the fills are ordered in front of
    # the call whatever the other thread has queued)
    s = torch.cuda.Stream(device=dev)
    for i in range(5):
        _want(sqy, oracle, QUANT, vols[i], 0, dev, keys[i])            # (the references on the default stream, cached for _check)
    with torch.cuda.stream(s):
        _check(sqy, oracle, QUANT, vols[:5], keys=keys[:5], stream=s.cuda_stream)
    sets = [[vols[0], vols[3], vols[6]], [vols[2], vols[7], vols[9]]]
    want = [[_want(sqy, oracle, QUANT, vols[i], 0, dev, keys[i]) for i in idx] for idx in ((0, 3, 6), (2, 7, 9))]
    streams = [torch.cuda.Stream(device=dev) for _ in sets]
    ok = [False, False]

    def one(t):
        good = True
        with torch.cuda.stream(streams[t]):
            for _ in range(3):
                rc, blobs = _batch(sqy, QUANT, sets[t], dev, stream=streams[t].cuda_stream)
                good = good and rc == 0 and blobs == want[t]
        ok[t] = good
    th = [threading.Thread(target=one, args=(t,)) for t in range(2)]
    for x in th:
        x.start()
    for x in th:
        x.join()
    assert all(ok)
