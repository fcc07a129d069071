"""SQYAMD_PipelineEncode_Batch_*: a set of separately allocated volumes -- shapes may differ -- becomes one blob each with one call.  Every blob
must be byte for byte the oracle's and SQYAMD_PipelineEncode_*_Device's for that volume, decode back to the source, and lie inside its own slot
of the destination (canary bytes around every slot hold), whichever way the volumes are grouped, on the joint path or without it."""
import threading

import numpy as np
import pytest

from sqeazy_amd import synth

pytestmark = pytest.mark.gpu

CANARY = 0xA5
GAP = 64                      # canary bytes in front of the first slot and behind the last

MIXED_SHAPES = ((16, 64, 128),        # exactly one 256 KiB chunk
                (20, 64, 128),        # two chunks, the short last one in mid-table
                (3, 5, 7),            # 105 voxels: a transposer tail
                (1, 1, 5),            # 10 bytes, below LZ4's minimum length
                (32, 64, 128))        # two whole chunks
BATCH_KERNELS = ("batch_bitswap1", "batch_lz4_chunks", "batch_lz4_chunks_dense", "batch_lz4_frame_scan", "batch_lz4_frame_gather")
SINGLE_KERNELS = ("bitswap1_u16", "bitswap1_u8", "lz4_chunks", "lz4_chunks_dense", "lz4_frame_scan", "lz4_frame_gather", "lz4_inplace_tail", "lz4_dedupe")


@pytest.fixture(scope="module")
def mixed():
    return [synth.stack(s, np.uint16, seed=300 + i) for i, s in enumerate(MIXED_SHAPES)]


_want_cache = {}


def _want(sqy, oracle, pipeline, vol, nthreads, dev, key=None):
    """the blob both references give for one volume (they must agree): the oracle's and SQYAMD_PipelineEncode_*_Device's"""
    import torch
    k = (pipeline, nthreads, key) if key is not None else None
    if k in _want_cache:
        return _want_cache[k]
    want = oracle.pipeline_encode(pipeline, vol, nthreads if nthreads > 0 else 2)
    d_vol = torch.from_numpy(vol.copy()).to(dev)
    cap = sqy.max_compressed_length(pipeline, vol.shape, vol.dtype) + 64
    out = torch.empty(cap, dtype=torch.uint8, device=dev)
    rc, n = sqy.encode_device(pipeline, d_vol.data_ptr(), vol.shape, vol.dtype, out.data_ptr(), cap, nthreads=nthreads)
    assert rc == 0
    assert bytes(out[:n].cpu().numpy().tobytes()) == want, "the single call differs from the oracle"
    if k is not None:
        _want_cache[k] = want
    return want


def _batch(sqy, pipeline, vols, dev, nthreads=0, cap=None, src_shift=0, stream=None, joint=None):
    """the batch call on device copies of vols (each src_shift bytes behind a 16-byte boundary) into slots of cap bytes filled with canaries,
    canaries in front of the first and behind the last; returns (rc, blobs or None).  The canaries around the slots must hold whatever rc
    is, and so must the rest of the slot of every volume in `joint` (None: all) -- the joint path writes the blob and nothing else; a
    volume that takes the single-call path may use its whole slot, the blob lies where offsets[i] says"""
    import torch
    dtype = vols[0].dtype
    srcs = []
    for v in vols:
        raw = torch.empty(v.nbytes + 32, dtype=torch.uint8, device=dev)
        assert raw.data_ptr() % 16 == 0
        raw[src_shift:src_shift + v.nbytes] = torch.from_numpy(np.frombuffer(v.tobytes(), dtype=np.uint8).copy()).to(dev)
        srcs.append(raw)
    if cap is None:
        cap = max(sqy.max_compressed_length(pipeline, v.shape, dtype) for v in vols) + 13          # (no multiple of 16)
    slot = cap
    buf = torch.full((2 * GAP + slot * len(vols),), CANARY, dtype=torch.uint8, device=dev)
    torch.cuda.current_stream(dev).synchronize()         # the sources and the fill are torch's stream's: the caller's to complete (sqeazy_amd.h)
    rc, offs, lens = sqy.encode_batch_device(pipeline, [r.data_ptr() + src_shift for r in srcs], [v.shape for v in vols], dtype, buf.data_ptr() + GAP, slot,
                                             nthreads=nthreads, stream=stream)
    torch.cuda.synchronize()
    h = buf.cpu().numpy()
    assert (h[:GAP] == CANARY).all() and (h[GAP + slot * len(vols):] == CANARY).all(), "written outside the slots"
    if rc:
        assert offs == [0] * len(vols) and lens == [0] * len(vols)
        return rc, None
    blobs = []
    for i in range(len(vols)):
        assert i * slot <= offs[i] and lens[i] > 0 and offs[i] + lens[i] <= (i + 1) * slot, (i, offs[i], lens[i])
        lo, hi = GAP + offs[i], GAP + offs[i] + lens[i]
        if joint is None or i in joint:
            assert offs[i] == i * slot and (h[hi:GAP + (i + 1) * slot] == CANARY).all(), "slot %d: written outside the blob" % i
        blobs.append(h[lo:hi].tobytes())
    return rc, blobs


def _check(sqy, oracle, pipeline, vols, dev, nthreads=0, keys=None, **kw):
    rc, blobs = _batch(sqy, pipeline, vols, dev, nthreads=nthreads, **kw)
    assert rc == 0
    for i, (v, b) in enumerate(zip(vols, blobs)):
        assert b == _want(sqy, oracle, pipeline, v, nthreads, dev, None if keys is None else keys[i]), (pipeline, i, v.shape)
        rc, back = sqy.decode(b)
        assert rc == 0 and np.array_equal(back, v), (pipeline, i)
    return blobs


def _profile(sqy, fn):
    sqy.profile_reset()
    sqy.profile_enable(True)
    try:
        out = fn()
    finally:
        sqy.profile_enable(False)
    got = sqy.profile_get()
    sqy.profile_reset()
    return out, got


def test_mixed_shapes(sqy, oracle, mixed):
    import torch
    dev = torch.device("cuda", 0)
    keys = ["mixed%d" % i for i in range(len(mixed))]
    (_, p) = _profile(sqy, lambda: _check(sqy, oracle, "bitswap1->lz4", mixed, dev, keys=keys))
    assert p["batch_lz4_chunks"][1] == 1 and p["batch_bitswap1"][1] == 1 and p["batch_lz4_frame_gather"][1] == 1, p
    _check(sqy, oracle, "bitswap1->lz4", mixed[:1], dev, keys=keys[:1])


@pytest.mark.parametrize("dtype", [np.uint16, np.uint8])
@pytest.mark.parametrize("pipeline", ["bitswap1->lz4(blocksize_kb=4,framestep_kb=4)", "lz4(n_chunks_of_input=7)"])
def test_small_chunks(sqy, oracle, pipeline, dtype):
    import torch
    dev = torch.device("cuda", 0)
    vols = [synth.stack((8, 32, 32), dtype, seed=11), synth.stack((7, 33, 31), dtype, seed=12)]
    (_, p) = _profile(sqy, lambda: _check(sqy, oracle, pipeline, vols, dev))
    assert p["batch_lz4_chunks"][1] == 1, p


def test_stored_and_compressed_side_by_side(sqy, oracle):
    import torch
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(3)
    vols = [rng.integers(0, 65536, (9, 64, 64), dtype=np.uint16), np.zeros((10, 64, 64), np.uint16), synth.stack((12, 64, 64), np.uint16, seed=5)]
    for pipeline in ("bitswap1->lz4", "lz4"):
        _check(sqy, oracle, pipeline, vols, dev)


def _short_match_run(block):
    """the longest run of matches shorter than 16 bytes in a row in one LZ4 block"""
    i, run, best = 0, 0, 0
    while i < len(block):
        tok = block[i]; i += 1
        lit = tok >> 4
        if lit == 15:
            while True:
                b = block[i]; i += 1; lit += b
                if b != 255:
                    break
        i += lit
        if i >= len(block):
            break
        i += 2
        ml = (tok & 15) + 4
        if (tok & 15) == 15:
            while True:
                b = block[i]; i += 1; ml += b
                if b != 255:
                    break
        run = run + 1 if ml < 16 else 0
        best = max(best, run)
    return best


def test_dense_pass(sqy, oracle):
    """0 / 1 bytes (the generator of test_gpu_linked's given-up blocks): a short match every few bytes sends the chunks to the dense pass"""
    import torch
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(77)
    dense = rng.integers(0, 2, (1, 3, 100000), dtype=np.uint8)           # two chunks, the second short
    assert _short_match_run(oracle.lz4_block_compress(dense.reshape(-1)[:65536].tobytes())) >= 128
    vols = [synth.stack((4, 64, 64), np.uint8, seed=8), dense, synth.stack((3, 50, 70), np.uint8, seed=9)]
    (_, p) = _profile(sqy, lambda: _check(sqy, oracle, "lz4", vols, dev))
    assert p["batch_lz4_chunks_dense"][1] == 1, p


def test_unaligned_sources_and_slots(sqy, oracle, mixed):
    import torch
    dev = torch.device("cuda", 0)
    keys = ["mixed%d" % i for i in range(len(mixed))]
    for pipeline in ("bitswap1->lz4", "lz4"):
        cap = max(sqy.max_compressed_length(pipeline, v.shape, np.uint16) for v in mixed) + 7
        assert cap % 16 != 0
        _check(sqy, oracle, pipeline, mixed, dev, keys=keys, src_shift=2, cap=cap)
    u8 = [synth.stack(s, np.uint8, seed=40 + i) for i, s in enumerate(((5, 40, 41), (3, 5, 7), (16, 128, 128)))]
    _check(sqy, oracle, "bitswap1->lz4", u8, dev, src_shift=3)


def test_several_groups_and_the_joint_switch(sqy, oracle, options, mixed):
    import torch
    dev = torch.device("cuda", 0)
    keys = ["mixed%d" % i for i in range(len(mixed))]
    # LZ4 input: 256 KiB, 320 KiB, 210 B, 10 B, 512 KiB -- at 400000 bytes a group: {0} | {1, 2, 3} | {4}
    options("encode_batch_group_bytes", 400000)
    (_, p) = _profile(sqy, lambda: _check(sqy, oracle, "bitswap1->lz4", mixed, dev, keys=keys))
    assert p["batch_lz4_chunks"][1] == 3 and p["batch_bitswap1"][1] == 3 and p["batch_lz4_frame_scan"][1] == 3 and p["batch_lz4_frame_gather"][1] == 3, p
    assert not any(k in p for k in SINGLE_KERNELS), p
    options("encode_batch_joint", 0)
    (_, p) = _profile(sqy, lambda: _check(sqy, oracle, "bitswap1->lz4", mixed, dev, keys=keys, joint=()))
    assert not any(k in p for k in BATCH_KERNELS), p
    assert p["lz4_chunks"][1] == len(mixed), p


def test_mixed_eligibility(sqy, oracle, mixed):
    import torch
    dev = torch.device("cuda", 0)
    # nthreads = 1: the volumes of more than one chunk take the serial layout, one block-linked frame -- not eligible
    (_, p) = _profile(sqy, lambda: _check(sqy, oracle, "bitswap1->lz4", mixed, dev, nthreads=1, joint=(0, 2, 3)))
    assert p["batch_lz4_chunks"][1] == 1, p
    (_, p) = _profile(sqy, lambda: _check(sqy, oracle, "diff3x3x1->bitswap1->lz4", [mixed[0], mixed[1], mixed[4]], dev, joint=()))
    assert not any(k in p for k in BATCH_KERNELS), p


def test_capacity(sqy, oracle, mixed):
    """slot_capacity itself: one byte short of the largest blob the call returns 1 and every canary holds, at exactly its size 0"""
    import torch
    dev = torch.device("cuda", 0)
    pipeline = "bitswap1->lz4"
    want = [_want(sqy, oracle, pipeline, v, 0, dev, "mixed%d" % i) for i, v in enumerate(mixed)]
    largest = max(len(w) for w in want)
    srcs = [torch.from_numpy(v.copy()).to(dev) for v in mixed]
    for cap, rc_want in ((largest - 1, 1), (largest, 0)):
        buf = torch.full((2 * GAP + cap * len(mixed),), CANARY, dtype=torch.uint8, device=dev)
        rc, offs, lens = sqy.encode_batch_device(pipeline, [s.data_ptr() for s in srcs], [v.shape for v in mixed], np.uint16, buf.data_ptr() + GAP, cap)
        torch.cuda.synchronize()
        h = buf.cpu().numpy()
        assert rc == rc_want
        assert (h[:GAP] == CANARY).all() and (h[GAP + cap * len(mixed):] == CANARY).all()
        for i, w in enumerate(want):
            slot = h[GAP + i * cap:GAP + (i + 1) * cap]
            if rc == 0:
                assert offs[i] == i * cap and lens[i] == len(w) and slot[:len(w)].tobytes() == w and (slot[len(w):] == CANARY).all(), i
            else:
                assert offs[i] == 0 and lens[i] == 0
                # a volume that fits may have been written -- inside its own slot; the one that does not fit wrote nothing
                assert (slot == CANARY).all() if len(w) > cap else (slot[len(w):] == CANARY).all(), i


def test_two_host_threads(sqy, oracle, mixed):
    import torch
    dev = torch.device("cuda", 0)
    sets = [mixed[:3], [synth.stack((9, 64, 64), np.uint16, seed=70), synth.stack((2, 31, 17), np.uint16, seed=71), mixed[4]]]
    want = [[_want(sqy, oracle, "bitswap1->lz4", v, 0, dev) for v in s] for s in sets]
    streams = [torch.cuda.Stream(device=dev) for _ in sets]
    ok = [False, False]

    def one(t):
        good = True
        for _ in range(3):
            rc, blobs = _batch(sqy, "bitswap1->lz4", sets[t], dev, stream=streams[t].cuda_stream)
            good = good and rc == 0 and blobs == want[t]
        ok[t] = good
    th = [threading.Thread(target=one, args=(t,)) for t in range(2)]
    for x in th:
        x.start()
    for x in th:
        x.join()
    assert all(ok)


def test_host_pointer_variants(sqy, oracle, mixed):
    import torch
    dev = torch.device("cuda", 0)
    blobs = sqy.encode_batch("bitswap1->lz4", mixed)
    assert blobs == [_want(sqy, oracle, "bitswap1->lz4", v, 0, dev, "mixed%d" % i) for i, v in enumerate(mixed)]
    u8 = [synth.stack(s, np.uint8, seed=90 + i) for i, s in enumerate(((6, 33, 65), (1, 1, 5)))]
    assert sqy.encode_batch("lz4", u8) == [_want(sqy, oracle, "lz4", v, 0, dev) for v in u8]
