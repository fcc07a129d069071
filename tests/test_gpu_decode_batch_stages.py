"""SQYAMD_Decode_Batch_*: the joint inverses behind a filter stage -- `quantiser->bitswap1->lz4` (one launch of the batched inverse transposer
with the look-up per group) and the 16-bit `diff3x3x1->bitswap1->lz4`, `diff3x3x1->lz4` in the chain geometry (one launch per chain step per
group, whatever the number of blobs).  Every blob is made by the oracle (nthreads = 2), so nothing here depends on the product's encoder.
Expected everywhere: byte for byte what SQYAMD_Decode_*_Device writes for that blob alone, for the diff pipelines the source volume, the 64
canary bytes around every destination intact, decoded_bytes right.  The helpers are tests/test_gpu_decode_batch.py's."""
import threading

import numpy as np
import pytest

from sqeazy_amd import synth
from test_gpu_decode_batch import CANARY, GAP, _alone, _dev, _first_compressed_frame, _pack, _profiled

pytestmark = pytest.mark.gpu

DIFF_PLANES, DIFF_PLAIN, QUANT = "diff3x3x1->bitswap1->lz4", "diff3x3x1->lz4", "quantiser->bitswap1->lz4"
# the chain geometry (K = 8 frames per chain step, strips of 32 rows, w chain columns of X)
CHAIN_SHAPES = ((1, 8, 8),              # one frame: nothing for the chain
                (2, 4, 8),              # hx = 0
                (3, 3, 8),              # one touched row
                (9, 5, 16),             # exactly K chain frames
                (10, 33, 16),           # K + 1 frames, w = X, a strip boundary at row 32
                (10, 70, 24),           # three strips, the last one partial, w < X
                (18, 32, 64),           # three chain steps
                (17, 64, 24),
                (16, 128, 128))
COUNT_SHAPES = ((9, 5, 16), (18, 32, 64), (16, 128, 128))
QUANT_SHAPES = ((3, 5, 7), (12, 64, 64), (7, 33, 31), (16, 128, 128))         # (3, 5, 7): 105 voxels, the tail
SINGLE_DIFF = ("diff3x3x1_decode", "bitswap1_decode", "lz4_frames_decode")
SINGLE_QUANT = ("bitswap1_quantiser_decode", "quantiser_decode")

_cache = {}


def _blob(oracle, pipeline, key, make, nthreads=2):
    """(volume, oracle blob) of `make()`, made once per session"""
    k = (pipeline, key, nthreads)
    if k not in _cache:
        vol = make()
        _cache[k] = (vol, oracle.pipeline_encode(pipeline, vol, nthreads=nthreads))
    return _cache[k]


def _chain_set(oracle, pipeline, shapes=CHAIN_SHAPES):
    """every shape twice: full-range random values (the residuals wrap) and a synth.stack volume"""
    out = []
    for i, s in enumerate(shapes):
        out.append(_blob(oracle, pipeline, ("rnd", s), lambda: np.random.default_rng(900 + i).integers(0, 65536, s, dtype=np.uint16)))
        out.append(_blob(oracle, pipeline, ("stack", s), lambda: synth.stack(s, np.uint16, seed=700 + i)))
    return out


class Dsts:
    """test_gpu_decode_batch.Dsts with a shift of its own for every destination"""

    def __init__(self, nbytes, shifts):
        import torch
        self.nbytes, self.shifts = list(nbytes), list(shifts)
        self.bufs = [torch.full((GAP + sh + nb + GAP,), CANARY, dtype=torch.uint8, device=_dev()) for nb, sh in zip(self.nbytes, self.shifts)]
        assert all(b.data_ptr() % 16 == 0 for b in self.bufs)
        self.ptrs = [b.data_ptr() + GAP + sh for b, sh in zip(self.bufs, self.shifts)]

    def read(self):
        import torch
        torch.cuda.synchronize()
        out = []
        for i, (b, nb, sh) in enumerate(zip(self.bufs, self.nbytes, self.shifts)):
            h = b.cpu().numpy()
            lo = GAP + sh
            assert (h[:lo] == CANARY).all() and (h[lo + nb:] == CANARY).all(), "written outside destination %d" % i
            out.append(h[lo:lo + nb].tobytes())
        return out


def _decode(sqy, pairs, dtype=np.uint16, shifts=None, stream=None, blobs=None):
    """one batch call on the pairs' blobs (3 bytes in front of each: the blobs are misaligned); -> buf, offs, lens, rc, decoded, bytes"""
    blobs = blobs or [b for _, b in pairs]
    nbytes = [v.nbytes for v, _ in pairs]
    buf, offs, lens = _pack(blobs)
    d = Dsts(nbytes, shifts or [0] * len(pairs))
    rc, decoded = sqy.decode_batch_device(buf.data_ptr(), offs, lens, d.ptrs, nbytes, dtype, stream=stream)
    return buf, offs, lens, rc, decoded, d.read()


def _check(sqy, pairs, res, lossless=True):
    buf, offs, lens, rc, decoded, got = res
    assert rc == 0 and decoded == [v.nbytes for v, _ in pairs]
    for i, (v, _) in enumerate(pairs):
        if lossless:
            assert got[i] == v.tobytes(), "blob %d differs from its source" % i
        rc1, alone = _alone(sqy, buf, offs[i], lens[i], v.nbytes, v.dtype)
        assert rc1 == 0 and got[i] == alone, "blob %d differs from the single call" % i


@pytest.mark.parametrize("pipeline", [DIFF_PLANES, DIFF_PLAIN])
def test_diff_chain_geometry_mixed_depths(sqy, oracle, pipeline):
    """nine shapes, each as random and as synthetic volume, in one batch: the copy launch and three chain steps for all eighteen blobs"""
    pairs = _chain_set(oracle, pipeline)
    res, prof = _profiled(sqy, lambda: _decode(sqy, pairs))
    _check(sqy, pairs, res)
    assert "batch_diff3x3x1_decode" in prof, prof
    assert prof["batch_diff3x3x1_decode"][1] == 1 + 3, prof                 # (18 frames: ceil(17 / 8) steps)
    assert not any(k.startswith(SINGLE_DIFF) for k in prof), prof
    assert prof["batch_lz4_decode"][1] == 1 and prof["batch_frame_index"][1] == 1, prof
    if pipeline == DIFF_PLANES:
        assert prof["batch_bitswap1_decode"][1] == 1, prof
    else:
        assert "batch_bitswap1_decode" not in prof and "batch_copy" not in prof, prof


@pytest.mark.parametrize("pipeline", [DIFF_PLANES, DIFF_PLAIN])
def test_launch_count_does_not_grow_with_the_batch(sqy, oracle, pipeline):
    three = [p for p in _chain_set(oracle, pipeline, COUNT_SHAPES)[1::2]]   # the synthetic volume of each shape
    counts = []
    for pairs in (three, three * 8):
        res, prof = _profiled(sqy, lambda: _decode(sqy, pairs))
        _check(sqy, pairs[:3], (res[0], res[1][:3], res[2][:3], res[3], res[4][:3], res[5][:3]))
        assert res[5] == [v.tobytes() for v, _ in pairs]
        assert prof["batch_lz4_decode"][1] == 1, prof
        counts.append(prof["batch_diff3x3x1_decode"][1])
    assert counts[0] == counts[1] == 1 + 3, counts


def test_diff_fallbacks_in_mid_batch(sqy, oracle):
    """blobs the joint diff inverse must leave to the stage-by-stage path, between eligible ones"""
    ok = _chain_set(oracle, DIFF_PLANES, ((9, 5, 16), (10, 70, 24), (17, 64, 24), (10, 33, 16)))[1::2]

    def stack(shape, seed, dtype=np.uint16):
        return _blob(oracle, DIFF_PLANES, ("stack", shape, np.dtype(dtype).name), lambda: synth.stack(shape, dtype, seed=seed))
    pairs = [ok[0], stack((2, 3, 8), 731),             # the `single` case
             ok[1], stack((20, 40, 16), 732),          # Z - 2 > X - 2: rows whose reach spills
             ok[2], stack((9, 32, 12), 733),           # X % 8 != 0
             ok[3], ok[1]]                             # .. and an eligible shape 2 bytes off the 16-byte grid
    res, prof = _profiled(sqy, lambda: _decode(sqy, pairs, shifts=[0] * 7 + [2]))
    _check(sqy, pairs, res)
    assert "batch_diff3x3x1_decode" in prof and "diff3x3x1_decode" in prof, prof
    assert prof["diff3x3x1_decode"][1] == 4 and prof["batch_lz4_decode"][1] == 1, prof
    # 8-bit voxels in a UI8 batch
    pairs = [stack((9, 16, 16), 734, np.uint8), stack((10, 33, 16), 735, np.uint8)]
    res, prof = _profiled(sqy, lambda: _decode(sqy, pairs, dtype=np.uint8))
    _check(sqy, pairs, res)
    assert "batch_diff3x3x1_decode" not in prof and prof["diff3x3x1_decode"][1] == 2 and prof["batch_lz4_decode"][1] == 1, prof


def _quant_set(oracle, shapes=QUANT_SHAPES, seed=760):
    return [_blob(oracle, QUANT, ("stack", s, seed + i), lambda: synth.stack(s, np.uint16, seed=seed + i)) for i, s in enumerate(shapes)]


def test_quantiser(sqy, oracle):
    """destinations alternately on the 16-byte grid and 2 bytes off it"""
    pairs = _quant_set(oracle)
    res, prof = _profiled(sqy, lambda: _decode(sqy, pairs, shifts=[0, 2, 0, 2]))
    _check(sqy, pairs, res, lossless=False)
    assert prof["batch_quantiser_decode"][1] == 1 and prof["batch_lz4_decode"][1] == 1, prof
    assert not any(k.startswith(SINGLE_QUANT) for k in prof), prof
    res = _decode(sqy, pairs, shifts=[2, 0, 2, 0])
    _check(sqy, pairs, res, lossless=False)


def test_quantiser_lut_from_a_file(sqy, oracle, tmp_path):
    """quantiser(decode_lut_path=...): the table is read from the file the header names, on the joint path as well"""
    lut = tmp_path / "decode.lut"
    vol = synth.stack((7, 33, 31), np.uint16, seed=770)
    pairs = [(vol, oracle.pipeline_encode("quantiser(decode_lut_path=%s)->bitswap1->lz4" % lut, vol, nthreads=2)), _quant_set(oracle)[1]]
    assert lut.exists()
    res, prof = _profiled(sqy, lambda: _decode(sqy, pairs))
    _check(sqy, pairs, res, lossless=False)
    assert prof["batch_quantiser_decode"][1] == 1 and not any(k.startswith(SINGLE_QUANT) for k in prof), prof


def test_mixed_batch(sqy, oracle):
    shape = (12, 64, 64)
    pipes = [("bitswap1->lz4", 2), ("lz4", 2), (QUANT, 2), (DIFF_PLANES, 2), (DIFF_PLAIN, 2), ("pass_through", 2),
             ("bitswap1->lz4(blocksize_kb=64,framestep_kb=64)", 1)]             # the last one: two chunks in the serial layout
    pairs = [_blob(oracle, p, ("stack", shape, 780 + i), lambda: synth.stack(shape, np.uint16, seed=780 + i), nthreads=t) for i, (p, t) in enumerate(pipes)]
    res, prof = _profiled(sqy, lambda: _decode(sqy, pairs))
    buf, offs, lens, rc, decoded, got = res
    assert rc == 0 and decoded == [v.nbytes for v, _ in pairs]
    for i, (v, _) in enumerate(pairs):
        if i != 2:
            assert got[i] == v.tobytes(), i
        rc1, alone = _alone(sqy, buf, offs[i], lens[i], v.nbytes, np.uint16)
        assert rc1 == 0 and got[i] == alone, i
    for name in ("batch_lz4_decode", "batch_bitswap1_decode", "batch_quantiser_decode", "batch_copy"):
        assert prof[name][1] == 1, (name, prof)
    assert prof["batch_diff3x3x1_decode"][1] == 1 + 2, prof                  # both diff blobs: 12 frames, two chain steps
    # the single path: the serial-layout blob (its index, its inverse transpose) and pass_through, nobody else
    assert "lz4_frame_index" in prof or "lz4_linked_decode" in prof, prof
    assert prof["bitswap1_decode"][1] == 1, prof
    assert not any(k.startswith(SINGLE_QUANT + ("diff3x3x1_decode",)) for k in prof), prof


def test_one_group_of_every_family_with_a_blob_the_ranking_refuses(sqy, oracle):
    """ONE group (one block size) with jobs in all four tables -- planes, plain, quantised, both diff forms -- and in their midst a blob in
    the serial layout (nthreads = 1): one LZ4 frame where the geometry has three chunks, so the frame ranking refuses it, the group's plan is
    made again with that member dropped, and the blob goes through the single path.  Every output: the oracle's decode of the same blob."""
    pipes = [("bitswap1->lz4", 2, (4, 16, 32)), ("lz4", 2, (5, 20, 40)), (QUANT, 2, (6, 24, 40)), (DIFF_PLANES, 2, (4, 16, 32)),
             ("bitswap1->lz4(n_chunks_of_input=3)", 1, (6, 24, 40)), (DIFF_PLAIN, 2, (5, 20, 40)), ("bitswap1->lz4(n_chunks_of_input=3)", 2, (6, 24, 40))]
    pairs = [_blob(oracle, p, ("stack", s, 820 + i), lambda: synth.stack(s, np.uint16, seed=820 + i), nthreads=t) for i, (p, t, s) in enumerate(pipes)]
    magic = bytes([0x04, 0x22, 0x4D, 0x18])
    assert pairs[4][1].count(magic) == 1 and pairs[6][1].count(magic) == 3      # the serial layout, and the same pipeline chunked
    res, prof = _profiled(sqy, lambda: _decode(sqy, pairs))
    _check(sqy, pairs, res, lossless=False)
    for i, (v, b) in enumerate(pairs):
        assert res[5][i] == np.ascontiguousarray(oracle.pipeline_decode(b)).tobytes(), "blob %d differs from the oracle's decode" % i
    for name in ("batch_frame_index", "batch_lz4_decode", "batch_bitswap1_decode", "batch_quantiser_decode", "batch_copy"):
        assert prof[name][1] == 1, (name, prof)                              # one group, one launch each
    assert prof["batch_diff3x3x1_decode"][1] == 1 + 1, prof                  # both diff blobs: at most 5 frames, one chain step
    # the single path: the refused blob (its own index and LZ4 decode, its inverse transpose), nobody else
    assert "lz4_frame_rank" in prof or "lz4_frame_index" in prof, prof
    assert "lz4_frames_decode" in prof or "lz4_linked_decode" in prof, prof
    assert prof["bitswap1_decode"][1] == 1, prof
    assert not any(k.startswith(SINGLE_QUANT + ("diff3x3x1_decode",)) for k in prof), prof


def test_groups_and_the_switch(sqy, oracle, options):
    pairs = _chain_set(oracle, DIFF_PLANES) + _quant_set(oracle)
    want = _decode(sqy, pairs)[5]
    assert want[:18] == [v.tobytes() for v, _ in pairs[:18]]
    options("decode_batch_group_bytes", 300000)
    res, prof = _profiled(sqy, lambda: _decode(sqy, pairs))
    assert res[3] == 0 and res[5] == want
    assert "batch_diff3x3x1_decode" in prof and "batch_quantiser_decode" in prof, prof
    assert prof["batch_lz4_decode"][1] >= 3 and prof["batch_lz4_decode"][1] == prof["batch_frame_index"][1], prof
    options("decode_batch_joint", 0)
    res, prof = _profiled(sqy, lambda: _decode(sqy, pairs))
    assert res[3] == 0 and res[5] == want
    assert not any(k.startswith("batch_") for k in prof), prof


@pytest.mark.parametrize("pipeline", [DIFF_PLANES, DIFF_PLAIN, QUANT])
def test_a_damaged_blob_in_mid_batch(sqy, oracle, pipeline):
    """one byte of the middle blob's first compressed frame flipped: the call returns what the single call returns for that blob, the
    other four are in place"""
    pairs = [_blob(oracle, pipeline, ("stack", (12, 64, 64), 800 + i), lambda: synth.stack((12, 64, 64), np.uint16, seed=800 + i)) for i in range(5)]
    blobs = [b for _, b in pairs]
    body, size = _first_compressed_frame(sqy, blobs[2])
    bad = bytearray(blobs[2])
    bad[body] ^= 0xff                                                       # (the first token: other literal and match lengths)
    blobs[2] = bytes(bad)
    buf, offs, lens, rc, decoded, got = _decode(sqy, pairs, blobs=blobs)
    rc_alone, alone = _alone(sqy, buf, offs[2], lens[2], pairs[2][0].nbytes, np.uint16)
    print("single call on the damaged blob:", rc_alone)
    assert rc_alone != 0
    assert rc == rc_alone and decoded == [v.nbytes for v, _ in pairs]
    for i in (0, 1, 3, 4):
        rc1, good = _alone(sqy, buf, offs[i], lens[i], pairs[i][0].nbytes, np.uint16)
        assert rc1 == 0 and got[i] == good, i
        if pipeline != QUANT:
            assert got[i] == pairs[i][0].tobytes(), i


def test_two_host_threads(sqy, oracle):
    import torch
    sets = []
    for t in range(2):
        pairs = _chain_set(oracle, (DIFF_PLANES, DIFF_PLAIN)[t], ((10, 70, 24), (18, 32, 64), (9, 5, 16)))[t::2] + _quant_set(oracle, seed=760 + 10 * t)
        sets.append((pairs, torch.cuda.Stream(device=_dev())))
    torch.cuda.synchronize()
    out = [None, None]

    def one(t):
        pairs, s = sets[t]
        out[t] = _decode(sqy, pairs, stream=s.cuda_stream)
    th = [threading.Thread(target=one, args=(t,)) for t in range(2)]
    for x in th:
        x.start()
    for x in th:
        x.join()
    for t in range(2):
        pairs = sets[t][0]
        buf, offs, lens, rc, decoded, got = out[t]
        assert rc == 0 and decoded == [v.nbytes for v, _ in pairs]
        for i, (v, _) in enumerate(pairs):
            if i < 3:
                assert got[i] == v.tobytes(), (t, i)
            rc1, alone = _alone(sqy, buf, offs[i], lens[i], v.nbytes, np.uint16)
            assert rc1 == 0 and got[i] == alone, (t, i)
