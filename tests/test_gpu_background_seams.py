"""GPU: rmbkrd_neighbor5x5x5 and rmestbkrd at the seams of their own kernels, on the constructed inputs of tests/bkrd_seam_cases.py
(tests/test_background_host.py holds the constructions to what they claim, without a GPU).
  * bkrd_neighbor5_kernel: 64 x 16 columns walked in chunks of 64 frames.  Planted voxels at every seam, the expectation from the DIRECT
    count (125 offsets one by one), not from the box sums the kernel and bkrd_restate.neighbor5_counts share; chunk ends where z_end is Z
    or X - 2 and the last centres' neighbours run past the volume's end -- not counted, the product's own rule: there the
    reference reads out of bounds and says nothing.
  * bkrd_face_histo_kernel / bkrd_support_kernel: faces that leave the 16384-bin window, a face of more than 32768 voxels, the 0.99
    crossing at the bins where the support walk changes threads.  Expectations from np.bincount (bkrd_restate.face_histograms / support).
Everything goes through _check of test_gpu_background.py: the blob byte for byte, and its decode."""
import numpy as np
import pytest

import bkrd_restate as R
import bkrd_seam_cases as S
from ref_stage_inputs import stage_input
from test_gpu_background import _check

pytestmark = pytest.mark.gpu

HEADER_END = b"|01307#!"
TAILS = ("", "->bitswap1->lz4")
_direct = {}                                                # (shape, seed, fraction) -> (want, n) as uint16, shared by both voxel types


def _nb(t, f):
    return "rmbkrd_neighbor5x5x5(threshold=%d,fraction=%r)" % (t, f)


def _payload(blob, dtype, shape):
    return np.frombuffer(blob[blob.index(HEADER_END) + len(HEADER_END):], dtype).reshape(shape)


def _shifted(sqy, oracle, pipeline, vol, l2=None, shift=2):
    """the device entry point with the source `shift` bytes behind a 16-byte boundary: the same blob"""
    import torch
    dev = torch.device("cuda", 0)
    raw = torch.zeros(vol.nbytes + 32, dtype=torch.uint8, device=dev)
    assert raw.data_ptr() % 16 == 0
    raw[shift:shift + vol.nbytes] = torch.from_numpy(np.frombuffer(vol.tobytes(), dtype=np.uint8).copy()).to(dev)
    cap = sqy.max_compressed_length(pipeline, vol.shape, vol.dtype)
    out = torch.empty(cap, dtype=torch.uint8, device=dev)
    rc, n = sqy.encode_device(pipeline, raw.data_ptr() + shift, vol.shape, vol.dtype, out.data_ptr(), cap, nthreads=2)
    assert rc == 0, pipeline
    got = bytes(out[:n].cpu().numpy().tobytes())
    l2 = sqy.get_option("host_l2_bytes") if l2 is None else l2
    assert got == R.expected_blob(oracle, pipeline, vol, l2), (pipeline, vol.shape, vol.dtype, shift)


# ---- rmbkrd_neighbor5x5x5 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.uint16, np.uint8])
@pytest.mark.parametrize("shape,seeds", S.PLANTED)
def test_neighbor5_planted_at_every_seam(sqy, oracle, shape, seeds, dtype):
    """cut 0: a centre is zeroed exactly when a planted voxel is among its 125 neighbours; cut 1.0044: when two are.  A count that is not
    carried across a seam shows as a kept voxel: the first one is named as (z, y, x, got, want, n)"""
    seen = {f: set() for f in S.PLANTED_FRACTIONS}
    for seed in seeds:
        vol = stage_input("planted", dtype, shape, seed)
        for f in S.PLANTED_FRACTIONS:
            key = (shape, seed, f)
            if key not in _direct:
                _direct[key] = S.neighbor5_direct(vol.astype(np.uint16), S.PLANTED_THRESHOLD, f) + (S.seam_outcomes(vol, seed, f),)
            want, n, outcomes = _direct[key]
            seen[f] |= outcomes
            pipeline = _nb(S.PLANTED_THRESHOLD, f)
            rc, blob = sqy.encode(pipeline, vol, nthreads=2)
            assert rc == 0, (pipeline, seed)
            diff = S.first_difference(_payload(blob, dtype, shape), want.astype(dtype), n)
            assert diff is None, "seed %d, fraction %r: first differing voxel (z, y, x, got, want, n) = %r" % (seed, f, diff)
            for tail in TAILS:
                _check(sqy, oracle, pipeline + tail, vol)
    for f in S.PLANTED_FRACTIONS:                           # both outcomes on both sides of every seam
        assert seen[f] >= S.seam_outcomes_wanted(shape), (f, sorted(S.seam_outcomes_wanted(shape) - seen[f]))


@pytest.mark.parametrize("dtype", [np.uint16, np.uint8])
@pytest.mark.parametrize("shape", [(72, 6, 70), (70, 20, 68), (129, 18, 70), (136, 18, 134)])
def test_neighbor5_low80_across_the_seams(sqy, oracle, shape, dtype):
    """dense data on both sides of the cut in every chunk (threshold 40, fraction 0.5 on the largest shape: thousands of centres each way),
    against the direct count and through _check"""
    vol = stage_input("low80", dtype, shape, sum(shape))
    for t, f in ((40, 0.5), (18, 0.25)):
        want, n = S.neighbor5_direct(vol, t, f)
        rc, blob = sqy.encode(_nb(t, f), vol, nthreads=2)
        assert rc == 0
        diff = S.first_difference(_payload(blob, dtype, shape), want, n)
        assert diff is None, "threshold %d, fraction %r: first differing voxel (z, y, x, got, want, n) = %r" % (t, f, diff)
        for tail in TAILS:
            _check(sqy, oracle, _nb(t, f) + tail, vol)


@pytest.mark.parametrize("dtype", [np.uint16, np.uint8])
@pytest.mark.parametrize("shape", S.CHUNK_END_SHAPES)
def test_neighbor5_chunk_ends(sqy, oracle, shape, dtype):
    """z_end = Z or X - 2 inside or at the start of the last chunk: 0 to 4 planes of centres there, neighbours past the end not counted"""
    vol = S.chunk_end_volume(shape, dtype)
    for t, f in S.CHUNK_END_CONFIGS:
        want, n = S.neighbor5_direct(vol, t, f)
        rc, blob = sqy.encode(_nb(t, f), vol, nthreads=2)
        assert rc == 0
        diff = S.first_difference(_payload(blob, dtype, shape), want, n)
        assert diff is None, "threshold %d, fraction %r: first differing voxel (z, y, x, got, want, n) = %r" % (t, f, diff)
        for tail in TAILS:
            _check(sqy, oracle, _nb(t, f) + tail, vol)
    _shifted(sqy, oracle, _nb(*S.CHUNK_END_CONFIGS[0]) + TAILS[1], vol)


def test_neighbor5_planted_from_a_shifted_source(sqy, oracle):
    for shape, seeds in S.PLANTED:
        for dtype in (np.uint16, np.uint8):
            _shifted(sqy, oracle, _nb(S.PLANTED_THRESHOLD, 0.0), stage_input("planted", dtype, shape, seeds[0]))


# ---- rmestbkrd --------------------------------------------------------------------------------------------------------------------------------
RM_PIPELINES = ("rmestbkrd", "rmestbkrd->bitswap1->lz4")     # between them the scalar and the 16-byte subtract


def _rmest(sqy, oracle, vol, l2):
    for pipeline in RM_PIPELINES:
        _check(sqy, oracle, pipeline, vol, l2)


@pytest.mark.parametrize("dtype", [np.uint16, np.uint8])
def test_rmestbkrd_faces_outside_the_window(sqy, oracle, options, dtype):
    """segments that start at 8192, 8193, 40000, 57343, 57344 and 65535 and hold values more than 8192 away on both sides (16-bit; 8-bit
    has all its bins in the window)"""
    options("host_l2_bytes", S.L2_ALL)
    vol = S.spread_volume(S.WINDOW_SHAPE, dtype)
    _rmest(sqy, oracle, vol, S.L2_ALL)
    _shifted(sqy, oracle, RM_PIPELINES[1], vol, S.L2_ALL)
    _shifted(sqy, oracle, RM_PIPELINES[0], vol, S.L2_ALL)


@pytest.mark.parametrize("dtype", [np.uint16, np.uint8])
def test_rmestbkrd_second_pass_over_a_face(sqy, oracle, options, dtype):
    """a z face of 33800 voxels, and face portions of 32768 (the second pass just not taken) and 32769 (by one voxel)"""
    options("host_l2_bytes", S.L2_ALL)
    _rmest(sqy, oracle, S.spread_volume(S.STRIDE_SHAPE, dtype, 5101), S.L2_ALL)
    vol = S.spread_volume(S.PORTION_SHAPE, dtype)
    _rmest(sqy, oracle, vol, S.L2_ALL)
    for portion, l2 in S.PORTION_L2.items():
        assert R.face_portion(vol.shape[1] * vol.shape[2], l2) == portion
        options("host_l2_bytes", l2)
        _rmest(sqy, oracle, vol, l2)


@pytest.mark.parametrize("dtype", [np.uint16, np.uint8])
def test_rmestbkrd_support_walk_at_thread_boundaries(sqy, oracle, options, dtype):
    """the 0.99 crossing one voxel on either side of (double)0.99f, at bins 0, 1, 255, 256, 257, 16384, 65535 (8-bit: 0, 1, 128, 255)"""
    options("host_l2_bytes", S.L2_ALL)
    for lo, hi, k in S.support_cases(dtype):
        vol = S.support_volume(dtype, lo, hi, k)
        t = R.rmestbkrd_threshold(vol, S.L2_ALL)
        assert t == S.support_threshold(lo, hi, k), (lo, hi, k, t)                # the case is the one it means to be
        rc, blob = sqy.encode("rmestbkrd", vol, nthreads=2)
        assert rc == 0
        got = _payload(blob, dtype, vol.shape)
        assert np.array_equal(got, R.rmestbkrd(vol, S.L2_ALL)), "values %d / %d, %d of 1000 at the upper: threshold %d, the payload implies %r" % (
            lo, hi, k, t, sorted({int(a) - int(b) for a, b in zip(vol.reshape(-1), got.reshape(-1)) if b})[:4])
        _rmest(sqy, oracle, vol, S.L2_ALL)
