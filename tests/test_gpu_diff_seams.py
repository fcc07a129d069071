"""GPU: diff3x3x1 at the seams of the kernels it runs through today, on the cases of tests/diff_seam_cases.py (tests/test_diff_seams_host.py
holds that table to what it claims, without a GPU): the rows kernel against the generic one at Z = X, X + 1, X + 2; the side path with
blocks whose rows run past Y, idle lanes and a rewritten last side column, and its near misses; the decode chain with 1 .. 8 frames in its
last launch, strips of one row, the second item slot, the widest image that fits and the first that does not; wide and narrow chains in
one batch launch.  Which kernel a call takes is restated in diff_seam_cases.py, not observed -- except for the batch calls, whose launch
counts the profile shows.
Expected everywhere: `diff3x3x1->lz4` and `diff3x3x1->bitswap1->lz4` encode to the oracle's blob byte for byte, and the oracle's blob decodes
to the volume, twice in a row.  A failure names the case, its branch and the first differing voxel."""
import ctypes

import numpy as np
import pytest

import diff_seam_cases as D
from test_gpu_decode_batch import CANARY, GAP, _dev, _profiled
from test_gpu_decode_batch_stages import _check, _decode

pytestmark = pytest.mark.gpu

PIPELINES = ("diff3x3x1->lz4", "diff3x3x1->bitswap1->lz4")
_want = {}


def _blob(oracle, case, pipeline):
    """the oracle's blob of a case, made once"""
    k = (case["name"], pipeline)
    if k not in _want:
        _want[k] = oracle.pipeline_encode(pipeline, D.volume(case), nthreads=2)
    return _want[k]


def _encode_failure(oracle, case, pipeline, got):
    """what to say about a blob that is not the oracle's: the first voxel the oracle's decode of it gets wrong is the first one the stage
    got wrong (every voxel in front of it decodes from right residuals)"""
    try:
        diff = D.first_difference(oracle.pipeline_decode(got), D.volume(case))
    except Exception as e:                                                      # noqa: BLE001 (whatever the oracle makes of a broken blob)
        diff = "the oracle cannot decode the blob: %s" % type(e).__name__
    return D.failure(case, "%s: blob of %d bytes differs from the oracle's of %d" % (pipeline, len(got), len(_blob(oracle, case, pipeline))), diff)


@pytest.mark.parametrize("case", D.CASES, ids=D.case_id)
def test_encode_is_the_oracles_blob(sqy, oracle, case):
    vol = D.volume(case)
    for pipeline in PIPELINES:
        rc, blob = sqy.encode(pipeline, vol, nthreads=2)
        assert rc == 0, D.describe(case)
        assert blob == _blob(oracle, case, pipeline), _encode_failure(oracle, case, pipeline, blob)


@pytest.mark.parametrize("case", D.CASES, ids=D.case_id)
def test_decode_restores_the_volume_twice(sqy, oracle, case):
    vol = D.volume(case)
    for pipeline in PIPELINES:
        blob = _blob(oracle, case, pipeline)
        for turn in (1, 2):
            rc, back = sqy.decode(blob)
            assert rc == 0, D.describe(case)
            assert back.shape == vol.shape and back.dtype == vol.dtype, D.describe(case)
            diff = D.first_difference(back, vol)
            assert diff is None, D.failure(case, "%s, decode %d" % (pipeline, turn), diff)


def _encode_device(sqy, pipeline, vol, shift):
    """encode_device from a source `shift` bytes behind a 16-byte boundary into a destination between canaries -> the blob"""
    import torch
    raw = torch.zeros(vol.nbytes + 32, dtype=torch.uint8, device=_dev())
    assert raw.data_ptr() % 16 == 0
    raw[shift:shift + vol.nbytes] = torch.from_numpy(np.frombuffer(vol.tobytes(), dtype=np.uint8).copy()).to(_dev())
    cap = sqy.max_compressed_length(pipeline, vol.shape, vol.dtype)
    out = torch.full((GAP + cap + GAP,), CANARY, dtype=torch.uint8, device=_dev())
    rc, n = sqy.encode_device(pipeline, raw.data_ptr() + shift, vol.shape, vol.dtype, out.data_ptr() + GAP, cap, nthreads=2)
    torch.cuda.synchronize()
    assert rc == 0 and 0 < n <= cap, (pipeline, vol.shape, shift, rc, n)
    h = out.cpu().numpy()
    assert (h[:GAP] == CANARY).all() and (h[GAP + cap:] == CANARY).all(), "written outside the destination: %s, %r, source %d bytes off" % (pipeline, vol.shape, shift)
    return h[GAP:GAP + n].tobytes()


@pytest.mark.parametrize("case", D.SIDE_CASES, ids=D.case_id)
def test_side_path_from_a_device_source_aligned_and_not(sqy, oracle, case):
    """2 bytes off a 16-byte boundary the driver drops the side path for the whole-volume rows kernel: the same blob"""
    vol = D.volume(case)
    for pipeline in PIPELINES:
        for shift in (0, 2):
            got = _encode_device(sqy, pipeline, vol, shift)
            assert got == _blob(oracle, case, pipeline), _encode_failure(oracle, case, "%s, source %d bytes off" % (pipeline, shift), got)


def _pairs(oracle, names, pipeline):
    return [(D.volume(D.BY_NAME[n]), _blob(oracle, D.BY_NAME[n], pipeline)) for n in names]


def _batch_voxels(names, pairs, res):
    for n, (vol, _), got in zip(names, pairs, res[5]):
        diff = D.first_difference(np.frombuffer(got, np.uint16).reshape(vol.shape), vol)
        assert diff is None, D.failure(D.BY_NAME[n], "batch decode", diff)


@pytest.mark.parametrize("pipeline", PIPELINES)
def test_batch_widest_and_narrowest_chain_in_one_launch(sqy, oracle, pipeline):
    """w = 320, 16 and 8 in one table: the launch sizes its LDS for the widest, every job computes its own pitch; 40 chain steps, of which
    the narrow jobs take part in the first two and the first"""
    pairs = _pairs(oracle, D.BATCH_JOINT, pipeline)
    res, prof = _profiled(sqy, lambda: _decode(sqy, pairs))
    assert res[3] == 0
    _batch_voxels(D.BATCH_JOINT, pairs, res)
    _check(sqy, pairs, res)
    steps = max(D.BY_NAME[n]["decode"]["launches"] for n in D.BATCH_JOINT)
    assert steps == 40 and prof["batch_diff3x3x1_decode"][1] == 1 + steps, prof
    assert "diff3x3x1_decode" not in prof, prof


@pytest.mark.parametrize("pipeline", PIPELINES)
def test_batch_keeps_a_chain_that_does_not_fit_off_the_joint_path(sqy, oracle, pipeline):
    """w = 328 next to w = 16: the wide blob takes the stage-by-stage path with its per-frame chain, the narrow one the joint launches"""
    pairs = _pairs(oracle, D.BATCH_MIXED, pipeline)
    res, prof = _profiled(sqy, lambda: _decode(sqy, pairs))
    assert res[3] == 0
    _batch_voxels(D.BATCH_MIXED, pairs, res)
    _check(sqy, pairs, res)
    assert prof["batch_diff3x3x1_decode"][1] == 1 + D.BY_NAME[D.BATCH_MIXED[1]]["decode"]["launches"], prof
    assert prof["diff3x3x1_decode"][1] == 1, prof


OFF_GRID = ("10x33x16-random", "64x5x256-random", "17x5x24-random")


@pytest.mark.parametrize("name", OFF_GRID)
def test_single_blob_into_a_destination_off_the_16_byte_grid(sqy, oracle, name):
    """SQYAMD_Decode_UI16_Device with the destination 2 bytes behind a 16-byte boundary: the chain needs aligned rows, so the inverse runs
    frame by frame through the generic kernel; the volume, and nothing outside it"""
    import torch
    case = D.BY_NAME[name]
    vol = D.volume(case)
    fn = sqy.lib().SQYAMD_Decode_UI16_Device
    for pipeline in PIPELINES:
        blob = _blob(oracle, case, pipeline)
        src = torch.from_numpy(np.frombuffer(blob, dtype=np.uint8).copy()).to(_dev())
        dst = torch.full((GAP + 2 + vol.nbytes + GAP,), CANARY, dtype=torch.uint8, device=_dev())
        assert dst.data_ptr() % 16 == 0
        rc = fn(ctypes.c_void_p(src.data_ptr()), ctypes.c_long(len(blob)), ctypes.c_void_p(dst.data_ptr() + GAP + 2), ctypes.c_long(vol.nbytes), None)
        torch.cuda.synchronize()
        assert rc == 0, D.describe(case)
        h = dst.cpu().numpy()
        lo = GAP + 2
        assert (h[:lo] == CANARY).all() and (h[lo + vol.nbytes:] == CANARY).all(), "%s: written outside the destination" % D.describe(case)
        diff = D.first_difference(np.frombuffer(h[lo:lo + vol.nbytes].tobytes(), np.uint16).reshape(vol.shape), vol)
        assert diff is None, D.failure(case, "%s, destination 2 bytes off" % pipeline, diff)
