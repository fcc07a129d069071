"""GPU: the background-removal head filters rmestbkrd and rmbkrd_neighbor5x5x5 through the C-ABI, byte for byte against the numpy
restatement (tests/bkrd_restate.py) plus the oracle for the stages behind them."""
import hashlib
import threading

import numpy as np
import pytest

import bkrd_restate as R
from sqeazy_amd import synth, multi

pytestmark = pytest.mark.gpu


def _vol(shape, dtype, lo, hi, seed):
    return np.random.default_rng(seed).integers(lo, hi, shape).astype(dtype)


def _check(sqy, oracle, pipeline, vol, l2=None, lossless=True):
    l2 = sqy.get_option("host_l2_bytes") if l2 is None else l2
    rc, blob = sqy.encode(pipeline, vol, nthreads=2)
    assert rc == 0, pipeline
    want = R.expected_blob(oracle, pipeline, vol, l2)
    assert blob == want, "%s on %r %s: %d vs %d bytes" % (pipeline, vol.shape, vol.dtype, len(blob), len(want))
    rc, back = sqy.decode(blob)
    assert rc == 0, pipeline
    if lossless and "frame_shuffle" not in pipeline:
        assert np.array_equal(back, R.filtered_volume(pipeline, vol, l2)), pipeline
    return blob


# cubes and non-cubes: X > Z, Z > X, Y = 5 / X = 6, centres whose neighbours run past the end, the wrap at x = X-2
NB_SHAPES = [(16, 16, 16), (6, 20, 40), (40, 12, 9), (10, 5, 6), (12, 10, 20), (33, 17, 70), (3, 9, 31), (64, 64, 64)]


@pytest.mark.parametrize("dtype", [np.uint16, np.uint8])
@pytest.mark.parametrize("shape", NB_SHAPES)
def test_neighbor5_parity(sqy, oracle, shape, dtype):
    vol = _vol(shape, dtype, 0, 80, sum(shape))
    for cfg in ("threshold=40,fraction=0.5", "threshold=20,fraction=0.25", "threshold=60,fraction=0.75"):
        _check(sqy, oracle, "rmbkrd_neighbor5x5x5(%s)->bitswap1->lz4" % cfg, vol)
    _check(sqy, oracle, "rmbkrd_neighbor5x5x5(threshold=40,fraction=0.5)", vol)
    _check(sqy, oracle, "rmbkrd_neighbor5x5x5->lz4", (vol > 30).astype(dtype))            # default threshold 1
    _check(sqy, oracle, "rmbkrd_neighbor5x5x5(threshold=40,fraction=0.25)->diff3x3x1->bitswap1->lz4", vol)


def test_neighbor5_boundary_count(sqy, oracle):
    """n exactly fraction * 124: kept (the reference zeroes only n > cut)"""
    shape = (20, 24, 24)
    for frac, p in ((0.5, 0.5), (0.25, 0.25), (0.75, 0.75)):
        rng = np.random.default_rng(int(frac * 100))
        vol = np.where(rng.random(shape) < p, 10, 200).astype(np.uint16)
        cut = np.float32(frac) * np.float32(124)
        n = R.neighbor5_counts(vol, 100)
        at = R.neighbor5_centres(shape) & (vol >= 100)
        assert (n[at] == cut).any() and (n[at] == cut + 1).any()                            # the data sits on both sides of the cut
        _check(sqy, oracle, "rmbkrd_neighbor5x5x5(threshold=100,fraction=%g)->lz4" % frac, vol)


def test_neighbor5_thresholds_that_wrap(sqy, oracle):
    vol = _vol((12, 16, 20), np.uint16, 4400, 4530, 7)
    _check(sqy, oracle, "rmbkrd_neighbor5x5x5(threshold=70000)->lz4", vol)                  # 70000 -> 4464 on 16 bits
    v8 = _vol((12, 16, 20), np.uint8, 80, 150, 8)
    _check(sqy, oracle, "rmbkrd_neighbor5x5x5(threshold=70000)->lz4", v8)                   # -> 112 on 8 bits
    _check(sqy, oracle, "rmbkrd_neighbor5x5x5(threshold=-1,fraction=-2)->lz4", vol)


@pytest.mark.parametrize("dtype", [np.uint16, np.uint8])
def test_rmestbkrd_parity(sqy, oracle, dtype, options):
    for shape in ((16, 64, 64), (5, 33, 70), (2, 16, 16), (3, 7, 300), (64, 128, 96)):
        vol = synth.stack(shape, dtype) if min(shape) >= 8 else _vol(shape, dtype, 0, 200, 3)
        for l2 in (None, 1000, 1, 0):                                                       # detected; the portion branch; empty z faces
            if l2 is not None:
                options("host_l2_bytes", l2)
            for pipeline in ("rmestbkrd->bitswap1->lz4", "rmestbkrd", "rmestbkrd->lz4", "rmestbkrd->rmbkrd_neighbor5x5x5(threshold=3)->lz4"):
                if pipeline.endswith("(threshold=3)->lz4") and not R.neighbor5_defined(shape):
                    continue
                _check(sqy, oracle, pipeline, vol)
    options("host_l2_bytes", 1)
    assert R.support(R.face_histograms(synth.stack((16, 64, 64), dtype), 1)[0]) == 0


def test_rmestbkrd_uint32_wrap(sqy, oracle, options):
    """a 512 x 512 face of one value >= 16384: bins[m] * m wraps in 32 bits (the reference's support is then not the value)"""
    options("host_l2_bytes", 1 << 30)
    vol = _vol((4, 512, 512), np.uint16, 8000, 9000, 11)
    vol[0] = 40000
    t = R.rmestbkrd_threshold(vol, 1 << 30)
    assert t == int(np.float32(np.uint32((262144 * 40000) & 0xffffffff)) / np.float32(262144))
    _check(sqy, oracle, "rmestbkrd->bitswap1->lz4", vol)
    _check(sqy, oracle, "rmestbkrd->quantiser->bitswap1->lz4", vol, lossless=False)


def test_pipelines_round_trip(sqy, oracle):
    vol = synth.stack((32, 64, 96))
    for pipeline in ("rmestbkrd->bitswap1->lz4", "rmestbkrd", "rmbkrd_neighbor5x5x5(threshold=40,fraction=0.25)->diff3x3x1->bitswap1->lz4",
                     "rmbkrd_neighbor5x5x5->bitswap1->lz4", "rmestbkrd->pass_through", "rmbkrd_neighbor5x5x5->raster_reorder->lz4"):
        _check(sqy, oracle, pipeline, vol)
    _check(sqy, oracle, "frame_shuffle->rmbkrd_neighbor5x5x5(threshold=300)->lz4", vol)
    v8 = synth.stack((32, 64, 96), np.uint8)
    for pipeline in ("rmestbkrd->bitswap1->lz4", "frame_shuffle->rmbkrd_neighbor5x5x5->lz4", "rmbkrd_neighbor5x5x5(threshold=5)"):
        _check(sqy, oracle, pipeline, v8)
    # quantiser behind rmestbkrd (lossy): bytes against the oracle; the decode is the quantiser's decode of the filtered volume
    l2 = sqy.get_option("host_l2_bytes")
    blob = _check(sqy, oracle, "rmestbkrd->quantiser->bitswap1->lz4", vol, lossless=False)
    rc, back = sqy.decode(blob)
    assert rc == 0 and np.array_equal(back, oracle.pipeline_decode(R.expected_blob(oracle, "quantiser->bitswap1->lz4", R.rmestbkrd(vol, l2))))


def test_refused_shapes_launch_nothing(sqy):
    import torch
    dev = torch.device("cuda", 0)
    cases = [("rmestbkrd->lz4", (1, 64, 64)), ("rmestbkrd", (64, 64)), ("rmbkrd_neighbor5x5x5->lz4", (3, 5, 6)),
             ("rmbkrd_neighbor5x5x5->lz4", (8, 5, 5)), ("rmbkrd_neighbor5x5x5->lz4", (8, 4, 9)), ("rmbkrd_neighbor5x5x5", (8, 9, 4)),
             ("frame_shuffle->rmbkrd_neighbor5x5x5->lz4", (20, 5, 5)), ("rmbkrd_neighbor5x5x5->lz4", (4096,))]
    for pipeline, shape in cases:
        for dtype, tdt in ((np.uint16, torch.int16), (np.uint8, torch.uint8)):
            vol = torch.full(shape, 7, dtype=tdt, device=dev)
            out = torch.full((1 << 16,), 0x5A, dtype=torch.uint8, device=dev)
            torch.cuda.synchronize()
            rc, n = sqy.encode_device(pipeline, vol.data_ptr(), shape, dtype, out.data_ptr(), out.numel())
            torch.cuda.synchronize()
            assert rc == 1, (pipeline, shape)
            assert bool((out == 0x5A).all()), (pipeline, shape)
            assert sqy.encode(pipeline, np.full(shape, 7, dtype))[0] == 1


def test_fullsize_rmestbkrd_bitswap1_lz4(sqy, oracle):
    import torch
    dev = torch.device("cuda", 0)
    pipeline, shape, dtype = "rmestbkrd->bitswap1->lz4", (512, 1024, 1024), np.uint16
    vol = synth.stack_torch(shape, dtype, dev)
    cap = sqy.max_compressed_length(pipeline, shape, dtype)
    out = torch.empty(cap, dtype=torch.uint8, device=dev)
    rc, n = sqy.encode_device(pipeline, vol.data_ptr(), shape, dtype, out.data_ptr(), cap, nthreads=0)
    assert rc == 0
    got = hashlib.sha256(out[:n].cpu().numpy().tobytes()).hexdigest()
    host = vol.cpu().numpy()
    del vol, out
    torch.cuda.empty_cache()
    want = R.expected_blob(oracle, pipeline, host, sqy.get_option("host_l2_bytes"))
    assert got == hashlib.sha256(want).hexdigest()


@pytest.mark.parametrize("pipeline,dtype", [("rmestbkrd->bitswap1->lz4", np.uint16), ("rmbkrd_neighbor5x5x5(threshold=300)->bitswap1->lz4", np.uint16),
                                            ("rmestbkrd->rmbkrd_neighbor5x5x5->lz4", np.uint8)])
def test_slabs_call_equals_single_calls(sqy, oracle, pipeline, dtype):
    import torch
    dev = torch.device("cuda", 0)
    shape, nslabs = (40, 128, 128), 4
    vol = synth.stack(shape, dtype)
    d_vol = torch.from_numpy(vol.copy()).to(dev)
    cap = (sqy.max_compressed_length(pipeline, (10,) + shape[1:], dtype) + 255) & ~255
    out = torch.zeros(cap * nslabs, dtype=torch.uint8, device=dev)
    rc, offs, lens = sqy.encode_slabs_device(pipeline, d_vol.data_ptr(), shape, dtype, nslabs, out.data_ptr(), cap, inflight=3)
    assert rc == 0
    l2 = sqy.get_option("host_l2_bytes")
    for i in range(nslabs):
        z0, nz = multi.slab_range(shape[0], i, nslabs)
        got = bytes(out[offs[i]:offs[i] + lens[i]].cpu().numpy().tobytes())
        single = sqy.encode(pipeline, vol[z0:z0 + nz], nthreads=0)[1]
        assert got == single == R.expected_blob(oracle, pipeline, vol[z0:z0 + nz], l2), (pipeline, i)


def test_four_calls_in_flight(sqy, oracle):
    vol = synth.stack((64, 256, 256))
    pipelines = ["rmestbkrd->bitswap1->lz4", "rmbkrd_neighbor5x5x5(threshold=300,fraction=0.25)->bitswap1->lz4"]
    want = {p: R.expected_blob(oracle, p, vol, sqy.get_option("host_l2_bytes")) for p in pipelines}
    got, errors = {}, []

    def worker(t):
        try:
            for k in range(3):
                p = pipelines[(t + k) % 2]
                rc, blob = sqy.encode(p, vol, nthreads=2)
                got[(t, k)] = (p, rc, blob)
        except Exception as e:                                  # pragma: no cover
            errors.append(e)
    threads = [threading.Thread(target=worker, args=(t,)) for t in range(4)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert not errors
    assert len(got) == 12
    for p, rc, blob in got.values():
        assert rc == 0 and blob == want[p], p
