"""The metric kernels of frame_shuffle / tile_shuffle on the table of tests/frame_metric_cases.py.  The sum never leaves the library; the
reorder_map in the header does, and every subject frame stands between witness frames whose exact sums are one ulp below, at and one ulp
above the reference's sequential binary32 sum of the subject -- tests/test_frame_metric_host.py shows, case by case, that a device sum one
ulp off in either direction gives another map.  Every case goes through the C-ABI as the stage alone (raw payload) and with lz4 behind it,
twice in a row (the second call meets the first one's block sums and records in the reused scratch), the blob must be the oracle's byte
for byte and decode to what the oracle's decodes to.  A failure is one line: the case, its claim, and what the device's map says about its
sum."""
import base64
import time

import numpy as np
import pytest

import frame_metric_cases as F

pytestmark = pytest.mark.gpu

NTHREADS = 2
EXTRA = 16 * 8 + 512                                     # room for the reorder_map of at most 8 units in the header
_wanted = {}


def _want(oracle, b, pipeline):
    key = (b.case.name, pipeline)
    if key not in _wanted:
        _wanted[key] = oracle.pipeline_encode(pipeline, b.volume, NTHREADS)
    return _wanted[key]


def _encode(sqy, b, pipeline):
    """the blob through the host-pointer C-ABI, or, for a case that asks for a source off a 16-byte boundary, the device entry point"""
    c = b.case
    if not c.src_shift:
        rc, blob = sqy.encode(pipeline, b.volume, nthreads=NTHREADS, extra_capacity=EXTRA)
        assert rc == 0, (c.name, pipeline)
        return blob
    import torch
    dev = torch.device("cuda", 0)
    raw = torch.empty(b.volume.nbytes + 32, dtype=torch.uint8, device=dev)
    assert raw.data_ptr() % 16 == 0
    raw[c.src_shift:c.src_shift + b.volume.nbytes] = torch.from_numpy(np.frombuffer(b.volume.tobytes(), dtype=np.uint8).copy()).to(dev)
    cap = sqy.max_compressed_length(pipeline, b.volume.shape, c.dtype) + EXTRA
    out = torch.empty(cap, dtype=torch.uint8, device=dev)
    rc, n = sqy.encode_device(pipeline, raw.data_ptr() + c.src_shift, b.volume.shape, c.dtype, out.data_ptr(), cap, nthreads=NTHREADS)
    assert rc == 0, (c.name, pipeline)
    return bytes(out[:n].cpu().numpy().tobytes())


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


def _header_map(oracle, blob):
    h = oracle.header_unpack(blob)
    stage = next(s for s in oracle.build_stages(h["pipename"]) if s.name in ("frame_shuffle", "tile_shuffle"))
    return np.frombuffer(base64.b64decode(stage.map[len("<verbatim>"):-len("</verbatim>")]), dtype="<u8")


def _explain(oracle, b, pipeline, got, want):
    c = b.case
    head = "%s [%s, %s] through %s: " % (c.name, c.family, b.claim(b.subjects[0][3]), pipeline)
    try:
        gmap = _header_map(oracle, got)
    except Exception as e:                                       # noqa: BLE001  (a blob that cannot be read is its own finding)
        return head + "the blob's header cannot be read (%s)" % e
    wmap = _header_map(oracle, want)
    assert np.array_equal(wmap, b.expected_map), "the oracle's map is not the case's"
    if gmap.size != wmap.size:
        return head + "the reorder_map has %d entries, the oracle's %d" % (gmap.size, wmap.size)
    return head + F.implied(b, gmap)


def _same(oracle, b, pipeline, got):
    want = _want(oracle, b, pipeline)
    if got != want:
        pytest.fail(_explain(oracle, b, pipeline, got, want), pytrace=False)


def _ran_on_its_path(b, prof):
    """the metric kernel ran once, under the name of the stage, and shape and alignment are the ones launch_frame_metric documents for the
    kernel the case is for"""
    c = b.case
    name = "tile_metric" if c.kind == F.TILE else "frame_metric"
    assert name in prof and prof[name][1] == 1, (c.name, prof)
    nbytes = c.per_unit * c.dtype.itemsize
    blocks = -(-nbytes // F.BLOCK_BYTES)
    if c.path == F.SIGNED:
        assert c.kind == F.TAIL and c.dtype.itemsize == 1
    elif c.path == F.PLANNED:
        assert nbytes % 16 == 0 and not c.src_shift and blocks >= F.PLANNED_MIN_BLOCKS and c.kind != F.TAIL
    elif c.path == F.SCAN:
        assert nbytes % 16 == 0 and not c.src_shift and blocks < F.PLANNED_MIN_BLOCKS and c.kind != F.TAIL
    else:
        assert c.path == F.SERIAL and (nbytes % 16 != 0 or c.src_shift % 16 != 0) and c.kind != F.TAIL


def _check(sqy, oracle, b):
    for pipeline in b.case.pipelines():
        assert sqy.pipeline_possible(pipeline, b.case.dtype), pipeline
        for _ in range(2):
            blob, prof = _profiled(sqy, lambda: _encode(sqy, b, pipeline))
            _ran_on_its_path(b, prof)
            _same(oracle, b, pipeline, blob)
        want = _want(oracle, b, pipeline)
        rc, back = sqy.decode(want)
        assert rc == 0 and np.array_equal(back, oracle.pipeline_decode(want)), (b.case.name, pipeline)


@pytest.mark.parametrize("name", F.SMALL)
def test_case(sqy, oracle, name):
    _check(sqy, oracle, F.built(name))


def test_short_frames_right_after_long_ones(sqy, oracle):
    """the scratch of the planned path is reused from call to call: 130 blocks per frame, then 16 (whose records lie where the long frames'
    block sums were), then the scan path, then 17 blocks with a partial last one, 16 again, and the long ones again"""
    for name in ("chain_130_blocks", "record_sum_ahead", "guard_pass_k3_scan", "chain_partial_last_block", "record_prefix_ahead_no_crossing",
                 "record_prefix_ahead", "chain_130_blocks"):
        b = F.built(name)
        for pipeline in b.case.pipelines():
            _same(oracle, b, pipeline, _encode(sqy, b, pipeline))


def test_stall_at_2p24(sqy, oracle):
    """2^24 + 5 * 4096 ones in a frame: the float sum stays at 2^24, an integer sum does not.  68 MB, alone in its test; the wall time is
    printed (pytest -s)"""
    t0 = time.perf_counter()
    b = F.built(F.BIG[0])
    t1 = time.perf_counter()
    pipeline = b.case.pipelines()[0]
    want = _want(oracle, b, pipeline)
    t2 = time.perf_counter()
    for _ in range(2):
        blob, prof = _profiled(sqy, lambda: _encode(sqy, b, pipeline))
        _ran_on_its_path(b, prof)
        _same(oracle, b, pipeline, blob)
    t3 = time.perf_counter()
    lz = b.case.pipelines()[1]
    _same(oracle, b, lz, _encode(sqy, b, lz))
    rc, back = sqy.decode(want)
    assert rc == 0 and np.array_equal(back, oracle.pipeline_decode(want))
    _wanted.clear()
    print("\nstall_at_2p24: %.2f s in all (volume %.2f s, oracle %.2f s, two encodes %.2f s, lz4 form and decode %.2f s)" % (
        time.perf_counter() - t0, t1 - t0, t2 - t1, t3 - t2, time.perf_counter() - t3))
