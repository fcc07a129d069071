"""Calls in flight on the library's lanes: what a call waits for on its way out, and the call stamps (option call_stamps,
SQYAMD_Call_Stamps).  A call that has seen its parse lane finish returns without
asking the lane again -- the next call may have queued its kernels there by then; no option value changes a byte, and calls that
change shape, pipeline or capacity from one call to the next on the same threads still give the oracle's blobs."""
import threading

import numpy as np
import pytest

from sqeazy_amd import synth

pytestmark = pytest.mark.gpu

ORDER = ("entry", "lanes_taken", "clear_launched", "transpose_launched", "parse_queued", "sync_returned", "returned")


class _Job:
    def __init__(self, sqy, oracle, pipeline, shape, dev, extra_cap=0):
        import torch
        self.pipeline, self.shape = pipeline, shape
        self.vol = synth.stack(shape, np.uint16)
        self.d_vol = torch.from_numpy(self.vol).to(dev)
        self.cap = sqy.max_compressed_length(pipeline, shape, np.uint16) + extra_cap
        self.want = oracle.pipeline_encode(pipeline, self.vol, nthreads=2)
        self.d_want = torch.frombuffer(bytearray(self.want), dtype=torch.uint8).to(dev)

    def run(self, sqy, out, stream):
        import torch
        rc, off, n = sqy.encode_device_at(self.pipeline, self.d_vol.data_ptr(), self.shape, np.uint16, out.data_ptr(), self.cap, nthreads=2,
                                          stream=stream.cuda_stream)
        assert rc == 0 and 0 <= off and off + n <= self.cap
        assert n == len(self.want) and torch.equal(out[off:off + n], self.d_want), (self.pipeline, self.shape, self.cap)


def _in_flight(nthreads, body):
    errors = []

    def worker(t):
        try:
            import torch
            torch.cuda.set_device(0)
            s = torch.cuda.Stream(device=torch.device("cuda", 0))
            with torch.cuda.stream(s):
                body(t, s)
                s.synchronize()
        except BaseException as e:   # pragma: no cover
            errors.append(repr(e)[:400])

    threads = [threading.Thread(target=worker, args=(t,)) for t in range(nthreads)]
    for th in threads:
        th.start()
    for th in threads:
        th.join(timeout=600)
    assert not errors, errors[:3]


def test_four_in_flight_then_shape_pipeline_capacity_change(sqy, oracle, options):
    """the bench pipeline four in flight on the lanes; then, on the same threads, another shape, another pipeline string, another
    capacity: every blob is the oracle's, every call left one record of stamps, in order"""
    import torch
    dev = torch.device("cuda", 0)
    phases = [_Job(sqy, oracle, "bitswap1->lz4", (64, 1024, 1024), dev),
              _Job(sqy, oracle, "bitswap1->lz4", (32, 512, 1024), dev),                             # the shape changes
              _Job(sqy, oracle, "bitswap1->lz4(accel=1)", (32, 512, 1024), dev),                    # .. the pipeline string
              _Job(sqy, oracle, "bitswap1->lz4(accel=1)", (32, 512, 1024), dev, extra_cap=4096 + 16)]   # .. the capacity
    options("stage_lanes", 1)
    options("lane_calls", 0)
    options("call_stamps", 1)
    per_phase = 6

    def body(t, s):
        out = torch.empty(max(j.cap for j in phases), dtype=torch.uint8, device=dev)
        for j in phases:
            for _ in range(per_phase):
                j.run(sqy, out, s)

    _in_flight(4, body)
    recs = sqy.call_stamps()
    ncalls = 4 * per_phase * len(phases)
    assert len(recs) == ncalls
    on_lanes = [r for r in recs if r["seq"] >= 0]
    assert len(on_lanes) == sqy.get_option("lane_calls") and len(on_lanes) >= ncalls // 2
    assert sorted(r["seq"] for r in on_lanes) == list(range(len(on_lanes)))
    assert len(set(r["thread"] for r in recs)) == 4
    for r in on_lanes:
        assert 0 <= r["lane"] < sqy.get_option("parse_lanes")
        ts = [r[k] for k in ORDER]
        assert all(a > 0 for a in ts) and ts == sorted(ts), r
    for r in recs:
        assert 0 < r["entry"] <= r["returned"]
    sqy.set_option("call_stamps", 0)
    j = phases[0]
    out = torch.empty(j.cap, dtype=torch.uint8, device=dev)
    s = torch.cuda.Stream(device=dev)
    j.run(sqy, out, s)
    assert len(sqy.call_stamps()) == ncalls                          # switched off: nothing is added


def test_return_does_not_wait_for_the_next_call_on_the_lane(sqy, oracle, options):
    """Three threads, ONE parse lane: when a call's tail kernel is done the next call's kernels are queued on the same lane nearly every
    time.  From the moment the calling thread has seen its lane finish to the return of the C call there is host work only (events
    given back, the lease, the context): the bound is 100 us for the median -- ten times what that work takes,
    and a quarter of the shortest thing it could be waiting for, the 0.4 ms of another call's parse of 256 MiB."""
    import torch
    dev = torch.device("cuda", 0)
    job = _Job(sqy, oracle, "bitswap1->lz4", (128, 1024, 1024), dev)
    options("stage_lanes", 1)
    options("parse_lanes", 1)
    options("lane_calls", 0)

    def body(t, s):
        out = torch.empty(job.cap, dtype=torch.uint8, device=dev)
        for _ in range(3):
            job.run(sqy, out, s)
        if t == 0:
            barrier.wait()
            sqy.set_option("call_stamps", 1)
            barrier.wait()
        else:
            barrier.wait()
            barrier.wait()
        for _ in range(20):
            job.run(sqy, out, s)

    barrier = threading.Barrier(3)
    _in_flight(3, body)
    recs = [r for r in sqy.call_stamps() if r["seq"] >= 0]
    sqy.set_option("call_stamps", 0)
    assert len(recs) >= 40, len(recs)
    waits = sorted((r["returned"] - r["sync_returned"]) / 1e3 for r in recs)
    device = sorted((r["sync_returned"] - r["parse_queued"]) / 1e3 for r in recs)
    print("sync -> return: median %.1f us, p90 %.1f us, max %.1f us; queued -> sync: median %.1f us" %
          (waits[len(waits) // 2], waits[9 * len(waits) // 10], waits[-1], device[len(device) // 2]))
    assert waits[len(waits) // 2] < 100.0
