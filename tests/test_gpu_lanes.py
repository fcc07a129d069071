"""The library's lanes (options stage_lanes / parse_lanes, include/sqeazy_amd.h): frames-in-place calls made on streams the callers
bring run on streams of the library's own -- one transpose lane, `parse_lanes` parse lanes.  No option value changes a byte; the
call still starts behind what the caller queued on its stream and is complete on return; a caller stream with a backlog delays
nobody else's call."""
import threading
import time

import numpy as np
import pytest

from sqeazy_amd import synth

pytestmark = pytest.mark.gpu

# the bench shape cut to 64 frames; a C3-type slab (bench.py: 2048 x 2048 frames, diff3x3x1 in front); a shape that is NOT frames in
# place (no whole transpose tiles: the ordinary path on the caller's stream, whatever the options say)
JOBS = [("bitswap1->lz4", (64, 1024, 1024)),
        ("diff3x3x1->bitswap1->lz4", (8, 2048, 2048)),
        ("bitswap1->lz4", (3, 50, 70))]


class _Job:
    def __init__(self, sqy, oracle, pipeline, shape, dev):
        import torch
        self.pipeline, self.shape = pipeline, shape
        self.vol = synth.stack(shape, np.uint16)
        self.d_vol = torch.from_numpy(self.vol).to(dev)
        self.cap = sqy.max_compressed_length(pipeline, shape, np.uint16)
        self.want = oracle.pipeline_encode(pipeline, self.vol, nthreads=2)
        self.d_want = torch.frombuffer(bytearray(self.want), dtype=torch.uint8).to(dev)

    def encode(self, sqy, out, stream):
        return sqy.encode_device_at(self.pipeline, self.d_vol.data_ptr(), self.shape, np.uint16, out.data_ptr(), self.cap, nthreads=2,
                                    stream=stream.cuda_stream if stream is not None else None)

    def check(self, out, rc, off, n):
        import torch
        assert rc == 0 and 0 <= off and off + n <= self.cap
        assert n == len(self.want) and torch.equal(out[off:off + n], self.d_want), (self.pipeline, self.shape)


@pytest.fixture(scope="module")
def jobs(sqy, oracle):
    """the three inputs on the device and their blobs: the oracle's, and equal to it the single-threaded blob with the lanes off"""
    import torch
    dev = torch.device("cuda", 0)
    js = [_Job(sqy, oracle, p, s, dev) for p, s in JOBS]
    old = sqy.get_option("stage_lanes")
    sqy.set_option("stage_lanes", 0)
    try:
        for j in js:
            out = torch.empty(j.cap, dtype=torch.uint8, device=dev)
            j.check(out, *j.encode(sqy, out, None))
    finally:
        sqy.set_option("stage_lanes", old)
    return js


COUNTERS = ("lane_calls", "lane_backlog_fallbacks", "lane_blocked_fallbacks")


def _reset_counters(sqy):
    for c in COUNTERS:
        sqy.set_option(c, 0)


def _counters(sqy):
    return {c: sqy.get_option(c) for c in COUNTERS}


def test_lane_options(sqy, options):
    assert sqy.get_option("stage_lanes") in (0, 1, 2) and 1 <= sqy.get_option("parse_lanes") <= 8
    L = sqy.lib()
    for bad in (0, 9, -1):
        assert L.SQYAMD_Set_Option(b"parse_lanes", bad) == 1
    assert L.SQYAMD_Set_Option(b"stage_lanes", 3) == 1 and L.SQYAMD_Set_Option(b"stage_lanes", -1) == 1
    for c in COUNTERS:
        assert L.SQYAMD_Set_Option(c.encode(), 1) == 1 and L.SQYAMD_Set_Option(c.encode(), 0) == 0 and sqy.get_option(c) == 0
    for n in range(1, 9):
        options("parse_lanes", n)
        assert sqy.get_option("parse_lanes") == n


@pytest.mark.parametrize("parse_lanes", [1, 3, 4])
@pytest.mark.parametrize("stage_lanes", [0, 1])
def test_six_threads_mixed_shapes(sqy, options, jobs, stage_lanes, parse_lanes):
    """6 threads x 8 calls of mixed shapes, each thread on a stream of its own: every blob equals the single-threaded one"""
    import torch
    dev = torch.device("cuda", 0)
    options("stage_lanes", stage_lanes)
    options("parse_lanes", parse_lanes)
    _reset_counters(sqy)
    errors = []

    def worker(t):
        try:
            torch.cuda.set_device(0)
            s = torch.cuda.Stream(device=dev)
            outs = [torch.empty(j.cap, dtype=torch.uint8, device=dev) for j in jobs]
            with torch.cuda.stream(s):
                for it in range(8):
                    k = (t + it) % len(jobs)
                    jobs[k].check(outs[k], *jobs[k].encode(sqy, outs[k], s))
                s.synchronize()
        except BaseException as e:   # pragma: no cover
            errors.append(repr(e)[:400])

    threads = [threading.Thread(target=worker, args=(t,)) for t in range(6)]
    for th in threads:
        th.start()
    for th in threads:
        th.join(timeout=600)
    assert not errors, errors[:3]
    # 48 calls, 32 of them frames in place (the third shape never is): with the lanes on every one of those ran on the lanes or says
    # why not, and most did (the streams carry nothing else; a lane is only ever asked for an answer when no other call is on the lanes)
    c = _counters(sqy)
    if stage_lanes == 0:
        assert c == {"lane_calls": 0, "lane_backlog_fallbacks": 0, "lane_blocked_fallbacks": 0}
    else:
        assert sum(c.values()) == 32 and c["lane_calls"] >= 24, c


def test_default_follows_the_callers_opt_in(sqy, options, jobs):
    """stage_lanes = 2 (default): lanes where the caller has set transpose_chain_caller_streams; the same bytes either way"""
    import torch
    dev = torch.device("cuda", 0)
    options("stage_lanes", 2)
    s = torch.cuda.Stream(device=dev)
    for chain in (0, 1, 0):
        options("transpose_chain_caller_streams", chain)
        for k, j in enumerate(jobs):
            out = torch.empty(j.cap, dtype=torch.uint8, device=dev)
            _reset_counters(sqy)
            with torch.cuda.stream(s):
                for _ in range(3):
                    j.check(out, *j.encode(sqy, out, s))
            c = _counters(sqy)
            # on the lanes only with the opt-in, and never the shape that is not frames in place
            assert sum(c.values()) == (3 if chain and k < 2 else 0) and c["lane_backlog_fallbacks"] == 0, (chain, k, c)


@pytest.mark.parametrize("stage_lanes", [0, 1])
def test_destination_filled_on_the_stream_just_before(sqy, oracle, options, jobs, stage_lanes):
    """the call starts behind what the caller queued on its stream: a fill of the destination queued right in front of the call (it
    overtook the transposes of the Slabs workers' streams in round 6) must not land on what the call wrote"""
    import torch
    dev = torch.device("cuda", 0)
    options("stage_lanes", stage_lanes)
    j = jobs[0]
    s = torch.cuda.Stream(device=dev)
    out = torch.empty(j.cap, dtype=torch.uint8, device=dev)
    with torch.cuda.stream(s):
        for it in range(6):
            out.fill_(0xA5 if it % 2 else 0x00)
            rc, off, n = j.encode(sqy, out, s)
            j.check(out, rc, off, n)
        blob = bytes(out[off:off + n].cpu().numpy().tobytes())
    rc, back = sqy.decode(blob)
    assert rc == 0 and np.array_equal(back, j.vol)


@pytest.mark.parametrize("stage_lanes,opt_in", [(0, 0), (1, 0), (2, 0)], ids=["lanes0", "lanes1", "lanes2_no_opt_in"])
def test_backlog_on_one_stream_delays_nobody_else(stage_lanes, opt_in):
    """Thread A's stream carries a long kernel in front of A's call; thread B's call on another stream, made while A waits, is not
    delayed by more than its own alone-time plus a margin.  In a child process (tests/lanes_backlog_child.py) that creates only
    the two callers' streams: which hardware queue a stream lands on depends on the streams created before it, and two streams
    behind one queue wait for each other whatever the library does.

    Bound: B's call may take  alone + (alone + margin):  `alone` = the median of nine of B's calls with nothing else running, the
    delay allowed is that alone-time again (what B may meet legitimately is one other call's kernels on the chip) plus `margin` =
    the spread of those nine (max - min: what the same call varies by with no cause at all).  The kernel in front of A spins for
    at least 100 alone-times, so a wait that leaks from A's stream into B's call cannot hide inside the bound.

    stage_lanes = 1: the lanes sit on all four hardware queues, so A's spin kernel is in front of one of them in its queue.  B's
    call is the only one on the lanes, asks the lanes it would take for an answer (a marker, 0.25 ms at most) and stays on its
    own stream when one is blocked: `lane_blocked_fallbacks`.  A's call never enters a lane: `lane_backlog_fallbacks`.
    Measured when written (MI355X, 64 x 1024 x 1024 `bitswap1->lz4`, wall time of the call from Python; spin kernel 112 ms): alone
    0.917 / 0.943 / 0.918 ms, margin 0.008 / 0.016 / 0.008 ms, bound 1.842 / 1.901 / 1.843 ms, B next to A's backlog 1.143 / 1.283 /
    1.101 ms for stage_lanes 0 / 1 / 2 without the opt-in (stage_lanes = 1: B ran on the lanes).  What the bound cannot cover is written
    down in DESIGN.md section 5: two caller streams that the runtime puts behind one hardware queue wait for each other with the
    lanes off, and a call that is not alone on the lanes does not ask them for an answer."""
    import json
    import os
    import subprocess
    import sys
    child = os.path.join(os.path.dirname(os.path.abspath(__file__)), "lanes_backlog_child.py")
    r = subprocess.run([sys.executable, child, str(stage_lanes), str(opt_in)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-3000:])
    d = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    alone = float(np.median(d["alone_s"]))
    margin = max(d["alone_s"]) - min(d["alone_s"])
    bound = 2 * alone + margin
    print("alone %.3f ms, margin %.3f ms, bound %.3f ms, B next to A's backlog %.3f ms, spin %.1f ms, A's call %.1f ms, counters %s" %
          (alone * 1e3, margin * 1e3, bound * 1e3, d["b_s"] * 1e3, d["spin_s"] * 1e3, d["a_s"] * 1e3, d["counters"]))
    assert d["a_ok"] and d["b_ok"] and d["b_decodes"]
    assert d["spin_s"] >= 100 * alone
    assert d["a_s"] >= 0.5 * d["spin_s"], "A's call did not wait for its own stream's backlog"
    c = d["counters"]
    if stage_lanes == 1:
        # A's backlog never enters a lane; B either ran on the lanes or found one blocked and stayed on its stream
        assert d["counters_after_a_called"]["lane_backlog_fallbacks"] == 1 and c["lane_backlog_fallbacks"] == 1
        assert c["lane_calls"] + c["lane_blocked_fallbacks"] == 1
    else:
        assert c == {"lane_calls": 0, "lane_backlog_fallbacks": 0, "lane_blocked_fallbacks": 0}
    assert d["b_s"] <= bound, "B's call took %.3f ms next to A's backlog, %.3f ms alone (bound %.3f ms)" % (d["b_s"] * 1e3, alone * 1e3, bound * 1e3)
