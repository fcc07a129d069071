"""Child process of tests/test_gpu_lanes.py::test_backlog_on_one_stream_delays_nobody_else: the scenario in a process that has created
nothing but the two callers' streams, so that the runtime's dealing of streams to hardware queues is the same from run to run.

    python tests/lanes_backlog_child.py <stage_lanes> <transpose_chain_caller_streams>

Thread A's stream carries a long spin kernel in front of A's call; thread B calls on its own stream while A waits.  Prints one JSON line:
B's nine alone-times, B's time next to A's backlog, the spin kernel's and A's call's time, the lane counters, whether both blobs are the
lanes-off blob and decode to the input."""
import json
import os
import sys
import threading
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main(stage_lanes, opt_in):
    import torch
    import sqeazy_amd
    from sqeazy_amd import synth
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    pipe, shape = "bitswap1->lz4", (64, 1024, 1024)
    vol = synth.stack(shape, np.uint16)
    d_vol = torch.from_numpy(vol).to(dev)
    cap = sqeazy_amd.max_compressed_length(pipe, shape, np.uint16)
    sa, sb = torch.cuda.Stream(device=dev), torch.cuda.Stream(device=dev)
    out_a = torch.empty(cap, dtype=torch.uint8, device=dev)
    out_b = torch.empty(cap, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()

    def call(out, s):
        t0 = time.perf_counter()
        rc, off, n = sqeazy_amd.encode_device_at(pipe, d_vol.data_ptr(), shape, np.uint16, out.data_ptr(), cap, nthreads=2, stream=s.cuda_stream)
        dt = time.perf_counter() - t0
        assert rc == 0
        return dt, out[off:off + n]

    sqeazy_amd.set_option("stage_lanes", 0)
    want = call(out_b, sb)[1].clone()
    sqeazy_amd.set_option("stage_lanes", stage_lanes)
    sqeazy_amd.set_option("transpose_chain_caller_streams", opt_in)
    for _ in range(3):
        call(out_b, sb)
    alone = [call(out_b, sb)[0] for _ in range(9)]
    # the spin kernel: at least 100 alone-times and 50 ms, calibrated here (the counter's rate is the device's business).  The first
    # launch of the spin kernel loads its code object, and any one launch can meet a stall of the host: a time that holds something
    # else than the kernel would end the calibration with a kernel far too short.  So one launch before any is timed, and a length
    # counts as long enough only by the shorter of two timings
    cycles, spin = 1 << 22, 0.0
    with torch.cuda.stream(sa):
        torch.cuda._sleep(1)
        sa.synchronize()
        for _ in range(12):
            timed = []
            for _ in range(2):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                torch.cuda._sleep(cycles)
                sa.synchronize()
                timed.append(time.perf_counter() - t0)
            spin = min(timed)
            if spin >= max(100 * float(np.median(alone)), 0.05):
                break
            cycles *= 4
    counters = ("lane_calls", "lane_backlog_fallbacks", "lane_blocked_fallbacks")
    for c in counters:
        sqeazy_amd.set_option(c, 0)
    sys.setswitchinterval(1e-4)
    res = {}

    def thread_a():
        torch.cuda.set_device(0)
        with torch.cuda.stream(sa):
            torch.cuda._sleep(cycles)
            res["a_s"], blob = call(out_a, sa)
            res["a_ok"] = bool(torch.equal(blob, want))

    torch.cuda.synchronize()
    ta = threading.Thread(target=thread_a)
    ta.start()
    time.sleep(0.25 * spin)                         # A's call has been made and sits behind the spin kernel
    after_a = {c: sqeazy_amd.get_option(c) for c in counters}
    b_s, blob = call(out_b, sb)
    with torch.cuda.stream(sb):
        b_ok = bool(torch.equal(blob, want))
        b_bytes = bytes(blob.cpu().numpy().tobytes())
    ta.join(timeout=600)
    rc, back = sqeazy_amd.decode(b_bytes)
    print(json.dumps({"alone_s": alone, "b_s": b_s, "spin_s": spin, "a_s": res.get("a_s"), "a_ok": res.get("a_ok"), "b_ok": b_ok,
                      "b_decodes": bool(rc == 0 and np.array_equal(back, vol)), "counters_after_a_called": after_a,
                      "counters": {c: sqeazy_amd.get_option(c) for c in counters}}))


if __name__ == "__main__":
    main(int(sys.argv[1]), int(sys.argv[2]))
