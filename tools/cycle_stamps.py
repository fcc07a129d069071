"""The in-flight leg of bench.py (1024x1024x512 u16 bitswap1->lz4, caller threads with a stream each, calls marshalled once, per-kernel
timing on, transpose_chain_caller_streams on) with the library's call stamps switched on; writes them as JSON for tools/inflight_timeline.py.

    rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- python tools/cycle_stamps.py <stamps.json> [calls] [in flight] [option=value ..]
    python tools/inflight_timeline.py <dir>/.../*_kernel_trace.csv <stamps.json>

Without rocprofv3 the stamps alone give the host-side terms (entry -> first launch, synchronise -> return, time outside the library)."""
import ctypes
import json
import os
import sys
import threading
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PIPELINE = "bitswap1->lz4"
SHAPE = (512, 1024, 1024)


def main():
    import torch
    import sqeazy_amd
    from sqeazy_amd import synth
    out_path = sys.argv[1]
    plain = [a for a in sys.argv[2:] if "=" not in a]
    opts = [a.split("=") for a in sys.argv[2:] if "=" in a]
    ncalls = int(plain[0]) if plain else 400
    inflight = int(plain[1]) if len(plain) > 1 else 4
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    vol = synth.stack_torch(SHAPE, np.uint16, dev)
    vols = [vol] + [vol.clone() for _ in range(inflight - 1)]
    cap = sqeazy_amd.max_compressed_length(PIPELINE, SHAPE, np.uint16)
    sys.setswitchinterval(1e-4)
    streams = [torch.cuda.Stream(device=dev) for _ in range(inflight)]
    outs = [[torch.empty(cap, dtype=torch.uint8, device=dev) for _ in range(2)] for _ in range(inflight)]
    torch.cuda.synchronize()
    entry = sqeazy_amd.lib().SQYAMD_PipelineEncode_UI16_DeviceAt
    pipe_b = PIPELINE.encode()
    shape_c = (ctypes.c_long * 3)(*SHAPE)

    def prepared(t, b):
        doff, dlen = ctypes.c_long(0), ctypes.c_long(0)
        return (pipe_b, ctypes.c_void_p(vols[t].data_ptr()), shape_c, ctypes.c_uint(3), ctypes.c_void_p(outs[t][b].data_ptr()), ctypes.c_long(cap),
                ctypes.byref(doff), ctypes.byref(dlen), ctypes.c_int(0), ctypes.c_void_p(streams[t].cuda_stream)), doff, dlen

    calls = [[prepared(t, b) for b in range(2)] for t in range(inflight)]
    lens = [0] * inflight

    def caller(t, k):
        torch.cuda.set_device(0)
        for i in range(k):
            args, _doff, dlen = calls[t][i & 1]
            if entry(*args):
                raise RuntimeError("encode failed")
            lens[t] = dlen.value

    def block(k):
        ths = [threading.Thread(target=caller, args=(t, k)) for t in range(inflight)]
        t0 = time.perf_counter()
        for th in ths:
            th.start()
        for th in ths:
            th.join()
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    for name, value in opts:
        sqeazy_amd.set_option(name, int(value))
    sqeazy_amd.set_option("transpose_chain_caller_streams", 1)
    block(2)
    block(5)
    sqeazy_amd.profile_reset()
    sqeazy_amd.profile_enable(True)
    sqeazy_amd.set_option("lane_calls", 0)
    sqeazy_amd.set_option("call_stamps", 1)
    per = max(1, ncalls // inflight)
    dt = block(per)
    sqeazy_amd.set_option("call_stamps", 0)
    sqeazy_amd.profile_enable(False)
    clocks = {n: time.clock_gettime_ns(getattr(time, n)) for n in ("CLOCK_MONOTONIC", "CLOCK_BOOTTIME", "CLOCK_REALTIME", "CLOCK_MONOTONIC_RAW") if hasattr(time, n)}
    res = {"ms_per_step": dt * 1e3 / (per * inflight), "calls": per * inflight, "inflight": inflight, "blob_bytes": lens, "options": dict((n, int(v)) for n, v in opts),
           "lane_calls": sqeazy_amd.get_option("lane_calls"), "clocks_ns": clocks,
           "fields": list(sqeazy_amd.CALL_STAMP_FIELDS), "stamps": [[r[f] for f in sqeazy_amd.CALL_STAMP_FIELDS] for r in sqeazy_amd.call_stamps()]}
    with open(out_path, "w") as f:
        json.dump(res, f)
    print("%.4f ms/step over %d calls, %d in flight, %d stamped, blob %s bytes" % (res["ms_per_step"], res["calls"], inflight, len(res["stamps"]), sorted(set(lens))))


if __name__ == "__main__":
    main()
