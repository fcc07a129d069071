"""a box read out of ONE large blob against the frame-range decode and a slice copy (GPU box):  python3 tools/decode_box_time.py [k] [pipeline ...]

Device time per call sequence (hipEvents around it on its stream, so the host's gaps between launches count), k interleaved repetitions
(default 7) after a warm-up, all in one process.  A 64x1024x1024 u16 synth.stack_torch stack encoded as ONE blob (`bitswap1->lz4` and
`quantiser->bitswap1->lz4`), boxes of 16 frames from frame 24 on:
  roi    -- 16x64x64
  half   -- 16x512x512
  frames -- the 16 frames whole
Columns:
  frames+slice -- what a caller does without the box entry point: SQYAMD_Decode_Frames_*_Device of the box's frames into scratch, then ONE
                  slice copy with torch into the view
  again        -- the same sequence once more in every repetition: frames+slice / again per pair is the spread a ratio has to beat
  box          -- SQYAMD_Decode_Box_*_Device into the view
  whole        -- .. with decode_box_subset = 0 (the whole blob decoded, one window copy): what the pruning is worth
Every column's view is checked against the full decode's voxels.  Per row: min-max per column, the per-pair ratios frames+slice / box and
frames+slice / again, whether every pair agrees and the median gain lies outside the spread, the scratch a caller holds against the box's
bytes, and the per-kernel device times of one profiled `box` call.  One JSON line per row."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import sqeazy_amd  # noqa: E402
from sqeazy_amd import synth  # noqa: E402

K = int(sys.argv[1]) if len(sys.argv) > 1 else 7
SHAPE = (64, 1024, 1024)
PIPELINES = sys.argv[2:] or ["bitswap1->lz4", "quantiser->bitswap1->lz4"]
BOXES = {"roi": ((24, 480, 480), (16, 64, 64)), "half": ((24, 256, 256), (16, 512, 512)), "frames": ((24, 0, 0), (16, 1024, 1024))}
COLUMNS = ("frames+slice", "again", "box", "whole")


def timed(fn, stream):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(stream)
    fn()
    b.record(stream)
    b.synchronize()
    return a.elapsed_time(b)


def profiled(fn):
    sqeazy_amd.profile_reset()
    sqeazy_amd.profile_enable(True)
    try:
        fn()
        torch.cuda.synchronize()
    finally:
        sqeazy_amd.profile_enable(False)
    got = {k: [round(v[0], 3), v[1]] for k, v in sorted(sqeazy_amd.profile_get().items())}
    sqeazy_amd.profile_reset()
    return got


def run(pipeline, dev, stream):
    sp = stream.cuda_stream
    vol = synth.stack_torch(SHAPE, np.uint16, dev)
    cap = sqeazy_amd.max_compressed_length(pipeline, SHAPE, np.uint16)
    blob = torch.empty(cap, dtype=torch.uint8, device=dev)
    rc, n = sqeazy_amd.encode_device(pipeline, vol.data_ptr(), SHAPE, np.uint16, blob.data_ptr(), cap, stream=sp)
    assert rc == 0
    del vol
    fb = SHAPE[1] * SHAPE[2] * 2
    full = torch.empty(SHAPE, dtype=torch.uint16, device=dev)           # the voxels every column is held to (quantiser: not the stack's)
    rc = sqeazy_amd.decode_frames_device(blob.data_ptr(), n, 0, SHAPE[0], full.data_ptr(), SHAPE[0] * fb, np.uint16, stream=sp)
    assert rc == 0
    torch.cuda.synchronize()
    for box_name, (origin, extent) in BOXES.items():
        view = torch.empty(extent, dtype=torch.uint16, device=dev)
        scratch = torch.empty((extent[0],) + SHAPE[1:], dtype=torch.uint16, device=dev)
        cut = tuple(slice(o, o + e) for o, e in zip(origin[1:], extent[1:]))

        def frames_slice():
            rc = sqeazy_amd.decode_frames_device(blob.data_ptr(), n, origin[0], extent[0], scratch.data_ptr(), extent[0] * fb, np.uint16, stream=sp)
            assert rc == 0
            view.copy_(scratch[(slice(None),) + cut])

        def box():
            rc = sqeazy_amd.decode_box_device(blob.data_ptr(), n, origin, view.data_ptr(), extent, None, np.uint16, stream=sp)
            assert rc == 0

        def whole():
            with sqeazy_amd.option("decode_box_subset", 0):
                box()

        fns = {"frames+slice": frames_slice, "again": frames_slice, "box": box, "whole": whole}
        want = full[tuple(slice(o, o + e) for o, e in zip(origin, extent))]
        for c in COLUMNS:                                   # warm-up, and every column's view against the full decode's
            view.fill_(0)
            fns[c]()
            torch.cuda.synchronize()
            assert torch.equal(view, want), (pipeline, box_name, c)
        ms = {c: [] for c in COLUMNS}
        for _ in range(K):
            for c in COLUMNS:
                ms[c].append(round(timed(fns[c], stream), 3))
        gain = [round(x / s, 3) for s, x in zip(ms["box"], ms["frames+slice"])]
        spread = [round(x / s, 3) for s, x in zip(ms["again"], ms["frames+slice"])]
        row = {"pipeline": pipeline, "box": box_name, "origin": list(origin), "extent": list(extent), "stack": list(SHAPE), "blob_bytes": n, "ms": ms,
               "min_max": {c: [min(ms[c]), max(ms[c])] for c in COLUMNS}, "frames+slice_over_box": gain, "frames+slice_over_again": spread,
               "whole_over_box": [round(x / s, 2) for s, x in zip(ms["box"], ms["whole"])],
               "scratch_bytes_frames": extent[0] * fb, "box_bytes": int(np.prod(extent)) * 2}
        row["box_faster_every_pair"] = all(g > 1 for g in gain)
        row["median_gain_outside_spread"] = bool(np.median(gain) > max(spread) or np.median(gain) < min(spread))
        row["box_kernel_ms"] = profiled(box)
        print(json.dumps(row), flush=True)
        del view, scratch
    del blob, full
    torch.cuda.empty_cache()


def main():
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev)
    for pipeline in PIPELINES:
        run(pipeline, dev, stream)


if __name__ == "__main__":
    main()
