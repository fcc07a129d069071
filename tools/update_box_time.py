"""a box written into ONE large blob against decode + paste + encode (GPU box):  python3 tools/update_box_time.py [k]

Device time per call sequence (hipEvents around it on its stream, so the host's gaps between launches count), k interleaved repetitions
(default 7) after a warm-up, all in one process.  A 64x1024x1024 u16 synth.stack_torch stack encoded as ONE `bitswap1->lz4` blob, boxes
from frame 24 on:
  roi     -- 16x64x64
  half    -- 16x512x512
  frames  -- 16 frames whole
  frame   -- 1 frame whole
Columns:
  decode+paste+encode -- what a caller does without the entry point: SQYAMD_Decode_UI16_Device into scratch, ONE torch slice assignment,
                         SQYAMD_PipelineEncode_UI16_Device
  again               -- the same sequence once more in every repetition: its ratio to the first per pair is the spread a gain has to beat
  update              -- SQYAMD_Update_Box_UI16_Device
Every column's blob is checked against the baseline's, byte for byte.  Per row: min-max per column, the per-pair ratios baseline / update
and baseline / again, whether every pair shows the update faster by more than the baseline's own spread, the scratch the caller no longer
holds, and the per-kernel device times of one profiled `update` call.  One JSON line per row.
Not measured here: 8-bit voxels, plain `lz4`, pitched views, the whole path (update_box_subset = 0)."""
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
PIPELINE = "bitswap1->lz4"
BOXES = {"roi": ((24, 480, 480), (16, 64, 64)), "half": ((24, 256, 256), (16, 512, 512)), "frames": ((24, 0, 0), (16, 1024, 1024)), "frame": ((24, 0, 0), (1, 1024, 1024))}
COLUMNS = ("decode+paste+encode", "again", "update")


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


def main():
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev)
    sp = stream.cuda_stream
    vol = synth.stack_torch(SHAPE, np.uint16, dev)
    cap = sqeazy_amd.max_compressed_length(PIPELINE, SHAPE, np.uint16)
    blob = torch.empty(cap, dtype=torch.uint8, device=dev)
    rc, n = sqeazy_amd.encode_device(PIPELINE, vol.data_ptr(), SHAPE, np.uint16, blob.data_ptr(), cap, stream=sp)
    assert rc == 0
    raw = vol.numel() * 2
    scratch = torch.empty(SHAPE, dtype=torch.uint16, device=dev)
    out_base, out_new = torch.empty(cap, dtype=torch.uint8, device=dev), torch.empty(cap, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    for box_name, (origin, extent) in BOXES.items():
        view = synth.stack_torch(extent, np.uint16, dev)                # the box's new voxels
        cut = tuple(slice(o, o + e) for o, e in zip(origin, extent))
        lens = {}

        def baseline():
            rc = sqeazy_amd.lib().SQYAMD_Decode_UI16_Device(blob.data_ptr(), n, scratch.data_ptr(), raw, sp)
            assert rc == 0
            scratch[cut] = view
            rc, lens["base"] = sqeazy_amd.encode_device(PIPELINE, scratch.data_ptr(), SHAPE, np.uint16, out_base.data_ptr(), cap, stream=sp)
            assert rc == 0

        def update():
            rc, lens["new"] = sqeazy_amd.update_box_device(PIPELINE, blob.data_ptr(), n, origin, view.data_ptr(), extent, None, np.uint16, out_new.data_ptr(), cap, stream=sp)
            assert rc == 0

        fns = {"decode+paste+encode": baseline, "again": baseline, "update": update}
        for c in COLUMNS:                                   # warm-up, and the update's blob against the baseline's
            fns[c]()
        torch.cuda.synchronize()
        assert lens["base"] == lens["new"] and torch.equal(out_base[:lens["base"]], out_new[:lens["new"]]), box_name
        ms = {c: [] for c in COLUMNS}
        for _ in range(K):
            for c in COLUMNS:
                ms[c].append(round(timed(fns[c], stream), 3))
        gain = [round(x / s, 3) for s, x in zip(ms["update"], ms["decode+paste+encode"])]
        spread = [round(x / s, 3) for s, x in zip(ms["again"], ms["decode+paste+encode"])]
        row = {"pipeline": PIPELINE, "box": box_name, "origin": list(origin), "extent": list(extent), "stack": list(SHAPE), "blob_bytes": n, "new_blob_bytes": lens["new"],
               "ms": ms, "min_max": {c: [min(ms[c]), max(ms[c])] for c in COLUMNS}, "baseline_over_update": gain, "baseline_over_again": spread,
               "pairs_update_faster": sum(g > 1 for g in gain), "pairs": K, "scratch_bytes_caller_no_longer_holds": raw}
        row["faster_every_pair_beyond_spread"] = bool(min(gain) > max(max(spread), 1 / min(spread)))
        row["update_kernel_ms"] = profiled(update)
        print(json.dumps(row), flush=True)
        del view


if __name__ == "__main__":
    main()
