"""many boxes written into ONE large blob in one call against a chain of single-box calls (GPU box):  python3 tools/update_boxes_time.py [k]

Device time per call sequence (hipEvents around it on its stream, so the host's gaps between launches count), k interleaved repetitions
(default 7) after a warm-up, all in one process.  A 64x1024x1024 u16 synth.stack_torch stack encoded as ONE `bitswap1->lz4` blob, K = 4,
16 and 64 boxes of 16x64x64, voxel-disjoint (box i at row 128 (i // 8), column 128 (i % 8)):
  same      -- every box in frames 24 .. 39
  disjoint  -- box i in frames 16 (i % 4) .. + 15: four z-ranges that do not meet (the stack has no room for more of 16 frames)
  overlap   -- box i from frame 5 i % 48 on: z-ranges that overlap their neighbours'
and one row of plain `lz4` (same, K = 16).
Columns:
  chain   -- what the parent of this entry point offers: K SQYAMD_Update_Box_UI16_Device calls, ping-ponging two caller buffers of
             max_compressed_length bytes
  again   -- the same sequence once more in every repetition: its ratio to the first per pair is the spread a gain has to beat
  boxes   -- ONE SQYAMD_Update_Boxes_UI16_Device call
The boxes' blob is checked against the chain's, byte for byte.  Per row: min-max per column, the per-pair ratios chain / boxes and
chain / again, whether every pair shows the one call faster by more than the chain's own spread (the project's rule for a claim), the
buffer the caller no longer holds, and the per-kernel device times of one profiled `boxes` call.  One JSON line per row.
Not measured here: 8-bit voxels, pitched views, overlapping voxels, the whole path (update_boxes_subset = 0), the host variants."""
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
EXTENT = (16, 64, 64)
PLACE = {"same": lambda i: 24, "disjoint": lambda i: 16 * (i % 4), "overlap": lambda i: 5 * i % 48}
ROWS = [("bitswap1->lz4", p, k) for p in ("same", "disjoint", "overlap") for k in (4, 16, 64)] + [("lz4", "same", 16)]
COLUMNS = ("chain", "again", "boxes")


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
    views = [synth.stack_torch(EXTENT, np.uint16, dev, seed=4000 + i) for i in range(64)]         # the boxes' new voxels
    blobs = {}
    for pipeline, place, nbox in ROWS:
        cap = sqeazy_amd.max_compressed_length(pipeline, SHAPE, np.uint16)
        if pipeline not in blobs:
            blob = torch.empty(cap, dtype=torch.uint8, device=dev)
            rc, n = sqeazy_amd.encode_device(pipeline, vol.data_ptr(), SHAPE, np.uint16, blob.data_ptr(), cap, stream=sp)
            assert rc == 0
            blobs[pipeline] = (blob, n)
        blob, n = blobs[pipeline]
        ping = [torch.empty(cap, dtype=torch.uint8, device=dev) for _ in range(2)]
        out_new = torch.empty(cap, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        origins = [(PLACE[place](i), 128 * (i // 8), 128 * (i % 8)) for i in range(nbox)]
        ptrs = [v.data_ptr() for v in views[:nbox]]
        lens = {}

        def chain():
            src, m = blob, n
            for i, o in enumerate(origins):
                rc, m = sqeazy_amd.update_box_device(pipeline, src.data_ptr(), m, o, ptrs[i], EXTENT, None, np.uint16, ping[i & 1].data_ptr(), cap, stream=sp)
                assert rc == 0
                src = ping[i & 1]
            lens["chain"], lens["at"] = m, src

        def boxes():
            rc, lens["boxes"] = sqeazy_amd.update_boxes_device(pipeline, blob.data_ptr(), n, origins, ptrs, [EXTENT] * nbox, None, np.uint16, out_new.data_ptr(), cap, stream=sp)
            assert rc == 0

        fns = {"chain": chain, "again": chain, "boxes": boxes}
        for c in COLUMNS:                                   # warm-up, and the one call's blob against the chain's
            fns[c]()
        torch.cuda.synchronize()
        assert lens["chain"] == lens["boxes"] and torch.equal(lens["at"][:lens["chain"]], out_new[:lens["boxes"]]), (pipeline, place, nbox)
        ms = {c: [] for c in COLUMNS}
        for _ in range(K):
            for c in COLUMNS:
                ms[c].append(round(timed(fns[c], stream), 3))
        gain = [round(x / s, 3) for s, x in zip(ms["boxes"], ms["chain"])]
        spread = [round(x / s, 3) for s, x in zip(ms["again"], ms["chain"])]
        row = {"pipeline": pipeline, "placement": place, "boxes": nbox, "extent": list(EXTENT), "stack": list(SHAPE), "blob_bytes": n, "new_blob_bytes": lens["boxes"], "ms": ms,
               "min_max": {c: [min(ms[c]), max(ms[c])] for c in COLUMNS}, "chain_over_boxes": gain, "chain_over_again": spread, "pairs_boxes_faster": sum(g > 1 for g in gain),
               "pairs": K, "buffer_bytes_caller_no_longer_holds": cap}
        row["faster_every_pair_beyond_spread"] = bool(min(gain) > max(max(spread), 1 / min(spread)))
        row["boxes_kernel_ms"] = profiled(boxes)
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
