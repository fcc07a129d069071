"""many boxes of ONE large blob with one call against a loop of single-box calls (GPU box):  python3 tools/decode_boxes_time.py [k] [pipeline ...]

Device time per call sequence (hipEvents around it on its stream, so the host's gaps between launches and every call's own synchronisation
count), k interleaved repetitions (default 7) after a warm-up, all in one process; a sample is REPS sequences in a row, divided by REPS.
A 64x1024x1024 u16 synth.stack_torch stack encoded as ONE blob (`bitswap1->lz4` and `quantiser->bitswap1->lz4`), K = 4, 16, 64 boxes of
16x64x64 into dense views, placed
  same     -- all in the same 16 frames (24 .. 39)
  disjoint -- spread over the four disjoint z-ranges of 16 frames
  overlap  -- z-ranges that begin 3 frames apart and overlap
Columns:
  loop   -- K SQYAMD_Decode_Box_*_Device calls: what a caller runs without the entry point
  again  -- the same loop once more in every repetition: loop / again per pair is the spread a ratio has to beat
  boxes  -- ONE SQYAMD_Decode_Boxes_*_Device call
  split  -- .. with decode_boxes_joint = 0 (admitted once, then box by box)
Every column's views are checked against the full decode's voxels.  Per row: min-max per column, the per-pair ratios loop / boxes,
loop / again and split / boxes, whether every pair is faster by more than the spread, and the per-kernel device times of one profiled
`boxes` call.  One JSON line per row."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import sqeazy_amd  # noqa: E402
from sqeazy_amd import synth  # noqa: E402

K = int(sys.argv[1]) if len(sys.argv) > 1 else 7
REPS = 3
SHAPE = (64, 1024, 1024)
EXTENT = (16, 64, 64)
PIPELINES = sys.argv[2:] or ["bitswap1->lz4", "quantiser->bitswap1->lz4"]
COUNTS = (4, 16, 64)
PLACEMENTS = {"same": lambda i: 24, "disjoint": lambda i: 16 * (i % 4), "overlap": lambda i: (3 * i) % (SHAPE[0] - EXTENT[0] + 1)}
COLUMNS = ("loop", "again", "boxes", "split")


def timed(fn, stream):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(stream)
    for _ in range(REPS):
        fn()
    b.record(stream)
    b.synchronize()
    return a.elapsed_time(b) / REPS


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


def origins_of(placement, count):
    z = PLACEMENTS[placement]
    per = SHAPE[1] // EXTENT[1] - 1
    return [(z(i), (97 * i % per) * EXTENT[1] + 5, (61 * i % per) * EXTENT[2] + 3) for i in range(count)]


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
    for placement in PLACEMENTS:
        for count in COUNTS:
            origins = origins_of(placement, count)
            extents = [EXTENT] * count
            views = torch.empty((count,) + EXTENT, dtype=torch.uint16, device=dev)
            ptrs = [views[i].data_ptr() for i in range(count)]

            def loop():
                for o, p in zip(origins, ptrs):
                    rc = sqeazy_amd.decode_box_device(blob.data_ptr(), n, o, p, EXTENT, None, np.uint16, stream=sp)
                    assert rc == 0

            def boxes():
                rc = sqeazy_amd.decode_boxes_device(blob.data_ptr(), n, origins, ptrs, extents, None, np.uint16, stream=sp)
                assert rc == 0

            def split():
                with sqeazy_amd.option("decode_boxes_joint", 0):
                    boxes()

            fns = {"loop": loop, "again": loop, "boxes": boxes, "split": split}
            want = torch.stack([full[tuple(slice(a, a + e) for a, e in zip(o, EXTENT))] for o in origins])
            for c in COLUMNS:                                   # warm-up, and every column's views against the full decode's
                views.fill_(0)
                fns[c]()
                torch.cuda.synchronize()
                assert torch.equal(views, want), (pipeline, placement, count, c)
            ms = {c: [] for c in COLUMNS}
            for _ in range(K):
                for c in COLUMNS:
                    ms[c].append(round(timed(fns[c], stream), 3))
            gain = [round(x / s, 3) for s, x in zip(ms["boxes"], ms["loop"])]
            spread = [round(x / s, 3) for s, x in zip(ms["again"], ms["loop"])]
            row = {"pipeline": pipeline, "placement": placement, "boxes": count, "extent": list(EXTENT), "stack": list(SHAPE), "blob_bytes": n,
                   "z_ranges": sorted(set(o[0] for o in origins)), "ms": ms, "min_max": {c: [min(ms[c]), max(ms[c])] for c in COLUMNS},
                   "loop_over_boxes": gain, "loop_over_again": spread, "split_over_boxes": [round(x / s, 3) for s, x in zip(ms["boxes"], ms["split"])],
                   "bytes_delivered": count * int(np.prod(EXTENT)) * 2}
            row["boxes_faster_every_pair_by_more_than_the_spread"] = bool(min(gain) > max(max(spread), 1 / min(spread)))
            row["boxes_kernel_ms"] = profiled(boxes)
            print(json.dumps(row), flush=True)
            del views, want
    del blob, full
    torch.cuda.empty_cache()


def main():
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev)
    for pipeline in PIPELINES:
        run(pipeline, dev, stream)


if __name__ == "__main__":
    main()
