"""many boxes of ONE large blob compared with resident voxels in one call, against what a caller can do without the entry point
(GPU box):  python3 tools/compare_boxes_time.py [k] [pipeline ...]

Device time per call sequence (hipEvents around it on its stream, so the host's gaps between launches and every call's own synchronisation
count), k interleaved repetitions (default 7) after a warm-up, all in one process; a sample is REPS sequences in a row, divided by REPS.
A 64x1024x1024 u16 synth.stack_torch stack encoded as ONE blob (`bitswap1->lz4` and `quantiser->bitswap1->lz4`), K = 4, 16, 64 boxes of
16x64x64 against dense resident views (the decoded boxes with every 97th voxel changed), placed
  same     -- all in the same 16 frames (24 .. 39)
  disjoint -- spread over the four disjoint z-ranges of 16 frames
  overlap  -- z-ranges that begin 3 frames apart and overlap
Columns:
  base     -- ONE SQYAMD_Decode_Boxes_*_Device call into scratch of the caller's (K boxes), then the torch reductions that give the same
              eight fields per box, batched over the K boxes, and one copy of the (K, 8) table to the host: what a caller runs without
              the entry point
  again    -- the same once more in every repetition: base / again per pair is the spread a ratio has to beat
  compare  -- ONE SQYAMD_Compare_Boxes_*_Device call (no scratch of the caller's)
Every column's rows are held to each other and to the rows torch computes from the full decode's voxels.  Per row: min-max per column, the
per-pair ratios base / compare and base / again, whether every pair is faster by more than the spread, the scratch bytes the baseline
holds, and the per-kernel device times of one profiled `compare` call.  One JSON line per row."""
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
COLUMNS = ("base", "again", "compare")


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


def fields(decoded, views):
    """the eight fields per box of two (K, ..) int16 tensors that hold 16-bit voxels, as a (K, 8) int64 table on the host"""
    k = decoded.shape[0]
    a = decoded.reshape(k, -1).to(torch.int64) & 0xffff
    b = views.reshape(k, -1).to(torch.int64) & 0xffff
    d = (a - b).abs()
    table = torch.stack([torch.full((k,), a.shape[1], dtype=torch.int64, device=a.device), (d != 0).sum(1), d.sum(1), (d * d).sum(1), d.amax(1), b.sum(1), b.amin(1), b.amax(1)], 1)
    return table.cpu().numpy()


def run(pipeline, dev, stream):
    sp = stream.cuda_stream
    vol = synth.stack_torch(SHAPE, np.uint16, dev)
    cap = sqeazy_amd.max_compressed_length(pipeline, SHAPE, np.uint16)
    blob = torch.empty(cap, dtype=torch.uint8, device=dev)
    rc, n = sqeazy_amd.encode_device(pipeline, vol.data_ptr(), SHAPE, np.uint16, blob.data_ptr(), cap, stream=sp)
    assert rc == 0
    del vol
    fb = SHAPE[1] * SHAPE[2] * 2
    full = torch.empty(SHAPE, dtype=torch.int16, device=dev)            # the voxels every column is held to (quantiser: not the stack's)
    rc = sqeazy_amd.decode_frames_device(blob.data_ptr(), n, 0, SHAPE[0], full.data_ptr(), SHAPE[0] * fb, np.uint16, stream=sp)
    assert rc == 0
    torch.cuda.synchronize()
    for placement in PLACEMENTS:
        for count in COUNTS:
            origins = origins_of(placement, count)
            extents = [EXTENT] * count
            truth = torch.stack([full[tuple(slice(a, a + e) for a, e in zip(o, EXTENT))] for o in origins])
            views = truth.clone()                                       # the resident voxels: every 97th differs from the blob's
            views.reshape(-1)[::97] += 3
            scratch = torch.empty_like(truth)                           # (the baseline's own: the new call needs none)
            vptrs = [views[i].data_ptr() for i in range(count)]
            sptrs = [scratch[i].data_ptr() for i in range(count)]
            want = fields(truth, views)
            got = {}

            def base():
                rc = sqeazy_amd.decode_boxes_device(blob.data_ptr(), n, origins, sptrs, extents, None, np.uint16, stream=sp)
                assert rc == 0
                got["base"] = got["again"] = fields(scratch, views)

            def compare():
                rc, stats = sqeazy_amd.compare_boxes_device(blob.data_ptr(), n, origins, vptrs, extents, None, np.uint16, stream=sp)
                assert rc == 0
                got["compare"] = stats.astype(np.int64)

            fns = {"base": base, "again": base, "compare": compare}
            for c in COLUMNS:                                   # warm-up, and every column's rows against the full decode's
                scratch.fill_(0)
                fns[c]()
                torch.cuda.synchronize()
                assert np.array_equal(got[c], want), (pipeline, placement, count, c)
            ms = {c: [] for c in COLUMNS}
            for _ in range(K):
                for c in COLUMNS:
                    ms[c].append(round(timed(fns[c], stream), 3))
            gain = [round(x / s, 3) for s, x in zip(ms["compare"], ms["base"])]
            spread = [round(x / s, 3) for s, x in zip(ms["again"], ms["base"])]
            row = {"pipeline": pipeline, "placement": placement, "boxes": count, "extent": list(EXTENT), "stack": list(SHAPE), "blob_bytes": n,
                   "z_ranges": sorted(set(o[0] for o in origins)), "ms": ms, "min_max": {c: [min(ms[c]), max(ms[c])] for c in COLUMNS},
                   "base_over_compare": gain, "base_over_again": spread, "baseline_scratch_bytes": int(scratch.numel()) * 2}
            row["compare_faster_every_pair_by_more_than_the_spread"] = bool(min(gain) > max(max(spread), 1 / min(spread)))
            row["compare_kernel_ms"] = profiled(compare)
            print(json.dumps(row), flush=True)
            del views, truth, scratch
    del blob, full
    torch.cuda.empty_cache()


def main():
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev)
    for pipeline in PIPELINES:
        run(pipeline, dev, stream)


if __name__ == "__main__":
    main()
