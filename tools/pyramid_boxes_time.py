"""a whole resolution pyramid of boxes of ONE large blob in one call, against one SQYAMD_Bin_Boxes_* call per level
(GPU box):  python3 tools/pyramid_boxes_time.py [k] [pipeline ...]

Device time per call sequence (hipEvents around it on its stream, so the host's gaps between launches and every call's own synchronisation
count), k interleaved repetitions (default 7) after a warm-up, all in one process; a sample is REPS sequences in a row, divided by REPS.
A 64x1024x1024 u16 synth.stack_torch stack encoded as ONE blob (`bitswap1->lz4` and `quantiser->bitswap1->lz4`).  Rows:
  whole stack, (1,2,2) (1,4,4) (1,8,8) (1,16,16)          -- sum and max; four levels, all fused
  whole stack, (2,2,2) (4,4,4) (8,8,8) (16,16,16)         -- sum and max; four levels, all fused
  K = 64 boxes of 16x64x64, (1,1,1) (2,2,2) (4,4,4)       -- sum; spread over the four disjoint z-ranges of 16 frames
  whole stack, (1,2,2) (1,4,4) (1,256,256)                -- max; a top cell of 128 x 128 level-0 cells per layer does not fit the
                                                             accumulators: the top level takes the tail launch
Columns:
  base     -- a loop of ONE SQYAMD_Bin_Boxes_*_Device call per level: what a caller runs without the entry point (those entry points are
              the same code before and after this one was added)
  again    -- the same once more in every repetition: base / again per pair is the spread a ratio has to beat
  pyramid  -- ONE SQYAMD_Pyramid_Boxes_*_Device call
  layered  -- the same call with "pyramid_boxes_fused" = 0: level 0 by the binning's launch, a pyramid_reduce launch per further level
Every column's outputs are held to the base's, level by level.  Per row: min-max per column, the per-pair ratios base / pyramid,
base / again and layered / pyramid, whether every pair is faster by more than the spread (and whether every pair is slower by more than
it), and the per-kernel device times of one profiled call per column.  One JSON line per row, then the rows once more as a table."""
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
PIPELINES = sys.argv[2:] or ["bitswap1->lz4", "quantiser->bitswap1->lz4"]
FINALS = ("bitswap1_bin_boxes", "bitswap1_quantiser_bin_boxes", "bitswap1_pyramid_boxes", "bitswap1_quantiser_pyramid_boxes", "pyramid_reduce", "lz4_frames_subset_decode")


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


def rows():
    flat = ((1, 2, 2), (1, 4, 4), (1, 8, 8), (1, 16, 16))
    cubes = ((2, 2, 2), (4, 4, 4), (8, 8, 8), (16, 16, 16))
    for name, pyramid in (("1,2,2 .. 1,16,16", flat), ("2,2,2 .. 16,16,16", cubes)):
        for op in ("sum", "max"):
            yield "whole stack %s %s" % (name, op), [(0, 0, 0)], SHAPE, pyramid, op
    per = SHAPE[1] // 64 - 1
    yield ("K=64 16x64x64 1,1,1 2,2,2 4,4,4 sum", [(16 * (i % 4), (97 * i % per) * 64 + 5, (61 * i % per) * 64 + 3) for i in range(64)], (16, 64, 64),
           ((1, 1, 1), (2, 2, 2), (4, 4, 4)), "sum")
    yield "whole stack 1,2,2 1,4,4 1,256,256 max (tail)", [(0, 0, 0)], SHAPE, ((1, 2, 2), (1, 4, 4), (1, 256, 256)), "max"


def run(pipeline, dev, stream, table):
    sp = stream.cuda_stream
    vol = synth.stack_torch(SHAPE, np.uint16, dev)
    cap = sqeazy_amd.max_compressed_length(pipeline, SHAPE, np.uint16)
    blob = torch.empty(cap, dtype=torch.uint8, device=dev)
    rc, n = sqeazy_amd.encode_device(pipeline, vol.data_ptr(), SHAPE, np.uint16, blob.data_ptr(), cap, stream=sp)
    assert rc == 0
    del vol
    torch.cuda.synchronize()
    for name, origins, extent, pyramid, op in rows():
        count, nlev = len(origins), len(pyramid)
        extents = [extent] * count
        shapes = [sqeazy_amd.bin_shape(extent, bins) for bins in pyramid]
        # two sets of outputs, one per level and all boxes of the level in one tensor: the base's and the column's under test
        ref = [torch.empty((count,) + sh, dtype=torch.int32, device=dev) for sh in shapes]
        out = [torch.empty((count,) + sh, dtype=torch.int32, device=dev) for sh in shapes]
        ref_ptrs = [[ref[l][i].data_ptr() for i in range(count)] for l in range(nlev)]
        out_ptrs = [[out[l][i].data_ptr() for l in range(nlev)] for i in range(count)]

        def base():
            for l, bins in enumerate(pyramid):
                rc = sqeazy_amd.bin_boxes_device(blob.data_ptr(), n, origins, extents, bins, op, ref_ptrs[l], None, np.uint16, stream=sp)
                assert rc == 0

        def pyramid_():
            rc = sqeazy_amd.pyramid_boxes_device(blob.data_ptr(), n, origins, extents, pyramid, op, out_ptrs, None, np.uint16, stream=sp)
            assert rc == 0

        def layered():
            sqeazy_amd.set_option("pyramid_boxes_fused", 0)
            try:
                pyramid_()
            finally:
                sqeazy_amd.set_option("pyramid_boxes_fused", 1)

        fns = {"base": base, "again": base, "pyramid": pyramid_, "layered": layered}
        columns = tuple(fns)
        base()
        torch.cuda.synchronize()
        for c in ("pyramid", "layered"):                        # warm-up, and the column's outputs against the base's, level by level
            for t in out:
                t.fill_(0x5A5A5A5A)
            fns[c]()
            torch.cuda.synchronize()
            assert all(torch.equal(a, b) for a, b in zip(out, ref)), (pipeline, name, c)
        ms = {c: [] for c in columns}
        for _ in range(K):
            for c in columns:
                ms[c].append(round(timed(fns[c], stream), 3))
        gain = [round(x / s, 3) for s, x in zip(ms["pyramid"], ms["base"])]
        spread = [round(x / s, 3) for s, x in zip(ms["again"], ms["base"])]
        fused = [round(x / s, 3) for s, x in zip(ms["pyramid"], ms["layered"])]
        bar = max(max(spread), 1 / min(spread))
        row = {"pipeline": pipeline, "row": name, "boxes": count, "extent": list(extent), "bins": [list(b) for b in pyramid], "op": op, "stack": list(SHAPE),
               "blob_bytes": n, "ms": ms, "min_max": {c: [min(ms[c]), max(ms[c])] for c in columns}, "base_over_pyramid": gain, "base_over_again": spread,
               "layered_over_pyramid": fused, "median_base_over_pyramid": float(np.median(gain))}
        row["pyramid_faster_every_pair_by_more_than_the_spread"] = bool(min(gain) > bar)
        row["pyramid_slower_every_pair_by_more_than_the_spread"] = bool(max(gain) < 1 / bar)
        row["fused_faster_than_layered_every_pair_by_more_than_the_spread"] = bool(min(fused) > bar)
        row["fused_slower_than_layered_every_pair_by_more_than_the_spread"] = bool(max(fused) < 1 / bar)
        row["pyramid_kernel_ms"] = profiled(pyramid_)
        row["layered_kernel_ms"] = profiled(layered)
        row["base_kernel_ms"] = profiled(base)
        print(json.dumps(row), flush=True)
        verdict = "faster" if row["pyramid_faster_every_pair_by_more_than_the_spread"] else "slower" if row["pyramid_slower_every_pair_by_more_than_the_spread"] else "level"
        inner = ("faster" if row["fused_faster_than_layered_every_pair_by_more_than_the_spread"] else
                 "slower" if row["fused_slower_than_layered_every_pair_by_more_than_the_spread"] else "level")
        kern = " | ".join(" ".join("%s %.3fx%d" % (k, v[0], v[1]) for k, v in sorted(row[r].items()) if k in FINALS)
                          for r in ("pyramid_kernel_ms", "layered_kernel_ms", "base_kernel_ms"))
        line = "%-25s %-46s" % (pipeline, name) + "".join("  %s %.3f - %.3f" % (c, min(ms[c]), max(ms[c])) for c in columns)
        line += "  base/pyramid %.3f - %.3f (median %.3f)  base/again %.3f - %.3f  %s  layered/pyramid %.3f - %.3f  %s  kernels (pyramid | layered | base) %s" % (
            min(gain), max(gain), float(np.median(gain)), min(spread), max(spread), verdict, min(fused), max(fused), inner, kern)
        table.append(line)
        del ref, out
        torch.cuda.empty_cache()
    del blob
    torch.cuda.empty_cache()


def main():
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev)
    table = []
    for pipeline in PIPELINES:
        run(pipeline, dev, stream, table)
    print()
    for line in table:
        print(line)


if __name__ == "__main__":
    main()
