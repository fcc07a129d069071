"""boxes of ONE large blob read at a coarser resolution in one call, against what a caller can do without the entry point
(GPU box):  python3 tools/bin_boxes_time.py [k] [pipeline ...]

Device time per call sequence (hipEvents around it on its stream, so the host's gaps between launches and every call's own synchronisation
count), k interleaved repetitions (default 7) after a warm-up, all in one process; a sample is REPS sequences in a row, divided by REPS.
A 64x1024x1024 u16 synth.stack_torch stack encoded as ONE blob (`bitswap1->lz4` and `quantiser->bitswap1->lz4`).  Rows:
  whole stack, bins (1,2,2), (2,2,2), (1,4,4), (4,4,4)  -- sum; the baseline decodes the whole volume into 128 MiB of scratch
  K = 64 boxes of 16x64x64, bins (2,2,2)                -- sum; spread over the four disjoint z-ranges of 16 frames
  one box 16x512x512, bins (1,512,1)                    -- max; a projection written as bins: 16 x 1 x 512 cells, 16 workgroups -- the
                                                           few-workgroup case; also timed against SQYAMD_Project_Boxes_* along axis 1
Columns:
  base     -- ONE SQYAMD_Decode_Boxes_*_Device call into scratch of the caller's, then the torch reduction that gives the same integers
              (the widened voxels reshaped to cells x bins, sum(dtype=int64) / amax / amin over the bins, cast to 32 bits): what a caller
              runs without the entry point
  again    -- the same once more in every repetition: base / again per pair is the spread a ratio has to beat
  bin      -- ONE SQYAMD_Bin_Boxes_*_Device call (no scratch of the caller's)
  project  -- the last row only: ONE SQYAMD_Project_Boxes_*_Device call along axis 1
Every column's outputs are held to each other and to the ones torch computes from the full decode's voxels.  Per row: min-max per column,
the per-pair ratios base / bin and base / again, whether every pair is faster by more than the spread (and whether every pair is slower by
more than it), the scratch bytes the baseline holds, and the per-kernel device times of one profiled `bin` call and one profiled `base`
call.  One JSON line per row, then the rows once more as a table."""
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
FINALS = ("bitswap1_bin_boxes", "bitswap1_quantiser_bin_boxes", "bitswap1_decode_boxes", "bitswap1_quantiser_decode_boxes", "bitswap1_project_boxes",
          "bitswap1_quantiser_project_boxes", "boxes_project_init", "lz4_frames_subset_decode")


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


def binned(voxels, bins, op):
    """the cells of a (K, Z, Y, X) int16 tensor that holds 16-bit voxels, extents that the bins divide, as int32 that holds the 32-bit elements"""
    k, z, y, x = voxels.shape
    wide = (voxels.to(torch.int32) & 0xffff).reshape(k, z // bins[0], bins[0], y // bins[1], bins[1], x // bins[2], bins[2])
    if op == "max":
        return wide.amax((2, 4, 6))
    if op == "min":
        return wide.amin((2, 4, 6))
    return wide.sum((2, 4, 6), dtype=torch.int64).to(torch.int32)


def rows():
    for bins in ((1, 2, 2), (2, 2, 2), (1, 4, 4), (4, 4, 4)):
        yield "whole stack bins %d,%d,%d" % bins, [(0, 0, 0)], SHAPE, bins, "sum", False
    per = SHAPE[1] // 64 - 1
    yield "K=64 16x64x64 bins 2,2,2", [(16 * (i % 4), (97 * i % per) * 64 + 5, (61 * i % per) * 64 + 3) for i in range(64)], (16, 64, 64), (2, 2, 2), "sum", False
    yield "one box 16x512x512 bins 1,512,1", [(24, 256, 256)], (16, 512, 512), (1, 512, 1), "max", True


def run(pipeline, dev, stream, table):
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
    for name, origins, extent, bins, op, with_project in rows():
        count = len(origins)
        extents = [extent] * count
        if count == 1 and tuple(extent) == SHAPE:
            want = binned(full[None], bins, op).cpu().numpy()
        else:
            truth = torch.stack([full[tuple(slice(a, a + e) for a, e in zip(o, extent))] for o in origins])
            want = binned(truth, bins, op).cpu().numpy()
            del truth
        scratch = torch.empty((count,) + tuple(extent), dtype=torch.int16, device=dev)      # (the baseline's own: the new call needs none)
        cells = torch.empty(want.shape, dtype=torch.int32, device=dev)
        sptrs = [scratch[i].data_ptr() for i in range(count)]
        cptrs = [cells[i].data_ptr() for i in range(count)]
        got = {}

        def base():
            rc = sqeazy_amd.decode_boxes_device(blob.data_ptr(), n, origins, sptrs, extents, None, np.uint16, stream=sp)
            assert rc == 0
            got["base"] = got["again"] = binned(scratch, bins, op)

        def bin_():
            rc = sqeazy_amd.bin_boxes_device(blob.data_ptr(), n, origins, extents, bins, op, cptrs, None, np.uint16, stream=sp)
            assert rc == 0
            got["bin"] = cells

        def project():                                          # (axis 1: the image is the cells with the kept dimension of 1 dropped)
            rc = sqeazy_amd.project_boxes_device(blob.data_ptr(), n, origins, extents, 1, op, cptrs, None, np.uint16, stream=sp)
            assert rc == 0
            got["project"] = cells

        fns = {"base": base, "again": base, "bin": bin_}
        if with_project:
            fns["project"] = project
        columns = tuple(fns)
        for c in columns:                                       # warm-up, and every column's outputs against the full decode's
            scratch.fill_(0)
            cells.fill_(0x5A5A5A5A)
            fns[c]()
            torch.cuda.synchronize()
            assert np.array_equal(got[c].cpu().numpy().reshape(want.shape), want), (pipeline, name, c)
        ms = {c: [] for c in columns}
        for _ in range(K):
            for c in columns:
                ms[c].append(round(timed(fns[c], stream), 3))
        gain = [round(x / s, 3) for s, x in zip(ms["bin"], ms["base"])]
        spread = [round(x / s, 3) for s, x in zip(ms["again"], ms["base"])]
        bar = max(max(spread), 1 / min(spread))
        row = {"pipeline": pipeline, "row": name, "boxes": count, "extent": list(extent), "bins": list(bins), "op": op, "stack": list(SHAPE), "blob_bytes": n,
               "ms": ms, "min_max": {c: [min(ms[c]), max(ms[c])] for c in columns}, "base_over_bin": gain, "base_over_again": spread,
               "baseline_scratch_bytes": int(scratch.numel()) * 2}
        row["bin_faster_every_pair_by_more_than_the_spread"] = bool(min(gain) > bar)
        row["bin_slower_every_pair_by_more_than_the_spread"] = bool(max(gain) < 1 / bar)
        if with_project:
            row["project_over_bin"] = [round(x / s, 3) for s, x in zip(ms["bin"], ms["project"])]
            row["project_kernel_ms"] = profiled(project)
        row["bin_kernel_ms"] = profiled(bin_)
        row["base_kernel_ms"] = profiled(base)
        print(json.dumps(row), flush=True)
        verdict = "faster" if row["bin_faster_every_pair_by_more_than_the_spread"] else "slower" if row["bin_slower_every_pair_by_more_than_the_spread"] else "level"
        kern = {k: v[0] for r in ("bin_kernel_ms", "base_kernel_ms", "project_kernel_ms") for k, v in row.get(r, {}).items() if k in FINALS}
        line = "%-25s %-32s" % (pipeline, name) + "".join("  %s %.3f - %.3f" % (c, min(ms[c]), max(ms[c])) for c in columns)
        line += "  base/bin %.3f - %.3f  base/again %.3f - %.3f  %s  kernels %s  scratch %d" % (min(gain), max(gain), min(spread), max(spread), verdict,
                                                                                                 " ".join("%s %.3f" % kv for kv in sorted(kern.items())),
                                                                                                 row["baseline_scratch_bytes"])
        table.append(line)
        got.clear()
        del scratch, cells
        torch.cuda.empty_cache()
    del blob, full
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
